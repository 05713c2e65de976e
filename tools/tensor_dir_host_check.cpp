// tensor_dir_host_check.cpp -- csrc/tensor_dir.h on the host alone, for a sanitizer run: add / match / check_access through every
// refusal and one accepted case, with the bad entry last and first.  tensor_dir.h is plain C++ that common.h includes after
// SISIC_REQUIRE; the library's error sink (api.cpp) links against the HIP runtime, so this program brings the macro and a
// sink of its own that keeps the last text.
//
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/tensor_dir_host_check.cpp -o /tmp/tensor_dir_check
//     /tmp/tensor_dir_check          prints "tensor_dir: <n> checks passed"; any other end is a failure
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../include/sisic.h"

namespace sisic {
static char last_error[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
}
}  // namespace sisic
#define SISIC_REQUIRE(cond, ...)                 \
    do {                                         \
        if (!(cond)) {                           \
            ::sisic::set_error(__VA_ARGS__);     \
            return SISIC_EINVAL;                 \
        }                                        \
    } while (0)

#include "../synt_isic_amd/csrc/tensor_dir.h"

static int checks = 0;
static void expect(bool ok, const char* what) {
    ++checks;
    if (!ok) {
        std::fprintf(stderr, "tensor_dir: FAILED %s (last error: %s)\n", what, sisic::last_error);
        std::exit(1);
    }
}
static void refused(int rc, const std::string& text, const char* what) {
    expect(rc == SISIC_EINVAL && text == sisic::last_error, what);
}

int main() {
    sisic::TensorDir dir;
    expect(dir.size() == 0 && dir.name(0) == nullptr, "an empty directory");
    expect(dir.add("a.weight", 6) == 0 && dir.add("a.bias", 2) == 1 && dir.add("b.weight", 1) == 2, "add returns the index");
    expect(dir.size() == 3 && std::string(dir.name(1)) == "a.bias" && !dir.name(-1) && !dir.name(3), "size and name");

    // heap buffers of exactly the expected sizes: a read past one is the sanitizer's to report
    std::vector<float> a(6, 1.0f), b(2, 2.0f), c(1, 3.0f);
    std::vector<int> slot;
    {   // accepted, in another order than the directory's
        std::vector<const char*> keys = {"b.weight", "a.weight", "a.bias"};
        std::vector<const float*> ptrs = {c.data(), a.data(), b.data()};
        std::vector<int64_t> counts = {1, 6, 2};
        expect(dir.match("x_load", 3, keys.data(), ptrs.data(), counts.data(), &slot) == SISIC_OK, "an accepted state dict");
        expect(slot == std::vector<int>({2, 0, 1}), "slot_of_entry");
    }
    for (int at : {2, 0}) {       // the bad entry last, then first
        const std::string i = std::to_string(at);
        std::vector<const char*> keys = {"a.weight", "a.bias", "b.weight"};
        std::vector<const float*> ptrs = {a.data(), b.data(), c.data()};
        std::vector<int64_t> counts = {6, 2, 1};
        refused(dir.match("x_load", 2, keys.data(), ptrs.data(), counts.data(), &slot), "x_load: state dict has 2 tensors, expected 3",
                "count");
        auto keys2 = keys; auto ptrs2 = ptrs; auto counts2 = counts;
        ptrs2[at] = nullptr;
        refused(dir.match("x_load", 3, keys.data(), ptrs2.data(), counts.data(), &slot), "x_load: entry " + i + " is null", "null pointer");
        keys2[at] = nullptr;
        refused(dir.match("x_load", 3, keys2.data(), ptrs.data(), counts.data(), &slot), "x_load: entry " + i + " is null", "null name");
        keys2[at] = "c.weight";
        refused(dir.match("x_load", 3, keys2.data(), ptrs.data(), counts.data(), &slot), "x_load: unexpected key 'c.weight'", "unexpected");
        const int twin = (at + 1) % 3;          // the entry takes its neighbour's name and count: whichever comes second is refused
        keys2[at] = keys[twin];
        counts2[at] = counts[twin];
        refused(dir.match("x_load", 3, keys2.data(), ptrs.data(), counts2.data(), &slot),
                std::string("x_load: duplicate key '") + keys[twin] + "'", "duplicate");
        counts2[at] = counts[at] + 1;
        refused(dir.match("x_load", 3, keys.data(), ptrs.data(), counts2.data(), &slot),
                std::string("x_load: '") + keys[at] + "' has " + std::to_string(counts2[at]) + " elements, expected " +
                    std::to_string(counts[at]), "element count");
    }
    dir.noun = "float tensors";
    refused(dir.match("y_load", 0, nullptr, nullptr, nullptr, &slot), "y_load: state dict has 0 float tensors, expected 3", "noun");

    expect(dir.check_access("x_read", 0, 6, a.data()) == SISIC_OK && dir.check_access("x_read", 2, 1, c.data()) == SISIC_OK, "access");
    refused(dir.check_access("x_read", 3, 1, a.data()), "x_read: bad arguments", "index past the end");
    refused(dir.check_access("x_read", -1, 1, a.data()), "x_read: bad arguments", "negative index");
    refused(dir.check_access("x_write", 0, 6, nullptr), "x_write: bad arguments", "null pointer");
    refused(dir.check_access("x_write", 1, 3, b.data()), "x_write: 'a.bias' has 2 elements", "element count of an access");
    std::printf("tensor_dir: %d checks passed\n", checks);
    return 0;
}
