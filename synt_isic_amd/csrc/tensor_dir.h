// tensor_dir.h -- the named tensors behind a handle (sisic_unet, sisic_resnet): what sisic_*_num_tensors / _tensor_name list, what
// sisic_*_load expects and what sisic_*_read / _write index.  Plain C++, no HIP: common.h includes it after SISIC_REQUIRE, whose
// error sink (set_error) carries every refusal; `who` names the entry point in the text ("unet_load", "resnet_read", ...).
#pragma once

namespace sisic {

struct TensorDir {
    std::vector<std::string> names;
    std::vector<int64_t> numels;
    std::map<std::string, int> index;
    const char* noun = "tensors";      // what match's count refusal calls the entries

    int add(const std::string& name, int64_t numel) {
        index[name] = size();
        names.push_back(name);
        numels.push_back(numel);
        return size() - 1;
    }
    int size() const { return (int)names.size(); }
    const char* name(int i) const { return i >= 0 && i < size() ? names[i].c_str() : nullptr; }

    // A caller's state dict against the directory, and nothing else: the count, then every entry (null, unexpected key, duplicate
    // key, element count).  SISIC_OK: slot_of_entry[i] is the tensor entry i holds.  A load calls this before it changes anything.
    int match(const char* who, int n, const char* const* keys, const float* const* host_ptrs, const int64_t* counts,
              std::vector<int>* slot_of_entry) const {
        SISIC_REQUIRE(n == size(), "%s: state dict has %d %s, expected %d", who, n, noun, size());
        std::vector<char> seen(names.size(), 0);
        slot_of_entry->clear();
        for (int i = 0; i < n; ++i) {
            SISIC_REQUIRE(keys[i] && host_ptrs[i], "%s: entry %d is null", who, i);
            auto it = index.find(keys[i]);
            SISIC_REQUIRE(it != index.end(), "%s: unexpected key '%s'", who, keys[i]);
            const int idx = it->second;
            SISIC_REQUIRE(!seen[idx], "%s: duplicate key '%s'", who, keys[i]);
            SISIC_REQUIRE(counts[i] == numels[idx], "%s: '%s' has %lld elements, expected %lld", who, keys[i], (long long)counts[i],
                          (long long)numels[idx]);
            seen[idx] = 1;
            slot_of_entry->push_back(idx);
        }
        return SISIC_OK;
    }
    // the arguments of a read or write of tensor i
    int check_access(const char* who, int i, int64_t numel, const void* host_ptr) const {
        SISIC_REQUIRE(host_ptr && i >= 0 && i < size(), "%s: bad arguments", who);
        SISIC_REQUIRE(numel == numels[i], "%s: '%s' has %lld elements", who, names[i].c_str(), (long long)numels[i]);
        return SISIC_OK;
    }
};

}  // namespace sisic
