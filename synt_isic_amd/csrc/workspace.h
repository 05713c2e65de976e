// workspace.h -- host only: the activation pool both network executors (unet.cpp, resnet.cpp) draw from, and the allocator
// of the UNet's derived weight buffers.  No .hip file includes this header.
#pragma once

#include <algorithm>
#include <vector>

#include "common.h"

namespace sisic {

// Exact-size free list.  get() hands out the FIRST free block, in the order the blocks were allocated, whose byte size equals
// the request, and allocates when there is none: a network run at one shape asks for the same sizes in the same order every
// time and so receives the same addresses every time (a captured sampling step and a recorded training forward rely on it).
class Pool {
public:
    int get(size_t floats, float** out) {
        const size_t bytes = floats * sizeof(float);
        for (auto& b : blocks_)
            if (b.free_ && b.bytes == bytes) { b.free_ = false; *out = b.p; return SISIC_OK; }
        void* p = nullptr;
        SISIC_HIP(hipMalloc(&p, bytes));
        blocks_.push_back({static_cast<float*>(p), bytes, false});
        *out = static_cast<float*>(p);
        return SISIC_OK;
    }
    void put(float* p) {
        for (auto& b : blocks_)
            if (b.p == p) { b.free_ = true; return; }
    }
    // hipFree of every block, handed out or not: the caller has synchronised and forgotten every address
    void release_all() {
        for (auto& b : blocks_) (void)hipFree(b.p);
        blocks_.clear();
    }
    int64_t bytes() const {
        int64_t n = 0;
        for (const auto& b : blocks_) n += (int64_t)b.bytes;
        return n;
    }

private:
    struct Block { float* p; size_t bytes; bool free_; };
    std::vector<Block> blocks_;
};

// The blocks one run has taken from a pool: whatever is still out when the scope ends goes back (error paths included).
class PoolScope {
public:
    explicit PoolScope(Pool& pool) : pool_(pool) {}
    PoolScope(const PoolScope&) = delete;
    PoolScope& operator=(const PoolScope&) = delete;
    ~PoolScope() { for (float* p : out_) pool_.put(p); }
    int get(size_t floats, float** out) {
        SISIC_TRY(pool_.get(floats, out));
        out_.push_back(*out);
        return SISIC_OK;
    }
    void put(float* p) {
        pool_.put(p);
        out_.erase(std::remove(out_.begin(), out_.end(), p), out_.end());
    }
    void disown() { out_.clear(); }      // a new owner (the training tape) returns the blocks

private:
    Pool& pool_;
    std::vector<float*> out_;
};

// A derived weight buffer, freed with `owned`.  Already allocated: left alone (the weights are derived again after every
// optimizer step, into the same buffers).
inline int dev_alloc(std::vector<float*>& owned, size_t floats, float** out) {
    if (*out) return SISIC_OK;
    void* p = nullptr;
    SISIC_HIP(hipMalloc(&p, std::max<size_t>(floats, 4) * sizeof(float)));
    owned.push_back(static_cast<float*>(p));
    *out = static_cast<float*>(p);
    return SISIC_OK;
}

}  // namespace sisic
