// workspace.h -- host only: the activation pool both network executors (unet.cpp, resnet.cpp) draw from, and the allocator
// of the UNet's derived weight buffers.  No .hip file includes this header.
#pragma once

#include <algorithm>
#include <vector>

#include "common.h"
#include "poison_switch.h"

namespace sisic {

// SISIC_POISON_ALLOC=1 (a test switch, off unless set; poison_alloc(), read once per process in conv_plan.cpp): every block the executors take -- from the pool,
// fresh or reused, and from hipMalloc for derived weights, grown rows, scratch and training state -- is filled with byte 0xFF
// (fp32: a NaN) before anything is written to it, so whatever a layer leaves unwritten no longer holds the previous run's nearly
// identical values.  Buffers the design zero-fills are zero-filled after it.  No launch and no address order changes; graph
// mode is off (no memset nodes go into captured steps).
// a fresh allocation: filled and waited for, so the fill precedes whatever any stream does with the block
inline int poison_fresh(void* p, size_t bytes) {
    if (poison_alloc() && p && bytes) {
        SISIC_HIP(hipMemset(p, 0xFF, bytes));
        SISIC_HIP(hipDeviceSynchronize());
    }
    return SISIC_OK;
}

// Exact-size free list.  get() hands out the FIRST free block, in the order the blocks were allocated, whose byte size equals
// the request, and allocates when there is none: a network run at one shape asks for the same sizes in the same order every
// time and so receives the same addresses every time (a captured sampling step and a recorded training forward rely on it).
class Pool {
public:
    // `s`: the stream of the run that takes the block (what the poison fill is ordered on; a reused block was returned by an
    // earlier run of the same stream or after a synchronisation)
    int get(size_t floats, float** out, hipStream_t s) {
        const size_t bytes = floats * sizeof(float);
        for (auto& b : blocks_)
            if (b.free_ && b.bytes == bytes) {
                if (poison_alloc() && bytes) SISIC_HIP(hipMemsetAsync(b.p, 0xFF, bytes, s));
                b.free_ = false; *out = b.p; return SISIC_OK;
            }
        void* p = nullptr;
        SISIC_HIP(hipMalloc(&p, bytes));
        blocks_.push_back({static_cast<float*>(p), bytes, false});
        *out = static_cast<float*>(p);
        if (poison_alloc() && bytes) SISIC_HIP(hipMemsetAsync(p, 0xFF, bytes, s));
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
    PoolScope(Pool& pool, hipStream_t s) : pool_(pool), s_(s) {}
    PoolScope(const PoolScope&) = delete;
    PoolScope& operator=(const PoolScope&) = delete;
    ~PoolScope() { for (float* p : out_) pool_.put(p); }
    int get(size_t floats, float** out) {
        SISIC_TRY(pool_.get(floats, out, s_));
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
    hipStream_t s_;
    std::vector<float*> out_;
};

// A derived weight buffer, freed with `owned`.  Already allocated: left alone (the weights are derived again after every
// optimizer step, into the same buffers).
inline int dev_alloc(std::vector<float*>& owned, size_t floats, float** out) {
    if (*out) return SISIC_OK;
    void* p = nullptr;
    SISIC_HIP(hipMalloc(&p, std::max<size_t>(floats, 4) * sizeof(float)));
    SISIC_TRY(poison_fresh(p, std::max<size_t>(floats, 4) * sizeof(float)));
    owned.push_back(static_cast<float*>(p));
    *out = static_cast<float*>(p);
    return SISIC_OK;
}

}  // namespace sisic
