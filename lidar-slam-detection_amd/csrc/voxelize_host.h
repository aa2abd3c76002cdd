// voxelize_host.h -- the host-only half of the detection front end (voxelize.hip): the grid of a range and a voxel size, and the bookkeeping of
// the sliding window of sweeps.  No device call, no HIP type: tools/voxelize_host_check.cpp runs it alone under the host sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace lio {
namespace voxelize {

// compute_grid_size (voxelization_kernel.cu:182-189): (int)std::round((max - min) / size) per axis in f32.  False for a non-finite value, a
// size <= 0, max <= min, or an axis outside [1, 2^31 - 1] (the reference's cast would be undefined there)
inline bool grid_of(const float* mn, const float* mx, const float* sz, int out[3]) {
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(mn[a]) || !std::isfinite(mx[a]) || !std::isfinite(sz[a]) || !(sz[a] > 0.f) || !(mx[a] > mn[a])) return false;
        const float q = std::round((mx[a] - mn[a]) / sz[a]);
        if (!(q >= 1.f && q < 2147483648.f)) return false;
        out[a] = (int)q;
    }
    return true;
}

// keys are 32 bits and 2^32 - 1 marks an empty slot: the product of the three must be below it (each is below 2^31: no overflow on the way)
inline bool grid_fits_key(const int g[3]) {
    const uint64_t plane = (uint64_t)g[0] * (uint64_t)g[1];
    return plane < 0xFFFFFFFFull && plane * (uint64_t)g[2] < 0xFFFFFFFFull;
}

// PreprocessImplement::forward's bookkeeping (preprocess_kernel.cu:60-97)
struct WindowBook {
    uint32_t max_points = 0;
    std::vector<int32_t> counts;  // rows per sweep, newest first
    uint64_t total = 0;           // rows in the window
    int cur = 0;                  // which half of the A/B buffer holds them

    void init(uint32_t max_points_, uint32_t frames) {
        max_points = max_points_;
        counts.assign(frames, 0);
        reset();
    }
    void reset() {
        std::fill(counts.begin(), counts.end(), 0);
        total = 0;
        cur = 0;
    }
    // the most rows the rule below can reach: a call into a full window still stores one row, at most max_frame_num - 1 times in a row before
    // a sweep is popped
    uint64_t max_rows() const { return (uint64_t)max_points + counts.size(); }

    // one call with n >= 1 rows offered (already clamped to max_points): the rows it stores; *moved = the older rows a realtime call rewrites
    // behind them (from the other half of the buffer: cur has been flipped)
    uint32_t step(uint32_t n, bool realtime, uint64_t* moved) {
        *moved = 0;
        if (realtime) {
            total -= (uint64_t)counts.back();  // pop out the last frame
            const int64_t room = (int64_t)max_points - (int64_t)total;
            n = (uint32_t)std::max<int64_t>(std::min<int64_t>((int64_t)n, room), 1);
            for (size_t i = counts.size() - 1; i >= 1; i--) counts[i] = counts[i - 1];
            cur ^= 1;
            *moved = total;
        } else {
            reset();  // the counts too: the reference keeps stale ones
        }
        counts[0] = (int32_t)n;
        total += n;
        return n;
    }
};

}  // namespace voxelize
}  // namespace lio
