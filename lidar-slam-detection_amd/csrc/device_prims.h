// device_prims.h -- the device-wide primitives the map-export files share (cloud.hip, knn_index.hip, ground.hip, bev.hip):
//
//   scan / radix   cloud.hip's device-wide exclusive scan and stable 8-bit radix pass, and the view of a lio_cloud's device points
//   compaction     stable stream compaction over tiles of 2048 items: compact_tile_count / compact_tile_write in the caller's two kernels
//                  (its predicate, loads and payload), compact_words / compact_finish on the host
//   helpers        ordered float words, the radix digit match, the long-run queue, tile / block arithmetic
//   handles        what every lio_*_create / reserve / download of these files does: typed alloc, grow, event times, device + stream + events
//
// voxelgrid.hip takes the ordered words and the digit match from here; its own tile layout (per-wave contiguous runs) is not this one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "lio_common.h"

struct lio_cloud;

namespace lio {
namespace cloud {

// device-wide exclusive prefix sum of m uint32 words in place; aux holds scan_aux_words(m) words
uint64_t scan_aux_words(uint64_t m);
int exclusive_scan(hipStream_t st, uint32_t* data, uint64_t m, uint32_t* aux);

// one stable pass of an LSD radix sort of (key, value) pairs by the 8-bit digit (key >> shift) & 255, kin/vin -> kout/vout (n <= 2^31 - 1);
// scratch holds radix_scratch_words(n) words
uint64_t radix_scratch_words(uint64_t n);
int radix_pass(hipStream_t st, const uint32_t* kin, const uint32_t* vin, uint32_t* kout, uint32_t* vout, uint32_t n, int shift, uint32_t* scratch);

// pcl::VoxelGrid over n device points (lio_cloud_voxel_downsample's launches and semantics) from `in` to `out`: the same buffer (in place) or
// another of n points (`in` is then left as it was).  scratch holds voxel_filter_words(n) words; the centroid launches are enqueued on st,
// not waited for
uint64_t voxel_filter_words(uint64_t n);
int voxel_filter(hipStream_t st, const float4* in, uint32_t n, float leaf, float4* out, uint32_t* scratch, uint64_t* n_out);

// the points of a cloud as they lie on the device, and the stream its appends and voxel grid run on
struct CloudView {
    const float4* pts;
    uint64_t n;
    hipStream_t stream;
    int device;
};
CloudView cloud_view(const lio_cloud* c);

}  // namespace cloud

// ---- small helpers ---------------------------------------------------------------------------------------------------------------------------
// f32 <-> a uint32 whose unsigned order is the float order
__host__ __device__ inline uint32_t f2ord(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ord2f(uint32_t u) { return __builtin_bit_cast(float, (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }

// the lanes of the wave whose 8-bit digit equals this lane's (valid lanes only)
__device__ inline unsigned long long match_digit(uint32_t d, bool valid) {
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

namespace prims {

constexpr int kThreads = 256;
constexpr int kItems = 8;
constexpr uint32_t kTile = kThreads * kItems;  // 2048 items per workgroup: points, keys or scan entries
constexpr int kWaves = kThreads / 64;

inline uint32_t tiles_of(uint64_t n) { return (uint32_t)((n + kTile - 1) / kTile); }
inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }
inline uint64_t round_words(uint64_t w) { return (w + 63) & ~63ull; }  // 256-byte steps: every carved sub-buffer stays 16-byte aligned

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// one lane per run: the lanes whose run is long put its number v on the queue for a wave-per-run kernel, one atomic per wave
__device__ __forceinline__ void queue_long_run(bool is_long, uint32_t v, uint32_t* __restrict__ longlist, uint32_t* __restrict__ n_long) {
    const unsigned long long lm = __ballot(is_long);
    if (lm) {
        const int lane = threadIdx.x & 63;
        const int leader = __ffsll((long long)lm) - 1;
        uint32_t qb = 0;
        if (lane == leader) qb = atomicAdd(n_long, (uint32_t)__popcll(lm));
        qb = __shfl(qb, leader);
        if (is_long) longlist[qb + __popcll(lm & ((1ull << lane) - 1ull))] = v;
    }
}

// ---- the Matrix4d rule ------------------------------------------------------------------------------------------------------------------------
// pcl::transformPointCloud(in, out, Matrix4d) (PCL 1.9.1 transforms.hpp) as lio_cloud_append_* and lio_scan_merge_* apply it: per point in
// f64, terms left to right, no contraction (-ffp-contract=off), one cast to f32; non-finite points are transformed too
struct XformArgs {
    double m[12];  // rows 0..2 of the row-major 4 x 4
    double zmin, zmax;
    float scale;   // intensity factor (numpy_to_pointcloud(.., multiply)); 1 = left alone
    int band;      // keep only zmin <= z <= zmax (compared in f64, as `p.z >= g_map_config.z_min` with double bounds)
};

__device__ __forceinline__ float4 xform(float4 p, const XformArgs& a) {
    const double x = p.x, y = p.y, z = p.z;
    float4 o;
    o.x = (float)(((a.m[0] * x + a.m[1] * y) + a.m[2] * z) + a.m[3]);
    o.y = (float)(((a.m[4] * x + a.m[5] * y) + a.m[6] * z) + a.m[7]);
    o.z = (float)(((a.m[8] * x + a.m[9] * y) + a.m[10] * z) + a.m[11]);
    o.w = (a.scale != 1.0f) ? p.w * a.scale : p.w;
    return o;
}

// ---- stable stream compaction ----------------------------------------------------------------------------------------------------------------
// A workgroup of kThreads owns tile blockIdx.x; item r of thread tid is i = blockIdx.x * kTile + r * kThreads + tid.  The caller's count
// kernel ends with compact_tile_count, the host calls compact_finish, the caller's write kernel hands its keep bits to compact_tile_write.

// c = the items this thread keeps; counts[blockIdx.x] = the tile's
__device__ __forceinline__ void compact_tile_count(uint32_t c, uint32_t* __restrict__ counts) {
    __shared__ uint32_t wc[kWaves];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (wc[0] + wc[1]) + (wc[2] + wc[3]);
}

// emit(r, o) for every kept item r of this thread, o = its place in input order: tile prefix (offs[blockIdx.x]) + kept items of rounds < r +
// kept of waves < w in round r + kept lanes < l
template <typename Emit>
__device__ __forceinline__ void compact_tile_write(const bool (&keep)[kItems], const uint32_t* __restrict__ offs, Emit emit) {
    __shared__ uint32_t wcnt[kItems][kWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long km[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        km[r] = __ballot(keep[r]);
        if (lane == 0) wcnt[r][wave] = (uint32_t)__popcll(km[r]);
    }
    __syncthreads();
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t run = offs[blockIdx.x];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        uint32_t woff = 0, rtot = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            const uint32_t t = wcnt[r][w];
            woff += (w < wave) ? t : 0u;
            rtot += t;
        }
        if ((km[r] >> lane) & 1ull) emit(r, run + woff + (uint32_t)__popcll(km[r] & lt));
        run += rtot;
    }
}

// words of scratch a compaction of n items takes: the tile counts and the total, then (256-byte aligned: the scan reads its tile sums as
// uint4) the scan's own scratch
inline uint64_t compact_words(uint64_t n) {
    const uint64_t m = (uint64_t)tiles_of(n) + 1;
    return round_words(m) + round_words(cloud::scan_aux_words(m) + 64);
}

// after the count kernel: counts[0 .. tiles) become the tiles' prefixes and the word behind them the total, whose device address is returned
// (NULL: the error is set)
inline const uint32_t* compact_finish(hipStream_t st, uint32_t* counts, uint64_t n) {
    const uint64_t m = (uint64_t)tiles_of(n) + 1;
    if (hipMemsetAsync(counts + m - 1, 0, sizeof(uint32_t), st) != hipSuccess) {
        set_error("compaction: clearing the total failed");
        return nullptr;
    }
    if (cloud::exclusive_scan(st, counts, m, counts + round_words(m)) != LIO_OK) return nullptr;
    return counts + m - 1;
}

// ---- host handles ----------------------------------------------------------------------------------------------------------------------------
template <typename T>
bool alloc(T** p, uint64_t count) {
    return hipMalloc(p, std::max<uint64_t>(count, 1) * sizeof(T)) == hipSuccess;
}

// a buffer of at least `need` elements, its old contents dropped (the stream is drained first); `who` opens the error
template <typename T>
int grow(const char* who, T** buf, uint64_t* cap, uint64_t need, hipStream_t st) {
    if (need <= *cap && *buf) return LIO_OK;
    LIO_HIP_TRY(hipStreamSynchronize(st));
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    if (!alloc(buf, need)) {
        (void)hipGetLastError();
        set_error("%s: %llu bytes of device memory not available", who, (unsigned long long)(need * sizeof(T)));
        return LIO_E_DEVICE;
    }
    *cap = need;
    return LIO_OK;
}

inline float elapsed_us(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms * 1000.f : 0.f;
}

// the opening of a lio_*_create (`who`): the device checked and made current, a non-blocking stream and n_ev events.  On failure nothing is
// left behind and the error is set.
inline bool open_device(const char* who, int device, hipStream_t* stream, hipEvent_t* ev, int n_ev) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) {
        (void)hipGetLastError();
        set_error("%s: no HIP device %d (there is no CPU fallback)", who, device);
        return false;
    }
    if (hipSetDevice(device) != hipSuccess) { set_error("%s: hipSetDevice(%d) failed", who, device); return false; }
    bool ok = hipStreamCreateWithFlags(stream, hipStreamNonBlocking) == hipSuccess;
    int made = 0;
    while (ok && made < n_ev) {
        ok = hipEventCreate(&ev[made]) == hipSuccess;
        made += ok ? 1 : 0;
    }
    if (ok) return true;
    (void)hipGetLastError();
    set_error("%s: stream / event creation failed", who);
    for (int i = 0; i < made; i++) { (void)hipEventDestroy(ev[i]); ev[i] = nullptr; }
    if (*stream) (void)hipStreamDestroy(*stream);
    *stream = nullptr;
    return false;
}

// n elements at src to the host array `out` of cap elements: n, or -n when cap is too small; `who` opens the error
template <typename T>
int64_t download(const char* who, int device, hipStream_t st, const T* src, uint64_t n, T* out, uint64_t cap) {
    if (n > cap) return -(int64_t)n;
    if (n == 0) return 0;
    if (!out) return LIO_E_INVALID;
    hipSetDevice(device);
    if (hipMemcpyAsync(out, src, n * sizeof(T), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        set_error("%s: download failed", who);
        return LIO_E_DEVICE;
    }
    return (int64_t)n;
}

}  // namespace prims
}  // namespace lio
