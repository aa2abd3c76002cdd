// cloud.hip -- a device-resident cloud that grows over a drive (lio_cloud) and the pcl::VoxelGrid of the WHOLE cloud on gfx950 (wave64).
//
// The map-export half of the reference's module (slam/src/graph_utils.cpp:160-200 export_points / dump_map_points, :398-446
// save_undistortion_cloud / accumulate_cloud / save_accumulate_cloud): every frame is moved into the world frame and appended to one cloud, and
// the cloud of a whole drive (10^7 - 10^8 points) goes through one VoxelGrid.  The per-scan chain of voxelgrid.hip is sized for <= 10^6 points
// (its scatter workgroups fold every tile's histogram row: O(tiles^2) reads); this file is the device-wide form:
//
//   append     xform + band -> device_prims.h's stable compaction [tile counts -> device-wide scan -> write]   (no band: one launch, in order)
//   bbox       per-workgroup records (grid-stride) -> one workgroup folds them and derives the grid (PCL's int32 guard included)
//   keys       voxel index per point + the histogram of its lowest digit, [digit][tile]
//   4 x        {tile histogram -> device-wide exclusive scan of the [digit][tile] table -> stable scatter}  (passes above the key's bits: skipped)
//   heads      tile counts of run heads -> the same scan -> compaction of the head positions, fused with the gather into sorted order
//   centroid   one lane per voxel for runs < 32 points; longer runs (the "monster" voxels of a dense map included) one wave each, 64 points per
//              step parked in LDS and summed by four lanes, one coordinate each -- PCL's sequential f32 sum in ascending input index either way
//
// Workgroups hand results to each other only at kernel boundaries (no look-back, no spin-waits: the XCDs' L2s are not coherent with each
// other and dispatch order is not guaranteed).  Point indices are 32-bit (PCL's own int limit: 2^31 - 1 points per filter call); byte offsets
// are 64-bit.  The sort scratch is allocated for the call and freed after it (lio_cloud_scratch_bytes tells its peak).
// The transform restates pcl::transformPointCloud(in, out, Matrix4d) (PCL 1.9.1 transforms.hpp) as slam_wrapper.cpp does for the static
// transform: per point in f64, terms left to right, no contraction (-ffp-contract=off), cast to f32; non-finite points are transformed too.
#include <algorithm>

#include "device_prims.h"

namespace lio {
namespace cloud {

using namespace prims;

constexpr uint32_t kBboxBlocks = 1024;         // workgroups of the bbox's first level (grid-stride): the fold reads 1024 records
constexpr uint32_t kLongRun = 32;              // runs of at least this many points are summed one wave per run
constexpr uint32_t kLongBlocks = 4096;         // one-wave workgroups of the long-run kernel (grid-stride over the queue)

// exclusive prefix of v over the 256 threads of a workgroup (fixed order); *total = the sum.  Uses `ws` (kWaves words of LDS).
__device__ inline uint32_t block_exclusive(uint32_t v, uint32_t* ws, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    __syncthreads();  // (ws may still be read by a previous call)
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        const uint32_t t = ws[w];
        pre += (w < wave) ? t : 0u;
        tot += t;
    }
    *total = tot;
    return pre + inc - v;
}

// ---- the scan primitive: device-wide exclusive prefix sum of m uint32 words, in place -------------------------------------------------------
// level 1: one word per tile of 2048 (cl_scan_reduce); the tile sums are scanned by the same primitive (recursively, ~m / 2^11 per level);
// level 2: every tile scans itself and adds its tile's prefix (cl_scan_apply).  Three launches per level, hand-off at the kernel boundaries.
__global__ __launch_bounds__(kThreads) void cl_scan_reduce(const uint32_t* __restrict__ in, uint64_t m, uint32_t* __restrict__ sums) {
    __shared__ uint32_t ws[kWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kItems;
    uint32_t s = 0;
    if (i + kItems <= m) {
        const uint4 a = *reinterpret_cast<const uint4*>(in + i), b = *reinterpret_cast<const uint4*>(in + i + 4);
        s = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w));
    } else {
        for (int k = 0; k < kItems; k++)
            if (i + k < m) s += in[i + k];
    }
    uint32_t tot;
    (void)block_exclusive(s, ws, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kThreads) void cl_scan_apply(uint32_t* __restrict__ data, uint64_t m, const uint32_t* __restrict__ offs) {
    __shared__ uint32_t ws[kWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kItems;
    uint32_t v[kItems];
    const bool full = i + kItems <= m;
    if (full) {
        const uint4 a = *reinterpret_cast<const uint4*>(data + i), b = *reinterpret_cast<const uint4*>(data + i + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < kItems; k++) v[k] = (i + k < m) ? data[i + k] : 0u;
    }
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kItems; k++) s += v[k];
    uint32_t tot;
    uint32_t run = block_exclusive(s, ws, &tot) + (offs ? offs[blockIdx.x] : 0u);
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const uint32_t t = v[k];
        v[k] = run;
        run += t;
    }
    if (full) {
        *reinterpret_cast<uint4*>(data + i) = make_uint4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<uint4*>(data + i + 4) = make_uint4(v[4], v[5], v[6], v[7]);
    } else {
        for (int k = 0; k < kItems; k++)
            if (i + k < m) data[i + k] = v[k];
    }
}

// words of scratch the scan of m entries needs for its tile sums (all levels)
uint64_t scan_aux_words(uint64_t m) {
    uint64_t w = 0;
    for (uint64_t nb = tiles_of(m); nb > 1; nb = tiles_of(nb)) w += round_words(nb);
    return w;
}

int exclusive_scan(hipStream_t st, uint32_t* data, uint64_t m, uint32_t* aux) {
    if (m == 0) return LIO_OK;
    const uint64_t nb = tiles_of(m);
    if (nb > 1) {
        cl_scan_reduce<<<dim3((uint32_t)nb), dim3(kThreads), 0, st>>>(data, m, aux);
        const int rc = exclusive_scan(st, aux, nb, aux + round_words(nb));
        if (rc != LIO_OK) return rc;
    }
    cl_scan_apply<<<dim3((uint32_t)nb), dim3(kThreads), 0, st>>>(data, m, nb > 1 ? aux : nullptr);
    LIO_HIP_TRY(hipGetLastError());
    return LIO_OK;
}

// ---- append: transform, band, stable compaction --------------------------------------------------------------------------------------------
// (XformArgs and xform, the Matrix4d rule of the append, live in device_prims.h: scanmerge.hip applies the same function)
__device__ __forceinline__ bool keep(const float4& o, const XformArgs& a) { return !a.band || ((double)o.z >= a.zmin && (double)o.z <= a.zmax); }

// kept points per tile (band only)
__global__ __launch_bounds__(kThreads) void cl_append_count(const float4* __restrict__ in, uint32_t n, XformArgs a, uint32_t* __restrict__ counts) {
    const uint32_t base = blockIdx.x * kTile;
    float4 p[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        p[r] = in[i < n ? i : n - 1u];
    }
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        c += (i < n && keep(xform(p[r], a), a)) ? 1u : 0u;
    }
    compact_tile_count(c, counts);
}

// the write: without a band every point lands at its own index; with one, the kept points in input order
__global__ __launch_bounds__(kThreads) void cl_append_write(const float4* __restrict__ in, uint32_t n, XformArgs a, const uint32_t* __restrict__ offs,
                                                            float4* __restrict__ out) {
    const uint32_t base = blockIdx.x * kTile;
    const int tid = threadIdx.x;
    float4 p[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + tid;
        p[r] = in[i < n ? i : n - 1u];
    }
    if (!a.band) {
#pragma unroll
        for (int r = 0; r < kItems; r++) {
            const uint32_t i = base + r * kThreads + tid;
            if (i < n) out[i] = xform(p[r], a);
        }
        return;
    }
    bool kept[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + tid;
        p[r] = xform(p[r], a);
        kept[r] = i < n && keep(p[r], a);
    }
    compact_tile_write(kept, offs, [&](int r, uint32_t o) { out[o] = p[r]; });
}

// ---- voxel grid ------------------------------------------------------------------------------------------------------------------------------
struct Grid {  // what the fold derives; the host reads it back once (pass-through, point counts, the radix passes to launch)
    uint32_t bmin[3], bmax[3];
    uint32_t n_valid, pass, total, nbits;
    int minb[3];
    int mul1, mul2;
    uint32_t n_long;  // long runs queued by cl_centroid
    uint32_t pad[2];
};

// bbox, level 1: kBboxBlocks workgroups over the cloud, one 8-word record each {min x y z, max x y z (order-preserving codes), finite points, -}
__global__ __launch_bounds__(kThreads) void cl_bbox_part(const float4* __restrict__ in, uint32_t n, uint32_t* __restrict__ parts) {
    float mn0 = INFINITY, mn1 = INFINITY, mn2 = INFINITY, mx0 = -INFINITY, mx1 = -INFINITY, mx2 = -INFINITY;
    uint32_t cnt = 0;
    const uint32_t stride = gridDim.x * kThreads;
    for (uint32_t i0 = blockIdx.x * kThreads + threadIdx.x; i0 < n; i0 += 4u * stride) {
        float4 q[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t j = (uint64_t)i0 + (uint64_t)k * stride;
            q[k] = in[j < n ? j : i0];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float4 p = q[k];
            if ((uint64_t)i0 + (uint64_t)k * stride < n && isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
                mn0 = fminf(mn0, p.x); mx0 = fmaxf(mx0, p.x);
                mn1 = fminf(mn1, p.y); mx1 = fmaxf(mx1, p.y);
                mn2 = fminf(mn2, p.z); mx2 = fmaxf(mx2, p.z);
                cnt++;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn0 = fminf(mn0, __shfl_xor(mn0, off)); mx0 = fmaxf(mx0, __shfl_xor(mx0, off));
        mn1 = fminf(mn1, __shfl_xor(mn1, off)); mx1 = fmaxf(mx1, __shfl_xor(mx1, off));
        mn2 = fminf(mn2, __shfl_xor(mn2, off)); mx2 = fmaxf(mx2, __shfl_xor(mx2, off));
        cnt += __shfl_xor(cnt, off);
    }
    __shared__ float red[kWaves][6];
    __shared__ uint32_t redc[kWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        red[wave][0] = mn0; red[wave][1] = mn1; red[wave][2] = mn2;
        red[wave][3] = mx0; red[wave][4] = mx1; red[wave][5] = mx2;
        redc[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; w++) {
            mn0 = fminf(mn0, red[w][0]); mn1 = fminf(mn1, red[w][1]); mn2 = fminf(mn2, red[w][2]);
            mx0 = fmaxf(mx0, red[w][3]); mx1 = fmaxf(mx1, red[w][4]); mx2 = fmaxf(mx2, red[w][5]);
            cnt += redc[w];
        }
        uint4* o = reinterpret_cast<uint4*>(parts + 8u * blockIdx.x);
        o[0] = make_uint4(f2ord(mn0), f2ord(mn1), f2ord(mn2), f2ord(mx0));
        o[1] = make_uint4(f2ord(mx1), f2ord(mx2), cnt, 0u);
    }
}

// bbox, level 2: one workgroup folds the records and derives the grid as voxelgrid.hip's vg_derive does (PCL's "leaf size is too small"
// guard: the voxel count of the box overflows int32 -> output = input)
__global__ __launch_bounds__(kThreads) void cl_bbox_fold(const uint32_t* __restrict__ parts, uint32_t nparts, float inv, Grid* __restrict__ g) {
    uint32_t bmin[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, bmax[3] = {0u, 0u, 0u}, n_valid = 0;
    for (uint32_t b = threadIdx.x; b < nparts; b += kThreads) {
        const uint4 r0 = reinterpret_cast<const uint4*>(parts)[2 * b], r1 = reinterpret_cast<const uint4*>(parts)[2 * b + 1];
        if (r1.z) {
            bmin[0] = min(bmin[0], r0.x); bmin[1] = min(bmin[1], r0.y); bmin[2] = min(bmin[2], r0.z);
            bmax[0] = max(bmax[0], r0.w); bmax[1] = max(bmax[1], r1.x); bmax[2] = max(bmax[2], r1.y);
            n_valid += r1.z;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            bmin[a] = min(bmin[a], (uint32_t)__shfl_xor((int)bmin[a], off));
            bmax[a] = max(bmax[a], (uint32_t)__shfl_xor((int)bmax[a], off));
        }
        n_valid += (uint32_t)__shfl_xor((int)n_valid, off);
    }
    __shared__ uint32_t sbox[kWaves][8];
    if ((threadIdx.x & 63) == 0) {
        uint32_t* o = sbox[threadIdx.x >> 6];
        o[0] = bmin[0]; o[1] = bmin[1]; o[2] = bmin[2]; o[3] = bmax[0]; o[4] = bmax[1]; o[5] = bmax[2]; o[6] = n_valid;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kWaves; w++) {
        for (int a = 0; a < 3; a++) { sbox[0][a] = min(sbox[0][a], sbox[w][a]); sbox[0][3 + a] = max(sbox[0][3 + a], sbox[w][3 + a]); }
        sbox[0][6] += sbox[w][6];
    }
    Grid r;
    for (int a = 0; a < 3; a++) { r.bmin[a] = sbox[0][a]; r.bmax[a] = sbox[0][3 + a]; }
    r.n_valid = sbox[0][6];
    r.pass = 0;
    r.total = 0;
    r.nbits = 0;
    r.minb[0] = r.minb[1] = r.minb[2] = 0;
    r.mul1 = r.mul2 = 0;
    r.n_long = 0;
    r.pad[0] = r.pad[1] = 0;
    if (r.n_valid) {
        float mn[3], mx[3];
        for (int a = 0; a < 3; a++) { mn[a] = ord2f(r.bmin[a]); mx[a] = ord2f(r.bmax[a]); }
        const long long dx = (long long)((mx[0] - mn[0]) * inv) + 1;
        const long long dy = (long long)((mx[1] - mn[1]) * inv) + 1;
        const long long dz = (long long)((mx[2] - mn[2]) * inv) + 1;
        long long divb[3];
        for (int a = 0; a < 3; a++) {
            r.minb[a] = (int)floorf(mn[a] * inv);
            divb[a] = (long long)((int)floorf(mx[a] * inv)) - r.minb[a] + 1;
        }
        const long long total = divb[0] * divb[1] * divb[2];
        if (dx * dy * dz > 2147483647LL || total > 0xFFFFFFF0LL) r.pass = 1;
        r.mul1 = (int)divb[0];
        r.mul2 = (int)(divb[0] * divb[1]);
        r.total = r.pass ? 0u : (uint32_t)total;
        r.nbits = r.total ? (32 - __clz(r.total)) : 0;  // keys 0..total (total = the non-finite marker) need bits(total)
    }
    *g = r;
}

// voxel index of every point (non-finite: `total`, behind every voxel) and the histogram of its lowest digit into table[digit][tile]
__global__ __launch_bounds__(kThreads) void cl_keys(const float4* __restrict__ in, uint32_t n, float inv, const Grid* __restrict__ gp,
                                                    uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ table, uint32_t ntiles) {
    __shared__ uint32_t h[256];
    const uint32_t base = blockIdx.x * kTile;
    float4 p[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        p[r] = in[i < n ? i : n - 1u];
    }
    const uint32_t total = gp->total;
    const int mb0 = gp->minb[0], mb1 = gp->minb[1], mb2 = gp->minb[2], mul1 = gp->mul1, mul2 = gp->mul2;
    h[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        if (i >= n) continue;
        uint32_t key = total;
        if (isfinite(p[r].x) && isfinite(p[r].y) && isfinite(p[r].z)) {
            const int i0 = (int)(floorf(p[r].x * inv) - (float)mb0);
            const int i1 = (int)(floorf(p[r].y * inv) - (float)mb1);
            const int i2 = (int)(floorf(p[r].z * inv) - (float)mb2);
            key = (uint32_t)i0 + (uint32_t)i1 * (uint32_t)mul1 + (uint32_t)i2 * (uint32_t)mul2;
        }
        keys[i] = key;
        vals[i] = i;
        atomicAdd(&h[key & 255u], 1u);
    }
    __syncthreads();
    table[(size_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(kThreads) void cl_hist(const uint32_t* __restrict__ keys, uint32_t n, int shift, uint32_t* __restrict__ table, uint32_t ntiles) {
    __shared__ uint32_t h[256];
    const uint32_t base = blockIdx.x * kTile;
    uint32_t k[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        k[r] = keys[i < n ? i : n - 1u];
    }
    h[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(k[r] >> shift) & 255u], 1u);
    }
    __syncthreads();
    table[(size_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// stable scatter of one 8-bit digit: the scanned table gives every (digit, tile) its global base; inside the tile each wave owns a contiguous
// run of 512 keys, so (wave, round, lane) order is input order, and the ranks come from eight ballots per item (the scheme of voxelgrid.hip)
__global__ __launch_bounds__(kThreads) void cl_scatter(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin, uint32_t* __restrict__ kout,
                                                       uint32_t* __restrict__ vout, uint32_t n, int shift, const uint32_t* __restrict__ table, uint32_t ntiles) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ uint32_t wcnt[kWaves][256];
    const uint32_t base = blockIdx.x * kTile + wave * (64 * kItems);
    uint32_t k[kItems], v[kItems];
    bool ok[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * 64 + lane;
        ok[r] = i < n;
        const uint32_t ic = ok[r] ? i : n - 1u;
        k[r] = kin[ic];
        v[r] = vin[ic];
    }
    const uint32_t gbase = table[(size_t)tid * ntiles + blockIdx.x];
    for (int j = tid; j < kWaves * 256; j += kThreads) (&wcnt[0][0])[j] = 0;
    __syncthreads();
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t below[kItems], total[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t d = (k[r] >> shift) & 255u;
        const unsigned long long peers = match_digit(d, ok[r]);
        below[r] = (uint32_t)__popcll(peers & lt);
        total[r] = (uint32_t)__popcll(peers);
        if (ok[r] && below[r] == 0) wcnt[wave][d] += total[r];
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {
        uint32_t g = gbase;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            const uint32_t t = wcnt[w][tid];
            wcnt[w][tid] = g;
            g += t;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t d = (k[r] >> shift) & 255u;
        uint32_t pos = 0;
        if (ok[r]) pos = wcnt[wave][d] + below[r];
        __builtin_amdgcn_wave_barrier();
        if (ok[r] && below[r] == 0) wcnt[wave][d] += total[r];
        __builtin_amdgcn_wave_barrier();
        if (ok[r]) { kout[pos] = k[r]; vout[pos] = v[r]; }
    }
}

// words of scratch one radix_pass over n keys takes: the [digit][tile] table (+1) and its scan's tile sums
uint64_t radix_scratch_words(uint64_t n) {
    const uint64_t tab = 256ull * tiles_of(n) + 1;
    return round_words(tab) + round_words(scan_aux_words(tab) + 64);
}

// one stable 8-bit pass of the key sort above for callers outside this file (knn_index.hip): tile histogram, device-wide scan of the
// [digit][tile] table, stable scatter -- the launches of lio_cloud_voxel_downsample's passes, with cl_hist for every digit
int radix_pass(hipStream_t st, const uint32_t* kin, const uint32_t* vin, uint32_t* kout, uint32_t* vout, uint32_t n, int shift, uint32_t* scratch) {
    if (n == 0) return LIO_OK;
    const uint32_t ntiles = (uint32_t)tiles_of(n);
    const uint64_t tab = 256ull * ntiles;
    uint32_t* table = scratch;
    uint32_t* aux = scratch + round_words(tab + 1);
    cl_hist<<<dim3(ntiles), dim3(kThreads), 0, st>>>(kin, n, shift, table, ntiles);
    LIO_HIP_TRY(hipGetLastError());
    const int rc = exclusive_scan(st, table, tab, aux);
    if (rc != LIO_OK) return rc;
    cl_scatter<<<dim3(ntiles), dim3(kThreads), 0, st>>>(kin, vin, kout, vout, n, shift, table, ntiles);
    LIO_HIP_TRY(hipGetLastError());
    return LIO_OK;
}

// run heads (first sorted position of every occupied voxel) per tile
__global__ __launch_bounds__(kThreads) void cl_head_count(const uint32_t* __restrict__ keys, uint32_t n, uint32_t total, uint32_t* __restrict__ counts) {
    const uint32_t base = blockIdx.x * kTile;
    uint32_t kc[kItems], kp[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        const uint32_t ic = i < n ? i : n - 1u;
        kc[r] = keys[ic];
        kp[r] = keys[ic ? ic - 1u : 0u];
    }
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        c += (i < n && kc[r] < total && (i == 0 || kp[r] != kc[r])) ? 1u : 0u;
    }
    compact_tile_count(c, counts);
}

// compaction of the heads in sorted order (hpos[v] = first sorted position of voxel v, hpos[n_vox] = n_valid: the non-finite points sort behind
// every voxel) and the gather of the finite points into sorted order
__global__ __launch_bounds__(kThreads) void cl_head_write(const float4* __restrict__ in, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                          uint32_t n, uint32_t n_valid, uint32_t total, const uint32_t* __restrict__ offs, uint32_t ntiles,
                                                          uint32_t* __restrict__ hpos, float4* __restrict__ sorted) {
    const int tid = threadIdx.x;
    const uint32_t base = blockIdx.x * kTile;
    uint32_t kc[kItems], kp[kItems], vv[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + tid;
        const uint32_t ic = i < n ? i : n - 1u;
        kc[r] = keys[ic];
        kp[r] = keys[ic ? ic - 1u : 0u];
        vv[r] = vals[ic];
    }
    bool head[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + tid;
        head[r] = i < n && kc[r] < total && (i == 0 || kp[r] != kc[r]);
    }
    compact_tile_write(head, offs, [&](int r, uint32_t o) { hpos[o] = base + r * kThreads + tid; });
    if (blockIdx.x == 0 && tid == 0) hpos[offs[ntiles]] = n_valid;
#pragma unroll
    for (int r0 = 0; r0 < kItems; r0 += 4) {
        float4 pt[4];
#pragma unroll
        for (int k = 0; k < 4; k++) pt[k] = in[vv[r0 + k]];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t i = base + (r0 + k) * kThreads + tid;
            if (i < n_valid) sorted[i] = pt[k];
        }
    }
}

// one lane per voxel: runs shorter than kLongRun summed by the lane (eight loads, then four at a time, in flight together), longer ones queued
// (one atomic per wave) for cl_long.  out may alias the cloud: the points are read from `sorted` only.
__global__ __launch_bounds__(kThreads) void cl_centroid(const float4* __restrict__ sorted, const uint32_t* __restrict__ hpos, uint32_t nvox,
                                                        float4* __restrict__ out, uint32_t* __restrict__ longlist, Grid* __restrict__ g) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    const bool live = v < nvox;
    const uint32_t a = hpos[live ? v : 0u], b = hpos[live ? v + 1u : 0u];
    const bool is_long = live && b - a >= kLongRun;
    queue_long_run(is_long, v, longlist, &g->n_long);
    if (!live || is_long) return;
    float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
    {
        float4 p[8];
#pragma unroll
        for (int k = 0; k < 8; k++) p[k] = sorted[(a + k < b) ? (a + k) : (b - 1)];
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (a + k < b) { sx = sx + p[k].x; sy = sy + p[k].y; sz = sz + p[k].z; sw = sw + p[k].w; }
    }
    for (uint32_t j = a + 8; j < b; j += 4) {
        float4 p[4];
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = sorted[(j + k < b) ? (j + k) : (b - 1)];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (j + k < b) { sx = sx + p[k].x; sy = sy + p[k].y; sz = sz + p[k].z; sw = sw + p[k].w; }
    }
    const float c = (float)(b - a);
    out[v] = make_float4(sx / c, sy / c, sz / c, sw / c);
}

// one wave (= one workgroup) per long run: 64 points per step loaded coalesced (the next step's already in flight), parked in LDS by coordinate,
// and summed by lanes 0..3 (one coordinate each) in ascending order -- the sequential f32 sum, ~1 add per point per lane.  A voxel of 10^5
// points (the ground under a slow stretch of a drive at 0.1 m) is ~1 600 steps of one wave; the other waves take the other runs meanwhile.
__global__ __launch_bounds__(64) void cl_long(const float4* __restrict__ sorted, const uint32_t* __restrict__ hpos, const uint32_t* __restrict__ longlist,
                                              const Grid* __restrict__ g, float4* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float park[4][64];
    const int lane = threadIdx.x;
    const uint32_t nl = g->n_long;
    for (uint32_t q = blockIdx.x; q < nl; q += gridDim.x) {
        const uint32_t v = longlist[q];
        const uint32_t a = hpos[v], b = hpos[v + 1];
        float s = 0.f;
        float4 cur = sorted[(a + lane < b) ? a + lane : b - 1u];
        for (uint32_t j = a; j < b; j += 64) {
            const uint32_t nj = j + 64;
            float4 nxt = cur;
            if (nj < b) nxt = sorted[(nj + lane < b) ? nj + lane : b - 1u];
            __syncthreads();  // the previous step's LDS reads are done
            park[0][lane] = cur.x; park[1][lane] = cur.y; park[2][lane] = cur.z; park[3][lane] = cur.w;
            __syncthreads();
            if (lane < 4) {
                const float4* pc = reinterpret_cast<const float4*>(park[lane]);
                const uint32_t cnt = (b - j < 64u) ? b - j : 64u;
                if (cnt == 64u) {
#pragma unroll
                    for (int k = 0; k < 16; k += 4) {
                        const float4 q0 = pc[k], q1 = pc[k + 1], q2 = pc[k + 2], q3 = pc[k + 3];
                        s = s + q0.x; s = s + q0.y; s = s + q0.z; s = s + q0.w;
                        s = s + q1.x; s = s + q1.y; s = s + q1.z; s = s + q1.w;
                        s = s + q2.x; s = s + q2.y; s = s + q2.z; s = s + q2.w;
                        s = s + q3.x; s = s + q3.y; s = s + q3.z; s = s + q3.w;
                    }
                } else {
                    for (uint32_t k = 0; k < cnt; k++) s = s + park[lane][k];
                }
            }
            cur = nxt;
        }
        if (lane < 4) reinterpret_cast<float*>(out + v)[lane] = s / (float)(b - a);
    }
}

}  // namespace cloud
}  // namespace lio

using namespace lio;
using namespace lio::cloud;

struct lio_cloud {
    int device;
    hipStream_t stream;
    float4* pts;       // the cloud, n of cap points
    uint64_t n, cap;
    float4* stage;     // host clouds land here before the transform
    uint64_t stage_cap;
    uint32_t* aux;     // the append's tile counts and their scan's tile sums
    uint64_t aux_cap;  // (words)
    hipEvent_t ev[5];  // append begin / end, voxel grid begin / end, the append's end for the scan's stream
    double append_us, voxel_us;
};

namespace lio {
namespace cloud {
CloudView cloud_view(const lio_cloud* c) { return CloudView{c->pts, c->n, c->stream, c->device}; }
}  // namespace cloud
}  // namespace lio

namespace {

// the sort scratch of one voxel grid over n points, carved from one allocation (256-byte aligned pieces)
struct VgLayout {
    uint64_t keys_a, keys_b, vals_a, vals_b, sorted, table, aux, parts, grid, total;
};
VgLayout vg_layout(uint64_t n) {
    const uint64_t ntiles = tiles_of(n);
    const uint64_t tab = 256ull * ntiles + 1;  // [digit][tile] (+1: the scanned total)
    VgLayout L;
    uint64_t w = 0;
    L.keys_a = w; w += round_words(n + 1);     // n + 1: the other key buffer holds hpos (n_vox + 1 <= n + 1 words)
    L.keys_b = w; w += round_words(n + 1);
    L.vals_a = w; w += round_words(n);         // the other value buffer holds the long-run queue
    L.vals_b = w; w += round_words(n);
    L.sorted = w; w += round_words(4 * n);
    L.table = w; w += std::max(round_words(tab), compact_words(n));  // also the heads' compaction scratch
    L.aux = w; w += round_words(scan_aux_words(tab) + 64);
    L.parts = w; w += round_words(8ull * kBboxBlocks);
    L.grid = w; w += round_words(sizeof(Grid) / 4);
    L.total = w;
    return L;
}

int cloud_reserve(lio_cloud* c, uint64_t need) {
    if (need <= c->cap) return LIO_OK;
    uint64_t want = std::max<uint64_t>(need, std::max<uint64_t>(2 * c->cap, 1ull << 16));
    float4* p = nullptr;
    if (hipMalloc(&p, want * sizeof(float4)) != hipSuccess) {
        (void)hipGetLastError();
        want = need;
        if (hipMalloc(&p, want * sizeof(float4)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("lio_cloud: %llu points (%llu bytes) of device memory not available", (unsigned long long)need,
                      (unsigned long long)(need * sizeof(float4)));
            return LIO_E_DEVICE;
        }
    }
    if (c->n) {
        if (hipMemcpyAsync(p, c->pts, c->n * sizeof(float4), hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) {
            (void)hipFree(p);
            set_error("lio_cloud: growing the cloud failed");
            return LIO_E_DEVICE;
        }
    }
    if (c->pts) (void)hipFree(c->pts);
    c->pts = p;
    c->cap = want;
    return LIO_OK;
}

XformArgs make_xform(const double T[16], float scale, int z_band, double z_min, double z_max) {
    XformArgs a;
    for (int i = 0; i < 12; i++) a.m[i] = T ? T[i] : ((i % 5 == 0) ? 1.0 : 0.0);
    a.zmin = z_min;
    a.zmax = z_max;
    a.scale = scale;
    a.band = z_band ? 1 : 0;
    return a;
}

// the append of n device points at `in` (on the cloud's stream)
int cloud_append(lio_cloud* c, const float4* in, uint64_t n, const XformArgs& a) {
    if (n == 0) return LIO_OK;
    if (n > 0x7FFFFFFFull) { set_error("lio_cloud: one append takes at most 2^31 - 1 points (%llu)", (unsigned long long)n); return LIO_E_CAPACITY; }
    const uint32_t nn = (uint32_t)n, ntiles = (uint32_t)tiles_of(n);
    hipEventRecord(c->ev[0], c->stream);
    uint64_t kept = n;
    if (a.band) {
        const int rc = grow("lio_cloud", &c->aux, &c->aux_cap, compact_words(n), c->stream);
        if (rc != LIO_OK) return rc;
        cl_append_count<<<dim3(ntiles), dim3(kThreads), 0, c->stream>>>(in, nn, a, c->aux);
        const uint32_t* d_kept = compact_finish(c->stream, c->aux, n);
        if (!d_kept) return LIO_E_DEVICE;
        cl_append_write<<<dim3(ntiles), dim3(kThreads), 0, c->stream>>>(in, nn, a, c->aux, c->pts + c->n);
        LIO_HIP_TRY(hipGetLastError());
        uint32_t k = 0;
        LIO_HIP_TRY(hipMemcpyAsync(&k, d_kept, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        hipEventRecord(c->ev[1], c->stream);
        LIO_HIP_TRY(hipStreamSynchronize(c->stream));
        kept = k;
    } else {
        cl_append_write<<<dim3(ntiles), dim3(kThreads), 0, c->stream>>>(in, nn, a, nullptr, c->pts + c->n);
        LIO_HIP_TRY(hipGetLastError());
        hipEventRecord(c->ev[1], c->stream);
        LIO_HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->append_us = elapsed_us(c->ev[0], c->ev[1]);
    c->n += kept;
    return LIO_OK;
}

}  // namespace

namespace lio {
namespace cloud {

uint64_t voxel_filter_words(uint64_t n) { return n ? vg_layout(n).total : 0; }

// the launches of lio_cloud_voxel_downsample over n points at `in` (1 <= n <= 2^31 - 1), the centroids written to `out`: `in` itself (the
// in-place form: the points are read from the sorted copy only) or another buffer of n points, in which case `in` is left as it was
// (lio_calib_imu's target staging).  PCL's overflow guard returns the input: out of place that is a device-to-device copy.  The last
// launches are enqueued, not waited for; the two words the host needs (the grid, the voxel count) are.
int voxel_filter(hipStream_t st, const float4* in, uint32_t n, float leaf, float4* out, uint32_t* base, uint64_t* n_out) {
    const float inv = 1.0f / leaf;
    const uint32_t ntiles = (uint32_t)tiles_of(n);
    const VgLayout L = vg_layout(n);
    uint32_t *ka = base + L.keys_a, *kb = base + L.keys_b, *va = base + L.vals_a, *vb = base + L.vals_b, *table = base + L.table, *aux = base + L.aux;
    float4* sorted = reinterpret_cast<float4*>(base + L.sorted);
    Grid* g = reinterpret_cast<Grid*>(base + L.grid);
    const uint64_t tab = 256ull * ntiles;
    Grid hg;
    uint64_t result = n;
    {
        const uint32_t nb = std::min<uint32_t>(ntiles, kBboxBlocks);
        cl_bbox_part<<<dim3(nb), dim3(kThreads), 0, st>>>(in, n, base + L.parts);
        cl_bbox_fold<<<dim3(1), dim3(kThreads), 0, st>>>(base + L.parts, nb, inv, g);
        LIO_HIP_TRY(hipGetLastError());
        LIO_HIP_TRY(hipMemcpyAsync(&hg, g, sizeof(Grid), hipMemcpyDeviceToHost, st));
        LIO_HIP_TRY(hipStreamSynchronize(st));
    }
    if (hg.pass) {
        result = n;  // PCL's overflow guard: the output is the input, non-finite points included
        if (out != in) LIO_HIP_TRY(hipMemcpyAsync(out, in, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, st));
    } else if (hg.n_valid == 0) {
        result = 0;
    } else {
        const int passes = (int)((hg.nbits + 7u) >> 3);
        cl_keys<<<dim3(ntiles), dim3(kThreads), 0, st>>>(in, n, inv, g, ka, va, table, ntiles);
        LIO_HIP_TRY(hipGetLastError());
        for (int p = 0; p < passes; p++) {
            const uint32_t* kin = (p & 1) ? kb : ka;
            const uint32_t* vin = (p & 1) ? vb : va;
            uint32_t* kout = (p & 1) ? ka : kb;
            uint32_t* vout = (p & 1) ? va : vb;
            if (p > 0) cl_hist<<<dim3(ntiles), dim3(kThreads), 0, st>>>(kin, n, 8 * p, table, ntiles);
            const int rc = exclusive_scan(st, table, tab, aux);
            if (rc != LIO_OK) return rc;
            cl_scatter<<<dim3(ntiles), dim3(kThreads), 0, st>>>(kin, vin, kout, vout, n, 8 * p, table, ntiles);
            LIO_HIP_TRY(hipGetLastError());
        }
        const bool odd = passes & 1;
        const uint32_t* keys = odd ? kb : ka;
        const uint32_t* vals = odd ? vb : va;
        uint32_t* hpos = odd ? ka : kb;     // the free key buffer (n + 1 words)
        uint32_t* longlist = odd ? va : vb;  // the free value buffer (n words)
        cl_head_count<<<dim3(ntiles), dim3(kThreads), 0, st>>>(keys, n, hg.total, table);
        const uint32_t* d_nvox = compact_finish(st, table, n);
        if (!d_nvox) return LIO_E_DEVICE;
        cl_head_write<<<dim3(ntiles), dim3(kThreads), 0, st>>>(in, keys, vals, n, hg.n_valid, hg.total, table, ntiles, hpos, sorted);
        LIO_HIP_TRY(hipGetLastError());
        uint32_t nvox = 0;
        LIO_HIP_TRY(hipMemcpyAsync(&nvox, d_nvox, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        LIO_HIP_TRY(hipStreamSynchronize(st));
        if (nvox) {
            cl_centroid<<<dim3((nvox + kThreads - 1) / kThreads), dim3(kThreads), 0, st>>>(sorted, hpos, nvox, out, longlist, g);
            cl_long<<<dim3(kLongBlocks), dim3(64), 0, st>>>(sorted, hpos, longlist, g, out);
            LIO_HIP_TRY(hipGetLastError());
        }
        result = nvox;
    }
    *n_out = result;
    return LIO_OK;
}

}  // namespace cloud
}  // namespace lio

extern "C" {

lio_cloud* lio_cloud_create(int device, uint64_t reserve_points) {
    lio_cloud* c = new lio_cloud();
    memset(c, 0, sizeof(*c));
    c->device = device;
    if (!open_device("lio_cloud_create", device, &c->stream, c->ev, 5)) {
        delete c;
        return nullptr;
    }
    if (reserve_points && cloud_reserve(c, reserve_points) != LIO_OK) {
        lio_cloud_destroy(c);
        return nullptr;
    }
    return c;
}

void lio_cloud_destroy(lio_cloud* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->pts) hipFree(c->pts);
    if (c->stage) hipFree(c->stage);
    if (c->aux) hipFree(c->aux);
    for (int i = 0; i < 5; i++)
        if (c->ev[i]) hipEventDestroy(c->ev[i]);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

int lio_cloud_clear(lio_cloud* c) {
    if (!c) return LIO_E_INVALID;
    c->n = 0;
    return LIO_OK;
}

int lio_cloud_size(lio_cloud* c, uint64_t* n) {
    if (!c || !n) return LIO_E_INVALID;
    *n = c->n;
    return LIO_OK;
}

int lio_cloud_append_scan(lio_cloud* c, lio_scan* s, const double T[16], float intensity_scale, int z_band, double z_min, double z_max) {
    if (!c || !s) return LIO_E_INVALID;
    if (s->device != c->device) { set_error("lio_cloud_append_scan: the scan lives on device %d, the cloud on %d", s->device, c->device); return LIO_E_INVALID; }
    hipSetDevice(c->device);
    const uint64_t n = s->n_raw;
    if (n == 0) return LIO_OK;
    int rc = cloud_reserve(c, c->n + n);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipEventRecord(c->ev[4], s->stream));  // the scan's upload / undistortion first
    LIO_HIP_TRY(hipStreamWaitEvent(c->stream, c->ev[4], 0));
    return cloud_append(c, s->raw, n, make_xform(T, intensity_scale, z_band, z_min, z_max));  // (waits for its stream: the scan may be reused at once)
}

int lio_cloud_append_host(lio_cloud* c, const float* xyzi, uint64_t n, const double T[16], float intensity_scale, int z_band, double z_min, double z_max) {
    if (!c || (!xyzi && n)) return LIO_E_INVALID;
    if (n == 0) return LIO_OK;
    if (n > 0x7FFFFFFFull) { set_error("lio_cloud: one append takes at most 2^31 - 1 points (%llu)", (unsigned long long)n); return LIO_E_CAPACITY; }
    hipSetDevice(c->device);
    int rc = cloud_reserve(c, c->n + n);
    if (rc != LIO_OK) return rc;
    rc = grow("lio_cloud", &c->stage, &c->stage_cap, n, c->stream);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipMemcpyAsync(c->stage, xyzi, n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    return cloud_append(c, c->stage, n, make_xform(T, intensity_scale, z_band, z_min, z_max));
}

int lio_cloud_scratch_bytes(lio_cloud* c, uint64_t* bytes) {
    if (!c || !bytes) return LIO_E_INVALID;
    *bytes = c->n ? vg_layout(c->n).total * sizeof(uint32_t) : 0;
    return LIO_OK;
}

int lio_cloud_voxel_downsample(lio_cloud* c, float leaf, uint64_t* n_out) {
    if (!c || !(leaf > 0.f)) return LIO_E_INVALID;
    if (c->n > 0x7FFFFFFFull) {
        set_error("lio_cloud_voxel_downsample: %llu points exceed pcl::VoxelGrid's int index range (2^31 - 1)", (unsigned long long)c->n);
        return LIO_E_CAPACITY;
    }
    hipSetDevice(c->device);
    const uint32_t n = (uint32_t)c->n;
    c->voxel_us = 0;
    if (n == 0) {
        if (n_out) *n_out = 0;
        return LIO_OK;
    }
    const uint64_t words = voxel_filter_words(n);
    uint32_t* base = nullptr;
    if (hipMalloc(&base, words * sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("lio_cloud_voxel_downsample: %llu bytes of sort scratch not available", (unsigned long long)(words * sizeof(uint32_t)));
        return LIO_E_DEVICE;
    }
    uint64_t result = n;
    int rc = LIO_OK;
    if (hipEventRecord(c->ev[2], c->stream) != hipSuccess) { set_error("lio_cloud_voxel_downsample: event record failed"); rc = LIO_E_DEVICE; }
    if (rc == LIO_OK) rc = voxel_filter(c->stream, c->pts, n, leaf, c->pts, base, &result);
    if (rc == LIO_OK && hipEventRecord(c->ev[3], c->stream) != hipSuccess) { set_error("lio_cloud_voxel_downsample: event record failed"); rc = LIO_E_DEVICE; }
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == LIO_OK) { set_error("lio_cloud_voxel_downsample: the stream failed"); rc = LIO_E_DEVICE; }
    (void)hipFree(base);
    if (rc != LIO_OK) return rc;
    c->voxel_us = elapsed_us(c->ev[2], c->ev[3]);
    c->n = result;
    if (n_out) *n_out = result;
    return LIO_OK;
}

int64_t lio_cloud_download(lio_cloud* c, float* xyzi, uint64_t cap) {
    if (!c || (!xyzi && c->n)) return LIO_E_INVALID;
    if (c->n > cap) return -(int64_t)c->n;
    hipSetDevice(c->device);
    if (c->n) LIO_HIP_TRY(hipMemcpyAsync(xyzi, c->pts, c->n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    LIO_HIP_TRY(hipStreamSynchronize(c->stream));
    return (int64_t)c->n;
}

int lio_cloud_last_times(lio_cloud* c, double* append_us, double* voxel_us) {
    if (!c) return LIO_E_INVALID;
    if (append_us) *append_us = c->append_us;
    if (voxel_us) *voxel_us = c->voxel_us;
    return LIO_OK;
}

}  // extern "C"
