// voxelize.hip -- the front end of the reference's detection network on gfx950 (wave64): the sliding window of sweeps
// (sensor_driver/inference/voxelize/preprocess_kernel.cu), the hash voxeliser and the mean VFE to f16 (voxelization_kernel.cu), as
// LidarInference::forward calls them (sensor_driver/inference/tensorRT/lidar_inference.cpp:81-85).  include/lio_hip.h states every rule: the
// result is the reference's kernels run one thread after another in index order, bit for bit, whatever order the device's threads arrive in.
//
//   vx_window  the old sweeps moved by the ego motion into the other half of an A/B buffer, behind the room of the new sweep.  Rows are 20 bytes;
//              a workgroup loads 256 of them as 1280 consecutive floats into LDS, each lane rewrites its row there (stride 5 words: no bank
//              conflict), and the tile goes out as consecutive floats again
//   vx_insert  per point the voxel key or "out"; an open-addressing table (a power of two of at least twice the points: there is always an empty
//              slot, every probe ends), the key claimed by atomicCAS, the slot's value the atomicMin of the point index = the voxel's first
//              point.  The slot of every point is kept: no later kernel probes
//   vx_heads   a point is a head iff its slot's value is its own index; device_prims.h's stable compaction ranks the heads in window order:
//              the rank is the voxel id.  The head writes the id beside the key, the voxel's index row, and empties the voxel's point slots
//   vx_slots   per point of a kept voxel: the voxel's max_points_per_voxel smallest point indices by an atomicMin cascade over the voxel's slots
//              (the displaced index is carried to the next slot): whatever order threads arrive in, the slots end up holding the smallest
//              indices in ascending order.  A point larger than the last slot's value leaves without an atomic
//   vx_mean    per voxel the kept rows gathered by index, summed per channel in slot order in f32, divided by the count, rounded to f16
//
// No floating-point atomic, no kernel uses scratch, one stream, one host wait per call (the 16-byte record with the voxel count).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "device_prims.h"
#include "voxelize_host.h"

namespace lio {
namespace voxelize {

using namespace prims;

constexpr int kFeat = 5;             // num_feature of the reference's call site: x y z intensity time
constexpr uint32_t kEmpty = 0xFFFFFFFFu;  // no key, no point, no slot
constexpr int kWinRows = 256;        // rows per workgroup of vx_window

struct Motion {
    float m[12];  // rows 0..2 of the row-major 4 x 4
};

struct Grid {
    float mn[3], mx[3], sz[3];
    int g[3];
};

// ---- window ------------------------------------------------------------------------------------------------------------------------------------
// transform_kernel of preprocess_kernel.cu:6-20: row r of src becomes row r of dst (the caller has moved dst behind the new sweep)
__global__ __launch_bounds__(kWinRows) void vx_window(const float* __restrict__ src, float* __restrict__ dst, uint32_t rows, Motion mo) {
    __shared__ float s[kWinRows * kFeat];
    const uint32_t row0 = blockIdx.x * kWinRows;
    const uint32_t nrow = min((uint32_t)kWinRows, rows - row0);
    const uint32_t nf = nrow * kFeat;
    const uint64_t base = (uint64_t)row0 * kFeat;
    for (uint32_t k = threadIdx.x; k < nf; k += kWinRows) s[k] = src[base + k];
    __syncthreads();
    if (threadIdx.x < nrow) {
        float* r = s + threadIdx.x * kFeat;
        const float x = r[0], y = r[1], z = r[2], t = r[4];
        r[0] = mo.m[0] * x + mo.m[1] * y + mo.m[2] * z + mo.m[3];
        r[1] = mo.m[4] * x + mo.m[5] * y + mo.m[6] * z + mo.m[7];
        r[2] = mo.m[8] * x + mo.m[9] * y + mo.m[10] * z + mo.m[11];
        r[4] = (float)((double)t + 0.1);  // the reference's 0.1 is a double
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < nf; k += kWinRows) dst[base + k] = s[k];
}

// ---- insert ------------------------------------------------------------------------------------------------------------------------------------
// MurmurHash3's 32-bit finaliser: where a key probes first (the result does not depend on it)
__device__ __forceinline__ uint32_t mix(uint32_t k) {
    k ^= k >> 16;
    k *= 0x85ebca6bu;
    k ^= k >> 13;
    k *= 0xc2b2ae35u;
    k ^= k >> 16;
    return k;
}

// the voxel index of one coordinate, or -1: floorf((p - min) / size) in f32 with min <= p < max and 0 <= index < grid
// (voxelization_kernel.cu:118-134); the float is compared before it is converted, so no conversion is out of int's range
__device__ __forceinline__ int axis_index(float p, float mn, float mx, float sz, int g) {
    if (!(p >= mn && p < mx)) return -1;
    const float f = floorf((p - mn) / sz);
    if (!(f >= 0.f && f < 2147483648.f)) return -1;
    const int i = (int)f;
    return i < g ? i : -1;
}

// pslot[i] = the table slot of point i's voxel, or kEmpty for a point that is not finite or not in range; stats[0] += points in range
__global__ __launch_bounds__(kThreads) void vx_insert(const float* __restrict__ rows, uint32_t n, Grid gr, uint32_t mask, uint32_t* __restrict__ t_key,
                                                      uint32_t* __restrict__ t_first, uint32_t* __restrict__ pslot, uint32_t* __restrict__ stats) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t key = kEmpty;
    if (i < n) {
        const float* r = rows + (uint64_t)i * kFeat;
        const float x = r[0], y = r[1], z = r[2];
        if (finite3(x, y, z)) {
            const int ix = axis_index(x, gr.mn[0], gr.mx[0], gr.sz[0], gr.g[0]);
            const int iy = axis_index(y, gr.mn[1], gr.mx[1], gr.sz[1], gr.g[1]);
            const int iz = axis_index(z, gr.mn[2], gr.mx[2], gr.sz[2], gr.g[2]);
            if (ix >= 0 && iy >= 0 && iz >= 0) key = ((uint32_t)iz * (uint32_t)gr.g[1] + (uint32_t)iy) * (uint32_t)gr.g[0] + (uint32_t)ix;
        }
    }
    const bool in = key != kEmpty;  // the grid's product is below 2^32 - 1: no key is the empty marker
    uint32_t found = kEmpty;
    if (in) {
        uint32_t slot = mix(key) & mask;
        for (uint32_t probe = 0; probe <= mask; probe++) {  // distinct keys <= points <= half the slots: an empty slot ends every probe
            const uint32_t prev = atomicCAS(&t_key[slot], kEmpty, key);
            if (prev == kEmpty || prev == key) {
                atomicMin(&t_first[slot], i);
                found = slot;
                break;
            }
            slot = (slot + 1) & mask;
        }
    }
    if (i < n) pslot[i] = found;
    const unsigned long long bm = __ballot(in);
    if (bm && (threadIdx.x & 63) == (uint32_t)(__ffsll((long long)bm) - 1)) atomicAdd(&stats[0], (uint32_t)__popcll(bm));
}

// ---- heads -------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_head(const uint32_t* __restrict__ pslot, const uint32_t* __restrict__ t_first, uint32_t i, uint32_t n) {
    if (i >= n) return false;
    const uint32_t s = pslot[i];
    return s != kEmpty && t_first[s] == i;
}

__global__ __launch_bounds__(kThreads) void vx_heads_count(const uint32_t* __restrict__ pslot, const uint32_t* __restrict__ t_first, uint32_t n,
                                                           uint32_t* __restrict__ counts) {
    const uint32_t base = blockIdx.x * kTile;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) c += is_head(pslot, t_first, base + r * kThreads + threadIdx.x, n) ? 1u : 0u;
    compact_tile_count(c, counts);
}

// the head of voxel `id` writes the id beside the key and, below the cap, the index row (save_result_by_order, voxelization_kernel.cu:97-105),
// a zero count and P empty point slots
__global__ __launch_bounds__(kThreads) void vx_heads_write(const uint32_t* __restrict__ pslot, const uint32_t* __restrict__ t_first,
                                                           const uint32_t* __restrict__ t_key, uint32_t n, const uint32_t* __restrict__ offs,
                                                           uint32_t gx, uint32_t gy, int order, uint32_t max_voxels, uint32_t P,
                                                           uint32_t* __restrict__ t_id, int4* __restrict__ indices, uint32_t* __restrict__ vcount,
                                                           uint32_t* __restrict__ vslots) {
    const uint32_t base = blockIdx.x * kTile;
    bool keep[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) keep[r] = is_head(pslot, t_first, base + r * kThreads + threadIdx.x, n);
    compact_tile_write(keep, offs, [&](int r, uint32_t id) {
        const uint32_t s = pslot[base + r * kThreads + threadIdx.x];
        t_id[s] = id;
        if (id < max_voxels) {
            const uint32_t key = t_key[s];
            const int x = (int)(key % gx), y = (int)((key / gx) % gy), z = (int)(key / gx / gy);
            indices[id] = (order == LIO_VOXEL_ORDER_XYZ) ? make_int4(0, x, y, z) : make_int4(0, z, y, x);
            vcount[id] = 0;
            for (uint32_t k = 0; k < P; k++) vslots[(uint64_t)id * P + k] = kEmpty;
        }
    });
}

// ---- slots -------------------------------------------------------------------------------------------------------------------------------------
// Every index of a voxel is offered to slot 0; an atomicMin that lowers a slot hands the displaced index on to the next slot.  Indices are
// distinct and each is in one place (a slot or a lane's hand) at any time; the index a lane carries beyond slot s is larger than what slot s
// holds from then on.  So slot s ends as the minimum of everything not left in slots 0 .. s - 1: the P smallest in ascending order, in any
// arrival order.  An index larger than the last slot's value has P smaller ones before it and cannot stay: it leaves before any atomic.
__global__ __launch_bounds__(kThreads) void vx_slots(const uint32_t* __restrict__ pslot, const uint32_t* __restrict__ t_id, uint32_t n, uint32_t max_voxels,
                                                     uint32_t P, uint32_t* __restrict__ vcount, uint32_t* __restrict__ vslots) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = pslot[i];
    if (s == kEmpty) return;
    const uint32_t id = t_id[s];
    if (id >= max_voxels) return;
    atomicAdd(&vcount[id], 1u);
    uint32_t* sl = vslots + (uint64_t)id * P;
    if (__hip_atomic_load(&sl[P - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < i) return;
    uint32_t v = i;
    for (uint32_t k = 0; k < P && v != kEmpty; k++) {
        const uint32_t old = atomicMin(&sl[k], v);
        if (old > v) v = old;
    }
}

// ---- mean --------------------------------------------------------------------------------------------------------------------------------------
// reduce_mean_kernel of voxelization_kernel.cu:158-180: the count clamped to P, per channel slot 0's value plus the others in slot order, over
// (float)count, to f16 (round to nearest even, subnormals kept, overflow to inf).  stats[1] += the kept points, stats[2] = the real voxels
__global__ __launch_bounds__(kThreads) void vx_mean(const float* __restrict__ rows, uint32_t n, const uint32_t* __restrict__ d_real, uint32_t max_voxels, uint32_t P,
                                                    uint32_t* __restrict__ vcount, const uint32_t* __restrict__ vslots, uint16_t* __restrict__ features,
                                                    uint32_t* __restrict__ stats) {
    const uint32_t real = *d_real;
    const uint32_t nv = min(real, max_voxels);
    const uint32_t id = blockIdx.x * kThreads + threadIdx.x;
    uint32_t cnt = 0;
    if (id < nv) {
        cnt = min(vcount[id], P);
        vcount[id] = cnt;
        const uint32_t* sl = vslots + (uint64_t)id * P;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
        for (uint32_t k = 0; k < cnt; k++) {
            const float* r = rows + (uint64_t)min(sl[k], n - 1) * kFeat;  // (a slot below the count always holds a point; no read leaves the window)
            const float r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
            if (k == 0) {
                a0 = r0; a1 = r1; a2 = r2; a3 = r3; a4 = r4;
            } else {
                a0 += r0; a1 += r1; a2 += r2; a3 += r3; a4 += r4;
            }
        }
        const float d = (float)(int)cnt;
        uint16_t* f = features + (uint64_t)id * kFeat;
        f[0] = __builtin_bit_cast(uint16_t, (_Float16)(a0 / d));
        f[1] = __builtin_bit_cast(uint16_t, (_Float16)(a1 / d));
        f[2] = __builtin_bit_cast(uint16_t, (_Float16)(a2 / d));
        f[3] = __builtin_bit_cast(uint16_t, (_Float16)(a3 / d));
        f[4] = __builtin_bit_cast(uint16_t, (_Float16)(a4 / d));
    }
    uint32_t c = cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&stats[1], c);
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[2] = real;
}

}  // namespace voxelize
}  // namespace lio

using namespace lio;
using namespace lio::voxelize;

struct lio_voxelizer {
    int device;
    hipStream_t stream;
    hipEvent_t ev[6];  // begin, window moved and sweep stored, inserted, ranked, slots filled, means written
    lio_voxelizer_params p;
    Grid grid;
    uint64_t max_rows;   // max_points + max_frame_num: a call into a full window still stores one point (lio_hip.h)
    uint32_t table_cap;  // a power of two >= 2 * max_rows
    float* buf[2];       // the A/B window
    WindowBook win;      // its counts, total and current half (voxelize_host.h)
    uint32_t *t_key, *t_first, *t_id, *pslot, *aux, *vcount, *vslots, *d_stats;
    int4* indices;
    uint16_t* features;
    uint32_t* h_stats;  // pinned: points in range, points kept, real voxels
    uint64_t num_voxels, real_voxels, in_range, kept;
    double us[6];
};

namespace {

int64_t forward(const char* who, lio_voxelizer* v, const float* points, uint32_t n, const float motion[16], int realtime, bool on_device) {
    if (!v) return LIO_E_INVALID;
    if (n == 0 || !points) { set_error("%s: at least one point is required", who); return LIO_E_INVALID; }
    if (realtime && !motion) { set_error("%s: a realtime call needs the motion", who); return LIO_E_INVALID; }
    hipSetDevice(v->device);
    hipStream_t st = v->stream;
    n = std::min(n, v->p.max_points);  // LidarInference::forward, lidar_inference.cpp:81
    const int src = v->win.cur;
    uint64_t moved = 0;
    n = v->win.step(n, realtime != 0, &moved);
    if (v->win.total > v->max_rows) {  // cannot happen (the bound is max_points + max_frame_num - 1); nothing is written if it does
        set_error("%s: the window would hold %llu rows", who, (unsigned long long)v->win.total);
        lio_voxelizer_reset(v);
        return LIO_E_INVALID;
    }
    v->num_voxels = v->real_voxels = v->in_range = v->kept = 0;
    LIO_HIP_TRY(hipEventRecord(v->ev[0], st));
    float* rows = v->buf[v->win.cur];
    if (moved > 0) {
        Motion mo;
        memcpy(mo.m, motion, sizeof(mo.m));
        vx_window<<<dim3((uint32_t)((moved + kWinRows - 1) / kWinRows)), dim3(kWinRows), 0, st>>>(v->buf[src], rows + (uint64_t)n * kFeat, (uint32_t)moved, mo);
        LIO_HIP_TRY(hipGetLastError());
    }
    LIO_HIP_TRY(hipMemcpyAsync(rows, points, (size_t)n * kFeat * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    LIO_HIP_TRY(hipEventRecord(v->ev[1], st));

    const uint32_t m = (uint32_t)v->win.total;
    uint32_t cap = 64;
    while (cap < 2 * (uint64_t)m) cap <<= 1;  // <= table_cap: m <= max_rows
    LIO_HIP_TRY(hipMemsetAsync(v->t_key, 0xFF, (size_t)cap * sizeof(uint32_t), st));
    LIO_HIP_TRY(hipMemsetAsync(v->t_first, 0xFF, (size_t)cap * sizeof(uint32_t), st));
    LIO_HIP_TRY(hipMemsetAsync(v->d_stats, 0, 4 * sizeof(uint32_t), st));
    vx_insert<<<dim3(blocks_of(m)), dim3(kThreads), 0, st>>>(rows, m, v->grid, cap - 1, v->t_key, v->t_first, v->pslot, v->d_stats);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(v->ev[2], st));

    const uint32_t ntiles = tiles_of(m);
    vx_heads_count<<<dim3(ntiles), dim3(kThreads), 0, st>>>(v->pslot, v->t_first, m, v->aux);
    const uint32_t* d_real = compact_finish(st, v->aux, m);
    if (!d_real) return LIO_E_DEVICE;
    const uint32_t P = v->p.max_points_per_voxel;
    vx_heads_write<<<dim3(ntiles), dim3(kThreads), 0, st>>>(v->pslot, v->t_first, v->t_key, m, v->aux, (uint32_t)v->grid.g[0], (uint32_t)v->grid.g[1], v->p.order,
                                                             v->p.max_voxels, P, v->t_id, v->indices, v->vcount, v->vslots);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(v->ev[3], st));

    vx_slots<<<dim3(blocks_of(m)), dim3(kThreads), 0, st>>>(v->pslot, v->t_id, m, v->p.max_voxels, P, v->vcount, v->vslots);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(v->ev[4], st));

    const uint32_t most = std::min(v->p.max_voxels, m);
    vx_mean<<<dim3(blocks_of(most)), dim3(kThreads), 0, st>>>(rows, m, d_real, v->p.max_voxels, P, v->vcount, v->vslots, v->features, v->d_stats);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(v->ev[5], st));
    LIO_HIP_TRY(hipMemcpyAsync(v->h_stats, v->d_stats, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    v->in_range = v->h_stats[0];
    v->kept = v->h_stats[1];
    v->real_voxels = v->h_stats[2];
    v->num_voxels = std::min<uint64_t>(v->real_voxels, v->p.max_voxels);
    for (int k = 0; k < 5; k++) v->us[k] = elapsed_us(v->ev[k], v->ev[k + 1]);
    v->us[5] = elapsed_us(v->ev[0], v->ev[5]);
    return (int64_t)v->num_voxels;
}

}  // namespace

extern "C" {

int lio_voxelize_grid_size(const float min_range[3], const float max_range[3], const float voxel_size[3], int out[3]) {
    if (!min_range || !max_range || !voxel_size || !out) return LIO_E_INVALID;
    if (!grid_of(min_range, max_range, voxel_size, out)) {
        set_error("lio_voxelize_grid_size: finite ranges with max > min and a voxel size > 0 are required, and at most 2^31 - 1 voxels per axis");
        return LIO_E_INVALID;
    }
    return LIO_OK;
}

lio_voxelizer* lio_voxelizer_create(int device, const lio_voxelizer_params* p) {
    if (!p) { set_error("lio_voxelizer_create: params are required"); return nullptr; }
    int g[3];
    if (!grid_of(p->min_range, p->max_range, p->voxel_size, g)) {
        set_error("lio_voxelizer_create: finite ranges with max > min and a voxel size > 0 are required, and at most 2^31 - 1 voxels per axis");
        return nullptr;
    }
    if (!grid_fits_key(g)) {
        set_error("lio_voxelizer_create: the grid %d x %d x %d does not fit a 32-bit key", g[0], g[1], g[2]);
        return nullptr;
    }
    if (p->max_points_per_voxel < 1 || p->max_points_per_voxel > 32) {
        set_error("lio_voxelizer_create: max_points_per_voxel in [1, 32] is required (%u given)", p->max_points_per_voxel);
        return nullptr;
    }
    if (p->order != LIO_VOXEL_ORDER_XYZ && p->order != LIO_VOXEL_ORDER_ZYX) {
        set_error("lio_voxelizer_create: order %d is neither XYZ (1) nor ZYX (2)", p->order);
        return nullptr;
    }
    if (p->max_voxels < 1 || p->max_points < 1 || p->max_frame_num < 1 || p->max_points > (1u << 30) || p->max_frame_num > 4096 ||
        (uint64_t)p->max_voxels * p->max_points_per_voxel > 0xFFFFFFFFull) {
        set_error("lio_voxelizer_create: max_voxels >= 1, max_points in [1, 2^30] and max_frame_num in [1, 4096] are required");
        return nullptr;
    }
    lio_voxelizer* v = new lio_voxelizer();
    v->device = device;
    v->p = *p;
    for (int a = 0; a < 3; a++) {
        v->grid.mn[a] = p->min_range[a];
        v->grid.mx[a] = p->max_range[a];
        v->grid.sz[a] = p->voxel_size[a];
        v->grid.g[a] = g[a];
    }
    v->win.init(p->max_points, p->max_frame_num);
    if (!open_device("lio_voxelizer_create", device, &v->stream, v->ev, 6)) {
        delete v;
        return nullptr;
    }
    v->max_rows = v->win.max_rows();
    v->table_cap = 64;
    while (v->table_cap < 2 * v->max_rows) v->table_cap <<= 1;
    const uint64_t mv = std::min<uint64_t>(p->max_voxels, v->max_rows);  // no more voxels than points
    const bool ok = alloc(&v->buf[0], v->max_rows * kFeat) && alloc(&v->buf[1], v->max_rows * kFeat) && alloc(&v->t_key, v->table_cap) &&
                    alloc(&v->t_first, v->table_cap) && alloc(&v->t_id, v->table_cap) && alloc(&v->pslot, v->max_rows) &&
                    alloc(&v->aux, compact_words(v->max_rows)) && alloc(&v->vcount, mv) && alloc(&v->vslots, mv * p->max_points_per_voxel) &&
                    alloc(&v->indices, mv) && alloc(&v->features, mv * kFeat) && alloc(&v->d_stats, 4) &&
                    hipHostMalloc(&v->h_stats, 4 * sizeof(uint32_t)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        set_error("lio_voxelizer_create: buffers for %u points and %u voxels not available", p->max_points, p->max_voxels);
        lio_voxelizer_destroy(v);
        return nullptr;
    }
    return v;
}

void lio_voxelizer_destroy(lio_voxelizer* v) {
    if (!v) return;
    hipSetDevice(v->device);
    if (v->stream) hipStreamSynchronize(v->stream);
    void* all[] = {v->buf[0], v->buf[1], v->t_key, v->t_first, v->t_id, v->pslot, v->aux, v->vcount, v->vslots, v->indices, v->features, v->d_stats};
    for (void* q : all)
        if (q) (void)hipFree(q);
    if (v->h_stats) hipHostFree(v->h_stats);
    for (int i = 0; i < 6; i++)
        if (v->ev[i]) hipEventDestroy(v->ev[i]);
    if (v->stream) hipStreamDestroy(v->stream);
    delete v;
}

int lio_voxelizer_reset(lio_voxelizer* v) {
    if (!v) return LIO_E_INVALID;
    v->win.reset();
    v->num_voxels = v->real_voxels = v->in_range = v->kept = 0;
    return LIO_OK;
}

int64_t lio_voxelizer_forward(lio_voxelizer* v, const float* points, uint32_t n, const float motion[16], int realtime) {
    return forward("lio_voxelizer_forward", v, points, n, motion, realtime, false);
}

int64_t lio_voxelizer_forward_device(lio_voxelizer* v, const float* d_points, uint32_t n, const float motion[16], int realtime) {
    return forward("lio_voxelizer_forward_device", v, d_points, n, motion, realtime, true);
}

int64_t lio_voxelizer_output(lio_voxelizer* v, uint16_t* features, int32_t* indices, uint32_t* counts, uint64_t cap) {
    if (!v) return LIO_E_INVALID;
    const uint64_t nv = v->num_voxels;
    if (nv > cap) return -(int64_t)nv;
    if (nv == 0) return 0;
    hipSetDevice(v->device);
    hipStream_t st = v->stream;
    if (features) LIO_HIP_TRY(hipMemcpyAsync(features, v->features, nv * kFeat * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    if (indices) LIO_HIP_TRY(hipMemcpyAsync(indices, v->indices, nv * sizeof(int4), hipMemcpyDeviceToHost, st));
    if (counts) LIO_HIP_TRY(hipMemcpyAsync(counts, v->vcount, nv * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    return (int64_t)nv;
}

int64_t lio_voxelizer_output_device(lio_voxelizer* v, const void** d_features, const int32_t** d_indices) {
    if (!v) return LIO_E_INVALID;
    if (d_features) *d_features = v->features;
    if (d_indices) *d_indices = reinterpret_cast<const int32_t*>(v->indices);
    return (int64_t)v->num_voxels;
}

int64_t lio_voxelizer_window(lio_voxelizer* v, float* rows, uint64_t cap) {
    if (!v) return LIO_E_INVALID;
    if (v->win.total > cap) return -(int64_t)v->win.total;
    if (v->win.total == 0) return 0;
    if (!rows) return LIO_E_INVALID;
    hipSetDevice(v->device);
    LIO_HIP_TRY(hipMemcpyAsync(rows, v->buf[v->win.cur], v->win.total * kFeat * sizeof(float), hipMemcpyDeviceToHost, v->stream));
    LIO_HIP_TRY(hipStreamSynchronize(v->stream));
    return (int64_t)v->win.total;
}

int64_t lio_voxelizer_window_counts(lio_voxelizer* v, int32_t* per_frame, uint32_t cap) {
    if (!v) return LIO_E_INVALID;
    const uint32_t f = (uint32_t)v->win.counts.size();
    if (f > cap) return -(int64_t)f;
    if (!per_frame) return LIO_E_INVALID;
    memcpy(per_frame, v->win.counts.data(), f * sizeof(int32_t));
    return (int64_t)f;
}

int64_t lio_voxelizer_window_device(lio_voxelizer* v, const float** d_rows) {
    if (!v) return LIO_E_INVALID;
    if (d_rows) *d_rows = v->buf[v->win.cur];
    return (int64_t)v->win.total;
}

int lio_voxelizer_last_counts(lio_voxelizer* v, uint64_t* real_voxels, uint64_t* points_in_range, uint64_t* points_kept) {
    if (!v) return LIO_E_INVALID;
    if (real_voxels) *real_voxels = v->real_voxels;
    if (points_in_range) *points_in_range = v->in_range;
    if (points_kept) *points_kept = v->kept;
    return LIO_OK;
}

int lio_voxelizer_last_times(lio_voxelizer* v, double* window_us, double* insert_us, double* rank_us, double* slots_us, double* mean_us, double* total_us) {
    if (!v) return LIO_E_INVALID;
    double* out[6] = {window_us, insert_us, rank_us, slots_us, mean_us, total_us};
    for (int k = 0; k < 6; k++)
        if (out[k]) *out[k] = v->us[k];
    return LIO_OK;
}

}  // extern "C"
