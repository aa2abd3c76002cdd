// keyframe.hip -- the mapping mode's key-frame producer on gfx950 (wave64): HdlGraphSlamNodelet::cloud_callback
// (slam/backend/hdl_graph_slam/apps/hdl_graph_slam_nodelet.cpp:163-246) with KeyframeUpdater (include/hdl_graph_slam/keyframe_updater.hpp:42-75)
// and InformationMatrixCalculator::calc_fitness_score (src/hdl_graph_slam/information_matrix_calculator.cpp:110-138), followed by the two
// filters SLAM::runMappingThread puts an elected frame through (slam/src/slam.cpp:105-108, 400-411; slam/common/slam_utils.cpp:236-241).
//
//   decide    prev^-1 * pose in f64 on the host; dx, da stored as f32 (is_update's float&), compared against D / 2, 3 D / 2 in f64
//   candidate the scan's undistortion (delta or pose list) and VoxelGrid: lio_scan_*, on the handle's one stream
//   fitness   one lane per downsampled point: the f32 transform of pcl::transformPointCloud(.., Matrix4f), walk<1> over the local map's
//             tree, gate d2 <= range; f64 sum and count per workgroup of 256 in a fixed order, the workgroups' records added in order on the host
//   ring      the local map: a device buffer of cap + one frame; append = transform (f64, the Matrix4d overload) behind the last point, drop
//             from the front = a device copy into the second buffer, then knn_index_dev.h's tree straight from it
//   radius    pcl::RadiusOutlierRemoval: finite rows compacted (device_prims.h) into a tree, one lane per leaf point in Morton order walks
//             it bounded by r^2 (walk_radius) and leaves at min_neighbours + 1; the keep flag goes to the point's input index
//   emit      flag && the range predicate -> a stable compaction in input order; three counts come back in one read, then the cloud
//
// The candidate and the best cloud are two buffers that swap by pointer.  Scratch grows geometrically and is kept.
#include <cfloat>
#include <cmath>
#include <deque>
#include <vector>

#include "device_prims.h"
#include "knn_index_dev.h"

namespace lio {
namespace keyframe {

using namespace prims;

struct Xf32 { float R[9], t[3]; };   // relpose.cast<float>()
struct Xf64 { double R[9], t[3]; };  // Isometry3d::matrix()

// finite rows per tile
__global__ __launch_bounds__(kThreads) void kf_finite_count(const float4* __restrict__ p, uint32_t n, uint32_t* __restrict__ counts) {
    const uint32_t base = blockIdx.x * kTile;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        if (i < n) {
            const float4 q = p[i];
            c += finite3(q.x, q.y, q.z) ? 1u : 0u;
        }
    }
    compact_tile_count(c, counts);
}

// the finite rows as the index takes them, in input order: {x, y, z, input index bits}
__global__ __launch_bounds__(kThreads) void kf_finite_write(const float4* __restrict__ p, uint32_t n, const uint32_t* __restrict__ offs, float4* __restrict__ out) {
    const uint32_t base = blockIdx.x * kTile;
    bool keep[kItems];
    float4 q[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        q[r] = p[i < n ? i : 0u];
        keep[r] = i < n && finite3(q[r].x, q[r].y, q[r].z);
    }
    compact_tile_write(keep, offs, [&](int r, uint32_t o) {
        out[o] = make_float4(q[r].x, q[r].y, q[r].z, __uint_as_float(base + r * kThreads + threadIdx.x));
    });
}

// one lane per leaf point (Morton order: the lanes of a wave share their path): kept iff `need` points, itself included, lie within r2
__global__ __launch_bounds__(kThreads) void kf_radius_flags(const float4* __restrict__ leaves, const uint32_t* __restrict__ d_n, const float4* __restrict__ nodes,
                                                            uint32_t P, int L, float r2, uint32_t need, uint8_t* __restrict__ flags, uint32_t* __restrict__ n_kept) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t nf = *d_n;
    bool keep = false;
    if (j < nf) {
        const float4 q = leaves[j];
        keep = knn_index::walk_radius(q.x, q.y, q.z, nodes, leaves, nf, P, L, r2, need) >= need;
        flags[__float_as_uint(q.w)] = keep ? 1 : 0;
    }
    const unsigned long long m = __ballot(keep);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(n_kept, (uint32_t)__popcll(m));  // (an integer count: the order of the waves does not matter)
}

// pointsDistanceFilter(cloud, out, 0, range): the f32 |x|, |y| compared with the doubles, strictly; range <= 0: no range filter
__device__ __forceinline__ bool in_range(const float4 q, double range) {
    if (!(range > 0.0)) return true;
    const double ax = (double)fabsf(q.x), ay = (double)fabsf(q.y);
    return ax > 0.0 && ax < range && ay > 0.0 && ay < range;
}

__global__ __launch_bounds__(kThreads) void kf_keep_count(const float4* __restrict__ p, const uint8_t* __restrict__ flags, uint32_t n, double range,
                                                          uint32_t* __restrict__ counts) {
    const uint32_t base = blockIdx.x * kTile;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        if (i < n && flags[i]) c += in_range(p[i], range) ? 1u : 0u;
    }
    compact_tile_count(c, counts);
}

__global__ __launch_bounds__(kThreads) void kf_keep_write(const float4* __restrict__ p, const uint8_t* __restrict__ flags, uint32_t n, double range,
                                                          const uint32_t* __restrict__ offs, float4* __restrict__ pout, uint32_t* __restrict__ iout) {
    const uint32_t base = blockIdx.x * kTile;
    bool keep[kItems];
    float4 q[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        q[r] = p[i < n ? i : 0u];
        keep[r] = i < n && flags[i] != 0 && in_range(q[r], range);
    }
    compact_tile_write(keep, offs, [&](int r, uint32_t o) {
        pout[o] = q[r];
        iout[o] = base + r * kThreads + threadIdx.x;
    });
}

// calc_fitness_score: record b = {sum of the gated squared distances, their number} of points [256 b, 256 b + 256)
__global__ __launch_bounds__(kThreads) void kf_fitness(const float4* __restrict__ src, uint32_t n, Xf32 X, const float4* __restrict__ leaves,
                                                       const float4* __restrict__ nodes, uint32_t nf, uint32_t P, int L, float max_range,
                                                       double* __restrict__ partial) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    double my_sum = 0.0;
    uint32_t my_cnt = 0;
    if (i < n) {
        const float4 p = src[i];
        // pcl::transformPointCloud with a Matrix4f: accumulated left to right (the rule of lio_ndt_overlap_score)
        const float tx = ((X.R[0] * p.x + X.R[1] * p.y) + X.R[2] * p.z) + X.t[0];
        const float ty = ((X.R[3] * p.x + X.R[4] * p.y) + X.R[5] * p.z) + X.t[1];
        const float tz = ((X.R[6] * p.x + X.R[7] * p.y) + X.R[8] * p.z) + X.t[2];
        if (finite3(tx, ty, tz)) {
            float kd[1] = {INFINITY};
            uint32_t ki[1] = {knn_index::kNone};
            knn_index::walk<1>(tx, ty, tz, nodes, leaves, nf, P, L, kd, ki);
            if (ki[0] != knn_index::kNone && kd[0] <= max_range) { my_sum = (double)kd[0]; my_cnt = 1; }
        }
    }
    __shared__ double ssum[kWaves];
    __shared__ uint32_t scnt[kWaves];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { my_sum += __shfl_xor(my_sum, off); my_cnt += __shfl_xor(my_cnt, off); }
    if ((threadIdx.x & 63) == 0) { ssum[threadIdx.x >> 6] = my_sum; scnt[threadIdx.x >> 6] = my_cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
        partial[2 * blockIdx.x + 1] = (double)((scnt[0] + scnt[1]) + (scnt[2] + scnt[3]));
    }
}

// pcl::transformPointCloud(in, out, Matrix4d): per point in f64, terms left to right, cast to f32; the intensity rides along
__global__ __launch_bounds__(kThreads) void kf_append(const float4* __restrict__ src, uint32_t n, Xf64 X, float4* __restrict__ dst) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = src[i];
    const double x = p.x, y = p.y, z = p.z;
    dst[i] = make_float4((float)(((X.R[0] * x + X.R[1] * y) + X.R[2] * z) + X.t[0]), (float)(((X.R[3] * x + X.R[4] * y) + X.R[5] * z) + X.t[1]),
                         (float)(((X.R[6] * x + X.R[7] * y) + X.R[8] * z) + X.t[2]), p.w);
}

// the local map as the index takes it: {x, y, z, position bits}
__global__ __launch_bounds__(kThreads) void kf_expand(const float4* __restrict__ p, uint32_t n, float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 q = p[i];
    out[i] = make_float4(q.x, q.y, q.z, __uint_as_float(i));
}

// ---- KeyframeUpdater on the host (f64) ----
void rel_pose(const double a[16], const double b[16], double R[9], double t[3]) {  // a^-1 * b of two rigid transforms
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[3 * i + j] = (a[i] * b[j] + a[4 + i] * b[4 + j]) + a[8 + i] * b[8 + j];
        t[i] = (a[i] * (b[3] - a[3]) + a[4 + i] * (b[7] - a[7])) + a[8 + i] * (b[11] - a[11]);
    }
}

// Eigen::AngleAxisd(R).angle(): through the quaternion (Shepperd's branches), 2 atan2(|vec|, |w|)
double rotation_angle(const double m[9]) {
    double q[4];  // x y z w
    double t = m[0] + (m[4] + m[8]);
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
    const double n = std::sqrt(q[0] * q[0] + (q[1] * q[1] + q[2] * q[2]));
    return n != 0.0 ? 2.0 * std::atan2(n, std::fabs(q[3])) : 0.0;
}

void decide(const double prev[16], const double pose[16], double D, double A, int* need, int* must, double* dx, double* da, double* dx64) {
    double R[9], t[3];
    rel_pose(prev, pose, R, t);
    const double d = std::sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    const double a = rotation_angle(R) / M_PI * 180.0;
    const float fx = (float)d, fa = (float)a;  // is_update(.., float& dx, float& da)
    const bool nd = !((double)fx < D / 2.0 && (double)fa < A / 2.0);
    const bool ms = nd && ((double)fx >= D * 3.0 / 2.0 || (double)fa >= A * 3.0 / 2.0);
    if (need) *need = nd ? 1 : 0;
    if (must) *must = ms ? 1 : 0;
    if (dx) *dx = (double)fx;
    if (da) *da = (double)fa;
    if (dx64) *dx64 = d;
}

bool finite16(const double* T) {
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(T[i])) return false;
    return true;
}

struct Emitted {
    std::vector<float> xyzi;
    double pose[16];
    uint64_t stamp;
    double accum_distance;
    uint32_t n_before, n_after_radius;
};

}  // namespace keyframe
}  // namespace lio

using namespace lio;
using namespace lio::keyframe;

struct lio_keyframer {
    int device;
    lio_keyframer_params par;
    lio_scan* scan;      // upload, undistortion, VoxelGrid; its stream is the handle's one stream
    hipStream_t stream;
    hipEvent_t ev[6];    // begin, candidate ready, fitness done, filters done, ring + rebuild done, (spare)
    // clouds
    uint64_t cloud_cap;  // points the candidate / best / filter buffers hold
    float4 *cand, *best, *stage, *kpts, *fout;
    uint32_t* fidx;
    uint8_t* flags;
    uint32_t* aux;       // two compactions' scratch
    uint64_t region;
    uint32_t* d_nrad;    // points the radius filter keeps
    uint32_t* h_words;   // pinned: finite rows, after the radius filter, after both
    knn_index::DeviceIndex* fi;  // the tree of the cloud being filtered
    // local map
    uint64_t lm_cap_alloc;
    float4 *lm, *lm_alt, *lm_k;
    uint32_t lm_n;
    knn_index::DeviceIndex* li;
    double* d_partial;
    double* h_partial;   // pinned
    uint64_t partial_cap;
    // KeyframeUpdater + the selector's state
    bool first;
    double prev[16], accum_distance;
    double best_score, best_inlier, average_score;
    int map_keyframe_count, map_keyframe_step;
    uint32_t best_n;
    double best_pose[16];
    uint64_t best_stamp;
    bool have_best;
    std::deque<Emitted>* fifo;
    // the last filter call and the last push
    uint32_t f_nf, f_nrad, f_nout;
    double t_candidate, t_fitness, t_filters, t_ring;
};

namespace {

void free_clouds(lio_keyframer* k) {
    void* all[] = {k->cand, k->best, k->stage, k->kpts, k->fout, k->fidx, k->flags, k->aux};
    for (void* p : all)
        if (p) (void)hipFree(p);
    k->cand = k->best = k->stage = k->kpts = k->fout = nullptr;
    k->fidx = k->aux = nullptr;
    k->flags = nullptr;
    k->cloud_cap = 0;
}

// room for clouds of n points in the candidate / best / filter buffers; the best cloud survives a growth
int reserve_clouds(lio_keyframer* k, uint64_t n) {
    if (n <= k->cloud_cap) return LIO_OK;
    if (n > 0x7FFFFFFFull) { set_error("lio_keyframer: %llu points exceed the int index range (2^31 - 1)", (unsigned long long)n); return LIO_E_CAPACITY; }
    const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(n, std::max<uint64_t>(2 * k->cloud_cap, 1ull << 16)), 0x7FFFFFFFull);
    LIO_HIP_TRY(hipStreamSynchronize(k->stream));
    float4* old_best = k->best;
    k->best = nullptr;
    free_clouds(k);
    k->region = compact_words(want);
    const bool ok = alloc(&k->cand, want) && alloc(&k->best, want) && alloc(&k->stage, want) && alloc(&k->kpts, want) && alloc(&k->fout, want) &&
                    alloc(&k->fidx, want) && alloc(&k->flags, want) && alloc(&k->aux, 2 * k->region);
    if (ok && old_best && k->have_best && k->best_n)
        (void)hipMemcpy(k->best, old_best, (uint64_t)k->best_n * sizeof(float4), hipMemcpyDeviceToDevice);
    if (old_best) (void)hipFree(old_best);
    if (!ok) {
        (void)hipGetLastError();
        free_clouds(k);
        k->have_best = false;
        set_error("lio_keyframer: device buffers for clouds of %llu points not available", (unsigned long long)want);
        return LIO_E_DEVICE;
    }
    k->cloud_cap = want;
    return LIO_OK;
}

// room for the ring (cap + one frame of n points) and the fitness records of a frame of n points
int reserve_ring(lio_keyframer* k, uint64_t n) {
    const uint64_t need = (uint64_t)k->par.local_map_cap + n;
    if (need > k->lm_cap_alloc) {
        const uint64_t want = std::max<uint64_t>(need, (uint64_t)k->par.local_map_cap + 2 * (k->lm_cap_alloc > k->par.local_map_cap ? k->lm_cap_alloc - k->par.local_map_cap : 0));
        LIO_HIP_TRY(hipStreamSynchronize(k->stream));
        float4 *a = nullptr, *b = nullptr, *c = nullptr;
        if (!(alloc(&a, want) && alloc(&b, want) && alloc(&c, want))) {
            (void)hipGetLastError();
            if (a) (void)hipFree(a);
            if (b) (void)hipFree(b);
            if (c) (void)hipFree(c);
            set_error("lio_keyframer: a local map of %llu points does not fit the device", (unsigned long long)want);
            return LIO_E_DEVICE;
        }
        if (k->lm && k->lm_n) (void)hipMemcpy(a, k->lm, (uint64_t)k->lm_n * sizeof(float4), hipMemcpyDeviceToDevice);
        if (k->lm) (void)hipFree(k->lm);
        if (k->lm_alt) (void)hipFree(k->lm_alt);
        if (k->lm_k) (void)hipFree(k->lm_k);
        k->lm = a; k->lm_alt = b; k->lm_k = c;
        k->lm_cap_alloc = want;
    }
    const uint64_t blocks = blocks_of(n) + 1;
    if (blocks > k->partial_cap) {
        LIO_HIP_TRY(hipStreamSynchronize(k->stream));
        if (k->d_partial) (void)hipFree(k->d_partial);
        if (k->h_partial) (void)hipHostFree(k->h_partial);
        k->d_partial = k->h_partial = nullptr;
        k->partial_cap = 0;
        const uint64_t want = std::max<uint64_t>(blocks, 1024);
        if (!alloc(&k->d_partial, 2 * want) || hipHostMalloc(reinterpret_cast<void**>(&k->h_partial), 2 * want * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("lio_keyframer: the fitness records do not fit");
            return LIO_E_DEVICE;
        }
        k->partial_cap = want;
    }
    return LIO_OK;
}

Xf64 xf64(const double T[16]) {
    Xf64 x;
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) x.R[3 * i + j] = T[4 * i + j]; x.t[i] = T[4 * i + 3]; }
    return x;
}
Xf32 xf32(const double T[16]) {
    Xf32 x;
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) x.R[3 * i + j] = (float)T[4 * i + j]; x.t[i] = (float)T[4 * i + 3]; }
    return x;
}

// src (n points, device) transformed by T behind the ring's last point; the front dropped down to the cap; the tree rebuilt
int ring_append(lio_keyframer* k, const float4* src, uint32_t n, const double T[16]) {
    hipStream_t st = k->stream;
    if (n) kf_append<<<dim3(blocks_of(n)), dim3(kThreads), 0, st>>>(src, n, xf64(T), k->lm + k->lm_n);
    uint32_t total = k->lm_n + n;
    if (total > k->par.local_map_cap) {
        const uint32_t drop = total - k->par.local_map_cap;
        total -= drop;
        if (total) LIO_HIP_TRY(hipMemcpyAsync(k->lm_alt, k->lm + drop, (uint64_t)total * sizeof(float4), hipMemcpyDeviceToDevice, st));
        std::swap(k->lm, k->lm_alt);
    }
    k->lm_n = total;
    if (total == 0) return LIO_OK;
    int rc = knn_index::device_index_reserve(*k->li, (uint64_t)k->par.local_map_cap);
    if (rc != LIO_OK) return rc;
    kf_expand<<<dim3(blocks_of(total)), dim3(kThreads), 0, st>>>(k->lm, total, k->lm_k);
    LIO_HIP_TRY(hipGetLastError());
    return knn_index::device_index_build(st, *k->li, k->lm_k, nullptr, total);
}

// calc_fitness_score of n device points against the local map
int fitness(lio_keyframer* k, const float4* src, uint32_t n, const double T[16], double* score, uint32_t* nr) {
    *score = DBL_MAX;
    *nr = 0;
    if (n == 0 || k->lm_n == 0) return LIO_OK;
    hipStream_t st = k->stream;
    const uint32_t blocks = blocks_of(n);
    kf_fitness<<<dim3(blocks), dim3(kThreads), 0, st>>>(src, n, xf32(T), k->li->leaves, k->li->nodes, k->lm_n, k->li->P, k->li->L, (float)k->par.fitness_range,
                                                       k->d_partial);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipMemcpyAsync(k->h_partial, k->d_partial, 2ull * blocks * sizeof(double), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipEventRecord(k->ev[2], st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    double sum = 0.0, cnt = 0.0;
    for (uint32_t b = 0; b < blocks; b++) { sum += k->h_partial[2 * b]; cnt += k->h_partial[2 * b + 1]; }
    if (cnt > 0) *score = sum / cnt;
    *nr = (uint32_t)cnt;
    return LIO_OK;
}

// the radius filter and (range > 0) the range filter over n device points at `in`: the survivors in input order in k->fout / k->fidx,
// the counts in k->f_*
int run_filters(lio_keyframer* k, const float4* in, uint32_t n, double radius, int min_neighbours, double range) {
    k->f_nf = k->f_nrad = k->f_nout = 0;
    if (n == 0) return LIO_OK;
    hipStream_t st = k->stream;
    int rc = knn_index::device_index_reserve(*k->fi, n);
    if (rc != LIO_OK) return rc;
    const uint32_t ntiles = tiles_of(n);
    const float r2 = (float)(radius * radius);
    uint32_t *c0 = k->aux, *c1 = k->aux + k->region;
    LIO_HIP_TRY(hipMemsetAsync(k->flags, 0, n, st));
    LIO_HIP_TRY(hipMemsetAsync(k->d_nrad, 0, sizeof(uint32_t), st));
    kf_finite_count<<<dim3(ntiles), dim3(kThreads), 0, st>>>(in, n, c0);
    const uint32_t* d_nf = compact_finish(st, c0, n);
    if (!d_nf) return LIO_E_DEVICE;
    kf_finite_write<<<dim3(ntiles), dim3(kThreads), 0, st>>>(in, n, c0, k->kpts);
    LIO_HIP_TRY(hipGetLastError());
    rc = knn_index::device_index_build(st, *k->fi, k->kpts, d_nf, n);
    if (rc != LIO_OK) return rc;
    kf_radius_flags<<<dim3(blocks_of(n)), dim3(kThreads), 0, st>>>(k->fi->leaves, d_nf, k->fi->nodes, k->fi->P, k->fi->L, r2, (uint32_t)min_neighbours + 1u, k->flags,
                                                                  k->d_nrad);
    kf_keep_count<<<dim3(ntiles), dim3(kThreads), 0, st>>>(in, k->flags, n, range, c1);
    const uint32_t* d_nout = compact_finish(st, c1, n);
    if (!d_nout) return LIO_E_DEVICE;
    kf_keep_write<<<dim3(ntiles), dim3(kThreads), 0, st>>>(in, k->flags, n, range, c1, k->fout, k->fidx);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipMemcpyAsync(k->h_words, d_nf, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipMemcpyAsync(k->h_words + 1, k->d_nrad, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipMemcpyAsync(k->h_words + 2, d_nout, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    k->f_nf = k->h_words[0];
    k->f_nrad = k->h_words[1];
    k->f_nout = k->h_words[2];
    return LIO_OK;
}

void reset_state(lio_keyframer* k) {
    k->first = true;
    k->accum_distance = 0.0;
    k->best_score = DBL_MAX;
    k->best_inlier = 0.0;
    k->average_score = 0.0;
    k->map_keyframe_count = 0;
    k->map_keyframe_step = std::max(1, (int)std::round(k->par.local_map_distance / k->par.key_frame_distance));
    k->best_n = 0;
    k->have_best = false;
    k->lm_n = 0;
    k->fifo->clear();
    k->t_candidate = k->t_fitness = k->t_filters = k->t_ring = 0;
}

bool params_ok(const lio_keyframer_params* p) {
    if (!p) return false;
    if (!(p->key_frame_distance > 0) || !(p->key_frame_degree > 0) || !(p->resolution > 0) || !(p->radius > 0) || p->min_neighbours < 0 ||
        p->min_neighbours > 1000000 || p->local_map_cap < 1 || p->local_map_cap > 0x3FFFFFFFu || !(p->local_map_distance > 0) || !(p->fitness_range > 0) ||
        !(p->scan_period > 0)) {
        set_error("lio_keyframer: distance, degree, resolution, scan_period, radius, local_map_distance and fitness_range must be positive, "
                  "min_neighbours >= 0, 1 <= local_map_cap < 2^30");
        return false;
    }
    return true;
}

// a scan that takes clouds of n points
int reserve_scan(lio_keyframer* k, uint64_t n) {
    if (k->scan && n <= k->scan->max_raw) return LIO_OK;
    if (n > 0x7FFFFFFFull) { set_error("lio_keyframer: %llu points exceed the int index range (2^31 - 1)", (unsigned long long)n); return LIO_E_CAPACITY; }
    const uint32_t want = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(n, std::max<uint64_t>(2ull * (k->scan ? k->scan->max_raw : 0), 1ull << 17)), 0x7FFFFFFFull);
    if (k->scan) lio_scan_destroy(k->scan);
    k->scan = lio_scan_create(k->device, want, want);
    k->stream = k->scan ? k->scan->stream : nullptr;
    return k->scan ? LIO_OK : LIO_E_DEVICE;
}

}  // namespace

extern "C" {

int lio_keyframe_decide(const double prev[16], const double pose[16], double dist_threshold, double degree_threshold, int* need, int* must, double* dx,
                        double* da) {
    if (!prev || !pose || !finite16(prev) || !finite16(pose)) return LIO_E_INVALID;
    decide(prev, pose, dist_threshold, degree_threshold, need, must, dx, da, nullptr);
    return LIO_OK;
}

void lio_keyframer_default_params(lio_keyframer_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->key_frame_distance = 1.0;
    p->key_frame_degree = 10.0;
    p->resolution = 0.2;
    p->key_frame_range = 50.0;
    p->scan_period = 0.1;          // SLAM::setParams, slam.cpp:103
    p->radius = 1.0;               // slam.cpp:106
    p->min_neighbours = 3;         // slam.cpp:107
    p->local_map_cap = 100000;     // ODOMETRY_LOCAL_MAP_NUM
    p->local_map_distance = 2.0;   // ODOMETRY_LOCAL_MAP_DIST
    p->fitness_range = 1.0;        // hdl_graph_slam_nodelet.cpp:202
}

lio_keyframer* lio_keyframer_create(int device, const lio_keyframer_params* params) {
    lio_keyframer_params def;
    lio_keyframer_default_params(&def);
    if (!params) params = &def;
    if (!params_ok(params)) return nullptr;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) {
        (void)hipGetLastError();
        set_error("lio_keyframer_create: no HIP device %d (there is no CPU fallback)", device);
        return nullptr;
    }
    lio_keyframer* k = new lio_keyframer();
    memset(k, 0, sizeof(*k));
    k->device = device;
    k->par = *params;
    k->fifo = new std::deque<Emitted>();
    k->fi = new knn_index::DeviceIndex();
    k->li = new knn_index::DeviceIndex();
    bool ok = reserve_scan(k, 1) == LIO_OK;
    for (int i = 0; ok && i < 6; i++) ok = hipEventCreate(&k->ev[i]) == hipSuccess;
    ok = ok && alloc(&k->d_nrad, 1) && hipHostMalloc(reinterpret_cast<void**>(&k->h_words), 64) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (!lio_last_error()[0]) set_error("lio_keyframer_create: stream / event / staging allocation failed");
        lio_keyframer_destroy(k);
        return nullptr;
    }
    reset_state(k);
    return k;
}

void lio_keyframer_destroy(lio_keyframer* k) {
    if (!k) return;
    hipSetDevice(k->device);
    if (k->stream) hipStreamSynchronize(k->stream);
    free_clouds(k);
    void* all[] = {k->lm, k->lm_alt, k->lm_k, k->d_partial, k->d_nrad};
    for (void* p : all)
        if (p) (void)hipFree(p);
    if (k->h_partial) hipHostFree(k->h_partial);
    if (k->h_words) hipHostFree(k->h_words);
    knn_index::device_index_free(*k->fi);
    knn_index::device_index_free(*k->li);
    for (int i = 0; i < 6; i++)
        if (k->ev[i]) hipEventDestroy(k->ev[i]);
    if (k->scan) lio_scan_destroy(k->scan);
    delete k->fi;
    delete k->li;
    delete k->fifo;
    delete k;
}

int lio_keyframer_reset(lio_keyframer* k) {
    if (!k) return LIO_E_INVALID;
    hipSetDevice(k->device);
    LIO_HIP_TRY(hipStreamSynchronize(k->stream));
    reset_state(k);
    return LIO_OK;
}

int lio_keyframer_push_host(lio_keyframer* k, const float* xyzi, const uint32_t* stamp_us, uint32_t n, uint64_t header_stamp_us, const double odom[16],
                            const double delta[16], const uint64_t* pose_stamp_us, const double* poses, uint32_t n_poses, lio_keyframe_report* rep) {
    if (!k || !odom || (n && (!xyzi || !stamp_us)) || (n_poses && (!pose_stamp_us || !poses)) || (!n_poses && !delta)) return LIO_E_INVALID;
    if (!finite16(odom)) { set_error("lio_keyframer_push_host: the odometry pose is not finite"); return LIO_E_INVALID; }
    lio_keyframe_report r;
    memset(&r, 0, sizeof(r));
    r.score = DBL_MAX;
    r.accum_distance = k->accum_distance;
    r.average_score = k->average_score;
    r.local_map_size = k->lm_n;
    k->t_candidate = k->t_fitness = k->t_filters = k->t_ring = 0;
    if (rep) *rep = r;
    if (n == 0) return LIO_OK;  // frame.points->cloud->empty(), :165-167
    hipSetDevice(k->device);
    const float leaf = (float)k->par.resolution;
    int rc;
    if (k->first) {  // :169-176
        r.first = 1;
        rc = reserve_scan(k, n);
        if (rc == LIO_OK) rc = lio_scan_upload(k->scan, xyzi, n);
        uint32_t nds = 0;
        if (rc == LIO_OK) rc = lio_scan_voxel_downsample(k->scan, leaf, 1, &nds);
        if (rc == LIO_OK) rc = reserve_ring(k, nds);
        if (rc != LIO_OK) return rc;
        LIO_HIP_TRY(hipEventRecord(k->ev[3], k->stream));
        k->lm_n = 0;
        rc = ring_append(k, k->scan->ds_body, nds, odom);
        if (rc != LIO_OK) return rc;
        LIO_HIP_TRY(hipEventRecord(k->ev[4], k->stream));
        LIO_HIP_TRY(hipStreamSynchronize(k->stream));
        k->t_ring = elapsed_us(k->ev[3], k->ev[4]);
        k->first = false;  // keyframe_updater->update(odom)
        memcpy(k->prev, odom, sizeof(k->prev));
        r.n_downsampled = nds;
        r.local_map_size = k->lm_n;
        if (rep) *rep = r;
        return LIO_OK;
    }
    int need = 0, must = 0;
    double dx64 = 0;
    decide(k->prev, odom, k->par.key_frame_distance, k->par.key_frame_degree, &need, &must, &r.dx, &r.da, &dx64);
    r.need = need;
    r.must = must;
    if (rep) *rep = r;
    if (!need) return LIO_OK;  // :181-183
    // undistortion and VoxelGrid, :185-194
    rc = reserve_scan(k, n);
    if (rc != LIO_OK) return rc;
    hipStream_t st = k->stream;
    LIO_HIP_TRY(hipEventRecord(k->ev[0], st));
    rc = lio_scan_upload(k->scan, xyzi, n);
    if (rc != LIO_OK) return rc;
    if (n_poses == 0) {
        float D[16];
        for (int i = 0; i < 16; i++) D[i] = (float)delta[i];  // (frame.points->T).cast<float>()
        rc = lio_scan_undistort_delta(k->scan, stamp_us, 0, D, k->par.scan_period);
    } else {
        rc = lio_scan_undistort_poses(k->scan, stamp_us, 0, header_stamp_us, pose_stamp_us, poses, n_poses);
    }
    uint32_t nds = 0;
    if (rc == LIO_OK) rc = lio_scan_voxel_downsample(k->scan, leaf, 1, &nds);
    if (rc == LIO_OK) rc = reserve_clouds(k, nds);
    if (rc == LIO_OK) rc = reserve_ring(k, nds);
    if (rc != LIO_OK) return rc;
    if (nds) LIO_HIP_TRY(hipMemcpyAsync(k->cand, k->scan->ds_body, (uint64_t)nds * sizeof(float4), hipMemcpyDeviceToDevice, st));
    LIO_HIP_TRY(hipEventRecord(k->ev[1], st));
    r.n_downsampled = nds;
    // the fitness score and the election, :200-209
    LIO_HIP_TRY(hipEventRecord(k->ev[2], st));
    rc = fitness(k, k->cand, nds, odom, &r.score, &r.nr);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipStreamSynchronize(st));
    k->t_candidate = elapsed_us(k->ev[0], k->ev[1]);
    k->t_fitness = elapsed_us(k->ev[1], k->ev[2]);
    const float inlier = (float)r.nr / (float)nds;  // float(nr) / size(): NaN for an empty cloud, which then never wins
    if ((r.score * 0.8 + (1.0 - (double)inlier) * 0.2) <= (k->best_score * 0.8 + (1.0 - k->best_inlier) * 0.2)) {
        k->best_score = r.score;
        k->best_inlier = (double)inlier;
        std::swap(k->cand, k->best);
        k->best_n = nds;
        memcpy(k->best_pose, odom, sizeof(k->best_pose));
        k->best_stamp = header_stamp_us;
        k->have_best = true;
        r.elected = 1;
    }
    if (must) {  // :211-243
        k->accum_distance += dx64;  // keyframe_updater->update(odom)
        memcpy(k->prev, odom, sizeof(k->prev));
        if (k->have_best) {
            // the two filters of SLAM::runMappingThread on the elected cloud
            LIO_HIP_TRY(hipEventRecord(k->ev[2], st));
            rc = run_filters(k, k->best, k->best_n, k->par.radius, k->par.min_neighbours, k->par.key_frame_range);
            if (rc != LIO_OK) return rc;
            Emitted e;
            e.xyzi.resize(4ull * k->f_nout);
            if (k->f_nout) LIO_HIP_TRY(hipMemcpyAsync(e.xyzi.data(), k->fout, (uint64_t)k->f_nout * sizeof(float4), hipMemcpyDeviceToHost, st));
            LIO_HIP_TRY(hipEventRecord(k->ev[3], st));
            memcpy(e.pose, k->best_pose, sizeof(e.pose));
            e.stamp = k->best_stamp;
            e.accum_distance = k->accum_distance;
            e.n_before = k->best_n;
            e.n_after_radius = k->f_nrad;
            k->map_keyframe_count += 1;
            k->average_score = (k->average_score * (k->map_keyframe_count - 1) + k->best_score) / k->map_keyframe_count;
            k->best_score = DBL_MAX;  // (best_inlier_ratio keeps its value, :224)
            if ((k->map_keyframe_count % k->map_keyframe_step) == 0) {
                rc = ring_append(k, k->best, k->best_n, k->best_pose);
                if (rc != LIO_OK) return rc;
            }
            LIO_HIP_TRY(hipEventRecord(k->ev[4], st));
            LIO_HIP_TRY(hipStreamSynchronize(st));
            k->t_filters = elapsed_us(k->ev[2], k->ev[3]);
            k->t_ring = elapsed_us(k->ev[3], k->ev[4]);
            k->fifo->push_back(std::move(e));
            r.emitted = 1;
        }
    }
    r.accum_distance = k->accum_distance;
    r.average_score = k->average_score;
    r.local_map_size = k->lm_n;
    if (rep) *rep = r;
    return LIO_OK;
}

int lio_keyframer_pending(lio_keyframer* k) { return k ? (int)k->fifo->size() : LIO_E_INVALID; }

int64_t lio_keyframer_pop(lio_keyframer* k, float* xyzi, uint64_t cap, double pose[16], uint64_t* stamp_us, double* accum_distance, uint32_t* n_before_filters,
                          uint32_t* n_after_radius) {
    if (!k) return LIO_E_INVALID;
    if (k->fifo->empty()) { set_error("lio_keyframer_pop: no key frame is pending"); return LIO_E_STATE; }
    const Emitted& e = k->fifo->front();
    const uint64_t n = e.xyzi.size() / 4;
    if (!xyzi || n > cap) return -(int64_t)n;  // a size query: the frame stays queued
    if (n) memcpy(xyzi, e.xyzi.data(), n * 4 * sizeof(float));
    if (pose) memcpy(pose, e.pose, sizeof(e.pose));
    if (stamp_us) *stamp_us = e.stamp;
    if (accum_distance) *accum_distance = e.accum_distance;
    if (n_before_filters) *n_before_filters = e.n_before;
    if (n_after_radius) *n_after_radius = e.n_after_radius;
    k->fifo->pop_front();
    return (int64_t)n;
}

int64_t lio_keyframe_filter_host(lio_keyframer* k, const float* xyzi, uint64_t n, double radius, int min_neighbours, double range, uint32_t* keep_idx, uint64_t cap,
                                 uint32_t* n_after_radius, uint32_t* n_dropped_nonfinite) {
    if (!k || (!xyzi && n) || !(radius > 0) || min_neighbours < 0 || min_neighbours > 1000000) return LIO_E_INVALID;
    hipSetDevice(k->device);
    int rc = reserve_clouds(k, n);
    if (rc != LIO_OK) return rc;
    if (n) LIO_HIP_TRY(hipMemcpyAsync(k->stage, xyzi, n * sizeof(float4), hipMemcpyHostToDevice, k->stream));
    LIO_HIP_TRY(hipEventRecord(k->ev[2], k->stream));
    rc = run_filters(k, k->stage, (uint32_t)n, radius, min_neighbours, range);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipEventRecord(k->ev[3], k->stream));
    LIO_HIP_TRY(hipStreamSynchronize(k->stream));
    k->t_filters = elapsed_us(k->ev[2], k->ev[3]);
    if (n_after_radius) *n_after_radius = k->f_nrad;
    if (n_dropped_nonfinite) *n_dropped_nonfinite = (uint32_t)n - k->f_nf;
    return download("lio_keyframe_filter_host", k->device, k->stream, k->fidx, k->f_nout, keep_idx, cap);
}

int64_t lio_radius_outlier_host(lio_keyframer* k, const float* xyzi, uint64_t n, double radius, int min_neighbours, uint32_t* keep_idx, uint64_t cap,
                                uint32_t* n_dropped_nonfinite) {
    return lio_keyframe_filter_host(k, xyzi, n, radius, min_neighbours, 0.0, keep_idx, cap, nullptr, n_dropped_nonfinite);
}

int lio_keyframer_fitness_host(lio_keyframer* k, const float* xyzi, uint32_t n, const double T[16], double* score, uint32_t* nr) {
    if (!k || (!xyzi && n) || !T || !score || !nr) return LIO_E_INVALID;
    hipSetDevice(k->device);
    int rc = reserve_clouds(k, n);
    if (rc == LIO_OK) rc = reserve_ring(k, n);
    if (rc != LIO_OK) return rc;
    if (n) LIO_HIP_TRY(hipMemcpyAsync(k->stage, xyzi, (uint64_t)n * sizeof(float4), hipMemcpyHostToDevice, k->stream));
    LIO_HIP_TRY(hipEventRecord(k->ev[1], k->stream));
    LIO_HIP_TRY(hipEventRecord(k->ev[2], k->stream));
    rc = fitness(k, k->stage, n, T, score, nr);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipStreamSynchronize(k->stream));
    k->t_fitness = elapsed_us(k->ev[1], k->ev[2]);
    return LIO_OK;
}

int lio_keyframer_append_local_map_host(lio_keyframer* k, const float* xyzi, uint32_t n, const double T[16]) {
    if (!k || (!xyzi && n) || !T || !finite16(T)) return LIO_E_INVALID;
    hipSetDevice(k->device);
    int rc = reserve_clouds(k, n);
    if (rc == LIO_OK) rc = reserve_ring(k, n);
    if (rc != LIO_OK) return rc;
    if (n) LIO_HIP_TRY(hipMemcpyAsync(k->stage, xyzi, (uint64_t)n * sizeof(float4), hipMemcpyHostToDevice, k->stream));
    LIO_HIP_TRY(hipEventRecord(k->ev[3], k->stream));
    rc = ring_append(k, k->stage, n, T);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipEventRecord(k->ev[4], k->stream));
    LIO_HIP_TRY(hipStreamSynchronize(k->stream));
    k->t_ring = elapsed_us(k->ev[3], k->ev[4]);
    return (int)k->lm_n;
}

int64_t lio_keyframer_download_local_map(lio_keyframer* k, float* xyzi, uint64_t cap) {
    if (!k) return LIO_E_INVALID;
    return download("lio_keyframer_download_local_map", k->device, k->stream, (const float4*)k->lm, (uint64_t)k->lm_n, reinterpret_cast<float4*>(xyzi), cap);
}

int lio_keyframer_last_times(lio_keyframer* k, double* candidate_us, double* fitness_us, double* filters_us, double* ring_us) {
    if (!k) return LIO_E_INVALID;
    if (candidate_us) *candidate_us = k->t_candidate;
    if (fitness_us) *fitness_us = k->t_fitness;
    if (filters_us) *filters_us = k->t_filters;
    if (ring_us) *ring_us = k->t_ring;
    return LIO_OK;
}

}  // extern "C"
