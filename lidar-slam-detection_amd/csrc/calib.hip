// calib.hip -- the lidar-INS calibration on gfx950 (wave64): the cost of one candidate extrinsic (sensor_driver/calibration/lidar_ins/src/
// aligner.cpp:15-80 over sensor.cpp:88-120) as a fixed chain on one stream, and Aligner::lidarOdomTransform (aligner.cpp:82-190) around it.
//
//   resident    the kept raw points of all scans, scan-major in input order (getCombinedPointcloud's order), {x, y, z, scan bits}
//   poses       host, f32 (calib_host.cpp): M_s = matrix(T_o0_ot_s * T_o_l) per scan, through a pinned staging buffer
//   ci_assemble one lane per point: {x', y', z', combined index bits}, x' = ((m00 x + m01 y) + m02 z) + m03 in separately rounded f32 -- the
//               project's statement of pcl::transformPoint (sensor.cpp:96), which cannot be pinned without PCL
//   index       knn_index_dev.h's device_index_build over the combined cloud
//   ci_terms<K> one lane per leaf point (the leaves are in Morton order: a self-query needs no query sort), K = k + 1 because the cloud is
//               searched against itself (aligner.cpp:47-51).  The cap goes into the walk: kd[] starts at the cap instead of +inf.  walk<K>
//               prunes a box only when its bound is strictly greater than kd[K - 1], and a neighbour at d2 >= cap contributes exactly the cap
//               to min(d2, cap) whether or not it is found -- the terms are unchanged, and an isolated point stops climbing at once.  The cap
//               is compared with the SQUARED distance, as the reference does (aligner.cpp:25-28).  Each lane adds its K terms in ascending
//               order in f64; a wave is reduced by xor shuffles (32, 16, .. 1), the four waves through LDS as (w0 + w1) + (w2 + w3): one
//               record per workgroup, no float atomics.
//   ci_fold     one workgroup: thread t adds records t, t + 256, .. in index order, then the same fixed tree.  The sum is a function of the
//               cloud and the launch shape, not of timing.
//
// No host synchronisation inside the chain; the 8-byte result is read at its end.  DEVIATION from the reference: it adds the terms in f32 per
// batch of 1000 points and then over batches; the f64 sum differs from that by the f32 sum's own rounding.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <limits>
#include <mutex>
#include <vector>

#include "calib_host.h"
#include "device_prims.h"
#include "knn_index_dev.h"

namespace lio {
namespace calib {

using namespace prims;

__global__ __launch_bounds__(kThreads) void ci_assemble(const float4* __restrict__ raw, uint32_t n, const float* __restrict__ mats, float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = raw[i];
    const float* m = mats + 12ull * __float_as_uint(p.w);
    float4 o;
    o.x = ((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3];
    o.y = ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7];
    o.z = ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11];
    o.w = __uint_as_float(i);
    out[i] = o;
}

// the fixed tree of a workgroup of kThreads: xor shuffles inside a wave, then (w0 + w1) + (w2 + w3); valid in thread 0
__device__ __forceinline__ double block_sum(double v) {
    __shared__ double ws[kWaves];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    return (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

template <int K>
__global__ __launch_bounds__(kThreads) void ci_terms(const float4* __restrict__ leaves, uint32_t n, const float4* __restrict__ nodes, uint32_t P, int L,
                                                     float cap, float start, float* __restrict__ terms, double* __restrict__ parts) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    double s = 0.0;
    if (j < n) {
        const float4 q = leaves[j];
        float kd[K];
        uint32_t ki[K];
#pragma unroll
        for (int t = 0; t < K; t++) { kd[t] = start; ki[t] = knn_index::kNone; }
        knn_index::walk<K>(q.x, q.y, q.z, nodes, leaves, n, P, L, kd, ki);
        const uint64_t row = (uint64_t)__float_as_uint(q.w) * K;
#pragma unroll
        for (int t = 0; t < K; t++) {
            const float e = fminf(kd[t], cap);
            if (terms) terms[row + t] = e;
            s += (double)e;
        }
    }
    const double b = block_sum(s);
    if (threadIdx.x == 0) parts[blockIdx.x] = b;
}

__global__ __launch_bounds__(kThreads) void ci_fold(const double* __restrict__ parts, uint32_t n_parts, double* __restrict__ out) {
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < n_parts; i += kThreads) s += parts[i];
    const double b = block_sum(s);
    if (threadIdx.x == 0) *out = b;
}

}  // namespace calib
}  // namespace lio

using namespace lio;
using namespace lio::calib;

struct lio_calib_ins {
    int device;
    hipStream_t stream;
    hipEvent_t ev[4];  // the chain's begin, after assemble, after the build, after the fold
    // the scans
    std::vector<float4> raw;         // host copy of the resident points
    std::vector<uint32_t> scan_off;  // S + 1
    std::vector<int64_t> scan_stamp;
    std::vector<Se3f> scan_pose;     // T_o0_ot per scan (identity until set)
    float4* d_raw;
    float4* d_pts;
    uint64_t cap_pts;
    float* d_mats;
    float* h_mats;     // pinned, LIO_CALIB_MAX_SCANS x 12
    double* d_parts;
    uint64_t cap_parts;
    double* d_sum;
    double* h_sum;     // pinned
    float* d_terms;
    uint64_t cap_terms;
    knn_index::DeviceIndex index;
    // the odometry track
    std::vector<int64_t> odom_stamp;
    std::vector<Se3f> odom_T;
    Se3f cur, best;
    std::mutex mu;  // best, against lio_calib_ins_result from another thread
    std::atomic<int32_t> evals;
    std::atomic<double> best_err;
    std::atomic<int32_t> finished;
    double assemble_us, build_us, terms_us;
};

namespace {

constexpr double kErrorStart = 1e8;  // Aligner::error_ (aligner.cpp:6)

void default_params(lio_calib_params* p) {
    p->local_only = 0;
    p->time_cal = 1;
    p->max_time_offset = 0.2;
    p->max_evals = 500;
    p->knn_batch_size = 1000;
    p->xtol = 0.0001;
    p->local_knn_k = 1;
    p->global_knn_k = 3;
    p->local_knn_max_dist = 1.0f;
    p->global_knn_max_dist = 10.0f;
    p->direct_epsilon = 1e-4;
    const double step[7] = {0.25, 0.25, 0.25, 0.05, 0.05, 0.05, 0.02};
    for (int i = 0; i < 7; i++) p->nm_step[i] = step[i];
}

bool params_ok(const lio_calib_params* p) {
    return p->max_evals >= 1 && p->xtol >= 0.0 && p->local_knn_k >= 1 && p->local_knn_k <= 7 && p->global_knn_k >= 1 && p->global_knn_k <= 7 &&
           p->local_knn_max_dist >= 0.f && p->global_knn_max_dist >= 0.f && p->max_time_offset >= 0.0 && std::isfinite(p->max_time_offset) &&
           p->direct_epsilon >= 0.0;
}

// Lidar::setOdomOdomTransforms (sensor.cpp:122-127, 72-86)
int set_scan_poses(lio_calib_ins* h, double time_offset) {
    if (h->odom_stamp.size() < 2) {
        set_error("lio_calib_ins: %zu odometry entries, the interpolation needs two", h->odom_stamp.size());
        return LIO_E_STATE;
    }
    if (!std::isfinite(time_offset) || std::fabs(time_offset) > 9e12) return LIO_E_INVALID;
    uint32_t idx = 0;
    for (size_t s = 0; s < h->scan_stamp.size(); s++) {
        const int64_t ts = h->scan_stamp[s] + static_cast<int64_t>(1000000.0 * time_offset);
        h->scan_pose[s] = interpolate(h->odom_stamp.data(), h->odom_T.data(), (uint32_t)h->odom_stamp.size(), ts, idx, &idx);
    }
    return LIO_OK;
}

// M_s = matrix(T_o0_ot_s * T_o_l) into out (S x 16)
int scan_matrices(lio_calib_ins* h, float* out) {
    for (size_t s = 0; s < h->scan_pose.size(); s++) {
        float* M = out + 16 * s;
        se3_matrix(se3_mul(h->scan_pose[s], h->cur), M);
        for (int i = 0; i < 12; i++)
            if (!std::isfinite(M[i])) {
                set_error("lio_calib_ins: the pose of scan %zu is not finite (two odometry entries with one stamp?)", s);
                return LIO_E_INVALID;
            }
    }
    return LIO_OK;
}

int set_x(lio_calib_ins* h, const double* x, int nx) {
    if (!x || (nx != 6 && nx != 7)) return LIO_E_INVALID;
    for (int i = 0; i < nx; i++)
        if (!std::isfinite(x[i])) return LIO_E_INVALID;
    if (nx == 7) {
        const int rc = set_scan_poses(h, x[6]);
        if (rc != LIO_OK) return rc;
    }
    float v[6];
    for (int i = 0; i < 6; i++) v[i] = (float)x[i];
    h->cur = se3_exp(v);
    return LIO_OK;
}

int reserve_points(lio_calib_ins* h, uint64_t n) {
    if (n <= h->cap_pts) return LIO_OK;
    const uint64_t want = std::max<uint64_t>(n, std::max<uint64_t>(2 * h->cap_pts, 1ull << 17));
    LIO_HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->d_raw) (void)hipFree(h->d_raw);
    if (h->d_pts) (void)hipFree(h->d_pts);
    h->d_raw = h->d_pts = nullptr;
    h->cap_pts = 0;
    if (!alloc(&h->d_raw, want) || !alloc(&h->d_pts, want)) {
        (void)hipGetLastError();
        set_error("lio_calib_ins: device memory for %llu points not available", (unsigned long long)want);
        return LIO_E_DEVICE;
    }
    h->cap_pts = want;
    const uint64_t have = h->raw.size();  // what was resident goes back
    if (have) LIO_HIP_TRY(hipMemcpyAsync(h->d_raw, h->raw.data(), have * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    LIO_HIP_TRY(hipStreamSynchronize(h->stream));
    return LIO_OK;
}

template <int K>
void launch_terms(lio_calib_ins* h, uint32_t n, float cap, float start, float* terms) {
    ci_terms<K><<<dim3(blocks_of(n)), dim3(kThreads), 0, h->stream>>>(h->index.leaves, n, h->index.nodes, h->index.P, h->index.L, cap, start, terms,
                                                                     h->d_parts);
}

// the chain at the current transform and scan poses; terms: device n x K or NULL
int run_chain(lio_calib_ins* h, int k, float cap, bool uncapped, float* terms, double* err) {
    const int K = k + 1;
    const uint64_t n64 = h->raw.size();
    if (n64 < (uint64_t)K) {
        set_error("lio_calib_ins: %llu points in the combined cloud, the metric needs %d", (unsigned long long)n64, K);
        return LIO_E_STATE;
    }
    const uint32_t n = (uint32_t)n64, S = (uint32_t)h->scan_pose.size();
    float M[16 * LIO_CALIB_MAX_SCANS];
    int rc = scan_matrices(h, M);
    if (rc != LIO_OK) return rc;
    for (uint32_t s = 0; s < S; s++) memcpy(h->h_mats + 12 * s, M + 16 * s, 12 * sizeof(float));
    rc = knn_index::device_index_reserve(h->index, n);
    if (rc != LIO_OK) return rc;
    rc = grow("lio_calib_ins", &h->d_parts, &h->cap_parts, (uint64_t)blocks_of(n), h->stream);
    if (rc != LIO_OK) return rc;
    hipStream_t st = h->stream;
    LIO_HIP_TRY(hipMemcpyAsync(h->d_mats, h->h_mats, 12ull * S * sizeof(float), hipMemcpyHostToDevice, st));
    LIO_HIP_TRY(hipEventRecord(h->ev[0], st));
    ci_assemble<<<dim3(blocks_of(n)), dim3(kThreads), 0, st>>>(h->d_raw, n, h->d_mats, h->d_pts);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(h->ev[1], st));
    rc = knn_index::device_index_build(st, h->index, h->d_pts, nullptr, n);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipEventRecord(h->ev[2], st));
    const float start = uncapped ? INFINITY : cap;
    switch (K) {
        case 2: launch_terms<2>(h, n, cap, start, terms); break;
        case 3: launch_terms<3>(h, n, cap, start, terms); break;
        case 4: launch_terms<4>(h, n, cap, start, terms); break;
        case 5: launch_terms<5>(h, n, cap, start, terms); break;
        case 6: launch_terms<6>(h, n, cap, start, terms); break;
        case 7: launch_terms<7>(h, n, cap, start, terms); break;
        case 8: launch_terms<8>(h, n, cap, start, terms); break;
        default: return LIO_E_INVALID;
    }
    ci_fold<<<dim3(1), dim3(kThreads), 0, st>>>(h->d_parts, blocks_of(n), h->d_sum);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(h->ev[3], st));
    LIO_HIP_TRY(hipMemcpyAsync(h->h_sum, h->d_sum, sizeof(double), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    h->assemble_us = elapsed_us(h->ev[0], h->ev[1]);
    h->build_us = elapsed_us(h->ev[1], h->ev[2]);
    h->terms_us = elapsed_us(h->ev[2], h->ev[3]);
    *err = *h->h_sum;
    return LIO_OK;
}

bool metric_of(int metric, const lio_calib_params& p, int* k, float* cap, bool* uncapped) {
    *uncapped = (metric & LIO_CALIB_UNCAPPED) != 0;
    const int m = metric & ~LIO_CALIB_UNCAPPED;
    if (m != LIO_CALIB_GLOBAL && m != LIO_CALIB_LOCAL) return false;
    *k = m == LIO_CALIB_LOCAL ? p.local_knn_k : p.global_knn_k;
    *cap = m == LIO_CALIB_LOCAL ? p.local_knn_max_dist : p.global_knn_max_dist;
    return true;
}

// Aligner::lidarOdomTransform's state while it runs
struct Run {
    lio_calib_ins* h;
    lio_calib_params p;
    bool local;
    double error;  // Aligner::error_
    int rc;
};

// Aligner::LidarOdomMinimizer (aligner.cpp:82-107)
double minimizer(const double* x, int n, void* user) {
    Run* r = static_cast<Run*>(user);
    lio_calib_ins* h = r->h;
    double err = std::numeric_limits<double>::infinity();
    int rc = set_x(h, x, n);
    if (rc == LIO_OK) rc = run_chain(h, r->local ? r->p.local_knn_k : r->p.global_knn_k, r->local ? r->p.local_knn_max_dist : r->p.global_knn_max_dist, false, nullptr, &err);
    if (rc != LIO_OK) {
        r->rc = rc;
        return std::numeric_limits<double>::infinity();
    }
    if (r->error > err) {
        r->error = err;
        std::lock_guard<std::mutex> g(h->mu);
        h->best = h->cur;
        h->best_err.store(err);
    }
    h->evals.fetch_add(1);
    return err;
}

int stop_on_error(int, const double*, int, double, void* user) { return static_cast<Run*>(user)->rc != LIO_OK; }

// Aligner::optimize (aligner.cpp:109-135)
void optimize(Run* r, const std::vector<double>& lb, const std::vector<double>& ub, std::vector<double>* x) {
    const int n = (int)x->size();
    lio_dfo_params dp;
    lio_dfo_default_params(&dp);
    dp.max_evals = r->p.max_evals;
    dp.xtol_abs = r->p.xtol;
    dp.epsilon = r->p.direct_epsilon;
    for (int i = 0; i < n && i < 7; i++) dp.step[i] = r->p.nm_step[i];
    std::vector<double> out(*x);
    if (r->local) lio_dfo_nelder_mead(minimizer, r, n, x->data(), lb.data(), ub.data(), &dp, stop_on_error, r, out.data(), nullptr);
    else lio_dfo_direct_l(minimizer, r, n, lb.data(), ub.data(), &dp, stop_on_error, r, out.data(), nullptr);
    if (r->rc != LIO_OK) return;
    *x = out;
    minimizer(x->data(), n, r);  // the reference's evaluation at the optimiser's result (:130)
    float bx[6];
    {
        std::lock_guard<std::mutex> g(r->h->mu);
        se3_log(r->h->best, bx);
    }
    for (int i = 0; i < 6; i++) (*x)[i] = bx[i];
}

}  // namespace

extern "C" {

void lio_calib_default_params(lio_calib_params* p) {
    if (p) default_params(p);
}

lio_calib_ins* lio_calib_ins_create(int device) {
    lio_calib_ins* h = new lio_calib_ins();
    h->device = device;
    h->stream = nullptr;
    for (auto& e : h->ev) e = nullptr;
    h->d_raw = h->d_pts = nullptr;
    h->cap_pts = h->cap_parts = h->cap_terms = 0;
    h->d_mats = h->h_mats = h->d_terms = nullptr;
    h->d_parts = h->d_sum = h->h_sum = nullptr;
    h->cur = h->best = se3_identity();
    h->evals = 0;
    h->best_err = kErrorStart;
    h->finished = 0;
    h->assemble_us = h->build_us = h->terms_us = 0;
    h->scan_off.push_back(0);
    if (!open_device("lio_calib_ins_create", device, &h->stream, h->ev, 4)) {
        delete h;
        return nullptr;
    }
    const bool ok = alloc(&h->d_mats, 12 * LIO_CALIB_MAX_SCANS) && alloc(&h->d_sum, 1) &&
                    hipHostMalloc(&h->h_mats, 12 * LIO_CALIB_MAX_SCANS * sizeof(float)) == hipSuccess && hipHostMalloc(&h->h_sum, 64) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        set_error("lio_calib_ins_create: staging allocation failed");
        lio_calib_ins_destroy(h);
        return nullptr;
    }
    return h;
}

void lio_calib_ins_destroy(lio_calib_ins* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    void* dev[] = {h->d_raw, h->d_pts, h->d_mats, h->d_parts, h->d_sum, h->d_terms};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    knn_index::device_index_free(h->index);
    if (h->h_mats) hipHostFree(h->h_mats);
    if (h->h_sum) hipHostFree(h->h_sum);
    for (auto& e : h->ev)
        if (e) hipEventDestroy(e);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

int lio_calib_ins_reset(lio_calib_ins* h, const float init[16]) {
    if (!h || !init) return LIO_E_INVALID;
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(init[i])) return LIO_E_INVALID;
    h->raw.clear();
    h->scan_off.assign(1, 0);
    h->scan_stamp.clear();
    h->scan_pose.clear();
    h->odom_stamp.clear();
    h->odom_T.clear();
    {
        std::lock_guard<std::mutex> g(h->mu);
        h->cur = h->best = se3_from_matrix(init);
    }
    h->evals = 0;
    h->best_err = kErrorStart;
    h->finished = 0;
    return LIO_OK;
}

int lio_calib_ins_add_scan(lio_calib_ins* h, const float* xyz, uint64_t n, uint32_t stride, int64_t stamp_us) {
    if (!h || (n && !xyz) || stride < 3) return LIO_E_INVALID;
    if (h->scan_stamp.size() >= LIO_CALIB_MAX_SCANS) {
        set_error("lio_calib_ins_add_scan: %d scans held already", LIO_CALIB_MAX_SCANS);
        return LIO_E_CAPACITY;
    }
    if (n > 0x7FFFFFFFull) return LIO_E_CAPACITY;
    std::vector<uint8_t> keep(n);
    const int drawn = lio_calib_subsample(n, stamp_us, keep.data());
    if (drawn < 0) return drawn;
    const uint32_t scan = (uint32_t)h->scan_stamp.size();
    const size_t before = h->raw.size();
    for (uint64_t i = 0; i < n; i++) {
        if (!keep[i]) continue;
        const float* p = xyz + i * stride;
        if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
        float4 q;
        q.x = p[0]; q.y = p[1]; q.z = p[2];
        memcpy(&q.w, &scan, sizeof(float));
        h->raw.push_back(q);
    }
    const size_t kept = h->raw.size() - before;
    hipSetDevice(h->device);
    const size_t total = h->raw.size();
    int rc = LIO_OK;
    if (total > h->cap_pts) {
        rc = reserve_points(h, total);  // uploads everything held, the new scan included
    } else if (kept) {
        if (hipMemcpyAsync(h->d_raw + before, h->raw.data() + before, kept * sizeof(float4), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess) {
            set_error("lio_calib_ins_add_scan: upload failed");
            rc = LIO_E_DEVICE;
        }
    }
    if (rc != LIO_OK) {
        h->raw.resize(before);
        return rc;
    }
    h->scan_off.push_back((uint32_t)total);
    h->scan_stamp.push_back(stamp_us);
    h->scan_pose.push_back(se3_identity());
    return (int)kept;
}

int lio_calib_ins_add_odom(lio_calib_ins* h, const float T[16], int64_t stamp_us) {
    if (!h || !T) return LIO_E_INVALID;
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(T[i])) return LIO_E_INVALID;
    h->odom_stamp.push_back(stamp_us);
    h->odom_T.push_back(se3_from_matrix(T));
    return LIO_OK;
}

int lio_calib_ins_counts(lio_calib_ins* h, uint32_t* n_scans, uint32_t* n_odoms, uint64_t* n_points) {
    if (!h) return LIO_E_INVALID;
    if (n_scans) *n_scans = (uint32_t)h->scan_stamp.size();
    if (n_odoms) *n_odoms = (uint32_t)h->odom_stamp.size();
    if (n_points) *n_points = h->raw.size();
    return LIO_OK;
}

int lio_calib_ins_set_transform(lio_calib_ins* h, const double x[6]) {
    if (!h) return LIO_E_INVALID;
    return set_x(h, x, 6);
}

int lio_calib_ins_scan_matrices(lio_calib_ins* h, double time_offset, float* out) {
    if (!h || (!out && !h->scan_pose.empty())) return LIO_E_INVALID;
    const int rc = set_scan_poses(h, time_offset);
    if (rc != LIO_OK) return rc;
    return scan_matrices(h, out);
}

int64_t lio_calib_ins_combined(lio_calib_ins* h, const double* x, int nx, float* xyz_out, uint64_t cap) {
    if (!h) return LIO_E_INVALID;
    int rc = set_x(h, x, nx);
    if (rc != LIO_OK) return rc;
    const uint64_t n = h->raw.size();
    if (n > cap) return -(int64_t)n;
    if (n == 0) return 0;
    if (!xyz_out) return LIO_E_INVALID;
    float M[16 * LIO_CALIB_MAX_SCANS];
    rc = scan_matrices(h, M);
    if (rc != LIO_OK) return rc;
    const uint32_t S = (uint32_t)h->scan_pose.size();
    for (uint32_t s = 0; s < S; s++) memcpy(h->h_mats + 12 * s, M + 16 * s, 12 * sizeof(float));
    hipSetDevice(h->device);
    hipStream_t st = h->stream;
    LIO_HIP_TRY(hipMemcpyAsync(h->d_mats, h->h_mats, 12ull * S * sizeof(float), hipMemcpyHostToDevice, st));
    ci_assemble<<<dim3(blocks_of(n)), dim3(kThreads), 0, st>>>(h->d_raw, (uint32_t)n, h->d_mats, h->d_pts);
    LIO_HIP_TRY(hipGetLastError());
    std::vector<float4> tmp(n);
    LIO_HIP_TRY(hipMemcpyAsync(tmp.data(), h->d_pts, n * sizeof(float4), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    for (uint64_t i = 0; i < n; i++) {
        xyz_out[3 * i] = tmp[i].x;
        xyz_out[3 * i + 1] = tmp[i].y;
        xyz_out[3 * i + 2] = tmp[i].z;
    }
    return (int64_t)n;
}

int lio_calib_ins_error(lio_calib_ins* h, const double* x, int nx, int metric, double* err) {
    if (!h || !err) return LIO_E_INVALID;
    lio_calib_params p;
    default_params(&p);
    int k;
    float cap;
    bool uncapped;
    if (!metric_of(metric, p, &k, &cap, &uncapped)) return LIO_E_INVALID;
    const int rc = set_x(h, x, nx);
    if (rc != LIO_OK) return rc;
    hipSetDevice(h->device);
    return run_chain(h, k, cap, uncapped, nullptr, err);
}

int64_t lio_calib_ins_error_terms(lio_calib_ins* h, const double* x, int nx, int metric, float* terms, uint64_t cap_rows) {
    if (!h) return LIO_E_INVALID;
    lio_calib_params p;
    default_params(&p);
    int k;
    float cap;
    bool uncapped;
    if (!metric_of(metric, p, &k, &cap, &uncapped)) return LIO_E_INVALID;
    int rc = set_x(h, x, nx);
    if (rc != LIO_OK) return rc;
    const uint64_t n = h->raw.size(), K = (uint64_t)k + 1;
    if (n < K) {
        set_error("lio_calib_ins_error_terms: %llu points in the combined cloud, the metric needs %llu", (unsigned long long)n, (unsigned long long)K);
        return LIO_E_STATE;
    }
    if (n > cap_rows) return -(int64_t)n;
    if (!terms) return LIO_E_INVALID;
    hipSetDevice(h->device);
    rc = grow("lio_calib_ins_error_terms", &h->d_terms, &h->cap_terms, n * K, h->stream);
    if (rc != LIO_OK) return rc;
    double err = 0.0;
    rc = run_chain(h, k, cap, uncapped, h->d_terms, &err);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipMemcpyAsync(terms, h->d_terms, n * K * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    LIO_HIP_TRY(hipStreamSynchronize(h->stream));
    return (int64_t)n;
}

static int calibrate(lio_calib_ins* h, const lio_calib_params* params) {
    Run r;
    r.h = h;
    if (params) r.p = *params;
    else default_params(&r.p);
    if (!params_ok(&r.p)) return LIO_E_INVALID;
    r.local = r.p.local_only != 0;
    r.error = kErrorStart;
    r.rc = LIO_OK;
    if (hipSetDevice(h->device) != hipSuccess) {
        set_error("lio_calib_ins_calibrate: hipSetDevice(%d) failed", h->device);
        return LIO_E_DEVICE;
    }
    h->evals = 0;
    h->finished = 0;
    const size_t num_params = r.p.time_cal ? 7 : 6;
    std::vector<double> x(num_params, 0.0);
    if (!r.local) {
        std::vector<double> lb = {-100.0, -100.0, -10.0, -M_PI, -M_PI, -M_PI};
        std::vector<double> ub = {100.0, 100.0, 10.0, M_PI, M_PI, M_PI};
        {  // error_ = the global cost of the transform the lidar holds (aligner.cpp:157-158)
            double e0 = 0.0;
            const int rc = run_chain(h, r.p.global_knn_k, r.p.global_knn_max_dist, false, nullptr, &e0);
            if (rc != LIO_OK) return rc;
            r.error = e0;
            h->best_err.store(e0);
        }
        float ix[6];
        {
            std::lock_guard<std::mutex> g(h->mu);
            se3_log(h->best, ix);
        }
        std::vector<double> gx(6);
        for (int i = 0; i < 6; i++) gx[i] = ix[i];
        optimize(&r, lb, ub, &gx);
        if (r.rc != LIO_OK) return r.rc;
        r.local = true;
        for (int i = 0; i < 6; i++) x[i] = gx[i];
    }
    std::vector<double> lb = {-10.0, -10.0, -1.0, -1.0, -1.0, -1.0};
    std::vector<double> ub = {10.0, 10.0, 1.0, 1.0, 1.0, 1.0};
    for (size_t i = 0; i < 6; i++) {
        lb[i] += x[i];
        ub[i] += x[i];
    }
    if (r.p.time_cal) {
        ub.push_back(r.p.max_time_offset);
        lb.push_back(-r.p.max_time_offset);
    }
    optimize(&r, lb, ub, &x);
    return r.rc;
}

int lio_calib_ins_calibrate(lio_calib_ins* h, const lio_calib_params* params) {
    if (!h) return LIO_E_INVALID;
    const int rc = calibrate(h, params);
    h->finished = 1;  // a failed run is over as well: nobody waits for it
    return rc;
}

int lio_calib_ins_progress(lio_calib_ins* h, int32_t* evals, double* best_err, int32_t* finished) {
    if (!h) return LIO_E_INVALID;
    if (evals) *evals = h->evals.load();
    if (best_err) *best_err = h->best_err.load();
    if (finished) *finished = h->finished.load();
    return LIO_OK;
}

int lio_calib_ins_result(lio_calib_ins* h, float T[16]) {
    if (!h || !T) return LIO_E_INVALID;
    std::lock_guard<std::mutex> g(h->mu);
    se3_matrix(h->best, T);
    return LIO_OK;
}

int lio_calib_ins_last_times(lio_calib_ins* h, double* assemble_us, double* build_us, double* terms_us) {
    if (!h) return LIO_E_INVALID;
    if (assemble_us) *assemble_us = h->assemble_us;
    if (build_us) *build_us = h->build_us;
    if (terms_us) *terms_us = h->terms_us;
    return LIO_OK;
}

}  // extern "C"
