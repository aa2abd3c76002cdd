// overlap.hip -- overlap detection between two maps on gfx950 (wave64): OverlapDetector of the reference's map merge
// (slam/localization/include/overlap_merge.hpp, "OM"); include/lio_hip.h states the rules.  The handle works over a lio_loop bank
// (loop_internal.h): frames, covariances, the engine, the batch scratch and the LM step are the loop detector's.
//
//   gate        calc_fitness_score (OM:225-263) for many sources against one target: the target filtered in its own order (device_prims.h's
//               compaction), knn_index_dev.h's tree over what is left, then one launch over the table workgroup -> (source, first point):
//               {sum, inliers, survivors} per 256 consecutive source points, added in order on the host
//   align_pairs FAST_VGICP for (target, source) pairs of several targets in one set of rounds: every distinct target's Gaussian voxels are built
//               by the bank's engine (gicp_adopt_cloud + vgicp_build) and their hash table and voxel array copied into a pool; overlap_vgicp_eval
//               is loop_vgicp_eval with {table, mask, voxels} read per slot.  The per-point body is WRITTEN A SECOND TIME here (loop.hip's kernels
//               stay as they are, and so do their registers); a change to one belongs in the other
//   accumulate  OM:186-194 with kf_append's f64 rule, then gicp_cloud_covariances on an engine sized max_accum_points -- which is then the fine
//               matcher's target as it stands
//   detect      OM:63-110, 147-211 over a fragment
#include <cfloat>
#include <chrono>
#include <cmath>
#include <map>
#include <queue>
#include <set>
#include <vector>

#include "device_prims.h"
#include "gicp_dev.h"
#include "knn_index_dev.h"
#include "loop_internal.h"

namespace lio {
namespace overlap {

using namespace prims;
using loop::FitSlot;
using loop::LoopSlot;

struct OvTarget {  // a slot's target in the pool
    const Slot* table;
    const VgicpVoxel* vox;
    uint32_t mask, pad;
};
struct Xf64 { double R[9], t[3]; };

// loop_vgicp_eval (loop.hip) with the slot's own target: the same statements in the same order
template <bool LIN>
__global__ void __launch_bounds__(kGicpThreads) overlap_vgicp_eval(const uint2* __restrict__ tab, LoopSlot* __restrict__ slots, const OvTarget* __restrict__ targets,
                                                                   double vres) {
    const uint2 tb = tab[blockIdx.x];
    const LoopSlot& s = slots[tb.x];
    if (s.phase != (LIN ? 0 : 1)) return;
    const OvTarget tg = targets[tb.x];
    const VgicpVoxel* __restrict__ vox = tg.vox;
    const double* __restrict__ T = LIN ? s.x0 : s.xi;
    GicpXform X;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) { X.R[r * 3 + c] = T[r * 4 + c]; X.Rf[r * 3 + c] = (float)T[r * 4 + c]; }
        X.t[r] = T[r * 4 + 3];
        X.tf[r] = (float)T[r * 4 + 3];
    }
    const uint32_t i = tb.y + threadIdx.x;
    double acc[kGicpAcc];
#pragma unroll
    for (int a = 0; a < kGicpAcc; a++) acc[a] = 0.0;
    if (i < s.n) {
        double ta[3];
        gicp_transform_d(X, s.src[i], ta);
        double* __restrict__ mrow = s.maha + (size_t)i * 6;
        int32_t c;
        if (LIN) {
            const int cx = (int)floor(ta[0] / vres - 0.5), cy = (int)floor(ta[1] / vres - 0.5), cz = (int)floor(ta[2] / vres - 0.5);
            uint32_t ptr, cnt, slot;
            c = grid_find_slot(tg.table, tg.mask, cx, cy, cz, ptr, cnt, slot) ? (int32_t)slot : -1;
            s.corr[i] = c;
            if (c >= 0) gicp_mahalanobis(s.scov + (size_t)i * 6, vox[c].cov, X, mrow);
        } else {
            c = s.corr[i];
        }
        if (c >= 0) {
            const VgicpVoxel v = vox[c];
            const double er[3] = {v.mean[0] - ta[0], v.mean[1] - ta[1], v.mean[2] - ta[2]};
            const double M[9] = {mrow[0], mrow[1], mrow[2], mrow[1], mrow[3], mrow[4], mrow[2], mrow[4], mrow[5]};
            const double w = sqrt(v.n);
            double Me[3];
            for (int r = 0; r < 3; r++) Me[r] = M[r * 3] * er[0] + M[r * 3 + 1] * er[1] + M[r * 3 + 2] * er[2];
            acc[27] = w * (er[0] * Me[0] + er[1] * Me[1] + er[2] * Me[2]);
            acc[28] = 1.0;
            if (LIN) {
                double J[18] = {0, -ta[2], ta[1], -1, 0, 0, ta[2], 0, -ta[0], 0, -1, 0, -ta[1], ta[0], 0, 0, 0, -1};
                double MJ[18];
                for (int r = 0; r < 3; r++)
                    for (int cc = 0; cc < 6; cc++) MJ[r * 6 + cc] = M[r * 3] * J[cc] + M[r * 3 + 1] * J[6 + cc] + M[r * 3 + 2] * J[12 + cc];
                int t = 0;
                for (int r = 0; r < 6; r++)
                    for (int cc = r; cc < 6; cc++) acc[t++] = w * (J[r] * MJ[cc] + J[6 + r] * MJ[6 + cc] + J[12 + r] * MJ[12 + cc]);
                for (int r = 0; r < 6; r++) acc[21 + r] = w * (J[r] * Me[0] + J[6 + r] * Me[1] + J[12 + r] * Me[2]);
            }
        }
    }
    __shared__ double red[kGicpThreads / 64][kGicpAcc];
#pragma unroll
    for (int a = 0; a < kGicpAcc; a++) {
        double v = acc[a];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][a] = v;
    }
    __syncthreads();
    if (threadIdx.x < kGicpAcc) {
        double v = 0.0;
        for (int w2 = 0; w2 < kGicpThreads / 64; w2++) v += red[w2][threadIdx.x];
        s.partial[(size_t)(tb.y / kGicpThreads) * kGicpAcc + threadIdx.x] = v;
    }
}

// OM:213-217 filter(): f32 sqrtf((x*x) + (y*y)) < max_range && z > floor_height, both strict; a point that is not finite does not pass
__device__ __forceinline__ bool in_range(float x, float y, float z, float xy_range, float min_z) {
    const float xx = x * x, yy = y * y;
    const float dist = sqrtf(xx + yy);
    return finite3(x, y, z) && dist < xy_range && z > min_z;
}

__global__ __launch_bounds__(kThreads) void overlap_filter_count(const float4* __restrict__ p, uint32_t n, float xy_range, float min_z, uint32_t* __restrict__ counts) {
    const uint32_t base = blockIdx.x * kTile;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        if (i < n) {
            const float4 q = p[i];
            c += in_range(q.x, q.y, q.z, xy_range, min_z) ? 1u : 0u;
        }
    }
    compact_tile_count(c, counts);
}

// the survivors as the index takes them, in input order: {x, y, z, bits of the place among the survivors}
__global__ __launch_bounds__(kThreads) void overlap_filter_write(const float4* __restrict__ p, uint32_t n, float xy_range, float min_z, const uint32_t* __restrict__ offs,
                                                                 float4* __restrict__ out) {
    const uint32_t base = blockIdx.x * kTile;
    bool keep[kItems];
    float4 q[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        q[r] = p[i < n ? i : 0u];
        keep[r] = i < n && in_range(q[r].x, q[r].y, q[r].z, xy_range, min_z);
    }
    compact_tile_write(keep, offs, [&](int r, uint32_t o) { out[o] = make_float4(q[r].x, q[r].y, q[r].z, __uint_as_float(o)); });
}

// calc_fitness_score: record (workgroup) = {sum of the gated squared distances, their number, the survivors of the filter} of 256 consecutive
// points of the table's source; nf = the filtered target's size (0: nothing is searched)
__global__ void __launch_bounds__(loop::kFitThreads) overlap_gate(const uint2* __restrict__ tab, const FitSlot* __restrict__ fs, const float4* __restrict__ leaves,
                                                                  const float4* __restrict__ nodes, uint32_t nf, uint32_t P, int L, double max_range, float xy_range,
                                                                  float min_z, double* __restrict__ partial) {
    const uint2 tb = tab[blockIdx.x];
    const FitSlot& f = fs[tb.x];
    const uint32_t i = tb.y + threadIdx.x;
    double my_sum = 0.0;
    uint32_t my_cnt = 0, my_in = 0;
    if (i < f.n) {
        const float4 p = f.src[i];
        const float tx = ((f.R[0] * p.x + f.R[1] * p.y) + f.R[2] * p.z) + f.t[0];
        const float ty = ((f.R[3] * p.x + f.R[4] * p.y) + f.R[5] * p.z) + f.t[1];
        const float tz = ((f.R[6] * p.x + f.R[7] * p.y) + f.R[8] * p.z) + f.t[2];
        if (in_range(tx, ty, tz, xy_range, min_z)) {
            my_in = 1;
            if (nf) {
                float kd[1] = {INFINITY};
                uint32_t ki[1] = {knn_index::kNone};
                knn_index::walk<1>(tx, ty, tz, nodes, leaves, nf, P, L, kd, ki);
                if (ki[0] != knn_index::kNone && (double)kd[0] <= max_range) { my_sum = (double)kd[0]; my_cnt = 1; }
            }
        }
    }
    constexpr int kW = loop::kFitThreads / 64;
    __shared__ double ssum[kW];
    __shared__ uint32_t scnt[kW], sin_[kW];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { my_sum += __shfl_xor(my_sum, off); my_cnt += __shfl_xor(my_cnt, off); my_in += __shfl_xor(my_in, off); }
    if ((threadIdx.x & 63) == 0) { ssum[threadIdx.x >> 6] = my_sum; scnt[threadIdx.x >> 6] = my_cnt; sin_[threadIdx.x >> 6] = my_in; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[3 * (size_t)blockIdx.x] = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
        partial[3 * (size_t)blockIdx.x + 1] = (double)((scnt[0] + scnt[1]) + (scnt[2] + scnt[3]));
        partial[3 * (size_t)blockIdx.x + 2] = (double)((sin_[0] + sin_[1]) + (sin_[2] + sin_[3]));
    }
}

// pcl::transformPointCloud(in, out, Matrix4d): per point in f64, terms left to right, cast to f32; the intensity rides along (kf_append's rule)
__global__ __launch_bounds__(kThreads) void overlap_append(const float4* __restrict__ src, uint32_t n, Xf64 X, float4* __restrict__ dst) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = src[i];
    const double x = p.x, y = p.y, z = p.z;
    dst[i] = make_float4((float)(((X.R[0] * x + X.R[1] * y) + X.R[2] * z) + X.t[0]), (float)(((X.R[3] * x + X.R[4] * y) + X.R[5] * z) + X.t[1]),
                         (float)(((X.R[6] * x + X.R[7] * y) + X.R[8] * z) + X.t[2]), p.w);
}

struct FrameReport {
    lio_overlap_report rep;
    std::vector<int32_t> ids, ridx, conv, it;  // bank id; place in the call's reference list
    std::vector<double> ratio, score;
};

}  // namespace overlap
}  // namespace lio

using namespace lio;
using namespace lio::overlap;

struct lio_overlap {
    lio_loop* L = nullptr;
    lio_overlap_params par;
    lio_gicp* fine = nullptr;  // sized max_accum_points; made by the first accumulate
    // the pool of targets of one align_pairs call
    Slot* pool_tab = nullptr;
    VgicpVoxel* pool_vox = nullptr;
    uint64_t pool_slots = 0, pool_stride = 0;  // targets held; table entries per target
    OvTarget *d_tg = nullptr, *h_tg = nullptr;  // [max_candidates]
    // the gate: filtered target, its index, the records
    uint64_t gate_cap = 0;
    float4* g_pts = nullptr;
    uint32_t* g_counts = nullptr;
    knn_index::DeviceIndex gidx;
    double *d_gp = nullptr, *h_gp = nullptr;
    uint64_t gp_cap = 0;
    uint32_t* h_word = nullptr;  // pinned: a count read back
    // the accumulated cloud
    float4* acc_pts = nullptr;
    double* acc_cov = nullptr;
    uint32_t acc_n = 0;
    bool acc_valid = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    lio_overlap_times tm;
    std::vector<FrameReport> reports;
};

namespace {

struct Span {  // HIP events around a stretch of host-synchronous work on the bank's stream
    lio_overlap* h;
    double* acc;
    Span(lio_overlap* h_, double* a) : h(h_), acc(a) { hipEventRecord(h->ev[0], h->L->st); }
    ~Span() {
        float ms = 0.f;
        if (hipEventRecord(h->ev[1], h->L->st) == hipSuccess && hipEventSynchronize(h->ev[1]) == hipSuccess && hipEventElapsedTime(&ms, h->ev[0], h->ev[1]) == hipSuccess)
            *acc += (double)ms * 1000.0;
    }
};

bool bank_slot_ok(const lio_overlap* h, int id) { return id >= 0 && (size_t)id < h->L->frames.size(); }
bool bank_id_ok(const lio_overlap* h, int id) { return bank_slot_ok(h, id) && !h->L->frames[id].retired; }  // a retired frame (lio_loop_retire) is unknown to the stage doors

using ConnMap = std::map<int, std::set<int>>;

// OM:80-91
ConnMap build_connections(const int32_t* from, const int32_t* to, uint32_t n) {
    ConnMap m;
    for (uint32_t i = 0; i < n; i++) {
        m[from[i]].insert(to[i]);
        m[to[i]].insert(from[i]);
    }
    return m;
}

// OM:265-296
int connection_count(ConnMap& connection, int source, int target, int max_count) {
    int count = 0;
    std::map<int, bool> visited;
    for (auto& conn : connection) visited[conn.first] = false;
    std::queue<int> q;
    q.push(source);
    while (!q.empty()) {
        const int size = (int)q.size();
        for (int i = 0; i < size; i++) {
            const int curr = q.front();
            q.pop();
            if (curr == target) return count;
            visited[curr] = true;
            for (auto& adjacent : connection[curr])
                if (!visited[adjacent]) q.push(adjacent);
        }
        count++;
        if (max_count > 0 && count >= max_count) break;
    }
    return count;
}

// OM:113-145 under the project's rules
std::vector<int32_t> find_candidates(const double* pos, const int32_t* ids, uint32_t n, ConnMap& conn, int32_t new_id, const double q[3], const lio_overlap_params& p) {
    std::vector<int32_t> out;
    if (n == 0 || p.knn <= 0) return out;
    const float qx = (float)q[0], qy = (float)q[1], qz = (float)q[2];
    std::vector<std::pair<float, uint32_t>> d(n);
    for (uint32_t i = 0; i < n; i++) {
        const float dx = (float)pos[3 * i] - qx, dy = (float)pos[3 * i + 1] - qy, dz = (float)pos[3 * i + 2] - qz;
        d[i] = {((dx * dx) + dy * dy) + dz * dz, i};
    }
    const size_t k = std::min<size_t>((size_t)p.knn, n);
    std::partial_sort(d.begin(), d.begin() + k, d.end());  // (d2, index): equal distances go to the smaller index
    for (size_t j = 0; j < k; j++) {
        const uint32_t i = d[j].second;
        if (new_id == ids[i]) continue;
        if (conn[new_id].count(ids[i]) != 0) continue;
        if ((double)d[j].first < p.distance_thresh * p.distance_thresh) {
            const int cc = connection_count(conn, new_id, ids[i], p.candidate_link_dist);
            if (cc >= p.candidate_link_dist) out.push_back((int32_t)i);
        }
        if ((int)out.size() >= p.max_candidate_num) break;
    }
    return out;
}

// a^-1 * b of two rigid transforms in f64: Isometry3d::inverse() is R^T, -(R^T t); every sum of three products left to right
void rel_pose(const double a[16], const double b[16], double R[9], double t[3]) {
    for (int i = 0; i < 3; i++) {
        const double ti = -((a[i] * a[3] + a[4 + i] * a[7]) + a[8 + i] * a[11]);
        for (int j = 0; j < 3; j++) R[3 * i + j] = (a[i] * b[j] + a[4 + i] * b[4 + j]) + a[8 + i] * b[8 + j];
        t[i] = ((a[i] * b[3] + a[4 + i] * b[7]) + a[8 + i] * b[11]) + ti;
    }
}

int gate_reserve(lio_overlap* h, uint64_t n_target) {
    if (n_target <= h->gate_cap) return LIO_OK;
    hipStream_t st = h->L->st;
    uint64_t c = h->gate_cap ? h->gate_cap : 65536;
    while (c < n_target) c *= 2;
    uint64_t cap_pts = h->gate_cap, cap_cnt = h->gate_cap ? compact_words(h->gate_cap) : 0;
    h->gate_cap = 0;
    int rc = grow("lio_overlap", &h->g_pts, &cap_pts, c, st);
    if (rc != LIO_OK) return rc;
    rc = grow("lio_overlap", &h->g_counts, &cap_cnt, compact_words(c), st);
    if (rc != LIO_OK) return rc;
    rc = knn_index::device_index_reserve(h->gidx, c);
    if (rc != LIO_OK) return rc;
    h->gate_cap = c;
    return LIO_OK;
}

// the gate of n bank frames against the device cloud tgt[0, tn): one filter + index build, then the sources in launches of max_candidates
int gate_run(lio_overlap* h, const float4* tgt, uint32_t tn, const int32_t* src_ids, const double* T16, uint32_t n, double max_range, double* score, uint32_t* nr,
             uint32_t* n_in) {
    lio_loop* L = h->L;
    hipStream_t st = L->st;
    int rc = gate_reserve(h, tn);
    if (rc != LIO_OK) return rc;
    const float xyr = (float)h->par.xy_range, mz = h->par.min_z;
    uint32_t nf = 0;
    if (tn) {
        hipLaunchKernelGGL(overlap_filter_count, tiles_of(tn), kThreads, 0, st, tgt, tn, xyr, mz, h->g_counts);
        const uint32_t* d_nf = compact_finish(st, h->g_counts, tn);
        if (!d_nf) return LIO_E_DEVICE;
        hipLaunchKernelGGL(overlap_filter_write, tiles_of(tn), kThreads, 0, st, tgt, tn, xyr, mz, h->g_counts, h->g_pts);
        LIO_HIP_TRY(hipGetLastError());
        LIO_HIP_TRY(hipMemcpyAsync(h->h_word, d_nf, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        LIO_HIP_TRY(hipStreamSynchronize(st));
        nf = *h->h_word;
        if (nf > tn) { set_error("lio_overlap: the target's filter kept more points than it was given"); return LIO_E_STATE; }
        if (nf) {
            rc = knn_index::device_index_build(st, h->gidx, h->g_pts, nullptr, nf);
            if (rc != LIO_OK) return rc;
        }
    }
    const uint32_t maxB = L->par.max_candidates;
    for (uint32_t base = 0; base < n; base += maxB) {
        const uint32_t B = n - base < maxB ? n - base : maxB;
        uint64_t nblocks = 0;
        for (uint32_t k = 0; k < B; k++) nblocks += (L->frames[src_ids[base + k]].n + loop::kFitThreads - 1) / loop::kFitThreads;
        rc = loop::loop_reserve(L, 0, nblocks);
        if (rc != LIO_OK) return rc;
        if (3 * L->tab_cap > h->gp_cap) {
            LIO_HIP_TRY(hipStreamSynchronize(st));
            if (h->d_gp) hipFree(h->d_gp);
            if (h->h_gp) hipHostFree(h->h_gp);
            h->d_gp = h->h_gp = nullptr;
            h->gp_cap = 0;
            LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->d_gp), 3 * L->tab_cap * sizeof(double)));
            LIO_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->h_gp), 3 * L->tab_cap * sizeof(double), hipHostMallocDefault));
            h->gp_cap = 3 * L->tab_cap;
        }
        uint32_t b = 0;
        for (uint32_t k = 0; k < B; k++) {
            const loop::Frame& f = L->frames[src_ids[base + k]];
            const double* T = T16 + 16 * (size_t)(base + k);
            FitSlot& fs = L->h_fit[k];
            fs.src = f.pts; fs.n = f.n; fs.pad = 0;
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) fs.R[r * 3 + c] = (float)T[r * 4 + c]; fs.t[r] = (float)T[r * 4 + 3]; }
            for (uint32_t p0 = 0; p0 < f.n; p0 += loop::kFitThreads) L->h_tab[b++] = make_uint2(k, p0);
        }
        LIO_HIP_TRY(hipMemcpyAsync(L->d_fit, L->h_fit, sizeof(FitSlot) * B, hipMemcpyHostToDevice, st));
        LIO_HIP_TRY(hipMemcpyAsync(L->d_tab, L->h_tab, sizeof(uint2) * b, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(overlap_gate, b, loop::kFitThreads, 0, st, L->d_tab, L->d_fit, h->gidx.leaves, h->gidx.nodes, nf, h->gidx.P, h->gidx.L, max_range, xyr, mz, h->d_gp);
        LIO_HIP_TRY(hipGetLastError());
        LIO_HIP_TRY(hipMemcpyAsync(h->h_gp, h->d_gp, sizeof(double) * 3 * b, hipMemcpyDeviceToHost, st));
        LIO_HIP_TRY(hipStreamSynchronize(st));
        b = 0;
        for (uint32_t k = 0; k < B; k++) {
            double sum = 0.0, cnt = 0.0, in = 0.0;
            for (uint32_t p0 = 0; p0 < L->frames[src_ids[base + k]].n; p0 += loop::kFitThreads, b++) { sum += h->h_gp[3 * b]; cnt += h->h_gp[3 * b + 1]; in += h->h_gp[3 * b + 2]; }
            if (score) score[base + k] = cnt > 0 ? sum / cnt : DBL_MAX;
            if (nr) nr[base + k] = (uint32_t)cnt;
            if (n_in) n_in[base + k] = (uint32_t)in;
        }
    }
    return LIO_OK;
}

// room for `slots` targets of `stride` table entries each
int pool_reserve(lio_overlap* h, uint64_t slots, uint64_t stride) {
    if (slots <= h->pool_slots && stride == h->pool_stride) return LIO_OK;
    LIO_HIP_TRY(hipStreamSynchronize(h->L->st));
    if (h->pool_tab) hipFree(h->pool_tab);
    if (h->pool_vox) hipFree(h->pool_vox);
    h->pool_tab = nullptr; h->pool_vox = nullptr; h->pool_slots = 0; h->pool_stride = stride;
    if (hipMalloc(reinterpret_cast<void**>(&h->pool_tab), slots * stride * sizeof(Slot)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&h->pool_vox), slots * stride * sizeof(VgicpVoxel)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("lio_overlap: no room for the voxels of %llu targets", (unsigned long long)slots);
        return LIO_E_DEVICE;
    }
    h->pool_slots = slots;
    return LIO_OK;
}

// FAST_VGICP for n pairs: loop.hip's coarse_batch with the slot's target read from the pool
int align_pairs(lio_overlap* h, const int32_t* tgt_ids, const int32_t* src_ids, const double* guesses, uint32_t n, loop::AlignOut* out) {
    lio_loop* L = h->L;
    const lio_loop_params& par = L->par;
    hipStream_t st = L->st;
    h->tm.n_pairs += (int32_t)n;
    if (par.max_iterations <= 0) {  // computeTransformation's loop does not run: the guess stands
        for (uint32_t k = 0; k < n; k++) { memcpy(out[k].T, guesses + 16 * k, sizeof(out[k].T)); out[k].iterations = out[k].converged = 0; }
        return LIO_OK;
    }
    // the distinct targets in the order they first appear, their voxels into the pool
    std::vector<int32_t> distinct;
    std::vector<uint32_t> tslot(n);
    {
        std::map<int32_t, uint32_t> seen;
        for (uint32_t k = 0; k < n; k++) {
            auto it = seen.find(tgt_ids[k]);
            if (it == seen.end()) { it = seen.emplace(tgt_ids[k], (uint32_t)distinct.size()).first; distinct.push_back(tgt_ids[k]); }
            tslot[k] = it->second;
        }
    }
    std::vector<uint32_t> masks(distinct.size());
    {
        Span sp(h, &h->tm.targets_us);
        L->target_id = -1;  // the engine's target changes under the detector's feet
        for (size_t d = 0; d < distinct.size(); d++) {
            const loop::Frame& f = L->frames[distinct[d]];
            int rc = gicp_adopt_cloud(L->eng, 0, f.pts, f.cov, f.n);
            if (rc != LIO_OK) return rc;
            rc = vgicp_build(L->eng);
            if (rc != LIO_OK) return rc;
            const lio_map* vm = L->eng->vmap;
            if (d == 0) {
                rc = pool_reserve(h, distinct.size(), vm->table_cap);
                if (rc != LIO_OK) return rc;
            } else if (vm->table_cap != h->pool_stride) {
                set_error("lio_overlap: the engine's voxel table changed its size between two targets");
                return LIO_E_STATE;
            }
            masks[d] = vm->table_mask;
            LIO_HIP_TRY(hipMemcpyAsync(h->pool_tab + d * h->pool_stride, vm->table, h->pool_stride * sizeof(Slot), hipMemcpyDeviceToDevice, st));
            LIO_HIP_TRY(hipMemcpyAsync(h->pool_vox + d * h->pool_stride, L->eng->vvox, h->pool_stride * sizeof(VgicpVoxel), hipMemcpyDeviceToDevice, st));
            LIO_HIP_TRY(hipStreamSynchronize(st));  // the engine's table is cleared by the next target's build
        }
        h->tm.n_targets += (int32_t)distinct.size();
    }
    Span sp(h, &h->tm.coarse_us);
    lio_ndt_params dp;
    lio_ndt_default_params(&dp);
    const loop::LoopLmParams P{par.max_iterations, dp.lm_max_iterations, par.coarse_rotation_epsilon_deg, par.coarse_translation_epsilon, dp.lm_init_lambda_factor};
    const double vres = (double)(float)par.voxel_resolution;
    for (uint32_t base = 0; base < n; base += par.max_candidates) {
        const uint32_t B = n - base < par.max_candidates ? n - base : par.max_candidates;
        uint64_t pts = 0, blocks = 0;
        for (uint32_t k = 0; k < B; k++) { const uint32_t m = L->frames[src_ids[base + k]].n; pts += m; blocks += (m + kGicpThreads - 1) / kGicpThreads; }
        int rc = loop::loop_reserve(L, pts, blocks);
        if (rc != LIO_OK) return rc;
        uint64_t po = 0, bo = 0;
        for (uint32_t k = 0; k < B; k++) {
            const loop::Frame& f = L->frames[src_ids[base + k]];
            LoopSlot& s = L->h_slots[k];
            memset(&s, 0, sizeof(s));
            s.src = f.pts; s.scov = f.cov; s.n = f.n; s.nb = (f.n + kGicpThreads - 1) / kGicpThreads;
            s.corr = L->b_corr + po; s.maha = L->b_maha + po * 6; s.partial = L->b_partial + bo * kGicpAcc;
            po += f.n; bo += s.nb;
            memcpy(s.x0, guesses + 16 * (size_t)(base + k), sizeof(s.x0));
            s.lambda = -1.0;
            const uint32_t d = tslot[base + k];
            h->h_tg[k] = OvTarget{h->pool_tab + d * h->pool_stride, h->pool_vox + d * h->pool_stride, masks[d], 0};
        }
        LIO_HIP_TRY(hipMemcpyAsync(L->d_slots, L->h_slots, sizeof(LoopSlot) * B, hipMemcpyHostToDevice, st));
        LIO_HIP_TRY(hipMemcpyAsync(h->d_tg, h->h_tg, sizeof(OvTarget) * B, hipMemcpyHostToDevice, st));
        const int max_rounds = par.max_iterations * (dp.lm_max_iterations + 1) + 2;
        bool all_done = false;
        for (int r = 0; r < max_rounds && !all_done;) {
            uint32_t nt = 0;  // the table of the live slots
            for (uint32_t k = 0; k < B; k++)
                if (L->h_slots[k].phase != 2)
                    for (uint32_t p0 = 0; p0 < L->h_slots[k].n; p0 += kGicpThreads) L->h_tab[nt++] = make_uint2(k, p0);
            if (nt == 0) break;
            LIO_HIP_TRY(hipMemcpyAsync(L->d_tab, L->h_tab, sizeof(uint2) * nt, hipMemcpyHostToDevice, st));
            for (int k = 0; k < loop::kLookEvery && r < max_rounds; k++, r++) {
                hipLaunchKernelGGL(overlap_vgicp_eval<true>, nt, kGicpThreads, 0, st, L->d_tab, L->d_slots, h->d_tg, vres);
                hipLaunchKernelGGL(overlap_vgicp_eval<false>, nt, kGicpThreads, 0, st, L->d_tab, L->d_slots, h->d_tg, vres);
                loop::loop_launch_lm_step(st, B, L->d_slots, P);
                h->tm.coarse_rounds++;
            }
            LIO_HIP_TRY(hipGetLastError());
            LIO_HIP_TRY(hipMemcpyAsync(L->h_slots, L->d_slots, sizeof(LoopSlot) * B, hipMemcpyDeviceToHost, st));
            LIO_HIP_TRY(hipStreamSynchronize(st));  // (the table in pinned memory is rewritten next: its copy has completed)
            all_done = true;
            for (uint32_t k = 0; k < B; k++)
                if (L->h_slots[k].phase != 2) all_done = false;
        }
        for (uint32_t k = 0; k < B; k++) {
            const LoopSlot& s = L->h_slots[k];
            if (s.phase != 2) { set_error("lio_overlap: a slot of the coarse batch did not finish"); return LIO_E_STATE; }
            memcpy(out[base + k].T, s.x0, sizeof(s.x0));
            out[base + k].iterations = s.it_done;
            out[base + k].converged = s.conv;
        }
    }
    return LIO_OK;
}

int accumulate(lio_overlap* h, int best, const int32_t* nb, uint32_t n) {
    lio_loop* L = h->L;
    hipStream_t st = L->st;
    h->acc_valid = false;
    h->acc_n = 0;
    uint64_t total = L->frames[best].n;
    for (uint32_t k = 0; k < n; k++) total += L->frames[nb[k]].n;
    if (total > h->par.max_accum_points) {
        set_error("lio_overlap_accumulate: %llu points exceed max_accum_points %u", (unsigned long long)total, h->par.max_accum_points);
        return LIO_E_CAPACITY;
    }
    if (!h->fine) {
        h->fine = lio_gicp_create(L->device, L->par.grid_resolution, h->par.max_accum_points, L->par.k_correspondences);
        if (!h->fine) return LIO_E_DEVICE;
    }
    if (!h->acc_pts) {
        const size_t bytes = (size_t)h->par.max_accum_points * (sizeof(float4) + 6 * sizeof(double));
        LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->acc_pts), bytes));
        h->acc_cov = reinterpret_cast<double*>(h->acc_pts + h->par.max_accum_points);
    }
    const loop::Frame& fb = L->frames[best];
    LIO_HIP_TRY(hipMemcpyAsync(h->acc_pts, fb.pts, (size_t)fb.n * sizeof(float4), hipMemcpyDeviceToDevice, st));
    uint32_t at = fb.n;
    for (uint32_t k = 0; k < n; k++) {
        const loop::Frame& f = L->frames[nb[k]];
        Xf64 X;
        rel_pose(fb.pose, f.pose, X.R, X.t);
        hipLaunchKernelGGL(overlap_append, blocks_of(f.n), kThreads, 0, st, f.pts, f.n, X, h->acc_pts + at);
        at += f.n;
    }
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipStreamSynchronize(st));  // the engine works on its grid's stream
    const int rc = gicp_cloud_covariances(h->fine, 0, h->acc_pts, at, h->acc_cov);
    if (rc != LIO_OK) return rc;
    h->acc_n = at;
    h->acc_valid = true;
    return (int)at;
}

void blank_report(FrameReport& fr, int32_t new_id) {
    memset(&fr.rep, 0, sizeof(fr.rep));
    fr.rep.new_id = new_id;
    fr.rep.best = -1;
    fr.rep.reason = LIO_OVERLAP_NO_CANDIDATE;
    fr.rep.best_score = DBL_MAX;
    fr.rep.fine_score = DBL_MAX;
}

bool params_ok(const lio_overlap_params& p) {
    if (!(p.distance_thresh > 0) || p.candidate_link_dist < 0 || p.max_candidate_num < 1 || p.knn < 1 || !(p.fitness_score_max_range > 0) || !(p.gate_max_range > 0) ||
        !(p.xy_range > 0) || !(p.fine_max_corr_dist > 0) || !(p.fine_translation_epsilon > 0) || p.max_accum_points == 0 || p.max_accum_points > 0x7FFFFFFFu ||
        !(p.fitness_inlier_thresh >= 0) || !(p.fitness_score_thresh > 0) || !(p.min_z == p.min_z)) {
        set_error("lio_overlap: thresholds, ranges and epsilons must be positive, max_candidate_num, knn >= 1, 1 <= max_accum_points < 2^31");
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

void lio_overlap_default_params(lio_loop* bank, lio_overlap_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->distance_thresh = 30.0;
    p->candidate_link_dist = 10;
    p->max_candidate_num = 3;
    p->knn = 10;
    p->min_z = 0.5f;
    p->fitness_score_max_range = 25.0;
    p->fitness_score_thresh = 1.5;
    p->fitness_inlier_thresh = 0.2;
    p->gate_max_range = 1.0;
    p->xy_range = 100.0;
    p->fine_max_corr_dist = 0.5;
    p->fine_translation_epsilon = 0.001;
    const uint64_t m = 8ull * (bank ? bank->par.max_points : 65536u);
    p->max_accum_points = (uint32_t)std::min<uint64_t>(m, 0x7FFFFFFFull);
}

int lio_overlap_connection_count(const int32_t* from, const int32_t* to, uint32_t n_edges, int32_t source, int32_t target, int32_t max_count) {
    if (n_edges && (!from || !to)) return LIO_E_INVALID;
    ConnMap m = build_connections(from, to, n_edges);
    return connection_count(m, source, target, max_count);
}

int lio_overlap_find_candidates(const double* pos_xyz, const int32_t* ids, uint32_t n, const int32_t* edge_from, const int32_t* edge_to, uint32_t n_edges,
                                int32_t new_id, const double new_xyz[3], const lio_overlap_params* params, int32_t* out_idx, uint32_t cap) {
    if ((n && (!pos_xyz || !ids)) || (n_edges && (!edge_from || !edge_to)) || !new_xyz) return LIO_E_INVALID;
    lio_overlap_params p;
    if (params) p = *params; else lio_overlap_default_params(nullptr, &p);
    ConnMap m = build_connections(edge_from, edge_to, n_edges);
    const std::vector<int32_t> c = find_candidates(pos_xyz, ids, n, m, new_id, new_xyz, p);
    if (c.size() > cap || (!c.empty() && !out_idx)) return -(int)c.size();
    for (size_t k = 0; k < c.size(); k++) out_idx[k] = c[k];
    return (int)c.size();
}

lio_overlap* lio_overlap_create(lio_loop* bank, const lio_overlap_params* params) {
    if (!bank) { set_error("lio_overlap_create: no bank"); return nullptr; }
    lio_overlap_params p;
    if (params) p = *params; else lio_overlap_default_params(bank, &p);
    if (!params_ok(p)) return nullptr;
    if (hipSetDevice(bank->device) != hipSuccess) { set_error("lio_overlap_create: no HIP device %d (this library has no CPU fallback)", bank->device); return nullptr; }
    lio_overlap* h = new lio_overlap();
    h->L = bank;
    h->par = p;
    memset(&h->tm, 0, sizeof(h->tm));
    const bool ok = hipEventCreate(&h->ev[0]) == hipSuccess && hipEventCreate(&h->ev[1]) == hipSuccess &&
                    hipMalloc(reinterpret_cast<void**>(&h->d_tg), sizeof(OvTarget) * bank->par.max_candidates) == hipSuccess &&
                    hipHostMalloc(reinterpret_cast<void**>(&h->h_tg), sizeof(OvTarget) * bank->par.max_candidates, hipHostMallocDefault) == hipSuccess &&
                    hipHostMalloc(reinterpret_cast<void**>(&h->h_word), 64, hipHostMallocDefault) == hipSuccess;
    if (!ok) {
        set_error("lio_overlap_create: allocation failed");
        lio_overlap_destroy(h);
        return nullptr;
    }
    return h;
}

void lio_overlap_destroy(lio_overlap* h) {
    if (!h) return;
    hipSetDevice(h->L->device);
    if (h->L->st) hipStreamSynchronize(h->L->st);
    if (h->fine) lio_gicp_destroy(h->fine);
    knn_index::device_index_free(h->gidx);
    hipFree(h->pool_tab); hipFree(h->pool_vox); hipFree(h->d_tg); hipFree(h->g_pts); hipFree(h->g_counts); hipFree(h->d_gp); hipFree(h->acc_pts);
    if (h->h_tg) hipHostFree(h->h_tg);
    if (h->h_gp) hipHostFree(h->h_gp);
    if (h->h_word) hipHostFree(h->h_word);
    for (int i = 0; i < 2; i++)
        if (h->ev[i]) hipEventDestroy(h->ev[i]);
    delete h;
}

int lio_overlap_gate_batch(lio_overlap* h, int target_id, const int32_t* source_ids, uint32_t n, const double* T16, double max_range, double* score, uint32_t* nr,
                           uint32_t* n_in) {
    if (!h || (n && (!source_ids || !T16)) || !(max_range >= 0)) return LIO_E_INVALID;
    if (target_id != LIO_OVERLAP_ACCUM && !bank_id_ok(h, target_id)) return LIO_E_INVALID;
    if (target_id == LIO_OVERLAP_ACCUM && !h->acc_valid) { set_error("lio_overlap_gate_batch: no accumulated cloud"); return LIO_E_STATE; }
    for (uint32_t k = 0; k < n; k++)
        if (!bank_id_ok(h, source_ids[k])) return LIO_E_INVALID;
    if (n == 0) return LIO_OK;
    hipSetDevice(h->L->device);
    h->tm.gate_us = 0;
    Span sp(h, &h->tm.gate_us);
    if (target_id == LIO_OVERLAP_ACCUM) return gate_run(h, h->acc_pts, h->acc_n, source_ids, T16, n, max_range, score, nr, n_in);
    const loop::Frame& f = h->L->frames[target_id];
    return gate_run(h, f.pts, f.n, source_ids, T16, n, max_range, score, nr, n_in);
}

int lio_overlap_align_pairs(lio_overlap* h, const int32_t* target_ids, const int32_t* source_ids, uint32_t n, const double* guesses, double* out_T,
                            int32_t* iterations, int32_t* converged) {
    if (!h || (n && (!target_ids || !source_ids || !guesses))) return LIO_E_INVALID;
    for (uint32_t k = 0; k < n; k++)
        if (!bank_id_ok(h, target_ids[k]) || !bank_id_ok(h, source_ids[k])) return LIO_E_INVALID;
    if (n == 0) return LIO_OK;
    hipSetDevice(h->L->device);
    h->tm.targets_us = h->tm.coarse_us = 0;
    h->tm.coarse_rounds = h->tm.n_pairs = h->tm.n_targets = 0;
    std::vector<loop::AlignOut> res(n);
    const int rc = align_pairs(h, target_ids, source_ids, guesses, n, res.data());
    if (rc != LIO_OK) return rc;
    for (uint32_t k = 0; k < n; k++) {
        if (out_T) memcpy(out_T + 16 * (size_t)k, res[k].T, sizeof(res[k].T));
        if (iterations) iterations[k] = res[k].iterations;
        if (converged) converged[k] = res[k].converged;
    }
    return LIO_OK;
}

int lio_overlap_accumulate(lio_overlap* h, int best_id, const int32_t* neighbour_ids, uint32_t n) {
    if (!h || !bank_id_ok(h, best_id) || (n && !neighbour_ids)) return LIO_E_INVALID;
    for (uint32_t k = 0; k < n; k++)
        if (!bank_id_ok(h, neighbour_ids[k])) return LIO_E_INVALID;
    hipSetDevice(h->L->device);
    h->tm.accumulate_us = 0;
    Span sp(h, &h->tm.accumulate_us);
    return accumulate(h, best_id, neighbour_ids, n);
}

int lio_overlap_download_accum(lio_overlap* h, float* xyzi, double* cov6, uint32_t cap) {
    if (!h) return LIO_E_INVALID;
    if (!h->acc_valid) { set_error("lio_overlap_download_accum: no accumulated cloud"); return LIO_E_STATE; }
    if (h->acc_n > cap) return -(int)h->acc_n;
    hipSetDevice(h->L->device);
    if (xyzi) LIO_HIP_TRY(hipMemcpy(xyzi, h->acc_pts, (size_t)h->acc_n * sizeof(float4), hipMemcpyDeviceToHost));
    if (cov6) LIO_HIP_TRY(hipMemcpy(cov6, h->acc_cov, (size_t)h->acc_n * 6 * sizeof(double), hipMemcpyDeviceToHost));
    return (int)h->acc_n;
}

int lio_overlap_detect(lio_overlap* h, const int32_t* ref_ids, const int32_t* ref_kf, uint32_t n_ref, const int32_t* new_ids, const int32_t* new_kf, uint32_t n_new,
                       const int32_t* edge_from, const int32_t* edge_to, uint32_t n_edges, lio_overlap_edge* out, uint32_t cap) {
    if (!h || (n_ref && !ref_ids) || (n_new && !new_ids) || (n_edges && (!edge_from || !edge_to))) return LIO_E_INVALID;
    for (uint32_t k = 0; k < n_ref; k++)
        if (!bank_slot_ok(h, ref_ids[k])) return LIO_E_INVALID;
    for (uint32_t k = 0; k < n_new; k++)
        if (!bank_slot_ok(h, new_ids[k])) return LIO_E_INVALID;
    lio_loop* L = h->L;
    // a retired frame is skipped: as a reference it is left out of the list (so it is no candidate and no neighbour of the accumulated cloud), as a
    // new frame it keeps its place in the reports with no candidate
    std::vector<int32_t> live_ids, live_kf;
    bool any_retired = false;
    for (uint32_t k = 0; k < n_ref; k++) any_retired = any_retired || L->frames[ref_ids[k]].retired;
    if (any_retired) {
        for (uint32_t k = 0; k < n_ref; k++) {
            if (L->frames[ref_ids[k]].retired) continue;
            live_ids.push_back(ref_ids[k]);
            live_kf.push_back(ref_kf ? ref_kf[k] : ref_ids[k]);
        }
        n_ref = (uint32_t)live_ids.size();
        ref_ids = live_ids.data();
        ref_kf = live_kf.data();
    }
    hipSetDevice(L->device);
    memset(&h->tm, 0, sizeof(h->tm));
    h->reports.assign(n_new, FrameReport());
    auto kf_of_ref = [&](uint32_t k) { return ref_kf ? ref_kf[k] : ref_ids[k]; };
    auto kf_of_new = [&](uint32_t k) { return new_kf ? new_kf[k] : new_ids[k]; };
    ConnMap conn = build_connections(edge_from, edge_to, n_edges);
    std::map<int32_t, uint32_t> ref_index;  // keyframe_id_map (OM:94-97)
    std::vector<double> pos(3 * (size_t)n_ref);
    std::vector<int32_t> rkf(n_ref);
    for (uint32_t k = 0; k < n_ref; k++) {
        const double* T = L->frames[ref_ids[k]].pose;
        pos[3 * k] = T[3]; pos[3 * k + 1] = T[7]; pos[3 * k + 2] = T[11];
        rkf[k] = kf_of_ref(k);
        ref_index[rkf[k]] = k;
    }
    // candidates and the gate, frame by frame (the target of the gate is the new frame)
    struct Pair { uint32_t frame, cand; };
    std::vector<Pair> pairs;
    std::vector<int32_t> ptgt, psrc;
    std::vector<double> pguess;
    int rc = LIO_OK;
    for (uint32_t i = 0; i < n_new; i++) {
        FrameReport& fr = h->reports[i];
        blank_report(fr, new_ids[i]);
        const loop::Frame& nf = L->frames[new_ids[i]];
        if (nf.retired) continue;
        const auto t0 = std::chrono::steady_clock::now();
        const double q[3] = {nf.pose[3], nf.pose[7], nf.pose[11]};
        const std::vector<int32_t> cand = find_candidates(pos.data(), rkf.data(), n_ref, conn, kf_of_new(i), q, h->par);
        h->tm.candidates_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        const size_t K = cand.size();
        fr.rep.n_candidates = (int32_t)K;
        fr.ids.resize(K); fr.ridx = cand; fr.conv.assign(K, 0); fr.it.assign(K, 0); fr.ratio.assign(K, 0.0); fr.score.assign(K, DBL_MAX);
        if (K == 0) continue;
        std::vector<double> g(16 * K);
        for (size_t k = 0; k < K; k++) {
            fr.ids[k] = ref_ids[cand[k]];
            double R[9], t[3];
            rel_pose(nf.pose, L->frames[fr.ids[k]].pose, R, t);  // (new^-1 * candidate).cast<float>()
            double* G = &g[16 * k];
            for (int a = 0; a < 16; a++) G[a] = (a % 5 == 0) ? 1.0 : 0.0;
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) G[r * 4 + c] = (double)(float)R[r * 3 + c]; G[r * 4 + 3] = (double)(float)t[r]; }
        }
        std::vector<uint32_t> gnr(K), gin(K);
        { Span sp(h, &h->tm.gate_us); rc = gate_run(h, nf.pts, nf.n, fr.ids.data(), g.data(), (uint32_t)K, h->par.gate_max_range, nullptr, gnr.data(), gin.data()); }
        if (rc != LIO_OK) return rc;
        fr.rep.reason = LIO_OVERLAP_GATE;
        for (size_t k = 0; k < K; k++) {
            fr.ratio[k] = gnr[k] > 0 ? (double)gnr[k] / (double)gin[k] : 0.0;
            if (fr.ratio[k] < h->par.fitness_inlier_thresh) continue;
            pairs.push_back({i, (uint32_t)k});
            ptgt.push_back(new_ids[i]); psrc.push_back(fr.ids[k]);
            pguess.insert(pguess.end(), g.begin() + 16 * k, g.begin() + 16 * (k + 1));
            fr.rep.reason = LIO_OVERLAP_COARSE;
        }
    }
    // ONE coarse batch over the fragment
    std::vector<loop::AlignOut> res(pairs.size());
    if (!pairs.empty()) {
        rc = align_pairs(h, ptgt.data(), psrc.data(), pguess.data(), (uint32_t)pairs.size(), res.data());
        if (rc != LIO_OK) return rc;
    }
    // per new frame: getFitnessScore of the converged pairs, the best, the fine stage
    std::vector<lio_overlap_edge> found;
    size_t p0 = 0;
    for (uint32_t i = 0; i < n_new; i++) {
        FrameReport& fr = h->reports[i];
        size_t p1 = p0;
        while (p1 < pairs.size() && pairs[p1].frame == i) p1++;
        std::vector<int32_t> fid, fk;
        std::vector<double> fT;
        for (size_t p = p0; p < p1; p++) {
            const uint32_t k = pairs[p].cand;
            fr.conv[k] = res[p].converged; fr.it[k] = res[p].iterations;
            if (!res[p].converged) continue;
            fid.push_back(fr.ids[k]); fk.push_back((int32_t)p);
            fT.insert(fT.end(), res[p].T, res[p].T + 16);
        }
        p0 = p1;
        if (fid.empty()) continue;
        std::vector<double> fs(fid.size());
        std::vector<uint32_t> fn(fid.size());
        {
            Span sp(h, &h->tm.fitness_us);
            rc = loop::loop_prepare_target(L, new_ids[i]);
            if (rc == LIO_OK) rc = loop::loop_fitness_batch(L, fid.data(), fT.data(), (uint32_t)fid.size(), fs.data(), fn.data(), h->par.fitness_score_max_range);
        }
        if (rc != LIO_OK) return rc;
        double best_score = DBL_MAX;
        int bestp = -1;
        for (size_t j = 0; j < fid.size(); j++) {
            fr.score[pairs[fk[j]].cand] = fs[j];
            if (fs[j] > best_score) continue;
            best_score = fs[j];
            bestp = fk[j];
        }
        if (bestp < 0) continue;
        const uint32_t bk = pairs[bestp].cand;
        const int32_t best_id = fr.ids[bk];
        fr.rep.best = (int32_t)bk;
        fr.rep.best_score = best_score;
        // finetune: the best frame and its neighbours in std::set order (rising key-frame id)
        std::vector<int32_t> nb;
        const int32_t best_kf = rkf[fr.ridx[bk]];
        for (int c : conn[best_kf]) {
            auto it = ref_index.find(c);
            if (it == ref_index.end()) { fr.rep.n_neighbours_skipped++; continue; }  // deviation 1: OM:189 would take frame 0
            nb.push_back(ref_ids[it->second]);
        }
        // deviation 4: a hub frame whose neighbourhood does not fit max_accum_points keeps the neighbours that fit, in set order
        uint64_t total = L->frames[best_id].n;
        size_t n_fit = 0;
        while (n_fit < nb.size() && total + L->frames[nb[n_fit]].n <= h->par.max_accum_points) total += L->frames[nb[n_fit++]].n;
        fr.rep.n_neighbours_dropped = (int32_t)(nb.size() - n_fit);
        nb.resize(n_fit);
        { Span sp(h, &h->tm.accumulate_us); rc = accumulate(h, best_id, nb.data(), (uint32_t)nb.size()); }
        if (rc < 0) return rc;
        fr.rep.n_accum = (uint32_t)rc;
        // Isometry3f(relative_pose).inverse(): R^T, -(R^T t) in f32
        float Rf[9], tf[3];
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) Rf[r * 3 + c] = (float)res[bestp].T[r * 4 + c]; tf[r] = (float)res[bestp].T[r * 4 + 3]; }
        double guess[16];
        for (int a = 0; a < 16; a++) guess[a] = (a % 5 == 0) ? 1.0 : 0.0;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) guess[r * 4 + c] = (double)Rf[c * 3 + r];
            const float v = (Rf[0 * 3 + r] * tf[0] + Rf[1 * 3 + r] * tf[1]) + Rf[2 * 3 + r] * tf[2];
            guess[r * 4 + 3] = (double)(-v);
        }
        const loop::Frame& nf = L->frames[new_ids[i]];
        double fT16[16];
        int fit = 0, fconv = 0;
        double fscore = DBL_MAX;
        {
            Span sp(h, &h->tm.fine_us);
            rc = gicp_adopt_cloud(h->fine, 1, nf.pts, nf.cov, nf.n);
            if (rc == LIO_OK) {
                lio_ndt_params p;  // select_registration_method("FAST_GICP") with OM:59-60
                lio_ndt_default_params(&p);
                p.rotation_epsilon_deg = L->par.fine_rotation_epsilon_deg;
                p.transformation_epsilon = h->par.fine_translation_epsilon;
                p.max_iterations = L->par.max_iterations;
                p.max_process_time_ms = -1;
                rc = lio_gicp_align(h->fine, guess, &p, h->par.fine_max_corr_dist, fT16, &fit, &fconv);
            }
            if (rc == LIO_OK && fconv) {
                const int32_t sid = new_ids[i];
                rc = gate_run(h, h->acc_pts, h->acc_n, &sid, fT16, 1, h->par.fitness_score_max_range, &fscore, nullptr, nullptr);
            }
        }
        if (rc != LIO_OK) return rc;
        fr.rep.fine_converged = fconv;
        fr.rep.fine_iterations = fit;
        if (!fconv) { fr.rep.reason = LIO_OVERLAP_FINE_NOT_CONVERGED; continue; }
        fr.rep.fine_score = fscore;
        if (fscore > h->par.fitness_score_thresh) { fr.rep.reason = LIO_OVERLAP_FINE_SCORE; continue; }
        fr.rep.reason = LIO_OVERLAP_FOUND;
        lio_overlap_edge e;
        memset(&e, 0, sizeof(e));
        e.key1 = best_id;
        e.key2 = new_ids[i];
        for (int a = 0; a < 16; a++) e.relative_pose[a] = (float)fT16[a];
        e.score = fscore;
        lio_loop_information_matrix(fscore, e.information);
        found.push_back(e);
    }
    if (found.size() > cap || (!found.empty() && !out)) return -(int)found.size();
    for (size_t k = 0; k < found.size(); k++) out[k] = found[k];
    return (int)found.size();
}

int lio_overlap_last_report(lio_overlap* h, uint32_t k, lio_overlap_report* report, int32_t* candidate_ids, double* gate_ratio, int32_t* converged, int32_t* iterations,
                            double* scores, uint32_t cap) {
    if (!h || k >= h->reports.size()) return LIO_E_INVALID;
    const FrameReport& fr = h->reports[k];
    if (report) *report = fr.rep;
    const size_t K = fr.ids.size();
    if (K > cap) return -(int)K;
    for (size_t j = 0; j < K; j++) {
        if (candidate_ids) candidate_ids[j] = fr.ids[j];
        if (gate_ratio) gate_ratio[j] = fr.ratio[j];
        if (converged) converged[j] = fr.conv[j];
        if (iterations) iterations[j] = fr.it[j];
        if (scores) scores[j] = fr.score[j];
    }
    return (int)K;
}

int lio_overlap_last_times(lio_overlap* h, lio_overlap_times* t) {
    if (!h || !t) return LIO_E_INVALID;
    *t = h->tm;
    return LIO_OK;
}

}  // extern "C"
