// loop.hip -- loop detection over the key frames on gfx950 (wave64): hdl_graph_slam::LoopDetector
// (slam/backend/hdl_graph_slam/include/hdl_graph_slam/loop_detector.hpp, "LD") up to the loop edge; include/lio_hip.h states the rules.
// The records, the handle and the steps overlap.hip reuses on the same bank are in loop_internal.h.
//
//   bank      a key frame is uploaded once, in the caller's order, into one allocation that lives as long as the frame; its covariances come
//             from the engine's source grid (gicp_cloud_covariances: hash grid + gicp_cov_kernel, the path of lio_gicp_set_source) and are kept
//             in the same order.  A grid's own order (arrival inside a cell) differs from one insertion to the next, so nothing is summed in it
//   target    the new frame adopted as the engine's target (gicp_adopt_cloud: no neighbour search), its Gaussian voxels (vgicp_build), and
//             knn_index_dev.h's tree over its points for the fitness
//   coarse    FAST_VGICP (DIRECT1) for all candidates at once.  A round = {loop_vgicp_eval<true> for the slots that linearise,
//             loop_vgicp_eval<false> for the slots that try a step, loop_lm_step}: a table workgroup -> (slot, first point) packs the slots of
//             different sizes into one launch; a workgroup whose slot is in the other phase leaves at once.  lsq.h's lsq_align runs per slot
//             as a state machine on the device; the host reads the slot states every kLookEvery rounds and rebuilds the table without the
//             finished slots.  Every slot folds its own workgroup partials in gicp_report_kernel's order: no atomics, no dependence on the
//             slot's place or neighbours.
//   fitness   getFitnessScore for all converged slots in one launch (table again), {sum, count} per 256 consecutive points of a slot, added
//             in order on the host
//   fine      FAST_GICP of the best candidate: the single-pair lio_gicp_align on the engine, the candidate adopted as its source
#include <cfloat>
#include <cmath>
#include <deque>
#include <vector>

#include "gicp_dev.h"
#include "knn_index_dev.h"
#include "loop_internal.h"
#include "lsq.h"

namespace lio {
namespace loop {

// FastVGICP::linearize (LIN: update_correspondences at x0 first, fast_vgicp_impl.hpp:72-180) / compute_error (:182-204) of the slot the table
// gives this workgroup; per point the arithmetic of vgicp_corr_kernel + vgicp_cost_kernel (gicp.hip), DIRECT1
template <bool LIN>
__global__ void __launch_bounds__(kGicpThreads) loop_vgicp_eval(const uint2* __restrict__ tab, LoopSlot* __restrict__ slots, const Slot* __restrict__ vtable,
                                                                uint32_t vmask, const VgicpVoxel* __restrict__ vox, double vres) {
    const uint2 tb = tab[blockIdx.x];
    const LoopSlot& s = slots[tb.x];
    if (s.phase != (LIN ? 0 : 1)) return;
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
            c = grid_find_slot(vtable, vmask, cx, cy, cz, ptr, cnt, slot) ? (int32_t)slot : -1;
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

// per slot: the workgroup partials folded as gicp_report_kernel folds them (component c by 32 lanes, lane l adds workgroups l, l + 32, ..., then a
// fixed xor tree), then one lane runs the step of lsq_align (lsq.h) the slot is at
__global__ void __launch_bounds__(1024) loop_lm_step(LoopSlot* __restrict__ slots, LoopLmParams P) {
    LoopSlot& s = slots[blockIdx.x];
    if (s.phase == 2) return;
    __shared__ double acc[kGicpAcc];
    const int tid = threadIdx.x, c = tid >> 5, l = tid & 31;
    double sum = 0.0;
    if (c < kGicpAcc)
        for (uint32_t b = l; b < s.nb; b += 32) sum += s.partial[(size_t)b * kGicpAcc + c];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (c < kGicpAcc && l == 0) acc[c] = sum;
    __syncthreads();
    if (tid != 0) return;
    lio_ndt_params p;
    p.max_iterations = P.max_iterations; p.lm_max_iterations = P.lm_max_iterations; p.rotation_epsilon_deg = P.rotation_epsilon_deg;
    p.transformation_epsilon = P.transformation_epsilon; p.lm_init_lambda_factor = P.lm_init_lambda_factor; p.max_process_time_ms = -1;
    s.evals++;
    bool make_trial = false, end_iteration = false;
    if (s.phase == 0) {  // linearize(x0): the head of computeTransformation's loop
        int t = 0;
        for (int r = 0; r < 6; r++)
            for (int cc = r; cc < 6; cc++) { s.H[r * 6 + cc] = acc[t]; s.H[cc * 6 + r] = acc[t]; t++; }
        for (int k = 0; k < 6; k++) s.b[k] = acc[21 + k];
        s.y0 = acc[27];
        s.n_corr = (uint32_t)(acc[28] + 0.5);
        s.it_done = s.it;
        if (s.lambda < 0.0) {
            double mx = 0;
            for (int i = 0; i < 6; i++) mx = fmax(mx, fabs(s.H[i * 7]));
            s.lambda = p.lm_init_lambda_factor * mx;
        }
        s.nu = 2.0;
        s.trial = 0;
        if (p.lm_max_iterations > 0) make_trial = true;
        else { s.phase = 2; s.conv = 0; }  // step_lm's loop does not run: "lm not converged!!"
    } else {  // compute_error(xi): step_lm
        const double yi = acc[27];
        double den = 0;
        for (int k = 0; k < 6; k++) den += s.d[k] * (s.lambda * s.d[k] - s.b[k]);
        const double rho = (s.y0 - yi) / den;
        if (rho < 0) {
            if (converged_h(p, s.delta, 10.0)) end_iteration = true;
            else {
                s.lambda = s.nu * s.lambda;
                s.nu = 2 * s.nu;
                s.trial++;
                if (s.trial >= p.lm_max_iterations) { s.phase = 2; s.conv = 0; }  // "lm not converged!!"
                else make_trial = true;
            }
        } else {
            for (int k = 0; k < 16; k++) s.x0[k] = s.xi[k];
            s.lambda = s.lambda * fmax(1.0 / 3.0, 1 - pow(2 * rho - 1, 3));
            end_iteration = true;
        }
    }
    if (end_iteration) {
        s.conv = converged_h(p, s.delta, 1.0) ? 1 : 0;
        s.it++;
        s.phase = (s.conv || s.it >= p.max_iterations) ? 2 : 0;
    }
    if (make_trial) {
        double A[36], nb6[6];
        for (int k = 0; k < 36; k++) A[k] = s.H[k] + ((k % 7 == 0) ? s.lambda : 0.0);
        for (int k = 0; k < 6; k++) nb6[k] = -s.b[k];
        if (!ldlt_solve6(A, nb6, s.d)) { s.phase = 2; s.conv = 0; }
        else {
            se3_exp_h(s.d, s.delta);
            mul44_h(s.delta, s.x0, s.xi);
            s.phase = 1;
        }
    }
}

// getFitnessScore: record (workgroup) = {sum of the gated squared distances, their number} of 256 consecutive points of the table's slot
__global__ void __launch_bounds__(kFitThreads) loop_fitness(const uint2* __restrict__ tab, const FitSlot* __restrict__ fs, const float4* __restrict__ leaves,
                                                            const float4* __restrict__ nodes, uint32_t nf, uint32_t P, int L, double max_range,
                                                            double* __restrict__ partial) {
    const uint2 tb = tab[blockIdx.x];
    const FitSlot& f = fs[tb.x];
    const uint32_t i = tb.y + threadIdx.x;
    double my_sum = 0.0;
    uint32_t my_cnt = 0;
    if (i < f.n) {
        const float4 p = f.src[i];
        // pcl::transformPointCloud with a Matrix4f: accumulated left to right (the rule of lio_ndt_overlap_score and of the keyframer)
        const float tx = ((f.R[0] * p.x + f.R[1] * p.y) + f.R[2] * p.z) + f.t[0];
        const float ty = ((f.R[3] * p.x + f.R[4] * p.y) + f.R[5] * p.z) + f.t[1];
        const float tz = ((f.R[6] * p.x + f.R[7] * p.y) + f.R[8] * p.z) + f.t[2];
        if (tx - tx == 0.f && ty - ty == 0.f && tz - tz == 0.f) {
            float kd[1] = {INFINITY};
            uint32_t ki[1] = {knn_index::kNone};
            knn_index::walk<1>(tx, ty, tz, nodes, leaves, nf, P, L, kd, ki);
            if (ki[0] != knn_index::kNone && (double)kd[0] <= max_range) { my_sum = (double)kd[0]; my_cnt = 1; }
        }
    }
    __shared__ double ssum[kFitThreads / 64];
    __shared__ uint32_t scnt[kFitThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { my_sum += __shfl_xor(my_sum, off); my_cnt += __shfl_xor(my_cnt, off); }
    if ((threadIdx.x & 63) == 0) { ssum[threadIdx.x >> 6] = my_sum; scnt[threadIdx.x >> 6] = my_cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
        partial[2 * blockIdx.x + 1] = (double)((scnt[0] + scnt[1]) + (scnt[2] + scnt[3]));
    }
}

// the target's points as the index takes them: {x, y, z, position bits}
__global__ void __launch_bounds__(256) loop_stamp(const float4* __restrict__ p, uint32_t n, float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 q = p[i];
    out[i] = make_float4(q.x, q.y, q.z, __uint_as_float(i));
}

}  // namespace loop
}  // namespace lio

using namespace lio;
using namespace lio::loop;

namespace {

struct Span {  // HIP events around a stretch of host-synchronous work
    lio_loop* h;
    double* acc;
    Span(lio_loop* h_, double* a) : h(h_), acc(a) { hipEventRecord(h->ev[0], h->st); }
    ~Span() {
        float ms = 0.f;
        if (hipEventRecord(h->ev[1], h->st) == hipSuccess && hipEventSynchronize(h->ev[1]) == hipSuccess && hipEventElapsedTime(&ms, h->ev[0], h->ev[1]) == hipSuccess)
            *acc += (double)ms * 1000.0;
    }
};

void reset_report(lio_loop* h) {
    memset(&h->rep, 0, sizeof(h->rep));
    h->rep.new_id = -1;
    h->rep.best = -1;
    h->rep.reason = LIO_LOOP_NO_CANDIDATE;
    h->rep.best_score = DBL_MAX;
    h->rep.fine_score = DBL_MAX;
    h->rep_ids.clear(); h->rep_conv.clear(); h->rep_it.clear(); h->rep_score.clear();
}

// Eigen::Quaterniond(R).normalized().toRotationMatrix() of the rotation of a row-major 4 x 4
void renormalise(const double T[16], double R[9]) {
    const double tr = T[0] + T[5] + T[10];
    double w, q[3];
    if (tr > 0) {
        double t = sqrt(tr + 1.0);
        w = 0.5 * t; t = 0.5 / t;
        q[0] = (T[9] - T[6]) * t; q[1] = (T[2] - T[8]) * t; q[2] = (T[4] - T[1]) * t;
    } else {
        int i = 0;
        if (T[5] > T[0]) i = 1;
        if (T[10] > T[i * 5]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = sqrt(T[i * 5] - T[j * 5] - T[k * 5] + 1.0);
        q[i] = 0.5 * t; t = 0.5 / t;
        w = (T[k * 4 + j] - T[j * 4 + k]) * t;
        q[j] = (T[j * 4 + i] + T[i * 4 + j]) * t;
        q[k] = (T[k * 4 + i] + T[i * 4 + k]) * t;
    }
    const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + w * w);
    const double qw = w / nrm, qx = q[0] / nrm, qy = q[1] / nrm, qz = q[2] / nrm;
    const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    const double M[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
    memcpy(R, M, sizeof(M));
}

// LD:168-173: (new^-1 * candidate).cast<float>(), guess(2, 3) = 0, handed to align() which casts it back
void make_guess(const double pn[16], const double pc[16], double g[16]) {
    double Rn[9], Rc[9];
    renormalise(pn, Rn);
    renormalise(pc, Rc);
    double ti[3];  // Isometry3d::inverse(): R^T, -(R^T t)
    for (int r = 0; r < 3; r++) ti[r] = -(Rn[0 * 3 + r] * pn[3] + Rn[1 * 3 + r] * pn[7] + Rn[2 * 3 + r] * pn[11]);
    for (int k = 0; k < 16; k++) g[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) g[r * 4 + c] = Rn[0 * 3 + r] * Rc[0 * 3 + c] + Rn[1 * 3 + r] * Rc[1 * 3 + c] + Rn[2 * 3 + r] * Rc[2 * 3 + c];
        g[r * 4 + 3] = (Rn[0 * 3 + r] * pc[3] + Rn[1 * 3 + r] * pc[7] + Rn[2 * 3 + r] * pc[11]) + ti[r];
    }
    for (int k = 0; k < 16; k++) g[k] = (double)(float)g[k];
    g[11] = 0.0;
}

bool params_ok(const lio_loop_params& p) {
    if (!(p.fitness_score_max_range > 0) || !(p.voxel_resolution > 0) || !(p.fine_max_corr_dist > 0) || !(p.coarse_translation_epsilon > 0) ||
        !(p.coarse_rotation_epsilon_deg > 0) || !(p.fine_translation_epsilon > 0) || !(p.fine_rotation_epsilon_deg > 0) || p.max_iterations < 0 ||
        p.k_correspondences < 3 || p.k_correspondences > kGicpMaxK || !(p.grid_resolution > 0.f) || p.max_points < (uint32_t)p.k_correspondences ||
        p.max_points > 0x00FFFFFFu || p.max_candidates < 1 || p.max_candidates > 4096) {
        set_error("lio_loop: ranges, resolutions and epsilons must be positive, 3 <= k <= %d, k <= max_points < 2^24, 1 <= max_candidates <= 4096", kGicpMaxK);
        return false;
    }
    return true;
}

template <typename T>
bool regrow(T** p, size_t n, bool host) {
    if (*p) { if (host) hipHostFree(*p); else hipFree(*p); *p = nullptr; }
    return (host ? hipHostMalloc(reinterpret_cast<void**>(p), n * sizeof(T), hipHostMallocDefault) : hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T))) == hipSuccess;
}

// scratch for a batch of `pts` points in all and `tab` table entries
int reserve(lio_loop* h, uint64_t pts, uint64_t tab) {
    if (pts > h->pts_cap) {
        uint64_t c = h->pts_cap ? h->pts_cap : 65536;
        while (c < pts) c *= 2;
        if (!regrow(&h->b_corr, c, false) || !regrow(&h->b_maha, c * 6, false)) { h->pts_cap = 0; set_error("lio_loop: no room for the batch's pairs"); return LIO_E_DEVICE; }
        h->pts_cap = c;
    }
    if (tab > h->tab_cap) {
        uint64_t c = h->tab_cap ? h->tab_cap : 1024;
        while (c < tab) c *= 2;
        if (!regrow(&h->d_tab, c, false) || !regrow(&h->h_tab, c, true) || !regrow(&h->b_partial, c * kGicpAcc, false) || !regrow(&h->d_fitp, c * 2, false) ||
            !regrow(&h->h_fitp, c * 2, true)) { h->tab_cap = 0; set_error("lio_loop: no room for the batch's table"); return LIO_E_DEVICE; }
        h->tab_cap = c;
    }
    return LIO_OK;
}

// the frame as the engine's target: grid + covariances adopted, Gaussian voxels, the exact index
int prepare_target(lio_loop* h, int id) {
    if (h->target_id == id) return LIO_OK;
    h->target_id = -1;
    const Frame& f = h->frames[id];
    int rc = gicp_adopt_cloud(h->eng, 0, f.pts, f.cov, f.n);
    if (rc != LIO_OK) return rc;
    rc = vgicp_build(h->eng);
    if (rc != LIO_OK) return rc;
    rc = knn_index::device_index_reserve(h->index, h->par.max_points);
    if (rc != LIO_OK) return rc;
    hipLaunchKernelGGL(loop_stamp, (f.n + 255) / 256, 256, 0, h->st, f.pts, f.n, h->idx_pts);
    LIO_HIP_TRY(hipGetLastError());
    rc = knn_index::device_index_build(h->st, h->index, h->idx_pts, nullptr, f.n);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipStreamSynchronize(h->st));
    h->target_id = id;
    return LIO_OK;
}

// getFitnessScore of n (source frame, f64 transform) pairs against the prepared target: one launch (per max_candidates pairs); max_range < 0: the
// detector's fitness_score_max_range
int fitness_batch(lio_loop* h, const int32_t* src_ids, const double* T16, uint32_t n, double* score, uint32_t* nr, double max_range = -1.0) {
    const Frame& tgt = h->frames[h->target_id];
    for (uint32_t base = 0; base < n; base += h->par.max_candidates) {
        const uint32_t B = n - base < h->par.max_candidates ? n - base : h->par.max_candidates;
        uint64_t nblocks = 0;
        for (uint32_t k = 0; k < B; k++) nblocks += (h->frames[src_ids[base + k]].n + kFitThreads - 1) / kFitThreads;
        int rc = reserve(h, 0, nblocks);
        if (rc != LIO_OK) return rc;
        uint32_t b = 0;
        for (uint32_t k = 0; k < B; k++) {
            const Frame& f = h->frames[src_ids[base + k]];
            const double* T = T16 + 16 * (size_t)(base + k);
            FitSlot& fs = h->h_fit[k];
            fs.src = f.pts; fs.n = f.n; fs.pad = 0;
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) fs.R[r * 3 + c] = (float)T[r * 4 + c]; fs.t[r] = (float)T[r * 4 + 3]; }
            for (uint32_t p0 = 0; p0 < f.n; p0 += kFitThreads) h->h_tab[b++] = make_uint2(k, p0);
        }
        LIO_HIP_TRY(hipMemcpyAsync(h->d_fit, h->h_fit, sizeof(FitSlot) * B, hipMemcpyHostToDevice, h->st));
        LIO_HIP_TRY(hipMemcpyAsync(h->d_tab, h->h_tab, sizeof(uint2) * b, hipMemcpyHostToDevice, h->st));
        hipLaunchKernelGGL(loop_fitness, b, kFitThreads, 0, h->st, h->d_tab, h->d_fit, h->index.leaves, h->index.nodes, tgt.n, h->index.P, h->index.L,
                           max_range < 0 ? h->par.fitness_score_max_range : max_range, h->d_fitp);
        LIO_HIP_TRY(hipGetLastError());
        LIO_HIP_TRY(hipMemcpyAsync(h->h_fitp, h->d_fitp, sizeof(double) * 2 * b, hipMemcpyDeviceToHost, h->st));
        LIO_HIP_TRY(hipStreamSynchronize(h->st));
        b = 0;
        for (uint32_t k = 0; k < B; k++) {
            double sum = 0.0, cnt = 0.0;
            for (uint32_t p0 = 0; p0 < h->frames[src_ids[base + k]].n; p0 += kFitThreads, b++) { sum += h->h_fitp[2 * b]; cnt += h->h_fitp[2 * b + 1]; }
            score[base + k] = cnt > 0 ? sum / cnt : DBL_MAX;
            nr[base + k] = (uint32_t)cnt;
        }
    }
    return LIO_OK;
}

// the coarse batch: n candidates against the prepared target from their guesses; out[k].score / nr are not touched
int coarse_batch(lio_loop* h, const int32_t* src_ids, const double* guesses, uint32_t n, AlignOut* out, int* rounds_out) {
    const lio_loop_params& par = h->par;
    lio_gicp* g = h->eng;
    if (par.max_iterations <= 0) {  // computeTransformation's loop does not run: the guess stands
        for (uint32_t k = 0; k < n; k++) { memcpy(out[k].T, guesses + 16 * k, sizeof(out[k].T)); out[k].iterations = out[k].converged = 0; }
        return LIO_OK;
    }
    lio_ndt_params dp;
    lio_ndt_default_params(&dp);
    const LoopLmParams P{par.max_iterations, dp.lm_max_iterations, par.coarse_rotation_epsilon_deg, par.coarse_translation_epsilon, dp.lm_init_lambda_factor};
    const double vres = (double)(float)par.voxel_resolution;
    for (uint32_t base = 0; base < n; base += par.max_candidates) {
        const uint32_t B = n - base < par.max_candidates ? n - base : par.max_candidates;
        uint64_t pts = 0, blocks = 0;
        for (uint32_t k = 0; k < B; k++) { const uint32_t m = h->frames[src_ids[base + k]].n; pts += m; blocks += (m + kGicpThreads - 1) / kGicpThreads; }
        int rc = reserve(h, pts, blocks);
        if (rc != LIO_OK) return rc;
        uint64_t po = 0, bo = 0;
        for (uint32_t k = 0; k < B; k++) {
            const Frame& f = h->frames[src_ids[base + k]];
            LoopSlot& s = h->h_slots[k];
            memset(&s, 0, sizeof(s));
            s.src = f.pts; s.scov = f.cov; s.n = f.n; s.nb = (f.n + kGicpThreads - 1) / kGicpThreads;
            s.corr = h->b_corr + po; s.maha = h->b_maha + po * 6; s.partial = h->b_partial + bo * kGicpAcc;
            po += f.n; bo += s.nb;
            memcpy(s.x0, guesses + 16 * (base + k), sizeof(s.x0));
            s.lambda = -1.0;
        }
        LIO_HIP_TRY(hipMemcpyAsync(h->d_slots, h->h_slots, sizeof(LoopSlot) * B, hipMemcpyHostToDevice, h->st));
        const int max_rounds = par.max_iterations * (dp.lm_max_iterations + 1) + 2;
        bool all_done = false;
        for (int r = 0; r < max_rounds && !all_done;) {
            uint32_t nt = 0;  // the table of the live slots
            for (uint32_t k = 0; k < B; k++)
                if (h->h_slots[k].phase != 2)
                    for (uint32_t p0 = 0; p0 < h->h_slots[k].n; p0 += kGicpThreads) h->h_tab[nt++] = make_uint2(k, p0);
            if (nt == 0) break;
            LIO_HIP_TRY(hipMemcpyAsync(h->d_tab, h->h_tab, sizeof(uint2) * nt, hipMemcpyHostToDevice, h->st));
            for (int k = 0; k < kLookEvery && r < max_rounds; k++, r++) {
                hipLaunchKernelGGL(loop_vgicp_eval<true>, nt, kGicpThreads, 0, h->st, h->d_tab, h->d_slots, g->vmap->table, g->vmap->table_mask, g->vvox, vres);
                hipLaunchKernelGGL(loop_vgicp_eval<false>, nt, kGicpThreads, 0, h->st, h->d_tab, h->d_slots, g->vmap->table, g->vmap->table_mask, g->vvox, vres);
                hipLaunchKernelGGL(loop_lm_step, B, 1024, 0, h->st, h->d_slots, P);
                if (rounds_out) (*rounds_out)++;
            }
            LIO_HIP_TRY(hipGetLastError());
            LIO_HIP_TRY(hipMemcpyAsync(h->h_slots, h->d_slots, sizeof(LoopSlot) * B, hipMemcpyDeviceToHost, h->st));
            LIO_HIP_TRY(hipStreamSynchronize(h->st));  // (the table in pinned memory is rewritten next: its copy has completed)
            all_done = true;
            for (uint32_t k = 0; k < B; k++)
                if (h->h_slots[k].phase != 2) all_done = false;
        }
        for (uint32_t k = 0; k < B; k++) {
            const LoopSlot& s = h->h_slots[k];
            if (s.phase != 2) { set_error("lio_loop: a slot of the coarse batch did not finish"); return LIO_E_STATE; }
            memcpy(out[base + k].T, s.x0, sizeof(s.x0));
            out[base + k].iterations = s.it_done;
            out[base + k].converged = s.conv;
        }
    }
    return LIO_OK;
}

int fine_align(lio_loop* h, int src_id, const double guess[16], AlignOut* o) {
    const lio_loop_params& par = h->par;
    const Frame& f = h->frames[src_id];
    int rc = gicp_adopt_cloud(h->eng, 1, f.pts, f.cov, f.n);
    if (rc != LIO_OK) return rc;
    lio_ndt_params p;  // select_registration_method("FAST_GICP"), registrations.cpp:33-42
    lio_ndt_default_params(&p);
    p.rotation_epsilon_deg = par.fine_rotation_epsilon_deg;
    p.transformation_epsilon = par.fine_translation_epsilon;
    p.max_iterations = par.max_iterations;
    p.max_process_time_ms = -1;
    const double vr = h->eng->voxel_res;
    h->eng->voxel_res = 0.0;  // the kd-tree form on the same target (its voxels stay valid)
    int it = 0, conv = 0;
    rc = lio_gicp_align(h->eng, guess, &p, par.fine_max_corr_dist, o->T, &it, &conv);
    h->eng->voxel_res = vr;
    o->iterations = it;
    o->converged = conv;
    return rc;
}

// matching (LD:148-219) of new frame `id` against `cand`; a loop goes to h->edges and *found
int matching(lio_loop* h, int id, const std::vector<int32_t>& cand, bool* found) {
    *found = false;
    reset_report(h);
    h->rep.new_id = id;
    h->rep.n_candidates = (int32_t)cand.size();
    h->rep_ids = cand;
    const size_t K = cand.size();
    h->rep_conv.assign(K, 0); h->rep_it.assign(K, 0); h->rep_score.assign(K, DBL_MAX);
    if (cand.empty()) return LIO_OK;
    h->rep.reason = LIO_LOOP_COARSE_SCORE;
    const Frame& nf = h->frames[id];
    int rc;
    { Span sp(h, &h->t_target); rc = prepare_target(h, id); }
    if (rc != LIO_OK) return rc;
    std::vector<double> guesses(16 * K);
    for (size_t k = 0; k < K; k++) make_guess(nf.pose, h->frames[cand[k]].pose, &guesses[16 * k]);
    std::vector<AlignOut> res(K);
    { Span sp(h, &h->t_coarse); rc = coarse_batch(h, cand.data(), guesses.data(), (uint32_t)K, res.data(), &h->rep.coarse_rounds); }
    if (rc != LIO_OK) return rc;
    // the fitness of every converged candidate, the final transformation as the f32 matrix getFinalTransformation returns
    std::vector<int32_t> fid, fk;
    std::vector<double> fT;
    for (size_t k = 0; k < K; k++) {
        h->rep_conv[k] = res[k].converged; h->rep_it[k] = res[k].iterations;
        if (!res[k].converged) continue;
        fid.push_back(cand[k]); fk.push_back((int32_t)k);
        fT.insert(fT.end(), res[k].T, res[k].T + 16);
    }
    std::vector<double> fs(fid.size());
    std::vector<uint32_t> fn(fid.size());
    { Span sp(h, &h->t_fitness); rc = fitness_batch(h, fid.data(), fT.data(), (uint32_t)fid.size(), fs.data(), fn.data()); }
    if (rc != LIO_OK) return rc;
    double best_score = DBL_MAX;
    int best = -1;
    for (size_t j = 0; j < fid.size(); j++) {
        h->rep_score[fk[j]] = fs[j];
        if (fs[j] > best_score) continue;
        best_score = fs[j];
        best = fk[j];
    }
    h->rep.best = best;
    h->rep.best_score = best_score;
    if (best_score > 2.0 * h->par.fitness_score_thresh || best < 0) return LIO_OK;
    double guess[16];
    for (int k = 0; k < 16; k++) guess[k] = (double)(float)res[best].T[k];  // relative_pose is a Matrix4f
    AlignOut fo;
    {
        Span sp(h, &h->t_fine);
        rc = fine_align(h, cand[best], guess, &fo);
        if (rc == LIO_OK) { const int32_t sid = cand[best]; rc = fitness_batch(h, &sid, fo.T, 1, &fo.score, &fo.nr); }
    }
    if (rc != LIO_OK) return rc;
    h->rep.fine_converged = fo.converged;
    h->rep.fine_iterations = fo.iterations;
    if (!fo.converged) { h->rep.reason = LIO_LOOP_FINE_NOT_CONVERGED; return LIO_OK; }
    h->rep.fine_score = fo.score;
    if (fo.score > h->par.fitness_score_thresh) { h->rep.reason = LIO_LOOP_FINE_SCORE; return LIO_OK; }
    h->rep.reason = LIO_LOOP_FOUND;
    h->last_edge_accum = nf.accum;
    lio_loop_edge e;
    memset(&e, 0, sizeof(e));
    e.key1 = id;
    e.key2 = cand[best];
    for (int k = 0; k < 16; k++) e.relative_pose[k] = (float)fo.T[k];
    e.score = fo.score;
    lio_loop_information_matrix(fo.score, e.information);
    h->edges.push_back(e);
    *found = true;
    return LIO_OK;
}

void free_frames(lio_loop* h) {
    for (Frame& f : h->frames)
        if (f.pts) hipFree(f.pts);
    h->frames.clear();
}

bool id_ok(lio_loop* h, int id) { return h && id >= 0 && (size_t)id < h->frames.size(); }
bool live_ok(lio_loop* h, int id) { return id_ok(h, id) && !h->frames[id].retired; }  // a retired frame is no longer matched: to the matchers it is unknown

}  // namespace

namespace lio {
namespace loop {
int loop_reserve(lio_loop* h, uint64_t pts, uint64_t tab) { return reserve(h, pts, tab); }
int loop_prepare_target(lio_loop* h, int id) { return prepare_target(h, id); }

// what lio_gicp_fitness_score keeps on a matcher handle: the exact index over its target and the scratch of one fitness launch
struct GicpFit {
    knn_index::DeviceIndex index;
    FitSlot *d_fit = nullptr, *h_fit = nullptr;
    uint2 *d_tab = nullptr, *h_tab = nullptr;
    double *d_p = nullptr, *h_p = nullptr;
};
}  // namespace loop
void gicp_fit_free(lio_gicp* g) {
    loop::GicpFit* f = static_cast<loop::GicpFit*>(g->fit);
    if (!f) return;
    knn_index::device_index_free(f->index);
    hipFree(f->d_fit); hipFree(f->d_tab); hipFree(f->d_p);
    if (f->h_fit) hipHostFree(f->h_fit);
    if (f->h_tab) hipHostFree(f->h_tab);
    if (f->h_p) hipHostFree(f->h_p);
    delete f;
    g->fit = nullptr;
    g->fit_valid = false;
}
namespace loop {
int loop_fitness_batch(lio_loop* h, const int32_t* src_ids, const double* T16, uint32_t n, double* score, uint32_t* nr, double max_range) {
    return fitness_batch(h, src_ids, T16, n, score, nr, max_range);
}
void loop_launch_lm_step(hipStream_t st, uint32_t B, LoopSlot* d_slots, const LoopLmParams& P) { hipLaunchKernelGGL(loop_lm_step, B, 1024, 0, st, d_slots, P); }
}  // namespace loop
}  // namespace lio

extern "C" {

void lio_loop_default_params(lio_loop_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->distance_thresh = 15.0;
    p->accum_distance_thresh = 25.0;
    p->distance_from_last_edge_thresh = 15.0;
    p->distance_new_keyframe_thresh = 2.0;
    p->distance_keyframe_thresh = 2.0;
    p->fitness_score_max_range = 25.0;
    p->fitness_score_thresh = 1.5;
    p->fine_max_corr_dist = 0.5;
    p->voxel_resolution = 1.0;
    p->coarse_translation_epsilon = 0.1;
    p->coarse_rotation_epsilon_deg = 0.1;
    p->fine_translation_epsilon = 0.01;
    p->fine_rotation_epsilon_deg = 1e-2;
    p->max_iterations = 64;
    p->k_correspondences = 20;
    p->grid_resolution = 1.0f;
    p->max_points = 65536;
    p->max_candidates = 64;
}

int lio_loop_find_candidates(const double* accum, const double* pos_xy, uint32_t n, double new_accum, const double new_xy[2], double last_edge_accum,
                             const lio_loop_params* params, int32_t* out_idx, uint32_t cap) {
    if ((n && (!accum || !pos_xy)) || !new_xy) return LIO_E_INVALID;
    lio_loop_params p;
    if (params) p = *params; else lio_loop_default_params(&p);
    if (new_accum - last_edge_accum < p.distance_from_last_edge_thresh) return 0;  // too close to the last registered loop edge
    uint32_t count = 0;
    double accum_distance_keyframe = -100.0;
    for (uint32_t i = 0; i < n; i++) {
        if (new_accum - accum[i] < p.accum_distance_thresh) continue;
        if ((accum[i] - accum_distance_keyframe) < p.distance_keyframe_thresh) continue;
        const double dx = pos_xy[2 * i] - new_xy[0], dy = pos_xy[2 * i + 1] - new_xy[1];
        const double dist = sqrt(dx * dx + dy * dy);
        if (dist > p.distance_thresh) continue;
        accum_distance_keyframe = accum[i];
        if (out_idx && count < cap) out_idx[count] = (int32_t)i;
        count++;
    }
    return (count > cap || (count && !out_idx)) ? -(int)count : (int)count;
}

// getFitnessScore(max_range) of the matcher's own pair: loop_fitness over the source in the caller's order against an exact index over the
// target, the records added as fitness_batch adds them -- for a pair of bank frames the loop detector's numbers
int lio_gicp_fitness_score(lio_gicp* g, const double T[16], double max_range, double* score, uint32_t* nr) {
    if (!g || !T || !score || !(max_range >= 0)) return LIO_E_INVALID;
    for (int k = 0; k < 12; k++)
        if (!(T[k] - T[k] == 0.0)) { set_error("lio_gicp_fitness_score: the transform is not finite"); return LIO_E_INVALID; }
    if (!g->grid[0] || !g->grid[1] || g->n[0] == 0 || g->n[1] == 0) { set_error("lio_gicp_fitness_score: set target and source first"); return LIO_E_STATE; }
    if (g->src_order == 0) { set_error("lio_gicp_fitness_score: the source's own order was not kept (set it with lio_gicp_set_source)"); return LIO_E_STATE; }
    hipSetDevice(g->device);
    hipStream_t st = g->grid[0]->stream;
    GicpFit* f = static_cast<GicpFit*>(g->fit);
    const uint32_t max_blocks = (g->max_points + kFitThreads - 1) / kFitThreads;
    if (!f) {
        f = new GicpFit();
        g->fit = f;
        const bool ok = hipMalloc(reinterpret_cast<void**>(&f->d_fit), sizeof(FitSlot)) == hipSuccess && hipHostMalloc(reinterpret_cast<void**>(&f->h_fit), sizeof(FitSlot), hipHostMallocDefault) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void**>(&f->d_tab), sizeof(uint2) * max_blocks) == hipSuccess && hipHostMalloc(reinterpret_cast<void**>(&f->h_tab), sizeof(uint2) * max_blocks, hipHostMallocDefault) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void**>(&f->d_p), sizeof(double) * 2 * max_blocks) == hipSuccess && hipHostMalloc(reinterpret_cast<void**>(&f->h_p), sizeof(double) * 2 * max_blocks, hipHostMallocDefault) == hipSuccess;
        if (!ok) { (void)hipGetLastError(); gicp_fit_free(g); set_error("lio_gicp_fitness_score: allocation failed"); return LIO_E_DEVICE; }
    }
    const uint32_t nt = g->n[0], ns = g->n[1];
    if (!g->fit_valid) {
        int rc = knn_index::device_index_reserve(f->index, g->max_points);
        if (rc != LIO_OK) return rc;
        hipLaunchKernelGGL(loop_stamp, (nt + 255) / 256, 256, 0, st, g->grid[0]->pool, nt, g->stage);  // the index copies what it is given
        LIO_HIP_TRY(hipGetLastError());
        rc = knn_index::device_index_build(st, f->index, g->stage, nullptr, nt);
        if (rc != LIO_OK) return rc;
        g->fit_valid = true;
    }
    FitSlot& fs = *f->h_fit;
    fs.src = g->src_order == 1 ? g->src_rows : g->grid[1]->pool;
    fs.n = ns; fs.pad = 0;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) fs.R[r * 3 + c] = (float)T[r * 4 + c]; fs.t[r] = (float)T[r * 4 + 3]; }
    uint32_t b = 0;
    for (uint32_t p0 = 0; p0 < ns; p0 += kFitThreads) f->h_tab[b++] = make_uint2(0, p0);
    LIO_HIP_TRY(hipMemcpyAsync(f->d_fit, f->h_fit, sizeof(FitSlot), hipMemcpyHostToDevice, st));
    LIO_HIP_TRY(hipMemcpyAsync(f->d_tab, f->h_tab, sizeof(uint2) * b, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(loop_fitness, b, kFitThreads, 0, st, f->d_tab, f->d_fit, f->index.leaves, f->index.nodes, nt, f->index.P, f->index.L, max_range, f->d_p);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipMemcpyAsync(f->h_p, f->d_p, sizeof(double) * 2 * b, hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    double sum = 0.0, cnt = 0.0;
    for (uint32_t k = 0; k < b; k++) { sum += f->h_p[2 * k]; cnt += f->h_p[2 * k + 1]; }
    *score = cnt > 0 ? sum / cnt : DBL_MAX;
    if (nr) *nr = (uint32_t)cnt;
    return LIO_OK;
}

int lio_loop_information_matrix(double fitness_score, double out36[36]) {
    if (!out36) return LIO_E_INVALID;
    const double var_gain_a = 20.0, min_stddev_x = 0.1, max_stddev_x = 5.0, min_stddev_q = 0.05, max_stddev_q = 0.2, thresh = 0.5;
    const double min_var_x = pow(min_stddev_x, 2), max_var_x = pow(max_stddev_x, 2), min_var_q = pow(min_stddev_q, 2), max_var_q = pow(max_stddev_q, 2);
    auto weight = [](double a, double max_x, double min_y, double max_y, double x) {
        const double y = (1.0 - exp(-a * x)) / (1.0 - exp(-a * max_x));
        return min_y + (max_y - min_y) * y;
    };
    const float w_x = (float)weight(var_gain_a, thresh, min_var_x, max_var_x, fitness_score);
    const float w_q = (float)weight(var_gain_a, thresh, min_var_q, max_var_q, fitness_score);
    for (int k = 0; k < 36; k++) out36[k] = 0.0;
    for (int i = 0; i < 3; i++) { out36[i * 7] = 1.0 / (double)w_x; out36[(i + 3) * 7] = 1.0 / (double)w_q; }
    return LIO_OK;
}

lio_loop* lio_loop_create(int device, const lio_loop_params* params) {
    lio_loop_params p;
    if (params) p = *params; else lio_loop_default_params(&p);
    if (!params_ok(p)) return nullptr;
    if (hipSetDevice(device) != hipSuccess) { set_error("lio_loop_create: no HIP device %d (this library has no CPU fallback)", device); return nullptr; }
    lio_loop* h = new lio_loop();
    h->device = device;
    h->par = p;
    reset_report(h);
    h->eng = lio_gicp_create(device, p.grid_resolution, p.max_points, p.k_correspondences);
    bool ok = h->eng && lio_gicp_set_voxel_mode(h->eng, p.voxel_resolution, 1) == LIO_OK && hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreate(&h->ev[0]) == hipSuccess && hipEventCreate(&h->ev[1]) == hipSuccess &&
              hipMalloc(reinterpret_cast<void**>(&h->idx_pts), (size_t)p.max_points * sizeof(float4)) == hipSuccess &&
              hipMalloc(reinterpret_cast<void**>(&h->d_slots), sizeof(LoopSlot) * p.max_candidates) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void**>(&h->h_slots), sizeof(LoopSlot) * p.max_candidates, hipHostMallocDefault) == hipSuccess &&
              hipMalloc(reinterpret_cast<void**>(&h->d_fit), sizeof(FitSlot) * p.max_candidates) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void**>(&h->h_fit), sizeof(FitSlot) * p.max_candidates, hipHostMallocDefault) == hipSuccess;
    if (!ok) {
        if (h->eng) set_error("lio_loop_create: allocation failed");
        lio_loop_destroy(h);
        return nullptr;
    }
    return h;
}

void lio_loop_destroy(lio_loop* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->st) hipStreamSynchronize(h->st);
    free_frames(h);
    if (h->eng) lio_gicp_destroy(h->eng);
    knn_index::device_index_free(h->index);
    hipFree(h->idx_pts); hipFree(h->d_slots); hipFree(h->d_fit); hipFree(h->d_tab); hipFree(h->b_corr); hipFree(h->b_maha); hipFree(h->b_partial); hipFree(h->d_fitp);
    if (h->h_slots) hipHostFree(h->h_slots);
    if (h->h_fit) hipHostFree(h->h_fit);
    if (h->h_tab) hipHostFree(h->h_tab);
    if (h->h_fitp) hipHostFree(h->h_fitp);
    for (int i = 0; i < 2; i++)
        if (h->ev[i]) hipEventDestroy(h->ev[i]);
    if (h->st) hipStreamDestroy(h->st);
    delete h;
}

int lio_loop_reset(lio_loop* h) {
    if (!h) return LIO_E_INVALID;
    hipSetDevice(h->device);
    LIO_HIP_TRY(hipStreamSynchronize(h->st));
    free_frames(h);
    h->n_keyframes = 0;
    h->last_edge_accum = 0.0;
    h->edges.clear();
    h->target_id = -1;
    reset_report(h);
    h->t_insert = h->t_target = h->t_coarse = h->t_fitness = h->t_fine = 0;
    return LIO_OK;
}

int lio_loop_add_keyframe_host(lio_loop* h, const float* xyzi, uint32_t n, const double pose[16], double accum_distance) {
    if (!h || !pose || (!xyzi && n)) return LIO_E_INVALID;
    hipSetDevice(h->device);
    if ((int)n < h->par.k_correspondences) {  // (said as a warning too: a caller that feeds every key frame passes such a frame over and goes on)
        set_warning("lio_loop: key frame of %u points left out (a frame needs at least k = %d)", n, h->par.k_correspondences);
        set_error("lio_loop_add_keyframe_host: a key frame needs at least k = %d points", h->par.k_correspondences);
        return LIO_E_INVALID;
    }
    h->t_insert = 0;
    Span sp(h, &h->t_insert);
    if (n > h->par.max_points) { set_error("lio_loop_add_keyframe_host: key frame of %u points exceeds max_points %u", n, h->par.max_points); return LIO_E_CAPACITY; }
    Frame f;
    const size_t bytes = (size_t)n * (sizeof(float4) + 6 * sizeof(double));
    if (hipMalloc(reinterpret_cast<void**>(&f.pts), bytes) != hipSuccess) { set_error("lio_loop_add_keyframe_host: no room for a frame of %u points", n); return LIO_E_DEVICE; }
    f.cov = reinterpret_cast<double*>(f.pts + n);
    f.n = n;
    memcpy(f.pose, pose, sizeof(f.pose));
    f.accum = accum_distance;
    // the cloud stays in the caller's order: a grid's pool order is the points' arrival order inside a cell and differs from one insertion to
    // the next, and every sum over a frame (cost, fitness, voxel fold) runs in the frame's order
    hipError_t e = hipMemcpyAsync(f.pts, xyzi, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->st);
    if (e == hipSuccess) e = hipStreamSynchronize(h->st);
    if (e != hipSuccess) { hipFree(f.pts); set_error("lio_loop_add_keyframe_host: %s", hipGetErrorString(e)); return LIO_E_DEVICE; }
    const int rc = gicp_cloud_covariances(h->eng, 1, f.pts, n, f.cov);
    if (rc != LIO_OK) { hipFree(f.pts); return rc; }
    h->frames.push_back(f);
    return (int)h->frames.size() - 1;
}

int lio_loop_set_pose(lio_loop* h, int id, const double pose[16]) {
    if (!id_ok(h, id) || !pose) return LIO_E_INVALID;
    memcpy(h->frames[id].pose, pose, sizeof(h->frames[id].pose));
    return LIO_OK;
}

int lio_loop_retire(lio_loop* h, int frame) {
    if (!live_ok(h, frame)) return LIO_E_INVALID;
    h->frames[frame].retired = true;
    return LIO_OK;
}

int lio_loop_num_keyframes(lio_loop* h, int* n_queued) {
    if (!h) return LIO_E_INVALID;
    if (n_queued) *n_queued = (int)(h->frames.size() - h->n_keyframes);
    return (int)h->frames.size();
}

int lio_loop_download_keyframe(lio_loop* h, int id, float* xyzi, double* cov6, uint32_t cap) {
    if (!id_ok(h, id)) return LIO_E_INVALID;
    const Frame& f = h->frames[id];
    if (f.n > cap) return -(int)f.n;
    hipSetDevice(h->device);
    if (xyzi) LIO_HIP_TRY(hipMemcpy(xyzi, f.pts, (size_t)f.n * sizeof(float4), hipMemcpyDeviceToHost));
    if (cov6) LIO_HIP_TRY(hipMemcpy(cov6, f.cov, (size_t)f.n * 6 * sizeof(double), hipMemcpyDeviceToHost));
    return (int)f.n;
}

int lio_loop_detect(lio_loop* h, lio_loop_edge* out_loops, uint32_t cap) {
    if (!h) return LIO_E_INVALID;
    hipSetDevice(h->device);
    h->t_target = h->t_coarse = h->t_fitness = h->t_fine = 0;
    const size_t first_edge = h->edges.size();
    double accum_distance_new_keyframe = 0;
    std::vector<double> accum(h->n_keyframes), xy(2 * h->n_keyframes);
    std::vector<int32_t> cand, kept(h->n_keyframes);
    for (size_t id = h->n_keyframes; id < h->frames.size(); id++) {
        const Frame& f = h->frames[id];
        if (f.retired) continue;  // neither a new frame nor, below, a candidate: the search runs as if the frame had never been there
        if ((f.accum - accum_distance_new_keyframe) < h->par.distance_new_keyframe_thresh) continue;
        accum_distance_new_keyframe = f.accum;
        uint32_t nk = 0;
        for (size_t k = 0; k < h->n_keyframes; k++) {
            if (h->frames[k].retired) continue;
            accum[nk] = h->frames[k].accum; xy[2 * nk] = h->frames[k].pose[3]; xy[2 * nk + 1] = h->frames[k].pose[7];
            kept[nk++] = (int32_t)k;
        }
        cand.assign(nk, 0);
        const double nxy[2] = {f.pose[3], f.pose[7]};
        const int nc = lio_loop_find_candidates(accum.data(), xy.data(), nk, f.accum, nxy, h->last_edge_accum, &h->par, cand.data(), nk);
        cand.resize(nc > 0 ? nc : 0);
        for (int32_t& c : cand) c = kept[c];
        bool found = false;
        const int rc = matching(h, (int)id, cand, &found);
        if (rc != LIO_OK) {  // a device error: the queue is emptied all the same (the frame that failed and those behind it become key frames that
                             // were never matched), so a repeated call cannot match the same frames again against the state this one changed
            h->n_keyframes = h->frames.size();
            return rc;
        }
    }
    h->n_keyframes = h->frames.size();
    const size_t count = h->edges.size() - first_edge;
    if (count > cap || (count && !out_loops)) return -(int)count;
    for (size_t k = 0; k < count; k++) out_loops[k] = h->edges[first_edge + k];
    return (int)count;
}

int lio_loop_edges(lio_loop* h, lio_loop_edge* out, uint32_t cap) {
    if (!h) return LIO_E_INVALID;
    const size_t count = h->edges.size();
    if (count > cap || (count && !out)) return -(int)count;
    for (size_t k = 0; k < count; k++) out[k] = h->edges[k];
    return (int)count;
}

int lio_loop_last_report(lio_loop* h, lio_loop_report* report, int32_t* candidate_ids, int32_t* converged, int32_t* iterations, double* scores, uint32_t cap) {
    if (!h) return LIO_E_INVALID;
    if (report) *report = h->rep;
    const size_t K = h->rep_ids.size();
    if (K > cap) return -(int)K;
    for (size_t k = 0; k < K; k++) {
        if (candidate_ids) candidate_ids[k] = h->rep_ids[k];
        if (converged) converged[k] = h->rep_conv[k];
        if (iterations) iterations[k] = h->rep_it[k];
        if (scores) scores[k] = h->rep_score[k];
    }
    return (int)K;
}

int lio_loop_last_times(lio_loop* h, double* insert_us, double* target_us, double* coarse_us, double* fitness_us, double* fine_us) {
    if (!h) return LIO_E_INVALID;
    if (insert_us) *insert_us = h->t_insert;
    if (target_us) *target_us = h->t_target;
    if (coarse_us) *coarse_us = h->t_coarse;
    if (fitness_us) *fitness_us = h->t_fitness;
    if (fine_us) *fine_us = h->t_fine;
    return LIO_OK;
}

int lio_loop_align_candidates(lio_loop* h, int target_id, const int32_t* source_ids, uint32_t n, const double* guesses, double* out_T, int32_t* iterations,
                              int32_t* converged, double* scores, uint32_t* nr) {
    if (!live_ok(h, target_id) || (n && (!source_ids || !guesses))) return LIO_E_INVALID;
    for (uint32_t k = 0; k < n; k++)
        if (!live_ok(h, source_ids[k])) return LIO_E_INVALID;
    if (n == 0) return LIO_OK;
    hipSetDevice(h->device);
    h->t_target = h->t_coarse = h->t_fitness = h->t_fine = 0;
    int rc;
    { Span sp(h, &h->t_target); rc = prepare_target(h, target_id); }
    if (rc != LIO_OK) return rc;
    std::vector<AlignOut> res(n);
    { Span sp(h, &h->t_coarse); rc = coarse_batch(h, source_ids, guesses, n, res.data(), nullptr); }
    if (rc != LIO_OK) return rc;
    std::vector<int32_t> fid, fk;
    std::vector<double> fT;
    for (uint32_t k = 0; k < n; k++) {
        if (!res[k].converged) continue;
        fid.push_back(source_ids[k]); fk.push_back((int32_t)k);
        fT.insert(fT.end(), res[k].T, res[k].T + 16);
    }
    std::vector<double> fs(fid.size());
    std::vector<uint32_t> fn(fid.size());
    { Span sp(h, &h->t_fitness); rc = fitness_batch(h, fid.data(), fT.data(), (uint32_t)fid.size(), fs.data(), fn.data()); }
    if (rc != LIO_OK) return rc;
    for (uint32_t k = 0; k < n; k++) {
        if (out_T) memcpy(out_T + 16 * k, res[k].T, sizeof(res[k].T));
        if (iterations) iterations[k] = res[k].iterations;
        if (converged) converged[k] = res[k].converged;
        if (scores) scores[k] = DBL_MAX;
        if (nr) nr[k] = 0;
    }
    for (size_t j = 0; j < fid.size(); j++) {
        if (scores) scores[fk[j]] = fs[j];
        if (nr) nr[fk[j]] = fn[j];
    }
    return LIO_OK;
}

int lio_loop_align_fine(lio_loop* h, int target_id, int source_id, const double guess[16], double out_T[16], int32_t* iterations, int32_t* converged, double* score,
                        uint32_t* nr) {
    if (!live_ok(h, target_id) || !live_ok(h, source_id) || !guess) return LIO_E_INVALID;
    hipSetDevice(h->device);
    int rc = prepare_target(h, target_id);
    if (rc != LIO_OK) return rc;
    AlignOut fo;
    h->t_fine = 0;
    Span sp(h, &h->t_fine);
    rc = fine_align(h, source_id, guess, &fo);
    if (rc != LIO_OK) return rc;
    const int32_t sid = source_id;
    rc = fitness_batch(h, &sid, fo.T, 1, &fo.score, &fo.nr);
    if (rc != LIO_OK) return rc;
    if (out_T) memcpy(out_T, fo.T, sizeof(fo.T));
    if (iterations) *iterations = fo.iterations;
    if (converged) *converged = fo.converged;
    if (score) *score = fo.score;
    if (nr) *nr = fo.nr;
    return LIO_OK;
}

int lio_loop_pair_information(lio_loop* h, int id1, int id2, const double relpose[16], double* score, uint32_t* nr, double info36[36]) {
    if (!live_ok(h, id1) || !live_ok(h, id2) || !relpose) return LIO_E_INVALID;
    hipSetDevice(h->device);
    int rc = prepare_target(h, id1);
    if (rc != LIO_OK) return rc;
    const int32_t sid = id2;
    double sc = DBL_MAX;
    uint32_t n = 0;
    rc = fitness_batch(h, &sid, relpose, 1, &sc, &n, DBL_MAX);  // calc_fitness_score's max_range = std::numeric_limits<double>::max()
    if (rc != LIO_OK) return rc;
    if (score) *score = sc;
    if (nr) *nr = n;
    if (info36) return lio_loop_information_matrix(sc, info36);
    return LIO_OK;
}

}  // extern "C"
