// loop_internal.h -- what loop.hip shares with overlap.hip: the records of the coarse batch and of the fitness launch, a bank frame, the
// detector's handle, and the host-side steps the overlap detector reuses on the same bank (scratch, a frame as the engine's target with its
// exact index, the fitness launch, the LM step's launch).  Internal: include/lio_hip.h keeps lio_loop opaque.
#pragma once
#include <vector>

#include "gicp_dev.h"
#include "knn_index_dev.h"

namespace lio {
namespace loop {

constexpr int kFitThreads = 256;
constexpr int kLookEvery = 6;  // rounds between two looks of the host at the slot states

struct LoopSlot {
    const float4* src;   // the candidate's cloud and covariances (bank)
    const double* scov;
    int32_t* corr;       // [n] voxel slot of the point at the last linearisation, -1: none
    double* maha;        // [n x 6]
    double* partial;     // [nb x kGicpAcc]
    uint32_t n, nb;
    double x0[16], xi[16], delta[16], H[36], b[6], d[6];
    double y0, lambda, nu;
    int32_t phase;       // 0: linearise at x0; 1: the cost of the trial xi on the pairs of x0; 2: done
    int32_t it, trial, conv, evals, it_done;
    uint32_t n_corr, pad;
};
struct LoopLmParams {
    int32_t max_iterations, lm_max_iterations;
    double rotation_epsilon_deg, transformation_epsilon, lm_init_lambda_factor;
};
struct FitSlot {
    const float4* src;
    uint32_t n, pad;
    float R[9], t[3];  // final_transformation_ (f32)
};

struct Frame {
    float4* pts = nullptr;  // one allocation: n float4 then 6 n doubles
    double* cov = nullptr;
    uint32_t n = 0;
    double pose[16];
    double accum = 0;
    bool retired = false;  // lio_loop_retire: the slot and its storage stay, the frame is never matched again
};

struct AlignOut {
    double T[16];
    int32_t iterations, converged;
    double score;
    uint32_t nr;
};

}  // namespace loop
}  // namespace lio

struct lio_loop {
    int device = 0;
    lio_loop_params par;
    lio_gicp* eng = nullptr;
    hipStream_t st = nullptr;
    std::vector<lio::loop::Frame> frames;
    size_t n_keyframes = 0;  // frames [0, n_keyframes) are `keyframes`, the rest the new_keyframes queue
    double last_edge_accum = 0.0;
    std::vector<lio_loop_edge> edges;
    // the target the engine holds
    int target_id = -1;
    lio::knn_index::DeviceIndex index;
    float4* idx_pts = nullptr;
    // batch scratch (grown geometrically, kept)
    lio::loop::LoopSlot *d_slots = nullptr, *h_slots = nullptr;
    lio::loop::FitSlot *d_fit = nullptr, *h_fit = nullptr;
    uint2 *d_tab = nullptr, *h_tab = nullptr;
    uint64_t tab_cap = 0, pts_cap = 0;
    int32_t* b_corr = nullptr;
    double *b_maha = nullptr, *b_partial = nullptr, *d_fitp = nullptr, *h_fitp = nullptr;
    // report of the last matching
    lio_loop_report rep;
    std::vector<int32_t> rep_ids, rep_conv, rep_it;
    std::vector<double> rep_score;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double t_insert = 0, t_target = 0, t_coarse = 0, t_fitness = 0, t_fine = 0;
};

namespace lio {
namespace loop {
// scratch for a batch of `pts` points in all and `tab` table entries (h->d_tab / h_tab, b_corr, b_maha, b_partial, d_fitp / h_fitp)
int loop_reserve(lio_loop* h, uint64_t pts, uint64_t tab);
// bank frame `id` as the engine's target: grid + covariances adopted, Gaussian voxels, the exact index; remembered in h->target_id
int loop_prepare_target(lio_loop* h, int id);
// getFitnessScore of n (source frame, f64 transform) pairs against the prepared target; max_range < 0: the detector's fitness_score_max_range
int loop_fitness_batch(lio_loop* h, const int32_t* src_ids, const double* T16, uint32_t n, double* score, uint32_t* nr, double max_range);
// loop_lm_step for slots [0, B) of d_slots on `st`
void loop_launch_lm_step(hipStream_t st, uint32_t B, LoopSlot* d_slots, const LoopLmParams& P);
}  // namespace loop
}  // namespace lio
