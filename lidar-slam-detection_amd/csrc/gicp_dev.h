// gicp_dev.h -- what gicp.hip shares with loop.hip: the transform / voxel records its kernels take, the device helpers of the voxelised cost
// (voxel lookup, f64 transform, Mahalanobis matrix), the matcher handle, and the host-side steps the loop detector reuses on its key-frame
// bank (cloud + covariances, the Gaussian voxels of a target, a cloud adopted together with covariances computed earlier).  Internal.
#pragma once
#include "hashgrid.h"
#include "lio_common.h"

namespace lio {

constexpr int kGicpThreads = 128;
constexpr int kGicpMaxK = 32;
constexpr int kGicpAcc = 29;  // 21 H (upper), 6 b, err, count

struct GicpXform {
    double R[9], t[3];   // trans (double)
    float Rf[9], tf[3];  // trans.cast<float>()
};

__device__ inline bool grid_find_slot(const Slot* __restrict__ table, uint32_t mask, int cx, int cy, int cz, uint32_t& ptr, uint32_t& cnt, uint32_t& slot) {
    const unsigned long long want = pack_key(cx, cy, cz);
    BrickProbe bp = brick_probe(cx, cy, cz);
    for (uint32_t probe = 0; probe <= (mask >> 6); probe++) {
        const uint32_t h = brick_slot(bp, mask);
        const Slot sl = table[h];
        if (sl.key == want) { ptr = sl.ptr; cnt = sl.cnt; slot = h; return cnt > 0; }
        if (sl.key == kEmptyKey) return false;
        brick_next(bp);
    }
    return false;
}

// ---- the voxelised variant: fast_gicp::FastVGICP (fast_vgicp_impl.hpp:72-204, fast_vgicp_voxel.hpp:125-182) ----------------------------
// Target = Gaussian voxels of `voxel_resolution` (key floor(x / res - 0.5) in f64): mean of the points' positions and mean of their
// (regularised, 20-NN) covariances, ADDITIVE mode; a source point corresponds to the voxel(s) its transformed position falls in (DIRECT1:
// that voxel; DIRECT7 / 27: its neighbours too), weight sqrt(points in the voxel), Mahalanobis matrix (C_voxel + R C_A R^T)^-1.
struct __attribute__((aligned(16))) VgicpVoxel {
    double mean[3];
    double cov[6];
    double n;
};
struct VgicpOffsets {
    int n;
    int off[27][3];
};

__device__ inline void gicp_transform_d(const GicpXform& X, const float4 a, double ta[3]) {
    const double ax = (double)a.x, ay = (double)a.y, az = (double)a.z;
    ta[0] = (X.R[0] * ax + X.R[1] * ay) + (X.R[2] * az + X.t[0]);
    ta[1] = (X.R[3] * ax + X.R[4] * ay) + (X.R[5] * az + X.t[1]);
    ta[2] = (X.R[6] * ax + X.R[7] * ay) + (X.R[8] * az + X.t[2]);
}
__device__ inline void gicp_mahalanobis(const double* __restrict__ ca, const double* __restrict__ cb, const GicpXform& X, double* __restrict__ o) {
    const double A[9] = {ca[0], ca[1], ca[2], ca[1], ca[3], ca[4], ca[2], ca[4], ca[5]};
    double RA[9], M[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { double s = 0; for (int k2 = 0; k2 < 3; k2++) s += X.R[r * 3 + k2] * A[k2 * 3 + c]; RA[r * 3 + c] = s; }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { double s = 0; for (int k2 = 0; k2 < 3; k2++) s += RA[r * 3 + k2] * X.R[c * 3 + k2]; M[r * 3 + c] = s; }
    M[0] += cb[0]; M[1] += cb[1]; M[2] += cb[2]; M[3] += cb[1]; M[4] += cb[3]; M[5] += cb[4]; M[6] += cb[2]; M[7] += cb[4]; M[8] += cb[5];
    const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
    const double det = M[0] * c00 + M[1] * c01 + M[2] * c02;
    const double id = 1.0 / det;
    o[0] = c00 * id;
    o[1] = (M[2] * M[7] - M[1] * M[8]) * id;
    o[2] = (M[1] * M[5] - M[2] * M[4]) * id;
    o[3] = (M[0] * M[8] - M[2] * M[6]) * id;
    o[4] = (M[2] * M[3] - M[0] * M[5]) * id;
    o[5] = (M[0] * M[4] - M[1] * M[3]) * id;
}

struct GicpReport {
    double acc[kGicpAcc];
    uint32_t seq, pad;
};

}  // namespace lio

struct lio_gicp {
    int device = 0;
    float res = 1.0f;
    int k = 20;
    uint32_t max_points = 0;
    lio_map* grid[2] = {nullptr, nullptr};  // 0 target, 1 source: hash grids holding the clouds
    uint32_t n[2] = {0, 0};
    bool gridded[2] = {false, false};  // the cloud lies in its grid (not: a source adopted as it stands, which nothing searches)
    bool rows[2] = {false, false};  // the grid's copy carries, where the intensity was, the row its point has in the caller's cloud
    double* cov[2] = {nullptr, nullptr};
    int32_t* corr = nullptr;
    double* maha = nullptr;
    double* partial = nullptr;
    lio::GicpReport* report = nullptr;
    lio::GicpReport* report_dev = nullptr;
    uint32_t seq = 0;
    float4* stage = nullptr;
    // voxelised variant (FastVGICP): off while voxel_res == 0
    double voxel_res = 0.0;
    lio::VgicpOffsets offs;
    lio_map* vmap = nullptr;       // the target's Gaussian voxels: hash grid keyed as fast_vgicp_voxel.hpp does
    lio::VgicpVoxel* vvox = nullptr;    // one record per table slot
    uint32_t* vorder = nullptr;    // a voxel's points by rising row of an adopted target (vgicp_rank_rows_kernel); made on first use
    bool vmap_valid = false;
    int32_t* vcorr = nullptr;      // [n_src x offsets]
    double* vmaha = nullptr;
    double* vpartial = nullptr;
    uint32_t vblocks = 0;
    // lio_gicp_fitness_score (loop.hip): the source as the caller ordered it -- the fitness sum runs in that order -- and the exact index over
    // the target with the launch's scratch, both made when first needed
    float4* src_rows = nullptr;
    int src_order = 0;       // 0: not kept; 1: src_rows; 2: the source grid's pool is the caller's order (an adopted source)
    void* fit = nullptr;     // loop.hip's GicpFit
    bool fit_valid = false;  // the index is over the current target
    uint32_t* bad = nullptr;  // the count of the device entries' finite check; made on first use
    // gicp_stage_cloud's canonical pool order: the stamped / ordered cloud, the cells' first places (by lowest row), the lowest row per slot
    float4* canon = nullptr;
    uint32_t* canon_first = nullptr;
    uint32_t* canon_minrow = nullptr;
    uint64_t canon_minrow_cap = 0;
};

namespace lio {
GicpXform to_gx(const double T[16]);
// setInputTarget / setInputSource: the cloud into its hash grid (pool order), the regularised k-NN covariances beside it
int gicp_set_cloud(lio_gicp* g, int which, const float* xyzi, uint32_t n);
// the same for a cloud in HBM: finite check by a kernel, device-to-device staging copy, then the host entry's path
int gicp_set_cloud_device(lio_gicp* g, int which, const void* d_xyzi, uint32_t n);
// the same for a cloud on the device; the covariances also come back in the CLOUD's own row order (d_cov6_rows[i] belongs to d_pts[i]).
// The order of a grid's pool is the points' arrival order inside a cell, which is any order: what has to be the same from one insertion of a
// cloud to the next is kept by row
int gicp_cloud_covariances(lio_gicp* g, int which, const float4* d_pts, uint32_t n, double* d_cov6_rows);
// the same for a cloud that is already on the device together with its covariances (row i of d_cov6 belongs to d_pts[i]): no neighbour search.
// A target goes into its grid (the neighbour search of the single-pair cost needs one) and its Gaussian voxels are then folded by rising row;
// a source is only ever read row by row, so it is taken as it is, in its own order
int gicp_adopt_cloud(lio_gicp* g, int which, const float4* d_pts, const double* d_cov6, uint32_t n);
// create_voxelmap of the current target
int vgicp_build(lio_gicp* g);
// frees g->fit (loop.hip)
void gicp_fit_free(lio_gicp* g);
}  // namespace lio
