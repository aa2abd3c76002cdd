// ground.hip -- the reference's ground detector on gfx950 (wave64): detect_ground / plane_clip / normal_filtering of
// slam/src/graph_utils.cpp:285-382 (the same stage as floor_detection_nodelet.cpp:79-193), restated from PCL 1.9.1's published algorithms.
//
//   clip      keep iff x, y, z finite and sensor_height - clip_low <= z < sensor_height + clip_high (z compared in f64): PlaneClipper3D with
//             (0, 0, 1, .), inclusive, then the negated one (:337-338); input order kept, the original index beside every point
//   index     knn_index_dev.h's tree over the clipped points, built from device memory (their count never leaves the device)
//   normals   one lane per clipped point in Morton order: the walk with K = 10 (the point is its own first neighbour, as in
//             pcl::NormalEstimation with setKSearch(10)), then in the same kernel the centroid and the 3 x 3 scatter about it in f64 over the
//             neighbours in ascending (d2, index) order, cyclic Jacobi in f64 (registers only), the unit eigenvector of the smallest
//             eigenvalue, and the filter |n_z| > cos(normal_thresh) |n| (:316-320).  Fewer than 3 neighbours: NaN normal, dropped.
//             The m x 10 index table is never written.
//   compact   flags -> device_prims.h's stable compaction (three times: clip, filter, inliers)
//   ransac    pcl::RandomSampleConsensus over SampleConsensusModelPlane (ransac.hpp), 64 hypotheses per launch:
//             gr_planes draws three distinct indices per hypothesis from the counter-based generator of include/lio_hip.h and makes the
//             plane in separately rounded f32; gr_score holds the 64 planes in LDS, tests every point against every plane
//             (|((nx x + ny y) + nz z) + d| < threshold in f32), ballots and popcounts per wave, and adds once per wave and hypothesis
//             (integer atomics: the counts do not depend on the order).  The host replays PCL's sequential loop over the counts of the
//             batch (the only words that come back: 2 sizes + 64 counts + the 64 draws and planes for the log, one pinned copy per batch);
//             the result is what that loop returns for these draws, never "the best of the batch".
//   inliers   the winning plane's `<` test again, compacted in order (selectWithinDistance; no refit)
//
// One stream; scratch grows geometrically and is kept; no allocation in the steady state.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "device_prims.h"
#include "knn_index_dev.h"

namespace lio {
namespace ground {

using namespace prims;

constexpr int kBatch = 64;  // hypotheses per launch
constexpr int kScoreItems = 4;
constexpr int kK = 10;      // setKSearch(10), graph_utils.cpp:309

// one batch as it goes to the host
struct Batch {
    uint32_t n[2];  // clipped, filtered points
    uint32_t counts[kBatch];      // inliers of every hypothesis; ~0: a bad draw (not scored)
    uint32_t draws[3 * kBatch];
    float planes[4 * kBatch];     // (nx, ny, nz, d); NaN for a bad draw
};

__global__ __launch_bounds__(kThreads) void gr_clip_flags(const float4* __restrict__ p, uint32_t n, double zlo, double zhi, uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 q = p[i];
    const double z = (double)q.z;
    flags[i] = (isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && zlo <= z && z < zhi) ? 1 : 0;
}

// flagged items per tile of the first n (= *d_n when given, else n_max) items
__global__ __launch_bounds__(kThreads) void gr_count(const uint8_t* __restrict__ flags, const uint32_t* __restrict__ d_n, uint32_t n_max, uint32_t* __restrict__ counts) {
    const uint32_t n = d_n ? *d_n : n_max;
    const uint32_t base = blockIdx.x * kTile;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        c += (i < n && flags[i]) ? 1u : 0u;
    }
    compact_tile_count(c, counts);
}

// stable compaction of the flagged items: the point and its original index (iin = NULL: the item's own position)
__global__ __launch_bounds__(kThreads) void gr_write(const uint8_t* __restrict__ flags, const uint32_t* __restrict__ d_n, uint32_t n_max,
                                                     const uint32_t* __restrict__ offs, const float4* __restrict__ pin, const uint32_t* __restrict__ iin,
                                                     float4* __restrict__ pout, uint32_t* __restrict__ iout) {
    const uint32_t n = d_n ? *d_n : n_max;
    const uint32_t base = blockIdx.x * kTile;
    bool flagged[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        flagged[r] = i < n && flags[i] != 0;
    }
    compact_tile_write(flagged, offs, [&](int r, uint32_t o) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        pout[o] = pin[i];
        iout[o] = iin ? iin[i] : i;
    });
}

// the clipped points as the index takes them: {x, y, z, position bits}
__global__ __launch_bounds__(kThreads) void gr_expand(const float4* __restrict__ p, const uint32_t* __restrict__ d_n, float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= *d_n) return;
    const float4 q = p[i];
    out[i] = make_float4(q.x, q.y, q.z, __uint_as_float(i));
}

// one Jacobi rotation that annihilates a_pq; r is the third index; CP / CQ the columns of V
template <int CP, int CQ>
__device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq, double (&v)[3][3]) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double vp = v[k][CP], vq = v[k][CQ];
        v[k][CP] = c * vp - s * vq;
        v[k][CQ] = s * vp + c * vq;
    }
}

// the walk's epilogue: the normal of clipped point `pos` from its (up to) 10 neighbours, and the verticality flag
__global__ __launch_bounds__(kThreads) void gr_normals(const float4* __restrict__ leaves, const uint32_t* __restrict__ d_n, const float4* __restrict__ nodes,
                                                       uint32_t P, int L, const float4* __restrict__ cpt, double cos_t, float4* __restrict__ normals,
                                                       uint8_t* __restrict__ flags) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t nf = *d_n;
    if (j >= nf) return;
    const float4 q = leaves[j];
    const uint32_t pos = __float_as_uint(q.w);
    float kd[kK];
    uint32_t ki[kK];
#pragma unroll
    for (int s = 0; s < kK; s++) { kd[s] = INFINITY; ki[s] = knn_index::kNone; }
    knn_index::walk<kK>(q.x, q.y, q.z, nodes, leaves, nf, P, L, kd, ki);
    float4 nb[kK];
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < kK; s++) {
        const bool have = ki[s] != knn_index::kNone;
        nb[s] = cpt[have ? ki[s] : pos];
        cnt += have ? 1 : 0;
    }
    double cx = 0, cy = 0, cz = 0;
#pragma unroll
    for (int s = 0; s < kK; s++)
        if (s < cnt) { cx += (double)nb[s].x; cy += (double)nb[s].y; cz += (double)nb[s].z; }
    const double inv = 1.0 / (double)cnt;
    cx *= inv; cy *= inv; cz *= inv;
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
    for (int s = 0; s < kK; s++)
        if (s < cnt) {
            const double dx = (double)nb[s].x - cx, dy = (double)nb[s].y - cy, dz = (double)nb[s].z - cz;
            a00 += dx * dx; a01 += dx * dy; a02 += dx * dz;
            a11 += dy * dy; a12 += dy * dz; a22 += dz * dz;
        }
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 10; sweep++) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        jacobi_rot<0, 1>(a00, a11, a01, a02, a12, v);
        jacobi_rot<0, 2>(a00, a22, a02, a01, a12, v);
        jacobi_rot<1, 2>(a11, a22, a12, a01, a02, v);
    }
    const int m = (a00 <= a11 && a00 <= a22) ? 0 : (a11 <= a22 ? 1 : 2);
    double nx = m == 0 ? v[0][0] : (m == 1 ? v[0][1] : v[0][2]);
    double ny = m == 0 ? v[1][0] : (m == 1 ? v[1][1] : v[1][2]);
    double nz = m == 0 ? v[2][0] : (m == 1 ? v[2][1] : v[2][2]);
    const double len = sqrt(nx * nx + ny * ny + nz * nz);
    bool keep = false;
    if (cnt >= 3 && len > 0.0) {
        nx /= len; ny /= len; nz /= len;
        keep = fabs(nz) > cos_t * sqrt(nx * nx + ny * ny + nz * nz);
    } else {
        nx = ny = nz = (double)NAN;
    }
    normals[pos] = make_float4((float)nx, (float)ny, (float)nz, 0.f);
    flags[pos] = keep ? 1 : 0;
}

// ---- RANSAC ----
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// draw j of a run over N >= 3 points (include/lio_hip.h states the rule)
__host__ __device__ __forceinline__ void draw3(uint32_t seed, uint32_t j, uint32_t N, uint32_t out[3]) {
    const uint32_t s = mix32(seed ^ 0x9E3779B9u);
    const uint32_t r0 = mix32(s + 3u * j), r1 = mix32(s + 3u * j + 1u), r2 = mix32(s + 3u * j + 2u);
    const uint32_t i0 = (uint32_t)(((uint64_t)r0 * N) >> 32);
    uint32_t i1 = (uint32_t)(((uint64_t)r1 * (N - 1u)) >> 32);
    if (i1 >= i0) i1++;
    uint32_t i2 = (uint32_t)(((uint64_t)r2 * (N - 2u)) >> 32);
    const uint32_t lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    if (i2 >= lo) i2++;
    if (i2 >= hi) i2++;
    out[0] = i0; out[1] = i1; out[2] = i2;
}

// correctly rounded f32 square root and quotient whatever the compiler's f32 settings: the f64 operation is correctly rounded, and rounding
// its result to f32 is innocuous for operands of 24 bits (53 >= 2 * 24 + 2)
__device__ __forceinline__ float sqrt_rn(float a) { return (float)sqrt((double)a); }
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }

__global__ __launch_bounds__(kBatch) void gr_planes(const float4* __restrict__ fpt, const uint32_t* __restrict__ d_nc, const uint32_t* __restrict__ d_nf,
                                                    uint32_t seed, uint32_t j0, Batch* __restrict__ b) {
    const int t = threadIdx.x;
    const uint32_t N = *d_nf;
    if (t == 0) { b->n[0] = *d_nc; b->n[1] = N; }
    uint32_t d[3] = {0, 0, 0};
    float nx = NAN, ny = NAN, nz = NAN, dd = NAN;
    bool good = false;
    if (N >= 3u) {
        draw3(seed, j0 + (uint32_t)t, N, d);
        const float4 p0 = fpt[d[0]], p1 = fpt[d[1]], p2 = fpt[d[2]];
        const float ax = p1.x - p0.x, ay = p1.y - p0.y, az = p1.z - p0.z;
        const float bx = p2.x - p0.x, by = p2.y - p0.y, bz = p2.z - p0.z;
        const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const float l2 = (cx * cx + cy * cy) + cz * cz;
        if (l2 > 0.f && isfinite(l2)) {
            const float l = sqrt_rn(l2);
            nx = div_rn(cx, l); ny = div_rn(cy, l); nz = div_rn(cz, l);
            dd = -(((nx * p0.x) + ny * p0.y) + nz * p0.z);
            good = true;
        }
    }
    b->draws[3 * t] = d[0]; b->draws[3 * t + 1] = d[1]; b->draws[3 * t + 2] = d[2];
    b->planes[4 * t] = nx; b->planes[4 * t + 1] = ny; b->planes[4 * t + 2] = nz; b->planes[4 * t + 3] = dd;
    b->counts[t] = good ? 0u : 0xFFFFFFFFu;
}

// every point against the batch's planes; lane h of a wave carries the wave's count for hypothesis h
__global__ __launch_bounds__(kThreads) void gr_score(const float4* __restrict__ fpt, const uint32_t* __restrict__ d_nf, Batch* __restrict__ b, float thr) {
    __shared__ float4 pl[kBatch];
    const uint32_t N = *d_nf;
    if (blockIdx.x * (uint32_t)(kThreads * kScoreItems) >= N) return;
    if (threadIdx.x < kBatch) pl[threadIdx.x] = make_float4(b->planes[4 * threadIdx.x], b->planes[4 * threadIdx.x + 1], b->planes[4 * threadIdx.x + 2], b->planes[4 * threadIdx.x + 3]);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    float4 p[kScoreItems];
    bool ok[kScoreItems];
#pragma unroll
    for (int r = 0; r < kScoreItems; r++) {
        const uint32_t i = (blockIdx.x * kScoreItems + r) * kThreads + threadIdx.x;
        ok[r] = i < N;
        p[r] = fpt[ok[r] ? i : 0u];
    }
    uint32_t mine = 0;
    for (int h = 0; h < kBatch; h++) {
        const float4 w = pl[h];
        uint32_t c = 0;
#pragma unroll
        for (int r = 0; r < kScoreItems; r++) {
            const float v = ((w.x * p[r].x + w.y * p[r].y) + w.z * p[r].z) + w.w;
            c += (uint32_t)__popcll(__ballot(ok[r] && fabsf(v) < thr));
        }
        mine = (lane == h) ? c : mine;
    }
    if (mine) atomicAdd(&b->counts[lane], mine);  // (a bad draw's plane is NaN: no point passes, its ~0 stays)
}

__global__ __launch_bounds__(kThreads) void gr_inlier_flags(const float4* __restrict__ fpt, const uint32_t* __restrict__ d_nf, float4 w, float thr,
                                                            uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= *d_nf) return;
    const float4 p = fpt[i];
    const float v = ((w.x * p.x + w.y * p.y) + w.z * p.z) + w.w;
    flags[i] = fabsf(v) < thr ? 1 : 0;
}

}  // namespace ground
}  // namespace lio

using namespace lio;
using namespace lio::ground;

struct lio_ground {
    int device;
    hipStream_t stream;
    hipEvent_t ev[4];  // begin, the filter's end, RANSAC's end, the scan's stream
    uint64_t cap;      // points the buffers hold
    float4 *stage, *cpt, *kpts, *fpt, *ipt, *normals;
    uint32_t *cidx, *fidx, *iidx;
    uint8_t* flags;
    uint32_t* aux;     // three compactions' scratch: the clip, the filter and the inliers
    uint64_t region;   // words of each (compact_words)
    knn_index::DeviceIndex* index;
    Batch* d_batch;
    Batch* h_batch;    // pinned
    uint32_t* h_word;  // pinned: the inlier count
    // the last call
    uint32_t n_in, n_clipped, n_filtered, n_inliers;
    int used_filter, found, iterations, skipped, winner;
    uint32_t draws_used;
    std::vector<uint32_t>* log_draws;
    std::vector<uint32_t>* log_counts;
    std::vector<float>* log_planes;
    double filter_us, ransac_us;
};

namespace {

void free_buffers(lio_ground* g) {
    void* all[] = {g->stage, g->cpt, g->kpts, g->fpt, g->ipt, g->normals, g->cidx, g->fidx, g->iidx, g->flags, g->aux};
    for (void* p : all)
        if (p) (void)hipFree(p);
    g->stage = g->cpt = g->kpts = g->fpt = g->ipt = g->normals = nullptr;
    g->cidx = g->fidx = g->iidx = g->aux = nullptr;
    g->flags = nullptr;
    g->cap = 0;
}

int reserve(lio_ground* g, uint64_t n) {
    if (n <= g->cap) return LIO_OK;
    if (n > 0x7FFFFFFFull) { set_error("lio_ground: %llu points exceed the int index range (2^31 - 1)", (unsigned long long)n); return LIO_E_CAPACITY; }
    const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(n, std::max<uint64_t>(2 * g->cap, 1ull << 17)), 0x7FFFFFFFull);
    LIO_HIP_TRY(hipStreamSynchronize(g->stream));
    free_buffers(g);
    g->region = compact_words(want);
    const bool ok = alloc(&g->stage, want) && alloc(&g->cpt, want) && alloc(&g->kpts, want) && alloc(&g->fpt, want) && alloc(&g->ipt, want) &&
                    alloc(&g->normals, want) && alloc(&g->cidx, want) && alloc(&g->fidx, want) && alloc(&g->iidx, want) && alloc(&g->flags, want) &&
                    alloc(&g->aux, 3 * g->region);
    if (!ok) {
        (void)hipGetLastError();
        free_buffers(g);
        set_error("lio_ground: device scratch for %llu points not available", (unsigned long long)want);
        return LIO_E_DEVICE;
    }
    g->cap = want;
    return LIO_OK;
}

// flags[0 .. n) -> the flagged points and their indices, in order; the count stays on the device at the returned pointer
int compact(lio_ground* g, int which, const uint32_t* d_n, uint32_t n_max, const float4* pin, const uint32_t* iin, float4* pout, uint32_t* iout,
            const uint32_t** d_out_n) {
    const uint32_t ntiles = tiles_of(n_max);
    uint32_t* counts = g->aux + (uint64_t)which * g->region;
    gr_count<<<dim3(ntiles), dim3(kThreads), 0, g->stream>>>(g->flags, d_n, n_max, counts);
    *d_out_n = compact_finish(g->stream, counts, n_max);
    if (!*d_out_n) return LIO_E_DEVICE;
    gr_write<<<dim3(ntiles), dim3(kThreads), 0, g->stream>>>(g->flags, d_n, n_max, counts, pin, iin, pout, iout);
    LIO_HIP_TRY(hipGetLastError());
    return LIO_OK;
}

void clear_last(lio_ground* g) {
    g->n_in = g->n_clipped = g->n_filtered = g->n_inliers = 0;
    g->used_filter = g->found = g->iterations = g->skipped = 0;
    g->winner = -1;
    g->draws_used = 0;
    g->log_draws->clear();
    g->log_counts->clear();
    g->log_planes->clear();
    g->filter_us = g->ransac_us = 0;
}

// the detector over n device points at `raw` (already ordered after the stream's earlier work)
int detect(lio_ground* g, const float4* raw, uint32_t n, const lio_ground_params* p, int* found, float coeffs[4]) {
    clear_last(g);
    g->n_in = n;
    *found = 0;
    for (int i = 0; i < 4; i++) coeffs[i] = 0.f;
    if (n == 0) return LIO_OK;
    hipStream_t st = g->stream;
    const double zlo = p->sensor_height - p->clip_low, zhi = p->sensor_height + p->clip_high;
    const float thr = (float)p->distance_threshold;
    LIO_HIP_TRY(hipEventRecord(g->ev[0], st));
    // clip
    const uint32_t *d_nc = nullptr, *d_nf = nullptr, *d_ni = nullptr;
    gr_clip_flags<<<dim3(blocks_of(n)), dim3(kThreads), 0, st>>>(raw, n, zlo, zhi, g->flags);
    int rc = compact(g, 0, nullptr, n, raw, nullptr, g->cpt, g->cidx, &d_nc);
    if (rc != LIO_OK) return rc;
    // normals and the verticality filter
    const float4* fpt = g->cpt;
    const uint32_t* fidx = g->cidx;
    d_nf = d_nc;
    g->used_filter = p->use_normal_filter ? 1 : 0;
    if (p->use_normal_filter) {
        gr_expand<<<dim3(blocks_of(n)), dim3(kThreads), 0, st>>>(g->cpt, d_nc, g->kpts);
        rc = knn_index::device_index_build(st, *g->index, g->kpts, d_nc, n);
        if (rc != LIO_OK) return rc;
        gr_normals<<<dim3(blocks_of(n)), dim3(kThreads), 0, st>>>(g->index->leaves, d_nc, g->index->nodes, g->index->P, g->index->L, g->cpt,
                                                                 cos(p->normal_thresh_deg * M_PI / 180.0), g->normals, g->flags);
        rc = compact(g, 1, d_nc, n, g->cpt, g->cidx, g->fpt, g->fidx, &d_nf);
        if (rc != LIO_OK) return rc;
        fpt = g->fpt;
        fidx = g->fidx;
    }
    LIO_HIP_TRY(hipEventRecord(g->ev[1], st));
    // RANSAC: ransac.hpp's loop, replayed over the counts batch by batch
    const double log_probability = std::log(1.0 - p->probability);
    const uint32_t max_skip = (uint32_t)p->max_iterations * 10u;
    double k = 1.0;
    int64_t best = -1;
    uint32_t j = 0;
    bool running = true;
    const uint32_t score_blocks = (n + kThreads * kScoreItems - 1) / (kThreads * kScoreItems);
    while (running) {
        gr_planes<<<dim3(1), dim3(kBatch), 0, st>>>(fpt, d_nc, d_nf, p->seed, j, g->d_batch);
        gr_score<<<dim3(score_blocks), dim3(kThreads), 0, st>>>(fpt, d_nf, g->d_batch, thr);
        LIO_HIP_TRY(hipGetLastError());
        LIO_HIP_TRY(hipMemcpyAsync(g->h_batch, g->d_batch, sizeof(Batch), hipMemcpyDeviceToHost, st));
        LIO_HIP_TRY(hipStreamSynchronize(st));
        const Batch& b = *g->h_batch;
        g->n_clipped = b.n[0];
        g->n_filtered = b.n[1];
        if ((int64_t)g->n_filtered < (int64_t)p->min_points || g->n_filtered < 3u) break;  // too few points for RANSAC (graph_utils.cpp:342)
        g->log_draws->insert(g->log_draws->end(), b.draws, b.draws + 3 * kBatch);
        g->log_counts->insert(g->log_counts->end(), b.counts, b.counts + kBatch);
        g->log_planes->insert(g->log_planes->end(), b.planes, b.planes + 4 * kBatch);
        const double one_over = 1.0 / (double)g->n_filtered;
        for (int t = 0; t < kBatch; t++) {
            if (!((double)g->iterations < k && (uint32_t)g->skipped < max_skip)) { running = false; break; }
            const uint32_t c = b.counts[t];
            j++;
            if (c == 0xFFFFFFFFu) { g->skipped++; continue; }
            if ((int64_t)c > best) {
                best = c;
                g->winner = (int)(j - 1);
                const double w = (double)best * one_over;
                double p_no = 1.0 - std::pow(w, 3.0);
                p_no = std::max(DBL_EPSILON, p_no);
                p_no = std::min(1.0 - DBL_EPSILON, p_no);
                k = log_probability / std::log(p_no);
            }
            g->iterations++;
            if (g->iterations > p->max_iterations) { running = false; break; }
        }
    }
    g->draws_used = j;
    if (g->winner < 0) {
        LIO_HIP_TRY(hipEventRecord(g->ev[2], st));
        LIO_HIP_TRY(hipStreamSynchronize(st));
        g->filter_us = elapsed_us(g->ev[0], g->ev[1]);
        g->ransac_us = elapsed_us(g->ev[1], g->ev[2]);
        return LIO_OK;
    }
    const float* wp = g->log_planes->data() + 4ull * (uint32_t)g->winner;
    gr_inlier_flags<<<dim3(blocks_of(n)), dim3(kThreads), 0, st>>>(fpt, d_nf, make_float4(wp[0], wp[1], wp[2], wp[3]), thr, g->flags);
    rc = compact(g, 2, d_nf, n, fpt, fidx, g->ipt, g->iidx, &d_ni);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipMemcpyAsync(g->h_word, d_ni, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipEventRecord(g->ev[2], st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    g->filter_us = elapsed_us(g->ev[0], g->ev[1]);
    g->ransac_us = elapsed_us(g->ev[1], g->ev[2]);
    g->n_inliers = *g->h_word;
    if ((int64_t)g->n_inliers < (int64_t)p->min_points) return LIO_OK;                                          // too few inliers (:356)
    if (std::fabs((double)wp[2]) < std::cos(p->floor_normal_thresh_deg * M_PI / 180.0)) return LIO_OK;         // the normal is not vertical (:366-370)
    const float sgn = wp[2] < 0.0f ? -1.0f : 1.0f;                                                             // make the normal upward (:373-375)
    for (int i = 0; i < 4; i++) coeffs[i] = wp[i] * sgn;
    g->found = *found = 1;
    return LIO_OK;
}

bool params_ok(const lio_ground_params* p) {
    if (!p) return false;
    if (p->use_normal_filter && p->k != kK) { set_error("lio_ground: k = %d is not built (only 10, the reference's setKSearch)", p->k); return false; }
    if (p->max_iterations < 1 || p->max_iterations > 1000000 || !(p->probability > 0.0 && p->probability < 1.0) || p->min_points < 0 ||
        !(p->distance_threshold > 0.0)) {
        set_error("lio_ground: max_iterations in [1, 10^6], probability in (0, 1), min_points >= 0 and distance_threshold > 0 are required");
        return false;
    }
    return true;
}

int64_t download_u32(lio_ground* g, const uint32_t* src, uint64_t n, uint32_t* out, uint64_t cap) {
    return download("lio_ground", g->device, g->stream, src, n, out, cap);
}

}  // namespace

// the inlier cloud of the last call where it lies (render.hip paints it without a trip to the host); the detector's stream is idle
const float4* lio::ground::inliers_view(lio_ground* g, uint32_t* n) {
    *n = g->n_inliers;
    return g->ipt;
}

extern "C" {

void lio_ground_default_params(lio_ground_params* p, int preset) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->sensor_height = 0.0;
    p->clip_low = preset == 1 ? 2.0 : 1.5;   // floor_detection_nodelet.cpp:40-41 / graph_utils.cpp:331-332
    p->clip_high = preset == 1 ? 1.0 : 1.5;
    p->use_normal_filter = 1;
    p->normal_thresh_deg = 20.0;
    p->k = kK;
    p->distance_threshold = 0.1;
    p->min_points = 1024;
    p->floor_normal_thresh_deg = 10.0;
    p->max_iterations = 1000;  // pcl::SampleConsensus's defaults
    p->probability = 0.99;
    p->seed = 0;
}

void lio_ground_draw(uint32_t seed, uint32_t j, uint32_t n, uint32_t out[3]) {
    if (!out) return;
    out[0] = out[1] = out[2] = 0;
    if (n >= 3) draw3(seed, j, n, out);
}

lio_ground* lio_ground_create(int device) {
    lio_ground* g = new lio_ground();
    memset(g, 0, sizeof(*g));
    g->device = device;
    if (!open_device("lio_ground_create", device, &g->stream, g->ev, 4)) {
        delete g;
        return nullptr;
    }
    g->index = new knn_index::DeviceIndex();
    g->log_draws = new std::vector<uint32_t>();
    g->log_counts = new std::vector<uint32_t>();
    g->log_planes = new std::vector<float>();
    g->winner = -1;
    const bool ok = alloc(&g->d_batch, 1) && hipHostMalloc(&g->h_batch, sizeof(Batch)) == hipSuccess &&
         hipHostMalloc(&g->h_word, 64) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        set_error("lio_ground_create: stream / event / staging allocation failed");
        lio_ground_destroy(g);
        return nullptr;
    }
    return g;
}

void lio_ground_destroy(lio_ground* g) {
    if (!g) return;
    hipSetDevice(g->device);
    if (g->stream) hipStreamSynchronize(g->stream);
    free_buffers(g);
    knn_index::device_index_free(*g->index);
    if (g->d_batch) hipFree(g->d_batch);
    if (g->h_batch) hipHostFree(g->h_batch);
    if (g->h_word) hipHostFree(g->h_word);
    for (int i = 0; i < 4; i++)
        if (g->ev[i]) hipEventDestroy(g->ev[i]);
    if (g->stream) hipStreamDestroy(g->stream);
    delete g->index;
    delete g->log_draws;
    delete g->log_counts;
    delete g->log_planes;
    delete g;
}

static void report(lio_ground* g, uint32_t* n_clipped, uint32_t* n_filtered, uint32_t* n_inliers) {
    if (n_clipped) *n_clipped = g->n_clipped;
    if (n_filtered) *n_filtered = g->n_filtered;
    if (n_inliers) *n_inliers = g->n_inliers;
}

int lio_ground_detect_scan(lio_ground* g, lio_scan* s, const lio_ground_params* p, int replace, int* found, float coeffs[4], uint32_t* n_clipped,
                           uint32_t* n_filtered, uint32_t* n_inliers) {
    if (!g || !s || !found || !coeffs || !params_ok(p)) return LIO_E_INVALID;
    if (s->device != g->device) { set_error("lio_ground_detect_scan: the scan lives on device %d, the detector on %d", s->device, g->device); return LIO_E_INVALID; }
    hipSetDevice(g->device);
    const uint32_t n = s->n_raw;
    int rc = reserve(g, n);
    if (rc == LIO_OK && p->use_normal_filter) rc = knn_index::device_index_reserve(*g->index, n);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipEventRecord(g->ev[3], s->stream));  // the scan's upload / undistortion first
    LIO_HIP_TRY(hipStreamWaitEvent(g->stream, g->ev[3], 0));
    rc = detect(g, s->raw, n, p, found, coeffs);
    report(g, n_clipped, n_filtered, n_inliers);
    if (rc != LIO_OK || !*found || !replace) return rc;
    // extract.filter(*cloud), graph_utils.cpp:377-380: the scan's raw cloud becomes the inlier cloud (the detector's stream is idle on return)
    LIO_HIP_TRY(hipMemcpyAsync(s->raw_own, g->ipt, (uint64_t)g->n_inliers * sizeof(float4), hipMemcpyDeviceToDevice, g->stream));
    LIO_HIP_TRY(hipStreamSynchronize(g->stream));
    s->raw = s->raw_own;
    s->n_raw = g->n_inliers;
    return LIO_OK;
}

int lio_ground_detect_host(lio_ground* g, const float* xyzi, uint64_t n, const lio_ground_params* p, int* found, float coeffs[4], uint32_t* n_clipped,
                           uint32_t* n_filtered, uint32_t* n_inliers) {
    if (!g || (!xyzi && n) || !found || !coeffs || !params_ok(p)) return LIO_E_INVALID;
    hipSetDevice(g->device);
    int rc = reserve(g, n);
    if (rc == LIO_OK && p->use_normal_filter) rc = knn_index::device_index_reserve(*g->index, n);
    if (rc != LIO_OK) return rc;
    if (n) LIO_HIP_TRY(hipMemcpyAsync(g->stage, xyzi, n * sizeof(float4), hipMemcpyHostToDevice, g->stream));
    rc = detect(g, g->stage, (uint32_t)n, p, found, coeffs);
    report(g, n_clipped, n_filtered, n_inliers);
    return rc;
}

int64_t lio_ground_download_indices(lio_ground* g, int stage, uint32_t* out, uint64_t cap) {
    if (!g || stage < 0 || stage > 2) return LIO_E_INVALID;
    if (stage == 0) return download_u32(g, g->cidx, g->n_clipped, out, cap);
    if (stage == 1) return download_u32(g, g->used_filter ? g->fidx : g->cidx, g->n_filtered, out, cap);
    return download_u32(g, g->iidx, g->n_inliers, out, cap);
}

int64_t lio_ground_download_normals(lio_ground* g, float* out_n3, uint64_t cap) {
    if (!g) return LIO_E_INVALID;
    const uint64_t n = g->used_filter ? g->n_clipped : 0;
    if (n > cap) return -(int64_t)n;
    if (n == 0) return 0;
    if (!out_n3) return LIO_E_INVALID;
    hipSetDevice(g->device);
    std::vector<float4> tmp(n);
    LIO_HIP_TRY(hipMemcpyAsync(tmp.data(), g->normals, n * sizeof(float4), hipMemcpyDeviceToHost, g->stream));
    LIO_HIP_TRY(hipStreamSynchronize(g->stream));
    for (uint64_t i = 0; i < n; i++) { out_n3[3 * i] = tmp[i].x; out_n3[3 * i + 1] = tmp[i].y; out_n3[3 * i + 2] = tmp[i].z; }
    return (int64_t)n;
}

int64_t lio_ground_download_inliers(lio_ground* g, float* xyzi, uint64_t cap) {
    if (!g) return LIO_E_INVALID;
    const uint64_t n = g->n_inliers;
    if (n > cap) return -(int64_t)n;
    if (n == 0) return 0;
    if (!xyzi) return LIO_E_INVALID;
    hipSetDevice(g->device);
    LIO_HIP_TRY(hipMemcpyAsync(xyzi, g->ipt, n * sizeof(float4), hipMemcpyDeviceToHost, g->stream));
    LIO_HIP_TRY(hipStreamSynchronize(g->stream));
    return (int64_t)n;
}

int64_t lio_ground_download_draws(lio_ground* g, uint32_t* triples, uint32_t* counts, float* planes, uint64_t cap) {
    if (!g) return LIO_E_INVALID;
    const uint64_t n = g->log_counts->size();
    if (n > cap) return -(int64_t)n;
    if (n && triples) memcpy(triples, g->log_draws->data(), 3 * n * sizeof(uint32_t));
    if (n && counts) memcpy(counts, g->log_counts->data(), n * sizeof(uint32_t));
    if (n && planes) memcpy(planes, g->log_planes->data(), 4 * n * sizeof(float));
    return (int64_t)n;
}

int lio_ground_last_run(lio_ground* g, int* iterations, int* skipped, int* draws_used, int* winner) {
    if (!g) return LIO_E_INVALID;
    if (iterations) *iterations = g->iterations;
    if (skipped) *skipped = g->skipped;
    if (draws_used) *draws_used = (int)g->draws_used;
    if (winner) *winner = g->winner;
    return LIO_OK;
}

int lio_ground_last_times(lio_ground* g, double* filter_us, double* ransac_us) {
    if (!g) return LIO_E_INVALID;
    if (filter_us) *filter_us = g->filter_us;
    if (ransac_us) *ransac_us = g->ransac_us;
    return LIO_OK;
}

}  // extern "C"
