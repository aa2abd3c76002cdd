// calib_ground.hip -- the reference's lidar ground calibration on gfx950 (wave64): crop_points / test_point_in_polygon of
// calibration/lidar_calibration/filter.py, and is_colinear / get_plane_coefficient / fit_plane of fit.py, restated from their rules
// (include/lio_hip.h states every one).
//
//   crop      one lane per point, the polygon in LDS as f64 pairs (at most kMaxVertices): the crossing-number test in f64 over the point's x and
//             y widened from f32; the kept points leave in input order through device_prims.h's stable compaction, their positions beside them
//   planes    one lane per attempt of a batch: the triple (uploaded by the host: lio_ground_draw's or the caller's) -> the colinearity test and
//             the plane in separately rounded f32 (-ffp-contract=off)
//   score     the batch's planes (at most kBatch) in LDS, a lane holds kScoreItems points: every point against every plane, one ballot and
//             popcount per wave, plane and round; lane h of a wave carries the wave's count of planes h and h + 64 and adds each once
//             (integer atomics: the counts do not depend on the order or on the launch geometry)
//   loop      the host replays fit_plane's loop over the counts of the batch (one pinned copy per batch comes back: triples, flags, counts,
//             planes); the points are read once per batch, never once per hypothesis
//
// One stream; buffers grow geometrically and are kept; no allocation in the steady state.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_prims.h"

namespace lio {
namespace calib_ground {

using namespace prims;

constexpr int kMaxVertices = LIO_CALIB_GROUND_MAX_VERTICES;  // 256 f64 pairs: 4 KB of LDS
constexpr int kBatch = 128;                                  // attempts per launch: 2 KB of LDS for the planes
constexpr int kScoreItems = 4;
static_assert(kBatch == 2 * 64, "a lane of the score kernel carries the counts of planes `lane` and `lane + 64`");

// one batch as it goes to the host
struct Batch {
    uint32_t triples[3 * kBatch];
    uint32_t colinear[kBatch];
    uint32_t counts[kBatch];
    float planes[4 * kBatch];  // NaN for a colinear attempt
};

// the crossing-number test of point (x, y) against the nv vertices in LDS
__device__ __forceinline__ bool inside(const double2* __restrict__ poly, int nv, double x, double y) {
    uint32_t cn = 0;
    for (int e = 0; e < nv; e++) {
        const double2 p = poly[e], q = poly[e + 1 < nv ? e + 1 : 0];
        const bool pu = p.y > q.y;
        const double2 up = pu ? p : q, down = pu ? q : p;
        if (down.y < y && y < up.y) {
            const double xi = down.x + ((up.x - down.x) * (y - down.y)) / (up.y - down.y);
            cn += xi > x ? 1u : 0u;
        }
    }
    return (cn & 1u) != 0;
}

// the crop's predicate per point (kept in flags for the write kernel) and the tile's count
__global__ __launch_bounds__(kThreads) void cg_crop_count(const float* __restrict__ raw, uint32_t n, uint32_t stride, const double2* __restrict__ d_poly,
                                                          int nv, uint8_t* __restrict__ flags, uint32_t* __restrict__ counts) {
    __shared__ double2 poly[kMaxVertices];
    for (int v = threadIdx.x; v < nv; v += kThreads) poly[v] = d_poly[v];
    __syncthreads();
    const uint32_t base = blockIdx.x * kTile;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        if (i < n) {
            const float* p = raw + (uint64_t)i * stride;
            const bool in = inside(poly, nv, (double)p[0], (double)p[1]);
            flags[i] = in ? 1 : 0;
            c += in ? 1u : 0u;
        }
    }
    compact_tile_count(c, counts);
}

__global__ __launch_bounds__(kThreads) void cg_crop_write(const float* __restrict__ raw, uint32_t n, uint32_t stride, const uint8_t* __restrict__ flags,
                                                          const uint32_t* __restrict__ offs, float4* __restrict__ pout, uint32_t* __restrict__ iout) {
    const uint32_t base = blockIdx.x * kTile;
    bool keep[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        keep[r] = i < n && flags[i] != 0;
    }
    compact_tile_write(keep, offs, [&](int r, uint32_t o) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        const float* p = raw + (uint64_t)i * stride;
        pout[o] = make_float4(p[0], p[1], p[2], 0.f);
        iout[o] = i;
    });
}

// a cloud adopted as already cropped: every point, its own position beside it
__global__ __launch_bounds__(kThreads) void cg_adopt(const float* __restrict__ raw, uint32_t n, uint32_t stride, float4* __restrict__ pout,
                                                     uint32_t* __restrict__ iout) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float* p = raw + (uint64_t)i * stride;
    pout[i] = make_float4(p[0], p[1], p[2], 0.f);
    iout[i] = i;
}

// correctly rounded f32 square root and quotient whatever the compiler's f32 settings: the f64 operation is correctly rounded, and rounding
// its result to f32 is innocuous for operands of 24 bits (53 >= 2 * 24 + 2)
__device__ __forceinline__ float sqrt_rn(float a) { return (float)sqrt((double)a); }
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }

// attempt t of the batch: is_colinear and get_plane_coefficient of its triple; the count starts at 0
__global__ __launch_bounds__(kBatch) void cg_planes(const float4* __restrict__ cpt, uint32_t nb, Batch* __restrict__ b) {
    const uint32_t t = threadIdx.x;
    if (t >= nb) return;
    const float4 p1 = cpt[b->triples[3 * t]], p2 = cpt[b->triples[3 * t + 1]], p3 = cpt[b->triples[3 * t + 2]];
    const float ux = p2.x - p1.x, uy = p2.y - p1.y, uz = p2.z - p1.z;
    const float vx = p3.x - p1.x, vy = p3.y - p1.y, vz = p3.z - p1.z;
    const float a = uy * vz - vy * uz;
    const float bb = uz * vx - vz * ux;
    const float c = ux * vy - vx * uy;
    const bool colinear = (fabsf(a) + fabsf(bb)) + fabsf(c) < (float)1e-5;
    float4 w = make_float4(NAN, NAN, NAN, NAN);
    if (!colinear) {
        const float norm = sqrt_rn((a * a + bb * bb) + c * c);
        const float d = -((a * p1.x + bb * p1.y) + c * p1.z);
        w = make_float4(div_rn(a, norm), div_rn(bb, norm), div_rn(c, norm), div_rn(d, norm));
        if (!(c > 0.f)) w = make_float4(-w.x, -w.y, -w.z, -w.w);
    }
    b->colinear[t] = colinear ? 1u : 0u;
    b->counts[t] = 0u;
    b->planes[4 * t] = w.x; b->planes[4 * t + 1] = w.y; b->planes[4 * t + 2] = w.z; b->planes[4 * t + 3] = w.w;
}

// every point against the batch's nb planes
__global__ __launch_bounds__(kThreads) void cg_score(const float4* __restrict__ cpt, uint32_t n, uint32_t nb, Batch* __restrict__ b, float sigma) {
    __shared__ float4 pl[kBatch];
    if (threadIdx.x < nb) pl[threadIdx.x] = make_float4(b->planes[4 * threadIdx.x], b->planes[4 * threadIdx.x + 1], b->planes[4 * threadIdx.x + 2], b->planes[4 * threadIdx.x + 3]);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    float4 p[kScoreItems];
    bool ok[kScoreItems];
#pragma unroll
    for (int r = 0; r < kScoreItems; r++) {
        const uint32_t i = (blockIdx.x * kScoreItems + r) * kThreads + threadIdx.x;
        ok[r] = i < n;
        p[r] = cpt[ok[r] ? i : 0u];
    }
    uint32_t lo = 0, hi = 0;
    for (uint32_t h = 0; h < nb; h++) {
        const float4 w = pl[h];
        uint32_t c = 0;
#pragma unroll
        for (int r = 0; r < kScoreItems; r++) {
            const float v = ((w.x * p[r].x + w.y * p[r].y) + w.z * p[r].z) + w.w;
            c += (uint32_t)__popcll(__ballot(ok[r] && fabsf(v) < sigma));  // NaN: not counted
        }
        lo = (h == lane) ? c : lo;
        hi = (h == lane + 64u) ? c : hi;
    }
    if (lo) atomicAdd(&b->counts[lane], lo);
    if (hi) atomicAdd(&b->counts[lane + 64u], hi);
}

}  // namespace calib_ground
}  // namespace lio

using namespace lio;
using namespace lio::calib_ground;

struct lio_calib_ground {
    int device;
    hipStream_t stream;
    hipEvent_t ev[7];  // crop begin / end, fit begin / end, a batch's begin / planes' end / score's end
    float* raw;        // the cloud as it came, stride floats per point
    uint64_t raw_cap;  // floats
    uint64_t cap;      // points the other buffers hold
    uint8_t* flags;
    float4* cpt;
    uint32_t* cidx;
    uint32_t* aux;     // the compaction's scratch
    double2* d_poly;
    Batch* d_batch;
    Batch* h_batch;    // pinned
    uint32_t* h_word;  // pinned: the kept count
    uint32_t n_kept;
    // the last fit
    int found, iterations, attempts, skipped, winner, early_exit;
    std::vector<uint32_t>* log_triples;
    std::vector<uint32_t>* log_colinear;
    std::vector<uint32_t>* log_counts;
    std::vector<float>* log_planes;
    double crop_us, fit_us, planes_us, score_us;
};

namespace {

void free_buffers(lio_calib_ground* g) {
    void* all[] = {g->flags, g->cpt, g->cidx, g->aux};
    for (void* p : all)
        if (p) (void)hipFree(p);
    g->flags = nullptr;
    g->cpt = nullptr;
    g->cidx = g->aux = nullptr;
    g->cap = 0;
}

// room for n points of `stride` floats; what the handle held is dropped only when a buffer has to grow
int reserve(lio_calib_ground* g, uint64_t n, uint32_t stride) {
    int rc = grow("lio_calib_ground", &g->raw, &g->raw_cap, std::max<uint64_t>(n * stride, 1), g->stream);
    if (rc != LIO_OK) return rc;
    if (n <= g->cap) return LIO_OK;
    const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(n, std::max<uint64_t>(2 * g->cap, 1ull << 16)), 0x7FFFFFFFull);
    LIO_HIP_TRY(hipStreamSynchronize(g->stream));
    free_buffers(g);
    g->n_kept = 0;
    const bool ok = alloc(&g->flags, want) && alloc(&g->cpt, want) && alloc(&g->cidx, want) && alloc(&g->aux, compact_words(want));
    if (!ok) {
        (void)hipGetLastError();
        free_buffers(g);
        set_error("lio_calib_ground: device buffers for %llu points not available", (unsigned long long)want);
        return LIO_E_DEVICE;
    }
    g->cap = want;
    return LIO_OK;
}

bool cloud_ok(const char* who, const float* xyz, uint64_t n, uint32_t stride) {
    if ((!xyz && n) || stride < 3) { set_error("%s: a cloud of n points, stride_floats >= 3 apart, is required", who); return false; }
    if (n > 0x7FFFFFFFull || n * (uint64_t)stride > (1ull << 34)) { set_error("%s: %llu points of %u floats exceed the index range", who, (unsigned long long)n, stride); return false; }
    return true;
}

void clear_fit(lio_calib_ground* g) {
    g->found = g->iterations = g->attempts = g->skipped = g->early_exit = 0;
    g->winner = -1;
    g->log_triples->clear();
    g->log_colinear->clear();
    g->log_counts->clear();
    g->log_planes->clear();
    g->fit_us = g->planes_us = g->score_us = 0;
}

}  // namespace

extern "C" {

void lio_calib_ground_default_params(lio_calib_ground_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->sigma = 0.05;  // align_points_to_xyplane's (calib.py:25-27)
    p->num_iteration = 100;
    p->thresh = 0.9;
    p->seed = 0;
}

lio_calib_ground* lio_calib_ground_create(int device) {
    lio_calib_ground* g = new lio_calib_ground();
    memset(g, 0, sizeof(*g));
    g->device = device;
    if (!open_device("lio_calib_ground_create", device, &g->stream, g->ev, 7)) {
        delete g;
        return nullptr;
    }
    g->log_triples = new std::vector<uint32_t>();
    g->log_colinear = new std::vector<uint32_t>();
    g->log_counts = new std::vector<uint32_t>();
    g->log_planes = new std::vector<float>();
    g->winner = -1;
    const bool ok = alloc(&g->d_batch, 1) && alloc(&g->d_poly, kMaxVertices) && hipHostMalloc(&g->h_batch, sizeof(Batch)) == hipSuccess &&
                    hipHostMalloc(&g->h_word, 64) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        set_error("lio_calib_ground_create: staging allocation failed");
        lio_calib_ground_destroy(g);
        return nullptr;
    }
    return g;
}

void lio_calib_ground_destroy(lio_calib_ground* g) {
    if (!g) return;
    hipSetDevice(g->device);
    if (g->stream) hipStreamSynchronize(g->stream);
    free_buffers(g);
    if (g->raw) hipFree(g->raw);
    if (g->d_poly) hipFree(g->d_poly);
    if (g->d_batch) hipFree(g->d_batch);
    if (g->h_batch) hipHostFree(g->h_batch);
    if (g->h_word) hipHostFree(g->h_word);
    for (int i = 0; i < 7; i++)
        if (g->ev[i]) hipEventDestroy(g->ev[i]);
    if (g->stream) hipStreamDestroy(g->stream);
    delete g->log_triples;
    delete g->log_colinear;
    delete g->log_counts;
    delete g->log_planes;
    delete g;
}

int lio_calib_ground_crop_host(lio_calib_ground* g, const float* xyz, uint64_t n, uint32_t stride_floats, const double* poly_xy, int n_vertices,
                               uint32_t* n_kept) {
    if (!g) return LIO_E_INVALID;
    if (!cloud_ok("lio_calib_ground_crop_host", xyz, n, stride_floats)) return LIO_E_INVALID;
    if (!poly_xy || n_vertices < 3 || n_vertices > kMaxVertices) {
        set_error("lio_calib_ground_crop_host: a polygon of 3 to %d vertices is required (%d given)", kMaxVertices, n_vertices);
        return LIO_E_INVALID;
    }
    hipSetDevice(g->device);
    hipStream_t st = g->stream;
    int rc = reserve(g, n, stride_floats);
    if (rc != LIO_OK) return rc;
    g->n_kept = 0;
    g->crop_us = 0;
    if (n_kept) *n_kept = 0;
    if (n == 0) return LIO_OK;
    LIO_HIP_TRY(hipMemcpyAsync(g->raw, xyz, n * stride_floats * sizeof(float), hipMemcpyHostToDevice, st));
    LIO_HIP_TRY(hipMemcpyAsync(g->d_poly, poly_xy, (size_t)n_vertices * sizeof(double2), hipMemcpyHostToDevice, st));
    LIO_HIP_TRY(hipEventRecord(g->ev[0], st));
    const uint32_t ntiles = tiles_of(n);
    cg_crop_count<<<dim3(ntiles), dim3(kThreads), 0, st>>>(g->raw, (uint32_t)n, stride_floats, g->d_poly, n_vertices, g->flags, g->aux);
    const uint32_t* d_total = compact_finish(st, g->aux, n);
    if (!d_total) return LIO_E_DEVICE;
    cg_crop_write<<<dim3(ntiles), dim3(kThreads), 0, st>>>(g->raw, (uint32_t)n, stride_floats, g->flags, g->aux, g->cpt, g->cidx);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(g->ev[1], st));
    LIO_HIP_TRY(hipMemcpyAsync(g->h_word, d_total, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    g->crop_us = elapsed_us(g->ev[0], g->ev[1]);
    g->n_kept = *g->h_word;
    if (n_kept) *n_kept = g->n_kept;
    return LIO_OK;
}

int lio_calib_ground_set_points_host(lio_calib_ground* g, const float* xyz, uint64_t n, uint32_t stride_floats) {
    if (!g) return LIO_E_INVALID;
    if (!cloud_ok("lio_calib_ground_set_points_host", xyz, n, stride_floats)) return LIO_E_INVALID;
    hipSetDevice(g->device);
    hipStream_t st = g->stream;
    int rc = reserve(g, n, stride_floats);
    if (rc != LIO_OK) return rc;
    g->n_kept = 0;
    g->crop_us = 0;
    if (n == 0) return LIO_OK;
    LIO_HIP_TRY(hipMemcpyAsync(g->raw, xyz, n * stride_floats * sizeof(float), hipMemcpyHostToDevice, st));
    cg_adopt<<<dim3(blocks_of(n)), dim3(kThreads), 0, st>>>(g->raw, (uint32_t)n, stride_floats, g->cpt, g->cidx);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipStreamSynchronize(st));
    g->n_kept = (uint32_t)n;
    return LIO_OK;
}

int lio_calib_ground_fit(lio_calib_ground* g, const lio_calib_ground_params* params, const uint32_t* triples, uint64_t n_triples, int* found,
                         float coef[4]) {
    if (!g || !found || !coef) return LIO_E_INVALID;
    lio_calib_ground_params def;
    lio_calib_ground_default_params(&def);
    const lio_calib_ground_params* p = params ? params : &def;
    if (p->num_iteration < 1 || p->num_iteration > 1000000) { set_error("lio_calib_ground_fit: num_iteration in [1, 10^6] is required (%d given)", p->num_iteration); return LIO_E_INVALID; }
    const uint32_t n = g->n_kept;
    if (n < 3) { set_error("lio_calib_ground_fit: %u points are held, a plane takes 3", n); return LIO_E_INVALID; }
    if (!triples && n_triples) { set_error("lio_calib_ground_fit: n_triples without triples"); return LIO_E_INVALID; }
    for (uint64_t t = 0; triples && t < n_triples; t++) {
        const uint32_t i = triples[3 * t], j = triples[3 * t + 1], k = triples[3 * t + 2];
        if (i >= n || j >= n || k >= n || i == j || i == k || j == k) {
            set_error("lio_calib_ground_fit: triple %llu = (%u, %u, %u) is not three distinct indices below %u", (unsigned long long)t, i, j, k, n);
            return LIO_E_INVALID;
        }
    }
    hipSetDevice(g->device);
    hipStream_t st = g->stream;
    clear_fit(g);
    *found = 0;
    for (int i = 0; i < 4; i++) coef[i] = 0.f;
    const float sigma = (float)p->sigma;
    const double share = p->thresh * (double)n;
    // deviation: a cloud whose triples are all colinear ends here, not never
    const uint64_t max_attempts = std::min<uint64_t>(11ull * (uint64_t)p->num_iteration, triples ? n_triples : ~0ull);
    const uint32_t score_blocks = (n + kThreads * kScoreItems - 1) / (kThreads * kScoreItems);
    uint32_t best = 0;
    uint64_t scored = 0;
    bool running = true;
    LIO_HIP_TRY(hipEventRecord(g->ev[2], st));
    while (running && scored < max_attempts) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(kBatch, max_attempts - scored);
        Batch& hb = *g->h_batch;
        for (uint32_t t = 0; t < nb; t++) {
            if (triples) memcpy(&hb.triples[3 * t], &triples[3 * (scored + t)], 3 * sizeof(uint32_t));
            else lio_ground_draw(p->seed, (uint32_t)(scored + t), n, &hb.triples[3 * t]);
        }
        LIO_HIP_TRY(hipMemcpyAsync(g->d_batch->triples, hb.triples, 3ull * nb * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        LIO_HIP_TRY(hipEventRecord(g->ev[4], st));
        cg_planes<<<dim3(1), dim3(kBatch), 0, st>>>(g->cpt, nb, g->d_batch);
        LIO_HIP_TRY(hipEventRecord(g->ev[5], st));
        cg_score<<<dim3(score_blocks), dim3(kThreads), 0, st>>>(g->cpt, n, nb, g->d_batch, sigma);
        LIO_HIP_TRY(hipGetLastError());
        LIO_HIP_TRY(hipEventRecord(g->ev[6], st));
        LIO_HIP_TRY(hipMemcpyAsync(g->h_batch, g->d_batch, sizeof(Batch), hipMemcpyDeviceToHost, st));
        LIO_HIP_TRY(hipStreamSynchronize(st));
        g->planes_us += elapsed_us(g->ev[4], g->ev[5]);
        g->score_us += elapsed_us(g->ev[5], g->ev[6]);
        g->log_triples->insert(g->log_triples->end(), hb.triples, hb.triples + 3 * nb);
        g->log_colinear->insert(g->log_colinear->end(), hb.colinear, hb.colinear + nb);
        g->log_counts->insert(g->log_counts->end(), hb.counts, hb.counts + nb);
        g->log_planes->insert(g->log_planes->end(), hb.planes, hb.planes + 4 * nb);
        // fit_plane's loop over this batch's attempts, in order
        for (uint32_t t = 0; t < nb; t++) {
            const int attempt = (int)(scored + t);
            g->attempts++;
            if (hb.colinear[t]) { g->skipped++; continue; }
            g->iterations++;
            const uint32_t c = hb.counts[t];
            if ((double)c > share) {
                g->winner = attempt;
                g->early_exit = 1;
                running = false;
                break;
            }
            if (c > best) {
                best = c;
                g->winner = attempt;
            }
            if (g->iterations >= p->num_iteration) { running = false; break; }
        }
        scored += nb;
    }
    LIO_HIP_TRY(hipEventRecord(g->ev[3], st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    g->fit_us = elapsed_us(g->ev[2], g->ev[3]);
    if (g->winner >= 0) {
        memcpy(coef, g->log_planes->data() + 4ull * (uint32_t)g->winner, 4 * sizeof(float));
        g->found = *found = 1;
    }
    return LIO_OK;
}

int64_t lio_calib_ground_download_indices(lio_calib_ground* g, uint32_t* out, uint64_t cap) {
    if (!g) return LIO_E_INVALID;
    return download("lio_calib_ground", g->device, g->stream, g->cidx, g->n_kept, out, cap);
}

int64_t lio_calib_ground_download_points(lio_calib_ground* g, float* xyz, uint64_t cap) {
    if (!g) return LIO_E_INVALID;
    const uint64_t n = g->n_kept;
    if (n > cap) return -(int64_t)n;
    if (n == 0) return 0;
    if (!xyz) return LIO_E_INVALID;
    hipSetDevice(g->device);
    std::vector<float4> tmp(n);
    LIO_HIP_TRY(hipMemcpyAsync(tmp.data(), g->cpt, n * sizeof(float4), hipMemcpyDeviceToHost, g->stream));
    LIO_HIP_TRY(hipStreamSynchronize(g->stream));
    for (uint64_t i = 0; i < n; i++) { xyz[3 * i] = tmp[i].x; xyz[3 * i + 1] = tmp[i].y; xyz[3 * i + 2] = tmp[i].z; }
    return (int64_t)n;
}

int64_t lio_calib_ground_download_draws(lio_calib_ground* g, uint32_t* triples, uint32_t* colinear, uint32_t* counts, float* planes, uint64_t cap) {
    if (!g) return LIO_E_INVALID;
    const uint64_t n = g->log_counts->size();
    if (n > cap) return -(int64_t)n;
    if (n && triples) memcpy(triples, g->log_triples->data(), 3 * n * sizeof(uint32_t));
    if (n && colinear) memcpy(colinear, g->log_colinear->data(), n * sizeof(uint32_t));
    if (n && counts) memcpy(counts, g->log_counts->data(), n * sizeof(uint32_t));
    if (n && planes) memcpy(planes, g->log_planes->data(), 4 * n * sizeof(float));
    return (int64_t)n;
}

int lio_calib_ground_last_run(lio_calib_ground* g, int* iterations, int* attempts, int* skipped, int* winner, int* early_exit) {
    if (!g) return LIO_E_INVALID;
    if (iterations) *iterations = g->iterations;
    if (attempts) *attempts = g->attempts;
    if (skipped) *skipped = g->skipped;
    if (winner) *winner = g->winner;
    if (early_exit) *early_exit = g->early_exit;
    return LIO_OK;
}

int lio_calib_ground_last_times(lio_calib_ground* g, double* crop_us, double* fit_us, double* planes_us, double* score_us) {
    if (!g) return LIO_E_INVALID;
    if (crop_us) *crop_us = g->crop_us;
    if (fit_us) *fit_us = g->fit_us;
    if (planes_us) *planes_us = g->planes_us;
    if (score_us) *score_us = g->score_us;
    return LIO_OK;
}

}  // extern "C"
