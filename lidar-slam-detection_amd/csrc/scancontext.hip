// scancontext.hip -- the Scan Context bank and its searches on gfx950 (wave64): SCManager of the reference's relocalisation
// (slam/common/Scancontext/Scancontext.cpp, "SC") and GlobalLocalization::globalSearch (slam/localization/src/global_localization.cpp:387-413);
// include/lio_hip.h states the rules, tests/sc_cases.py restates them in numpy.
//
//   describe   makeScancontext (SC:159-199) for many clouds, or for one cloud under several (dx, dy) shifts, in one set of launches.  A table
//              row = (descriptor set, first point, points): a workgroup takes that slice and bins it under EVERY shift of the call into LDS --
//              a bin holds the order-preserving u32 image of the largest f32 height seen, integer atomicMax -- then merges what it touched into
//              the call's bins in global memory with integer atomicMax.  A maximum does not depend on the order it was taken in, so neither the
//              slice length nor the launch geometry shows in the result.  sc_finish (one wave per descriptor, a lane per column) turns the
//              bins that never rose above -1000 into 0, widens to f64 and writes the ring key, the sector key and the column norms
//   ring keys  f32 squared distances to the active frames in nanoflann's L2_Adaptor grouping as keys (distance bits << 32 | id), then the 10
//              smallest per query by ten rounds of a workgroup minimum over the keys above the last one taken: equal distances go to the smaller id
//   distance   distanceBtnScanContext (SC:124-156): one wave per (query, candidate) pair, both descriptors in LDS.  Lane s takes the sector-key
//              difference under shift s (60 terms in column order); lane j the column cosine of column j under each of the seven shifts (20
//              terms in row order); lanes 0..6 add a shift's 60 cosines in column order.  Every sum is sequential: with -ffp-contract=off the
//              result is the restatement's to the last bit
//   local      GlobalLocalization::localSearch (global_localization.cpp:350-385): the key frames' positions lie beside the descriptors; a key per
//              frame (f32 squared distance to the INS position << 32 | id), the same selection, the same distance kernel over the bank's rows
//              by id, and the walk over at most ten rows on the host
// No floating-point atomics; no workgroup waits for another.
#include <cfloat>
#include <cmath>
#include <vector>

#include "lio_common.h"

namespace lio {
namespace sc {

constexpr int kRings = LIO_SC_RINGS, kSectors = LIO_SC_SECTORS, kBins = kRings * kSectors, kCand = LIO_SC_CANDIDATES, kMaxShifts = LIO_SC_MAX_SHIFTS;
constexpr int kThreads = 256, kSlice = 2048;  // points of a table row
constexpr uint32_t kEmptyBin = 0x3B85FFFFu;   // enc(-1000.0f)
constexpr double kBig = 10000000.0;           // SC:104,142,269
constexpr unsigned long long kNoKey = 0xFFFFFFFFFFFFFFFFull;

// u32 image of an f32 whose unsigned order is the floats' order (-0 below +0, which no height can be: z + 0.5 == 0 only as +0)
__host__ __device__ __forceinline__ uint32_t enc(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float dec(uint32_t u) {
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

struct Shifts {
    int n;
    double dx[kMaxShifts], dy[kMaxShifts];
};

// SC:21-36 under the project's rule: the quotient in f32, atan and the scaling in f64, one rounding to f32 at the return
__device__ __forceinline__ float xy2theta(float x, float y) {
    const double k = 180.0 / M_PI;
    if (x >= 0.f && y >= 0.f) return (float)(k * atan((double)(y / x)));
    if (x < 0.f && y >= 0.f) return (float)(180.0 - k * atan((double)(y / (-x))));
    if (x < 0.f && y < 0.f) return (float)(180.0 + k * atan((double)(y / x)));
    if (x >= 0.f && y < 0.f) return (float)(360.0 - k * atan((double)((-y) / x)));
    return 0.f;
}

// max(min(N, int(ceil(v))), 1) with what is not a number at 1 (the origin's 0 / 0)
__device__ __forceinline__ int clamp_ceil(double v, int n) {
    const double c = ceil(v);
    if (!(c >= 1.0)) return 1;
    return c > (double)n ? n : (int)c;
}

// tab[blockIdx.x] = {descriptor set, first point, points, -}.  bins: [set][shift][kBins], filled with kEmptyBin before the launch
__global__ void __launch_bounds__(kThreads) sc_describe(const uint4* __restrict__ tab, const float4* __restrict__ pts, Shifts sh, uint32_t* __restrict__ bins,
                                                        unsigned long long* __restrict__ n_nonfinite) {
    __shared__ uint32_t lb[kMaxShifts * kBins];
    __shared__ uint32_t bad;
    const uint4 tb = tab[blockIdx.x];
    const int nb = sh.n * kBins;
    for (int b = threadIdx.x; b < nb; b += kThreads) lb[b] = kEmptyBin;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    uint32_t my_bad = 0;
    for (uint32_t k = threadIdx.x; k < tb.z; k += kThreads) {
        const float4 p = pts[tb.y + k];
        if (!(p.x - p.x == 0.f && p.y - p.y == 0.f && p.z - p.z == 0.f)) { my_bad++; continue; }
        const float z = (float)((double)p.z + 0.5);
        const uint32_t ze = enc(z);
        for (int s = 0; s < sh.n; s++) {
            const float x = (float)((double)p.x + sh.dx[s]), y = (float)((double)p.y + sh.dy[s]);
            const float xx = x * x, yy = y * y;
            const float range = sqrtf(xx + yy);
            if ((double)range > 80.0) continue;
            const float theta = xy2theta(x, y);
            const int ring = clamp_ceil(((double)range / 80.0) * 20.0, kRings);
            const int sector = clamp_ceil(((double)theta / 360.0) * 60.0, kSectors);
            atomicMax(&lb[s * kBins + (ring - 1) * kSectors + (sector - 1)], ze);
        }
    }
    if (my_bad) atomicAdd(&bad, my_bad);
    __syncthreads();
    uint32_t* __restrict__ out = bins + (size_t)tb.x * nb;
    for (int b = threadIdx.x; b < nb; b += kThreads)
        if (lb[b] > kEmptyBin) atomicMax(&out[b], lb[b]);
    if (threadIdx.x == 0 && bad) atomicAdd(n_nonfinite, (unsigned long long)bad);
}

// keys of the descriptor in d[kRings][kSectors] (LDS), lane = threadIdx.x of one wave: SC:202-231 with sequential sums, and the column norms
__device__ __forceinline__ void keys_of(const double (*d)[kSectors], int lane, float* __restrict__ ring, double* __restrict__ sector, double* __restrict__ norm) {
    if (lane < kSectors) {
        double s = 0.0, q = 0.0;
        for (int r = 0; r < kRings; r++) { const double v = d[r][lane]; s = s + v; q = q + v * v; }
        sector[lane] = s / (double)kRings;
        norm[lane] = sqrt(q);
    }
    if (ring && lane < kRings) {
        double s = 0.0;
        for (int c = 0; c < kSectors; c++) s = s + d[lane][c];
        ring[lane] = (float)(s / (double)kSectors);
    }
}

// descriptor blockIdx.x of the call: from its bins (BINS) or from a descriptor already at desc (keys only)
template <bool BINS>
__global__ void __launch_bounds__(64) sc_finish(const uint32_t* __restrict__ bins, double* __restrict__ desc, float* __restrict__ ring, double* __restrict__ sector,
                                                double* __restrict__ norm) {
    __shared__ double d[kRings][kSectors];
    const size_t k = blockIdx.x;
    double* __restrict__ dk = desc + k * kBins;
    for (int b = threadIdx.x; b < kBins; b += 64) {
        double v;
        if (BINS) {
            const uint32_t u = bins[k * kBins + b];
            v = u == kEmptyBin ? 0.0 : (double)dec(u);
            dk[b] = v;
        } else {
            v = dk[b];
        }
        d[b / kSectors][b % kSectors] = v;
    }
    __syncthreads();
    keys_of(d, threadIdx.x, ring ? ring + k * kRings : nullptr, sector + k * kSectors, norm + k * kSectors);
}

// nanoflann's L2_Adaptor::evalMetric over 20 floats: five groups of four, result += ((d0*d0 + d1*d1) + d2*d2) + d3*d3
__device__ __forceinline__ float ring_dist(const float* __restrict__ a, const float* __restrict__ b) {
    float result = 0.f;
    for (int g = 0; g < kRings; g += 4) {
        const float d0 = a[g] - b[g], d1 = a[g + 1] - b[g + 1], d2 = a[g + 2] - b[g + 2], d3 = a[g + 3] - b[g + 3];
        result += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
    }
    return result;
}

// keys[q][i] = distance bits << 32 | bank id of active frame i (active == null: the bank's first n frames)
__global__ void __launch_bounds__(kThreads) sc_ring_keys(const float* __restrict__ qring, const float* __restrict__ bank_ring, const int32_t* __restrict__ active,
                                                         uint32_t n_active, unsigned long long* __restrict__ keys) {
    __shared__ float q[kRings];
    if (threadIdx.x < kRings) q[threadIdx.x] = qring[(size_t)blockIdx.y * kRings + threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_active) return;
    const uint32_t id = active ? (uint32_t)active[i] : i;
    float b[kRings];
    const float4* __restrict__ br = reinterpret_cast<const float4*>(bank_ring + (size_t)id * kRings);
#pragma unroll
    for (int g = 0; g < kRings / 4; g++) { const float4 v = br[g]; b[4 * g] = v.x; b[4 * g + 1] = v.y; b[4 * g + 2] = v.z; b[4 * g + 3] = v.w; }
    const float d = ring_dist(q, b);
    keys[(size_t)blockIdx.y * n_active + i] = ((unsigned long long)__float_as_uint(d) << 32) | id;
}

// localSearch's kd-tree query: keys[i] = f32 squared distance bits << 32 | i of frame i's position (pos: n x 3) to (qx, qy, 0) -- the query's z is
// 0, the frame keeps its own.  A squared distance is never negative, so its bits order as the floats do (what is not a number: after all)
__global__ void __launch_bounds__(kThreads) sc_pos_keys(const float* __restrict__ pos, uint32_t n, float qx, float qy, unsigned long long* __restrict__ keys) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float dx = pos[3 * (size_t)i] - qx, dy = pos[3 * (size_t)i + 1] - qy, dz = pos[3 * (size_t)i + 2];
    const float d2 = ((dx * dx) + dy * dy) + dz * dz;
    keys[i] = ((unsigned long long)(__float_as_uint(d2) & 0x7FFFFFFFu) << 32) | i;
}

// the kCand smallest keys of query blockIdx.x in rising order; cand[q][k] = id or -1, cand_d[q][k] = the f32 distance
__global__ void __launch_bounds__(kThreads) sc_ring_select(const unsigned long long* __restrict__ keys, uint32_t n_active, int32_t* __restrict__ cand,
                                                           float* __restrict__ cand_d) {
    __shared__ unsigned long long wmin[kThreads / 64];
    const unsigned long long* __restrict__ kq = keys + (size_t)blockIdx.x * n_active;
    unsigned long long last = 0;
    bool have = false;
    for (int k = 0; k < kCand; k++) {
        unsigned long long m = kNoKey;
        for (uint32_t i = threadIdx.x; i < n_active; i += kThreads) {
            const unsigned long long v = kq[i];
            if ((!have || v > last) && v < m) m = v;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(m, off);
            m = o < m ? o : m;
        }
        if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = m;
        __syncthreads();
        m = wmin[0];
        for (int w = 1; w < kThreads / 64; w++) m = wmin[w] < m ? wmin[w] : m;
        __syncthreads();
        if (threadIdx.x == 0) {
            cand[(size_t)blockIdx.x * kCand + k] = m == kNoKey ? -1 : (int32_t)(uint32_t)m;
            cand_d[(size_t)blockIdx.x * kCand + k] = m == kNoKey ? INFINITY : __uint_as_float((uint32_t)(m >> 32));
        }
        last = m;
        have = true;
        if (m == kNoKey) {  // fewer than kCand active frames: the rest is empty
            if (threadIdx.x == 0)
                for (int r = k + 1; r < kCand; r++) { cand[(size_t)blockIdx.x * kCand + r] = -1; cand_d[(size_t)blockIdx.x * kCand + r] = INFINITY; }
            break;
        }
    }
}

struct DescSet {  // descriptors with their sector keys and column norms
    const double *desc, *sector, *norm;
};

// pair blockIdx.x: A[ia] against B[ib] (pairs == null: A[k] against B[k]); ib < 0: no candidate, {NaN, -1}
__global__ void __launch_bounds__(64) sc_distance(DescSet A, DescSet B, const int32_t* __restrict__ ia, const int32_t* __restrict__ ib, double* __restrict__ dist,
                                                  int32_t* __restrict__ shift) {
    __shared__ double a[kRings][kSectors], b[kRings][kSectors];
    __shared__ double va[kSectors], vb[kSectors], na[kSectors], nb[kSectors];
    __shared__ double vdiff[kSectors];
    __shared__ double cosv[7][kSectors];
    __shared__ double sdist[7];
    __shared__ int shifts[7];
    const int lane = threadIdx.x;
    const size_t k = blockIdx.x;
    const int32_t qa = ia ? ia[k] : (int32_t)k, qb = ib ? ib[k] : (int32_t)k;
    if (qb < 0 || qa < 0) {
        if (lane == 0) { dist[k] = (double)NAN; shift[k] = -1; }
        return;
    }
    const double* __restrict__ da = A.desc + (size_t)qa * kBins;
    const double* __restrict__ db = B.desc + (size_t)qb * kBins;
    for (int i = lane; i < kBins; i += 64) { a[i / kSectors][i % kSectors] = da[i]; b[i / kSectors][i % kSectors] = db[i]; }
    if (lane < kSectors) {
        va[lane] = A.sector[(size_t)qa * kSectors + lane]; na[lane] = A.norm[(size_t)qa * kSectors + lane];
        vb[lane] = B.sector[(size_t)qb * kSectors + lane]; nb[lane] = B.norm[(size_t)qb * kSectors + lane];
    }
    __syncthreads();
    // fastAlignUsingVkey (SC:101-121): lane = shift
    if (lane < kSectors) {
        double s = 0.0;
        for (int j = 0; j < kSectors; j++) {
            const double d = va[j] - vb[(j - lane + kSectors) % kSectors];
            s = s + d * d;
        }
        vdiff[lane] = sqrt(s);
    }
    __syncthreads();
    if (lane == 0) {
        int arg = 0;
        double best = kBig;
        for (int s = 0; s < kSectors; s++)
            if (vdiff[s] < best) { arg = s; best = vdiff[s]; }
        // SC:131-138: the shift and its three neighbours on either side, rising
        int v[7];
        v[0] = arg;
        for (int ii = 1; ii <= 3; ii++) { v[2 * ii - 1] = (arg + ii + kSectors) % kSectors; v[2 * ii] = (arg - ii + kSectors) % kSectors; }
        for (int i = 1; i < 7; i++) {
            const int x = v[i];
            int j = i - 1;
            while (j >= 0 && v[j] > x) { v[j + 1] = v[j]; j--; }
            v[j + 1] = x;
        }
        for (int i = 0; i < 7; i++) shifts[i] = v[i];
    }
    __syncthreads();
    // distDirectSC (SC:77-98): lane = column of the first descriptor
    if (lane < kSectors) {
        for (int t = 0; t < 7; t++) {
            const int jb = (lane - shifts[t] + kSectors) % kSectors;
            double c = (double)NAN;  // a skipped pair
            if (!(na[lane] == 0.0 || nb[jb] == 0.0)) {
                double dot = 0.0;
                for (int r = 0; r < kRings; r++) dot = dot + a[r][lane] * b[r][jb];
                c = dot / (na[lane] * nb[jb]);
            }
            cosv[t][lane] = c;
        }
    }
    __syncthreads();
    if (lane < 7) {
        double sum = 0.0;
        int cnt = 0;
        for (int j = 0; j < kSectors; j++) {
            const int jb = (j - shifts[lane] + kSectors) % kSectors;
            if (na[j] == 0.0 || nb[jb] == 0.0) continue;
            sum = sum + cosv[lane][j];
            cnt++;
        }
        sdist[lane] = 1.0 - sum / (double)cnt;  // cnt == 0: 0 / 0, which wins no `<`
    }
    __syncthreads();
    if (lane == 0) {
        int arg = 0;
        double best = kBig;
        for (int t = 0; t < 7; t++)
            if (sdist[t] < best) { arg = shifts[t]; best = sdist[t]; }
        dist[k] = best;
        shift[k] = arg;
    }
}

}  // namespace sc
}  // namespace lio

using namespace lio;
using namespace lio::sc;

struct lio_sc {
    int device = 0;
    hipStream_t st = nullptr;
    uint32_t max_frames = 0, max_points = 0, n_frames = 0;
    // the bank
    double *desc = nullptr, *sector = nullptr, *norm = nullptr;
    float* ring = nullptr;
    float* pos = nullptr;  // the key frames' positions, n_pos rows
    uint32_t n_pos = 0;
    int32_t* d_active = nullptr;
    std::vector<int32_t> active;
    bool all_active = true;
    // a call's clouds, table and bins
    float4* pts = nullptr;
    uint4 *d_tab = nullptr, *h_tab = nullptr;
    uint64_t tab_cap = 0;
    uint32_t* bins = nullptr;
    uint64_t bins_cap = 0;  // descriptors
    unsigned long long* d_bad = nullptr;
    uint64_t n_bad = 0;
    // query side: descriptors handed in or described here (A), a second set for lio_sc_distance (B)
    uint64_t q_cap = 0;
    double *q_desc[2] = {nullptr, nullptr}, *q_sector[2] = {nullptr, nullptr}, *q_norm[2] = {nullptr, nullptr};
    float* q_ring = nullptr;
    unsigned long long* keys = nullptr;
    uint64_t keys_cap = 0;
    int32_t *cand = nullptr, *cand_q = nullptr, *cand_shift = nullptr;
    float* cand_rd = nullptr;
    double* cand_dist = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double t_describe = 0, t_ring = 0, t_dist = 0;
    // the last local search
    int32_t loc_n = 0, loc_ids[kCand], loc_shift[kCand], loc_match_shift = 0;
    float loc_d2[kCand];
    double loc_dist[kCand];
};

namespace {

struct Span {  // HIP events around a stretch of work on the handle's stream
    lio_sc* h;
    double* acc;
    Span(lio_sc* h_, double* a) : h(h_), acc(a) { hipEventRecord(h->ev[0], h->st); }
    ~Span() {
        float ms = 0.f;
        if (hipEventRecord(h->ev[1], h->st) == hipSuccess && hipEventSynchronize(h->ev[1]) == hipSuccess && hipEventElapsedTime(&ms, h->ev[0], h->ev[1]) == hipSuccess)
            *acc += (double)ms * 1000.0;
    }
};

template <typename T>
int regrow(T** p, uint64_t n, bool host = false) {
    if (*p) { if (host) hipHostFree(*p); else hipFree(*p); *p = nullptr; }
    const hipError_t e = host ? hipHostMalloc(reinterpret_cast<void**>(p), n * sizeof(T), hipHostMallocDefault) : hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T));
    if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; set_error("lio_sc: allocation of %llu bytes failed", (unsigned long long)(n * sizeof(T))); return LIO_E_DEVICE; }
    return LIO_OK;
}

int reserve_tab(lio_sc* h, uint64_t rows) {
    if (rows <= h->tab_cap) return LIO_OK;
    LIO_HIP_TRY(hipStreamSynchronize(h->st));
    uint64_t c = h->tab_cap ? h->tab_cap : 1024;
    while (c < rows) c *= 2;
    h->tab_cap = 0;
    int rc = regrow(&h->d_tab, c);
    if (rc == LIO_OK) rc = regrow(&h->h_tab, c, true);
    if (rc != LIO_OK) return rc;
    h->tab_cap = c;
    return LIO_OK;
}

int reserve_bins(lio_sc* h, uint64_t n_desc) {
    if (n_desc <= h->bins_cap) return LIO_OK;
    LIO_HIP_TRY(hipStreamSynchronize(h->st));
    uint64_t c = h->bins_cap ? h->bins_cap : 64;
    while (c < n_desc) c *= 2;
    h->bins_cap = 0;
    const int rc = regrow(&h->bins, c * kBins);
    if (rc != LIO_OK) return rc;
    h->bins_cap = c;
    return LIO_OK;
}

// room for n query descriptors in both sets, their candidates and results
int reserve_queries(lio_sc* h, uint64_t n) {
    if (n <= h->q_cap) return LIO_OK;
    LIO_HIP_TRY(hipStreamSynchronize(h->st));
    uint64_t c = h->q_cap ? h->q_cap : 16;
    while (c < n) c *= 2;
    h->q_cap = 0;
    int rc = LIO_OK;
    for (int s = 0; s < 2 && rc == LIO_OK; s++) {
        rc = regrow(&h->q_desc[s], c * kBins);
        if (rc == LIO_OK) rc = regrow(&h->q_sector[s], c * kSectors);
        if (rc == LIO_OK) rc = regrow(&h->q_norm[s], c * kSectors);
    }
    if (rc == LIO_OK) rc = regrow(&h->q_ring, c * kRings);
    if (rc == LIO_OK) rc = regrow(&h->cand, c * kCand);
    if (rc == LIO_OK) rc = regrow(&h->cand_q, c * kCand);
    if (rc == LIO_OK) rc = regrow(&h->cand_shift, c * kCand);
    if (rc == LIO_OK) rc = regrow(&h->cand_rd, c * kCand);
    if (rc == LIO_OK) rc = regrow(&h->cand_dist, c * kCand);
    if (rc != LIO_OK) return rc;
    h->q_cap = c;
    return LIO_OK;
}

// describe the clouds staged in h->pts: set k is points [off[k], off[k + 1]) under every shift; descriptor (k, s) goes to place k * sh.n + s of the outputs
int describe_staged(lio_sc* h, const uint64_t* off, uint32_t n_sets, const Shifts& sh, double* desc, float* ring, double* sector, double* norm) {
    const uint64_t n_desc = (uint64_t)n_sets * sh.n;
    if (n_desc == 0) return LIO_OK;
    uint64_t rows = 0;
    for (uint32_t k = 0; k < n_sets; k++) rows += (off[k + 1] - off[k] + kSlice - 1) / kSlice;
    int rc = reserve_tab(h, rows);
    if (rc == LIO_OK) rc = reserve_bins(h, n_desc);
    if (rc != LIO_OK) return rc;
    uint64_t r = 0;
    for (uint32_t k = 0; k < n_sets; k++)
        for (uint64_t p0 = off[k]; p0 < off[k + 1]; p0 += kSlice) h->h_tab[r++] = make_uint4(k, (uint32_t)(p0 - off[0]), (uint32_t)std::min<uint64_t>(kSlice, off[k + 1] - p0), 0);
    LIO_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->bins), (int)kEmptyBin, n_desc * kBins, h->st));
    if (rows) {
        LIO_HIP_TRY(hipMemcpyAsync(h->d_tab, h->h_tab, sizeof(uint4) * rows, hipMemcpyHostToDevice, h->st));
        hipLaunchKernelGGL(sc_describe, (uint32_t)rows, kThreads, 0, h->st, h->d_tab, h->pts, sh, h->bins, h->d_bad);
    }
    hipLaunchKernelGGL(sc_finish<true>, (uint32_t)n_desc, 64, 0, h->st, h->bins, desc, ring, sector, norm);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipStreamSynchronize(h->st));  // the pinned table is rewritten by the next call
    return LIO_OK;
}

int read_bad(lio_sc* h) {
    unsigned long long v = 0;
    LIO_HIP_TRY(hipMemcpy(&v, h->d_bad, sizeof(v), hipMemcpyDeviceToHost));
    h->n_bad = v;
    return LIO_OK;
}

int stage_cloud(lio_sc* h, const float* xyzi, uint64_t n) {
    if (n) LIO_HIP_TRY(hipMemcpyAsync(h->pts, xyzi, n * sizeof(float4), hipMemcpyHostToDevice, h->st));
    return LIO_OK;
}

uint32_t n_active_of(const lio_sc* h) { return h->all_active ? h->n_frames : (uint32_t)h->active.size(); }

// candidates, distances and shifts of the n queries in set A (their ring keys in q_ring) against the active frames; results stay on the device
int search_staged(lio_sc* h, uint32_t n) {
    const uint32_t na = n_active_of(h);
    {
        Span sp(h, &h->t_ring);
        if (na) {
            const uint64_t need = (uint64_t)n * na;
            if (need > h->keys_cap) {
                LIO_HIP_TRY(hipStreamSynchronize(h->st));
                h->keys_cap = 0;
                const int rc = regrow(&h->keys, need);
                if (rc != LIO_OK) return rc;
                h->keys_cap = need;
            }
            hipLaunchKernelGGL(sc_ring_keys, dim3((na + kThreads - 1) / kThreads, n), kThreads, 0, h->st, h->q_ring, h->ring, h->all_active ? nullptr : h->d_active, na, h->keys);
        }
        hipLaunchKernelGGL(sc_ring_select, n, kThreads, 0, h->st, h->keys, na, h->cand, h->cand_rd);
        LIO_HIP_TRY(hipGetLastError());
    }
    {
        Span sp(h, &h->t_dist);
        std::vector<int32_t> qa((size_t)n * kCand);
        for (size_t i = 0; i < qa.size(); i++) qa[i] = (int32_t)(i / kCand);
        LIO_HIP_TRY(hipMemcpyAsync(h->cand_q, qa.data(), qa.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->st));
        const DescSet A{h->q_desc[0], h->q_sector[0], h->q_norm[0]}, B{h->desc, h->sector, h->norm};
        hipLaunchKernelGGL(sc_distance, n * kCand, 64, 0, h->st, A, B, h->cand_q, h->cand, h->cand_dist, h->cand_shift);
        LIO_HIP_TRY(hipGetLastError());
        LIO_HIP_TRY(hipStreamSynchronize(h->st));  // qa leaves scope
    }
    return LIO_OK;
}

}  // namespace

extern "C" {

lio_sc* lio_sc_create(int device, uint32_t max_frames, uint32_t max_points_per_call) {
    if (max_frames == 0 || max_points_per_call == 0 || max_frames > 0x7FFFFFFFu) { set_error("lio_sc_create: 1 <= max_frames < 2^31, max_points_per_call >= 1"); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); set_error("lio_sc_create: no HIP device %d (this library has no CPU fallback)", device); return nullptr; }
    lio_sc* h = new lio_sc();
    h->device = device;
    h->max_frames = max_frames;
    h->max_points = max_points_per_call;
    bool ok = hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) == hipSuccess && hipEventCreate(&h->ev[0]) == hipSuccess && hipEventCreate(&h->ev[1]) == hipSuccess;
    ok = ok && regrow(&h->desc, (uint64_t)max_frames * kBins) == LIO_OK && regrow(&h->sector, (uint64_t)max_frames * kSectors) == LIO_OK &&
         regrow(&h->norm, (uint64_t)max_frames * kSectors) == LIO_OK && regrow(&h->ring, (uint64_t)max_frames * kRings) == LIO_OK && regrow(&h->pos, (uint64_t)max_frames * 3) == LIO_OK &&
         regrow(&h->d_active, (uint64_t)max_frames) == LIO_OK && regrow(&h->pts, (uint64_t)max_points_per_call) == LIO_OK && regrow(&h->d_bad, 1) == LIO_OK &&
         regrow(&h->keys, 1) == LIO_OK;
    if (!ok) {
        if (h->st) set_error("lio_sc_create: allocation failed");
        else set_error("lio_sc_create: no stream on HIP device %d", device);
        lio_sc_destroy(h);
        return nullptr;
    }
    h->keys_cap = 1;
    return h;
}

void lio_sc_destroy(lio_sc* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->st) hipStreamSynchronize(h->st);
    hipFree(h->desc); hipFree(h->sector); hipFree(h->norm); hipFree(h->ring); hipFree(h->pos); hipFree(h->d_active); hipFree(h->pts); hipFree(h->d_tab); hipFree(h->bins); hipFree(h->d_bad);
    for (int s = 0; s < 2; s++) { hipFree(h->q_desc[s]); hipFree(h->q_sector[s]); hipFree(h->q_norm[s]); }
    hipFree(h->q_ring); hipFree(h->keys); hipFree(h->cand); hipFree(h->cand_q); hipFree(h->cand_shift); hipFree(h->cand_rd); hipFree(h->cand_dist);
    if (h->h_tab) hipHostFree(h->h_tab);
    for (int i = 0; i < 2; i++)
        if (h->ev[i]) hipEventDestroy(h->ev[i]);
    if (h->st) hipStreamDestroy(h->st);
    delete h;
}

int lio_sc_reset(lio_sc* h) {
    if (!h) return LIO_E_INVALID;
    h->n_frames = 0;
    h->n_pos = 0;
    h->active.clear();
    h->all_active = true;
    return LIO_OK;
}

int lio_sc_num_frames(lio_sc* h) { return h ? (int)h->n_frames : LIO_E_INVALID; }

int lio_sc_add_frames_host(lio_sc* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames) {
    if (!h || !offsets) return LIO_E_INVALID;
    for (uint32_t k = 0; k < n_frames; k++) {
        if (offsets[k + 1] < offsets[k]) { set_error("lio_sc_add_frames_host: offsets must not fall"); return LIO_E_INVALID; }
        if (offsets[k + 1] - offsets[k] > h->max_points) { set_error("lio_sc_add_frames_host: frame %u has %llu points, max_points_per_call is %u", k, (unsigned long long)(offsets[k + 1] - offsets[k]), h->max_points); return LIO_E_CAPACITY; }
    }
    if (n_frames && offsets[n_frames] > offsets[0] && !xyzi) return LIO_E_INVALID;
    if ((uint64_t)h->n_frames + n_frames > h->max_frames) { set_error("lio_sc_add_frames_host: %u + %u frames exceed max_frames %u", h->n_frames, n_frames, h->max_frames); return LIO_E_CAPACITY; }
    hipSetDevice(h->device);
    h->t_describe = 0;
    LIO_HIP_TRY(hipMemsetAsync(h->d_bad, 0, sizeof(unsigned long long), h->st));
    const int first = (int)h->n_frames;
    Shifts sh;
    memset(&sh, 0, sizeof(sh));
    sh.n = 1;
    // launch sets of as many whole frames as fit max_points_per_call
    for (uint32_t k0 = 0; k0 < n_frames;) {
        uint32_t k1 = k0 + 1;
        while (k1 < n_frames && offsets[k1 + 1] - offsets[k0] <= h->max_points) k1++;
        Span sp(h, &h->t_describe);
        int rc = stage_cloud(h, xyzi + 4 * offsets[k0], offsets[k1] - offsets[k0]);
        const size_t at = (size_t)first + k0;
        if (rc == LIO_OK) rc = describe_staged(h, offsets + k0, k1 - k0, sh, h->desc + at * kBins, h->ring + at * kRings, h->sector + at * kSectors, h->norm + at * kSectors);
        if (rc != LIO_OK) return rc;
        k0 = k1;
    }
    const int rc = read_bad(h);
    if (rc != LIO_OK) return rc;
    h->n_frames += n_frames;
    return first;
}

int lio_sc_download_frame(lio_sc* h, int id, double* desc, float* ringkey, double* sectorkey) {
    if (!h || id < 0 || (uint32_t)id >= h->n_frames) return LIO_E_INVALID;
    hipSetDevice(h->device);
    if (desc) LIO_HIP_TRY(hipMemcpy(desc, h->desc + (size_t)id * kBins, kBins * sizeof(double), hipMemcpyDeviceToHost));
    if (ringkey) LIO_HIP_TRY(hipMemcpy(ringkey, h->ring + (size_t)id * kRings, kRings * sizeof(float), hipMemcpyDeviceToHost));
    if (sectorkey) LIO_HIP_TRY(hipMemcpy(sectorkey, h->sector + (size_t)id * kSectors, kSectors * sizeof(double), hipMemcpyDeviceToHost));
    return LIO_OK;
}

static int describe_query(lio_sc* h, const char* who, const float* xyzi, uint32_t n, const double* shifts_xy, uint32_t n_shifts) {
    if (n > h->max_points) { set_error("%s: %u points, max_points_per_call is %u", who, n, h->max_points); return LIO_E_CAPACITY; }
    Shifts sh;
    memset(&sh, 0, sizeof(sh));
    sh.n = (int)n_shifts;
    for (uint32_t s = 0; s < n_shifts; s++) {
        sh.dx[s] = shifts_xy[2 * s]; sh.dy[s] = shifts_xy[2 * s + 1];
        if (!(sh.dx[s] - sh.dx[s] == 0.0 && sh.dy[s] - sh.dy[s] == 0.0)) { set_error("%s: a shift is not finite", who); return LIO_E_INVALID; }
    }
    int rc = reserve_queries(h, n_shifts);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipMemsetAsync(h->d_bad, 0, sizeof(unsigned long long), h->st));
    Span sp(h, &h->t_describe);
    rc = stage_cloud(h, xyzi, n);
    const uint64_t off[2] = {0, n};
    if (rc == LIO_OK) rc = describe_staged(h, off, 1, sh, h->q_desc[0], h->q_ring, h->q_sector[0], h->q_norm[0]);
    if (rc == LIO_OK) rc = read_bad(h);
    return rc;
}

int lio_sc_describe_host(lio_sc* h, const float* xyzi, uint32_t n, const double* shifts_xy, uint32_t n_shifts, double* desc, float* ringkey, double* sectorkey) {
    if (!h || (n && !xyzi) || !shifts_xy || n_shifts < 1 || n_shifts > (uint32_t)kMaxShifts) return LIO_E_INVALID;
    hipSetDevice(h->device);
    h->t_describe = 0;
    const int rc = describe_query(h, "lio_sc_describe_host", xyzi, n, shifts_xy, n_shifts);
    if (rc != LIO_OK) return rc;
    if (desc) LIO_HIP_TRY(hipMemcpy(desc, h->q_desc[0], (size_t)n_shifts * kBins * sizeof(double), hipMemcpyDeviceToHost));
    if (ringkey) LIO_HIP_TRY(hipMemcpy(ringkey, h->q_ring, (size_t)n_shifts * kRings * sizeof(float), hipMemcpyDeviceToHost));
    if (sectorkey) LIO_HIP_TRY(hipMemcpy(sectorkey, h->q_sector[0], (size_t)n_shifts * kSectors * sizeof(double), hipMemcpyDeviceToHost));
    return LIO_OK;
}

int lio_sc_set_active(lio_sc* h, const int32_t* ids, int32_t n) {
    if (!h || (n > 0 && !ids)) return LIO_E_INVALID;
    if (n < 0) { h->all_active = true; h->active.clear(); return LIO_OK; }
    std::vector<uint8_t> seen(h->n_frames, 0);
    for (int32_t k = 0; k < n; k++) {
        if (ids[k] < 0 || (uint32_t)ids[k] >= h->n_frames || seen[ids[k]]) { set_error("lio_sc_set_active: id %d is not a frame of the bank, or is named twice", ids[k]); return LIO_E_INVALID; }
        seen[ids[k]] = 1;
    }
    hipSetDevice(h->device);
    if (n) LIO_HIP_TRY(hipMemcpy(h->d_active, ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    h->active.assign(ids, ids + n);
    h->all_active = false;
    return LIO_OK;
}

int lio_sc_distance(lio_sc* h, const double* desc_a, const double* desc_b, uint32_t n_pairs, double* dist, int32_t* shift) {
    if (!h || (n_pairs && (!desc_a || !desc_b || !dist || !shift))) return LIO_E_INVALID;
    if (n_pairs == 0) return LIO_OK;
    hipSetDevice(h->device);
    int rc = reserve_queries(h, n_pairs);  // a pair takes a query's place in both descriptor sets
    if (rc != LIO_OK) return rc;
    h->t_dist = 0;
    Span sp(h, &h->t_dist);
    const size_t bytes = (size_t)n_pairs * kBins * sizeof(double);
    LIO_HIP_TRY(hipMemcpyAsync(h->q_desc[0], desc_a, bytes, hipMemcpyHostToDevice, h->st));
    LIO_HIP_TRY(hipMemcpyAsync(h->q_desc[1], desc_b, bytes, hipMemcpyHostToDevice, h->st));
    for (int s = 0; s < 2; s++) hipLaunchKernelGGL(sc_finish<false>, n_pairs, 64, 0, h->st, nullptr, h->q_desc[s], (float*)nullptr, h->q_sector[s], h->q_norm[s]);
    const DescSet A{h->q_desc[0], h->q_sector[0], h->q_norm[0]}, B{h->q_desc[1], h->q_sector[1], h->q_norm[1]};
    hipLaunchKernelGGL(sc_distance, n_pairs, 64, 0, h->st, A, B, (const int32_t*)nullptr, (const int32_t*)nullptr, h->cand_dist, h->cand_shift);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipMemcpyAsync(dist, h->cand_dist, (size_t)n_pairs * sizeof(double), hipMemcpyDeviceToHost, h->st));
    LIO_HIP_TRY(hipMemcpyAsync(shift, h->cand_shift, (size_t)n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
    LIO_HIP_TRY(hipStreamSynchronize(h->st));
    return LIO_OK;
}

static int download_candidates(lio_sc* h, uint32_t n, int32_t* cand_ids, double* cand_dist, int32_t* cand_shift, int32_t* n_cand) {
    const size_t m = (size_t)n * kCand;
    if (cand_ids) LIO_HIP_TRY(hipMemcpyAsync(cand_ids, h->cand, m * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
    if (cand_dist) LIO_HIP_TRY(hipMemcpyAsync(cand_dist, h->cand_dist, m * sizeof(double), hipMemcpyDeviceToHost, h->st));
    if (cand_shift) LIO_HIP_TRY(hipMemcpyAsync(cand_shift, h->cand_shift, m * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
    LIO_HIP_TRY(hipStreamSynchronize(h->st));
    const uint32_t na = n_active_of(h);
    if (n_cand)
        for (uint32_t q = 0; q < n; q++) n_cand[q] = (int32_t)(na < (uint32_t)kCand ? na : (uint32_t)kCand);
    return LIO_OK;
}

int lio_sc_search(lio_sc* h, const double* desc, const float* ringkey, uint32_t n_queries, int32_t* cand_ids, double* cand_dist, int32_t* cand_shift, int32_t* n_cand) {
    if (!h || (n_queries && (!desc || !ringkey))) return LIO_E_INVALID;
    if (n_queries == 0) return LIO_OK;
    if (n_queries > 65535u) { set_error("lio_sc_search: at most 65535 queries a call"); return LIO_E_CAPACITY; }
    hipSetDevice(h->device);
    int rc = reserve_queries(h, n_queries);
    if (rc != LIO_OK) return rc;
    h->t_ring = h->t_dist = 0;
    LIO_HIP_TRY(hipMemcpyAsync(h->q_desc[0], desc, (size_t)n_queries * kBins * sizeof(double), hipMemcpyHostToDevice, h->st));
    LIO_HIP_TRY(hipMemcpyAsync(h->q_ring, ringkey, (size_t)n_queries * kRings * sizeof(float), hipMemcpyHostToDevice, h->st));
    hipLaunchKernelGGL(sc_finish<false>, n_queries, 64, 0, h->st, nullptr, h->q_desc[0], (float*)nullptr, h->q_sector[0], h->q_norm[0]);
    LIO_HIP_TRY(hipGetLastError());
    rc = search_staged(h, n_queries);
    if (rc != LIO_OK) return rc;
    return download_candidates(h, n_queries, cand_ids, cand_dist, cand_shift, n_cand);
}

float lio_sc_shift_to_yaw(int32_t shift) {
    const float deg = (float)((double)shift * 6.0);  // SC:322: deg2rad(float) of nn_align * PC_UNIT_SECTORANGLE
    return (float)((double)deg * M_PI / 180.0);
}

int lio_sc_global_search_host(lio_sc* h, const float* xyzi, uint32_t n, double dist_thres, int32_t* match_id, float* yaw, double* score, int32_t* shift) {
    if (!h || (n && !xyzi)) return LIO_E_INVALID;
    hipSetDevice(h->device);
    h->t_describe = h->t_ring = h->t_dist = 0;
    static const double kSearch[2 * kMaxShifts] = {0, 0, -4, 0, 4, 0, 0, -4, 0, 4, -4, -4, -4, 4, 4, -4, 4, 4};  // global_localization.cpp:388-390
    int rc = describe_query(h, "lio_sc_global_search_host", xyzi, n, kSearch, kMaxShifts);
    if (rc != LIO_OK) return rc;
    rc = search_staged(h, kMaxShifts);
    if (rc != LIO_OK) return rc;
    int32_t ids[kMaxShifts * kCand], sh[kMaxShifts * kCand];
    double d[kMaxShifts * kCand];
    rc = download_candidates(h, kMaxShifts, ids, d, sh, nullptr);
    if (rc != LIO_OK) return rc;
    const uint32_t na = n_active_of(h);
    const int nc = (int)(na < (uint32_t)kCand ? na : (uint32_t)kCand);
    // globalSearch over detectClosestMatch (SC:262-326): both keep the first of equal scores
    double min_dist = DBL_MAX;
    int32_t best_id = -1, best_shift = 0;
    for (int q = 0; q < kMaxShifts; q++) {
        double sc_dist = 1.0;  // global_localization.cpp:397: what an empty bank leaves
        int32_t id = -1, align = 0;
        if (nc > 0) {
            double m = kBig;
            int32_t nn_idx = 0;
            for (int c = 0; c < nc; c++)
                if (d[q * kCand + c] < m) { m = d[q * kCand + c]; align = sh[q * kCand + c]; nn_idx = ids[q * kCand + c]; }
            sc_dist = m;
            if (m < dist_thres) id = nn_idx;
        }
        if (sc_dist < min_dist) { min_dist = sc_dist; best_id = id; best_shift = align; }
    }
    if (match_id) *match_id = best_id;
    if (yaw) *yaw = lio_sc_shift_to_yaw(best_shift);
    if (score) *score = min_dist;
    if (shift) *shift = best_shift;
    return LIO_OK;
}

int lio_sc_set_positions(lio_sc* h, const float* xyz, uint32_t n_frames) {
    if (!h || (n_frames && !xyz)) return LIO_E_INVALID;
    if (n_frames > h->max_frames) { set_error("lio_sc_set_positions: %u positions exceed max_frames %u", n_frames, h->max_frames); return LIO_E_CAPACITY; }
    hipSetDevice(h->device);
    LIO_HIP_TRY(hipStreamSynchronize(h->st));
    if (n_frames) LIO_HIP_TRY(hipMemcpy(h->pos, xyz, (size_t)n_frames * 3 * sizeof(float), hipMemcpyHostToDevice));
    h->n_pos = n_frames;
    return LIO_OK;
}

int lio_sc_local_search(lio_sc* h, const float* xyzi, uint32_t n, const double ins_xyz[3], double precision, int32_t* match_id, float* yaw, double* score,
                        int32_t* n_examined) {
    if (!h || (n && !xyzi) || !ins_xyz) return LIO_E_INVALID;
    if (!(ins_xyz[0] - ins_xyz[0] == 0.0 && ins_xyz[1] - ins_xyz[1] == 0.0 && precision - precision == 0.0)) {  // (both gates are false for what is not a number)
        set_error("lio_sc_local_search: the INS position or the precision is not finite");
        return LIO_E_INVALID;
    }
    if (h->n_pos != h->n_frames) { set_error("lio_sc_local_search: %u positions for a bank of %u frames (lio_sc_set_positions)", h->n_pos, h->n_frames); return LIO_E_STATE; }
    hipSetDevice(h->device);
    h->t_describe = h->t_ring = h->t_dist = 0;
    const uint32_t F = h->n_frames;
    const int nc = (int)(F < (uint32_t)kCand ? F : (uint32_t)kCand);
    h->loc_n = nc;
    h->loc_match_shift = 0;
    for (int k = 0; k < kCand; k++) { h->loc_ids[k] = -1; h->loc_shift[k] = -1; h->loc_d2[k] = INFINITY; h->loc_dist[k] = (double)NAN; }
    int32_t best_id = -1, best_shift = 0, examined = 0;
    double min_dist = 1.0;
    if (nc > 0) {  // (an empty tree: nearestKSearch answers 0 and localSearch returns before it describes the cloud)
        static const double kHere[2] = {0, 0};
        int rc = describe_query(h, "lio_sc_local_search", xyzi, n, kHere, 1);
        if (rc != LIO_OK) return rc;
        {
            Span sp(h, &h->t_ring);
            if (F > h->keys_cap) {
                LIO_HIP_TRY(hipStreamSynchronize(h->st));
                h->keys_cap = 0;
                rc = regrow(&h->keys, F);
                if (rc != LIO_OK) return rc;
                h->keys_cap = F;
            }
            hipLaunchKernelGGL(sc_pos_keys, (F + kThreads - 1) / kThreads, kThreads, 0, h->st, h->pos, F, (float)ins_xyz[0], (float)ins_xyz[1], h->keys);
            hipLaunchKernelGGL(sc_ring_select, 1, kThreads, 0, h->st, h->keys, F, h->cand, h->cand_rd);
            LIO_HIP_TRY(hipGetLastError());
        }
        {
            Span sp(h, &h->t_dist);
            LIO_HIP_TRY(hipMemsetAsync(h->cand_q, 0, nc * sizeof(int32_t), h->st));  // every pair takes query 0
            const DescSet A{h->q_desc[0], h->q_sector[0], h->q_norm[0]}, B{h->desc, h->sector, h->norm};
            hipLaunchKernelGGL(sc_distance, nc, 64, 0, h->st, A, B, h->cand_q, h->cand, h->cand_dist, h->cand_shift);
            LIO_HIP_TRY(hipGetLastError());
        }
        LIO_HIP_TRY(hipMemcpyAsync(h->loc_d2, h->cand_rd, kCand * sizeof(float), hipMemcpyDeviceToHost, h->st));
        rc = download_candidates(h, 1, h->loc_ids, h->loc_dist, h->loc_shift, nullptr);  // ends with the stream's synchronisation: loc_d2 is in too
        if (rc != LIO_OK) return rc;
        for (int k = nc; k < kCand; k++) { h->loc_dist[k] = (double)NAN; h->loc_shift[k] = -1; }  // places no pair was launched for
        // the walk of global_localization.cpp:366-381
        const double p2 = precision * precision;
        for (int i = 0; i < nc; i++) {
            const double d2 = (double)h->loc_d2[i];
            if (best_id == -1 && d2 > p2) break;  // far away from the map (best_id is -1: the answer)
            if (best_id != -1 && d2 > p2 / 10.0) break;
            examined++;
            if (h->loc_dist[i] < min_dist) { min_dist = h->loc_dist[i]; best_id = h->loc_ids[i]; best_shift = h->loc_shift[i]; }
        }
    }
    h->loc_match_shift = best_shift;
    if (match_id) *match_id = best_id;
    if (yaw) *yaw = lio_sc_shift_to_yaw(best_shift);
    if (score) *score = min_dist;
    if (n_examined) *n_examined = examined;
    return LIO_OK;
}

int lio_sc_last_local(lio_sc* h, int32_t* ids, float* d2, double* dist, int32_t* shift, int32_t* match_shift) {
    if (!h) return LIO_E_INVALID;
    if (ids) memcpy(ids, h->loc_ids, sizeof(h->loc_ids));
    if (d2) memcpy(d2, h->loc_d2, sizeof(h->loc_d2));
    if (dist) memcpy(dist, h->loc_dist, sizeof(h->loc_dist));
    if (shift) memcpy(shift, h->loc_shift, sizeof(h->loc_shift));
    if (match_shift) *match_shift = h->loc_match_shift;
    return h->loc_n;
}

int lio_sc_last_dropped(lio_sc* h, uint64_t* n_nonfinite) {
    if (!h || !n_nonfinite) return LIO_E_INVALID;
    *n_nonfinite = h->n_bad;
    return LIO_OK;
}

int lio_sc_last_times(lio_sc* h, double* describe_us, double* ringkey_us, double* distance_us) {
    if (!h) return LIO_E_INVALID;
    if (describe_us) *describe_us = h->t_describe;
    if (ringkey_us) *ringkey_us = h->t_ring;
    if (distance_us) *distance_us = h->t_dist;
    return LIO_OK;
}

}  // extern "C"
