// bev.hip -- the bird's-eye intensity image of a dense map on gfx950 (wave64): tools/postprocessing/convert_cloud_image.py of the reference
// (load_pointcloud, filter_noise, scatter, convert / intensity_normalize, bev_generate), function by function.  include/lio_hip.h states
// every rule; tests/bev_cases.py restates them in numpy.
//
//   bounds     finite flags, f32 min / max of x and y as ordered words (integer atomics: any order gives the same bits); the host derives the
//              image size in f64
//   noise      stable LSD radix sort (device_prims.h, 4 passes) of (canonical intensity, input index); ranks [int(m 0.01), int(m 0.999)) stay
//   scatter    pixel key ys w + xs of the kept points in that order, a second stable sort by the key (only the passes the key has bits for),
//              run heads by device_prims.h's stable compaction, then the sequential f32 sums of intensity and z per pixel in
//              ascending (intensity, input index) order: one lane per pixel, one wave for a pixel of 64 points or more
//   rows       for every image row and node column the range of the occupied-pixel list that lies in the column's window (binary searches)
//   nodes      one workgroup per equalisation node: occupied pixels of its window from the row ranges, 1024-bin histogram in LDS (integer
//              atomics), numpy's density / cumulative sum in f64 by one lane (a sequential sum, as numpy's), then the clip-limit search:
//              every mean is a sum of 2^-16 fixed-point terms in 64-bit integers (exact in any order), so the first failing step of the
//              reference's scan is found by bisection over the tabulated steps (a window with a negative value: the linear scan)
//   render     one lane per occupied pixel: the last running node (xi major, yi minor) whose inner region holds it, the clipped product as
//              f32, rint, the grey table, the uint16 image
//
// Workgroups hand results to each other only at kernel boundaries.  One stream; scratch grows geometrically and is kept.
#include <algorithm>
#include <cmath>
#include <vector>

#include "device_prims.h"

namespace lio {
namespace bev {

using namespace prims;

constexpr int kBins = 1024;
constexpr int kMaxSteps = 1280;     // (120 - 1) / 0.1 = 1190 steps at the most, with room for the drift of the f32 accumulation
constexpr uint32_t kLongRun = 64;   // pixels of at least this many points are summed one wave per pixel
constexpr uint32_t kLongBlocks = 2048;
constexpr double kBright = 20480.0; // BRIGHTNESS = 80 * 256
constexpr double kTermMax = 8388608.0;  // 2^23 > 65535 * 120: the clamp of a fixed-point term
constexpr uint32_t kMinCount = 100;

struct Bounds {  // ordered words of the f32 extremes over the finite points
    uint32_t xmin, xmax, ymin, ymax, n_finite, bad;
};

struct Geo {  // the image and the node grid
    uint32_t w, h;      // image_w, image_h of load_pointcloud
    uint32_t W, H;      // padded
    int32_t P, hp, q;   // patch, half, quarter
    uint32_t nx, ny;    // nodes
};

__device__ __forceinline__ bool finite_pt(const float4& p) { return finite3(p.x, p.y, p.w); }  // (z may be anything)

__global__ __launch_bounds__(kThreads) void bv_bounds(const float4* __restrict__ p, uint32_t n, Bounds* __restrict__ b) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t xlo = 0xFFFFFFFFu, xhi = 0u, ylo = 0xFFFFFFFFu, yhi = 0u;
    bool ok = false;
    if (i < n) {
        const float4 q = p[i];
        ok = finite_pt(q);
        if (ok) { xlo = xhi = f2ord(q.x); ylo = yhi = f2ord(q.y); }
    }
    const uint32_t c = (uint32_t)__popcll(__ballot(ok));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        xlo = min(xlo, (uint32_t)__shfl_xor((int)xlo, off));
        xhi = max(xhi, (uint32_t)__shfl_xor((int)xhi, off));
        ylo = min(ylo, (uint32_t)__shfl_xor((int)ylo, off));
        yhi = max(yhi, (uint32_t)__shfl_xor((int)yhi, off));
    }
    if ((threadIdx.x & 63) == 0 && c) {
        atomicMin(&b->xmin, xlo);
        atomicMax(&b->xmax, xhi);
        atomicMin(&b->ymin, ylo);
        atomicMax(&b->ymax, yhi);
        atomicAdd(&b->n_finite, c);
    }
}

// the sort key of the noise filter (-0.0 sorts as +0.0, a dropped point behind every finite one) and the pixel of every point
__global__ __launch_bounds__(kThreads) void bv_point_keys(const float4* __restrict__ p, uint32_t n, float xmin, float ymax, float ppm, uint32_t w, uint32_t h,
                                                          uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, int2* __restrict__ xy,
                                                          Bounds* __restrict__ b) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 q = p[i];
    vals[i] = i;
    if (!finite_pt(q)) {
        keys[i] = 0xFFFFFFFFu;
        xy[i] = make_int2(-1, -1);
        return;
    }
    keys[i] = f2ord(q.w == 0.f ? 0.f : q.w);
    const float fx = rintf((q.x - xmin) * ppm);
    const float fy = rintf((-(q.y - ymax)) * ppm);
    const bool in = fx >= 0.f && fx < (float)w && fy >= 0.f && fy < (float)h;
    if (!in) atomicOr(&b->bad, 1u);
    xy[i] = in ? make_int2((int)fx, (int)fy) : make_int2(-1, -1);
}

// the kept ranks [lo, lo + nk) of the intensity order: their input indices and pixel keys
__global__ __launch_bounds__(kThreads) void bv_pixel_keys(const uint32_t* __restrict__ order, uint32_t lo, uint32_t nk, const int2* __restrict__ xy, uint32_t w,
                                                          uint32_t* __restrict__ kept, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= nk) return;
    const uint32_t i = order[lo + j];
    const int2 c = xy[i];
    kept[j] = i;
    vals[j] = i;
    keys[j] = c.x < 0 ? 0u : (uint32_t)c.y * w + (uint32_t)c.x;
}

// run heads per tile
__global__ __launch_bounds__(kThreads) void bv_head_count(const uint32_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ counts) {
    const uint32_t base = blockIdx.x * kTile;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        c += (i < n && (i == 0 || keys[i - 1] != keys[i])) ? 1u : 0u;
    }
    compact_tile_count(c, counts);
}

// hpos[v] = first sorted position of occupied pixel v, hpos[npix] = n; pkey[v] = its key
__global__ __launch_bounds__(kThreads) void bv_head_write(const uint32_t* __restrict__ keys, uint32_t n, const uint32_t* __restrict__ offs, uint32_t ntiles,
                                                          uint32_t* __restrict__ hpos, uint32_t* __restrict__ pkey) {
    const int tid = threadIdx.x;
    const uint32_t base = blockIdx.x * kTile;
    bool head[kItems];
    uint32_t kc[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + tid;
        kc[r] = i < n ? keys[i] : 0u;
        head[r] = i < n && (i == 0 || keys[i - 1] != kc[r]);
    }
    compact_tile_write(head, offs, [&](int r, uint32_t o) {
        hpos[o] = base + r * kThreads + tid;
        pkey[o] = kc[r];
    });
    if (blockIdx.x == 0 && tid == 0) hpos[offs[ntiles]] = n;
}

// one lane per occupied pixel: the sequential f32 sums of intensity and z over its points in sorted order; long runs are queued
__global__ __launch_bounds__(kThreads) void bv_mean(const float4* __restrict__ p, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ hpos,
                                                    const uint32_t* __restrict__ d_npix, float* __restrict__ pI, float* __restrict__ pz,
                                                    uint32_t* __restrict__ longlist, uint32_t* __restrict__ n_long) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t npix = *d_npix;
    const bool live = v < npix;
    const uint32_t a = hpos[live ? v : 0u], b = hpos[live ? v + 1u : 0u];
    const bool is_long = live && b - a >= kLongRun;
    queue_long_run(is_long, v, longlist, n_long);
    if (!live || is_long) return;
    float si = 0.f, sz = 0.f;
    for (uint32_t j = a; j < b; j += 4) {
        float4 q[4];
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = p[vals[(j + k < b) ? (j + k) : (b - 1u)]];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (j + k < b) { si = si + q[k].w; sz = sz + q[k].z; }
    }
    const float c = (float)(b - a);
    pI[v] = si / c;
    pz[v] = sz / c;
}

// one wave per long pixel: 64 points per step parked in LDS, lanes 0 and 1 add them in order
__global__ __launch_bounds__(64) void bv_mean_long(const float4* __restrict__ p, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ hpos,
                                                   const uint32_t* __restrict__ longlist, const uint32_t* __restrict__ n_long, float* __restrict__ pI,
                                                   float* __restrict__ pz) {
    __shared__ float park[2][64];
    const int lane = threadIdx.x;
    const uint32_t nl = *n_long;
    for (uint32_t qi = blockIdx.x; qi < nl; qi += gridDim.x) {
        const uint32_t v = longlist[qi];
        const uint32_t a = hpos[v], b = hpos[v + 1];
        float s = 0.f;
        for (uint32_t j = a; j < b; j += 64) {
            const float4 cur = p[vals[(j + lane < b) ? j + lane : b - 1u]];
            __syncthreads();
            park[0][lane] = cur.w;
            park[1][lane] = cur.z;
            __syncthreads();
            if (lane < 2) {
                const uint32_t cnt = (b - j < 64u) ? b - j : 64u;
                for (uint32_t k = 0; k < cnt; k++) s = s + park[lane][k];
            }
        }
        const float c = (float)(b - a);
        if (lane == 0) pI[v] = s / c;
        if (lane == 1) pz[v] = s / c;
    }
}

// ---- equalisation ----
__device__ __forceinline__ uint32_t lower_bound(const uint32_t* __restrict__ keys, uint32_t n, uint32_t target) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < target) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// rows[(y nx + ix) 2 + {0, 1}]: the occupied pixels of row y with x in [ix hp - P, ix hp + P], as a range of the list
__global__ __launch_bounds__(kThreads) void bv_rows(const uint32_t* __restrict__ pkey, uint32_t npix, Geo g, uint32_t* __restrict__ rows) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (uint64_t)g.h * g.nx) return;
    const uint32_t y = (uint32_t)(t / g.nx), ix = (uint32_t)(t % g.nx);
    const int64_t xi = (int64_t)ix * g.hp;
    const int64_t xlo = std::min<int64_t>(std::max<int64_t>(xi - g.P, 0), g.w), xhi1 = std::min<int64_t>(xi + g.P + 1, g.w);
    const uint32_t base = y * g.w;  // (y + 1) w <= w h fits 32 bits (checked by the host)
    const uint32_t a = lower_bound(pkey, npix, base + (uint32_t)xlo);
    const uint32_t b = xhi1 > xlo ? lower_bound(pkey, npix, base + (uint32_t)xhi1) : a;
    rows[2 * t] = a;
    rows[2 * t + 1] = b;
}

// numpy's linspace(0, 65535, 1025) as f32: edge i = f32(i * (65535 / 1024)), the product exact in f64
__host__ __device__ __forceinline__ float edge_of(int i) { return (float)((double)(i * 65535) / 1024.0); }

// numpy's uniform-bin search: the estimate in f32, then one step down or up against the edges; v in [0, 65535]
__device__ __forceinline__ int bin_of(float v) {
    const float f = (float)((double)v / 65535.0) * 1024.0f;  // the f32 quotient, correctly rounded through f64
    int i = (int)f;
    if (i == kBins) i = kBins - 1;
    if (v < edge_of(i)) i--;
    else if (v >= edge_of(i + 1) && i != kBins - 1) i++;
    return i;
}

__device__ __forceinline__ double interp_cdf(float v, const double* __restrict__ cdf, const double* __restrict__ slope) {
    if (v < 0.f) return cdf[0];
    if (v >= edge_of(kBins - 1)) return cdf[kBins - 1];
    const int j = bin_of(v);
    const double x = (double)v, xj = (double)edge_of(j);
    if (x == xj) return cdf[j];
    return slope[j] * (x - xj) + cdf[j];
}

__device__ __forceinline__ long long fixed_term(double t) {
    if (!(t == t)) return 0;
    t = fmin(fmax(t, -kTermMax), kTermMax);
    return __double2ll_rn(t * 65536.0);
}

__device__ __forceinline__ double equalised(float v, double f, double c) {
    const double amp = f / (double)fmaxf(v, 0.001f);
    return (double)v * fmin(amp, c);
}

struct NodeOut {
    uint32_t* count;
    int32_t* step;
    double* clip;
    double* cdf;    // nodes x 1024
    double* slope;  // nodes x 1024
};

__global__ __launch_bounds__(kThreads) void bv_node(const float* __restrict__ pI, const uint32_t* __restrict__ rows, Geo g, NodeOut out) {
    __shared__ uint32_t hist[kBins];
    __shared__ double cdf[kBins];
    __shared__ double slope[kBins];
    __shared__ double ctab[kMaxSteps];
    __shared__ unsigned long long acc;
    __shared__ uint32_t s_count, s_neg;
    __shared__ int s_kmax;
    __shared__ unsigned long long s_total;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t node = blockIdx.x;
    const uint32_t ix = node / g.ny, iy = node % g.ny;
    const int64_t yi = (int64_t)iy * g.hp;
    const int64_t y0 = std::max<int64_t>(yi - g.P, 0), y1 = std::min<int64_t>(yi + g.P, (int64_t)g.h - 1);
    for (int i = tid; i < kBins; i += kThreads) hist[i] = 0;
    if (tid == 0) { acc = 0; s_count = 0; s_neg = 0; }
    __syncthreads();
    {
        uint32_t c = 0;
        for (int64_t y = y0 + tid; y <= y1; y += kThreads) {
            const uint64_t t = ((uint64_t)y * g.nx + ix) * 2;
            c += rows[t + 1] - rows[t];
        }
        if (c) atomicAdd(&s_count, c);
    }
    __syncthreads();
    const uint32_t count = s_count;
    if (count <= kMinCount) {
        if (tid == 0) { out.count[node] = count; out.step[node] = -1; out.clip[node] = 0.0; }
        return;
    }
    // histogram, the sum of v, any negative v
    {
        long long s = 0;
        bool neg = false;
        for (int64_t y = y0 + wave; y <= y1; y += kWaves) {
            const uint64_t t = ((uint64_t)y * g.nx + ix) * 2;
            const uint32_t a = rows[t], b = rows[t + 1];
            for (uint32_t j = a + lane; j < b; j += 64) {
                const float v = pI[j] * 65535.0f;
                if (v >= 0.f && v <= 65535.0f) atomicAdd(&hist[bin_of(v)], 1u);
                neg = neg || v < 0.f;
                s += fixed_term((double)v);
            }
        }
        atomicAdd(&acc, (unsigned long long)s);
        if (neg) atomicOr(&s_neg, 1u);
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long tot = 0;
        for (int i = 0; i < kBins; i++) tot += hist[i];
        s_total = tot;
        if (tot) {
            double cum = 0.0;
            for (int i = 0; i < kBins; i++) {
                const float db = edge_of(i + 1) - edge_of(i);
                cum += ((double)hist[i] / (double)db) / (double)tot;
                cdf[i] = cum;
            }
        }
        // the steps of the clip limit: c0 = 20480 / mean(v) as an f32 quotient and f32 steps, or 1.0 and f64 steps when that is not above 1
        const long long s0 = (long long)acc;
        const float m32 = (float)(((double)s0 / 65536.0) / (double)count);
        const float c0 = (float)(kBright / (double)m32);
        int k = 0;
        if (c0 > 1.0f) {
            float c = c0;
            ctab[0] = (double)c;
            while (c < 120.0f && k < kMaxSteps - 1) { c = c + 0.1f; ctab[++k] = (double)c; }
        } else {
            double c = 1.0;
            ctab[0] = c;
            while (c < 120.0 && k < kMaxSteps - 1) { c = c + 0.1; ctab[++k] = c; }
        }
        s_kmax = k;
    }
    __syncthreads();
    if (s_total == 0) {
        if (tid == 0) { out.count[node] = count; out.step[node] = -1; out.clip[node] = 0.0; }
        return;
    }
    {
        const double last = cdf[kBins - 1];
        __syncthreads();
        for (int i = tid; i < kBins; i += kThreads) cdf[i] = (65535.0 * cdf[i]) / last;
        __syncthreads();
        for (int i = tid; i < kBins; i += kThreads)
            slope[i] = i < kBins - 1 ? (cdf[i + 1] - cdf[i]) / ((double)edge_of(i + 1) - (double)edge_of(i)) : 0.0;
    }
    __syncthreads();
    const bool linear = s_neg != 0;
    const long long target = (long long)count * (long long)(kBright * 65536.0);
    int lo = 0, hi = s_kmax;
    while (lo < hi) {
        const int mid = linear ? lo : (lo + hi) / 2;
        const double c = ctab[mid];
        if (tid == 0) acc = 0;
        __syncthreads();
        long long s = 0;
        for (int64_t y = y0 + wave; y <= y1; y += kWaves) {
            const uint64_t t = ((uint64_t)y * g.nx + ix) * 2;
            const uint32_t a = rows[t], b = rows[t + 1];
            for (uint32_t j = a + lane; j < b; j += 64) {
                const float v = pI[j] * 65535.0f;
                s += fixed_term(equalised(v, interp_cdf(v, cdf, slope), c));
            }
        }
        atomicAdd(&acc, (unsigned long long)s);
        __syncthreads();
        const bool reached = (long long)acc >= target;
        __syncthreads();
        if (linear) {
            if (reached) hi = lo; else lo = lo + 1;
        } else {
            if (reached) hi = mid; else lo = mid + 1;
        }
    }
    if (tid == 0) { out.count[node] = count; out.step[node] = lo; out.clip[node] = ctab[lo]; }
    for (int i = tid; i < kBins; i += kThreads) {
        out.cdf[(uint64_t)node * kBins + i] = cdf[i];
        out.slope[(uint64_t)node * kBins + i] = slope[i];
    }
}

// the value of every occupied pixel and the image
__global__ __launch_bounds__(kThreads) void bv_render(const uint32_t* __restrict__ pkey, const float* __restrict__ pI, uint32_t npix, Geo g, NodeOut nd,
                                                      const uint16_t* __restrict__ grey, float* __restrict__ eq, uint16_t* __restrict__ image) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= npix) return;
    const uint32_t key = pkey[p];
    const uint32_t x = key % g.w, y = key / g.w;
    const float raw = pI[p];
    float o = raw;
    const uint32_t ixa = x / (uint32_t)g.hp, iya = y / (uint32_t)g.hp;
    const int rx = (int)(x - ixa * (uint32_t)g.hp), ry = (int)(y - iya * (uint32_t)g.hp);
    bool done = false;
#pragma unroll
    for (int dx = 1; dx >= 0; dx--) {
        const bool cx = dx ? (g.hp - rx <= g.q) : (rx <= g.q);
#pragma unroll
        for (int dy = 1; dy >= 0; dy--) {
            const bool cy = dy ? (g.hp - ry <= g.q) : (ry <= g.q);
            const uint32_t ix = ixa + dx, iy = iya + dy;
            if (done || !cx || !cy || ix >= g.nx || iy >= g.ny) continue;
            const uint32_t node = ix * g.ny + iy;
            if (nd.step[node] < 0) continue;
            const float v = raw * 65535.0f;
            const double f = interp_cdf(v, nd.cdf + (uint64_t)node * kBins, nd.slope + (uint64_t)node * kBins);
            const double t = equalised(v, f, nd.clip[node]);
            o = (float)fmin(fmax(t, 0.0), 65535.0);  // (fmin / fmax drop a NaN: it becomes 0)
            done = true;
        }
    }
    eq[p] = o;
    const float r = rintf(o);
    const int gi = r >= 0.f ? (r > 65535.f ? 65535 : (int)r) : 0;
    image[(uint64_t)y * g.W + x] = grey[gi];
}

}  // namespace bev
}  // namespace lio

using namespace lio;
using namespace lio::bev;

struct lio_bev {
    int device;
    hipStream_t stream;
    hipEvent_t ev[5];  // preprocess begin / end, convert begin / end, the cloud's stream
    // per-point buffers (cap points)
    uint64_t cap;
    float4* stage;
    uint32_t *ka, *kb, *va, *vb, *kept, *hpos, *pkey, *longlist;
    int2* xy;
    float *pI, *pz, *eq;
    uint32_t* radix;   // one radix pass's scratch
    uint32_t* heads;   // tile counts of the heads and their scan's tile sums
    Bounds* d_bounds;
    uint32_t* d_word;  // the long-pixel counter
    uint16_t* d_grey;
    // per-image buffers
    uint32_t* rows;
    uint64_t rows_cap;
    uint32_t* ncount;
    int32_t* nstep;
    double *nclip, *ncdf, *nslope;
    uint64_t ncap[5];
    uint16_t* image;
    uint64_t image_cap;
    // the last calls
    lio_bev_info info;
    Geo geo;
    int have_pixels, have_points, have_image;
    double preprocess_us, convert_us;
};

namespace {

void free_points(lio_bev* b) {
    void* all[] = {b->stage, b->ka, b->kb, b->va, b->vb, b->kept, b->hpos, b->pkey, b->longlist, b->xy, b->pI, b->pz, b->eq, b->radix, b->heads};
    for (void* p : all)
        if (p) (void)hipFree(p);
    b->stage = nullptr;
    b->ka = b->kb = b->va = b->vb = b->kept = b->hpos = b->pkey = b->longlist = b->radix = b->heads = nullptr;
    b->xy = nullptr;
    b->pI = b->pz = b->eq = nullptr;
    b->cap = 0;
}

int reserve(lio_bev* b, uint64_t n) {
    if (n <= b->cap) return LIO_OK;
    if (n > 0x7FFFFFFFull) { set_error("lio_bev: %llu points exceed the int index range (2^31 - 1)", (unsigned long long)n); return LIO_E_CAPACITY; }
    const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(n, std::max<uint64_t>(2 * b->cap, 1ull << 17)), 0x7FFFFFFFull);
    LIO_HIP_TRY(hipStreamSynchronize(b->stream));
    free_points(b);
    const bool ok = alloc(&b->stage, want) && alloc(&b->ka, want) && alloc(&b->kb, want) && alloc(&b->va, want) && alloc(&b->vb, want) &&
                    alloc(&b->kept, want) && alloc(&b->hpos, want + 1) && alloc(&b->pkey, want) && alloc(&b->longlist, want) && alloc(&b->xy, want) &&
                    alloc(&b->pI, want) && alloc(&b->pz, want) && alloc(&b->eq, want) && alloc(&b->radix, cloud::radix_scratch_words(want)) &&
                    alloc(&b->heads, compact_words(want));
    if (!ok) {
        (void)hipGetLastError();
        free_points(b);
        set_error("lio_bev: device scratch for %llu points not available", (unsigned long long)want);
        return LIO_E_DEVICE;
    }
    b->cap = want;
    return LIO_OK;
}

// the sizes load_pointcloud derives, and the limits of the 32-bit pixel key
int image_size(double lo, double hi, double ppm, uint32_t* out) {
    const double s = std::ceil((hi - lo) * ppm) + 1.0;
    if (!(s >= 1.0) || s > 4194304.0) { set_error("lio_bev: an image side of %.0f pixels exceeds 2^22 (f32 pixel coordinates)", s); return LIO_E_CAPACITY; }
    *out = (uint32_t)s;
    return LIO_OK;
}

bool ppm_ok(double ppm) {
    if (ppm > 0.0 && std::isfinite(ppm)) return true;
    set_error("lio_bev: pixel_per_meter must be positive and finite");
    return false;
}

// load_pointcloud + filter_noise + scatter over n device points at `raw` (ordered after the stream's earlier work)
int preprocess(lio_bev* b, const float4* raw, uint32_t n, double ppm) {
    hipStream_t st = b->stream;
    b->have_pixels = b->have_points = b->have_image = 0;
    memset(&b->info, 0, sizeof(b->info));
    b->info.n_in = n;
    b->info.pixel_per_meter = ppm;
    if (n == 0) { set_error("lio_bev: an empty cloud has no bounds"); return LIO_E_INVALID; }
    LIO_HIP_TRY(hipEventRecord(b->ev[0], st));
    Bounds hb;
    LIO_HIP_TRY(hipMemsetAsync(b->d_bounds, 0, sizeof(Bounds), st));
    LIO_HIP_TRY(hipMemsetAsync(&b->d_bounds->xmin, 0xFF, sizeof(uint32_t), st));
    LIO_HIP_TRY(hipMemsetAsync(&b->d_bounds->ymin, 0xFF, sizeof(uint32_t), st));
    bv_bounds<<<dim3(blocks_of(n)), dim3(kThreads), 0, st>>>(raw, n, b->d_bounds);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipMemcpyAsync(&hb, b->d_bounds, sizeof(hb), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    const uint32_t m = hb.n_finite;
    b->info.n_dropped = n - m;
    if (m == 0) { set_error("lio_bev: no point with finite x, y and intensity among %u", n); return LIO_E_INVALID; }
    const float xmin = ord2f(hb.xmin), xmax = ord2f(hb.xmax), ymin = ord2f(hb.ymin), ymax = ord2f(hb.ymax);
    b->info.x_min = xmin; b->info.x_max = xmax; b->info.y_min = ymin; b->info.y_max = ymax;
    uint32_t w = 0, h = 0;
    int rc = image_size(xmin, xmax, ppm, &w);
    if (rc == LIO_OK) rc = image_size(ymin, ymax, ppm, &h);
    if (rc != LIO_OK) return rc;
    if ((uint64_t)w * h > 0xFFFFFFFFull) { set_error("lio_bev: %u x %u pixels do not fit the 32-bit pixel key", w, h); return LIO_E_CAPACITY; }
    b->info.image_w = w;
    b->info.image_h = h;
    // the noise filter's order
    bv_point_keys<<<dim3(blocks_of(n)), dim3(kThreads), 0, st>>>(raw, n, xmin, ymax, (float)ppm, w, h, b->ka, b->va, b->xy, b->d_bounds);
    LIO_HIP_TRY(hipGetLastError());
    uint32_t *ki = b->ka, *vi = b->va, *ko = b->kb, *vo = b->vb;
    for (int shift = 0; shift < 32; shift += 8) {
        rc = cloud::radix_pass(st, ki, vi, ko, vo, n, shift, b->radix);
        if (rc != LIO_OK) return rc;
        std::swap(ki, ko);
        std::swap(vi, vo);
    }
    const uint32_t lo = (uint32_t)((double)m * 0.01), hi = (uint32_t)((double)m * 0.999);
    const uint32_t nk = hi > lo ? hi - lo : 0u;
    b->info.n_kept = nk;
    b->info.rank_lo = lo;
    b->info.rank_hi = hi;
    uint32_t npix = 0;
    if (nk) {
        // (ki, vi) hold the order; the pixel keys go to the other pair, whose sort then ping-pongs over both
        bv_pixel_keys<<<dim3(blocks_of(nk)), dim3(kThreads), 0, st>>>(vi, lo, nk, b->xy, w, b->kept, ko, vo);
        LIO_HIP_TRY(hipGetLastError());
        std::swap(ki, ko);
        std::swap(vi, vo);
        const uint64_t top = (uint64_t)w * h - 1;
        for (int shift = 0; shift < 32 && (top >> shift) != 0; shift += 8) {
            rc = cloud::radix_pass(st, ki, vi, ko, vo, nk, shift, b->radix);
            if (rc != LIO_OK) return rc;
            std::swap(ki, ko);
            std::swap(vi, vo);
        }
        const uint32_t ntiles = tiles_of(nk);
        uint32_t* counts = b->heads;
        LIO_HIP_TRY(hipMemsetAsync(b->d_word, 0, sizeof(uint32_t), st));
        bv_head_count<<<dim3(ntiles), dim3(kThreads), 0, st>>>(ki, nk, counts);
        const uint32_t* d_npix = compact_finish(st, counts, nk);
        if (!d_npix) return LIO_E_DEVICE;
        bv_head_write<<<dim3(ntiles), dim3(kThreads), 0, st>>>(ki, nk, counts, ntiles, b->hpos, b->pkey);
        bv_mean<<<dim3(blocks_of(nk)), dim3(kThreads), 0, st>>>(raw, vi, b->hpos, d_npix, b->pI, b->pz, b->longlist, b->d_word);
        bv_mean_long<<<dim3(kLongBlocks), dim3(64), 0, st>>>(raw, vi, b->hpos, b->longlist, b->d_word, b->pI, b->pz);
        LIO_HIP_TRY(hipGetLastError());
        LIO_HIP_TRY(hipMemcpyAsync(&npix, d_npix, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    LIO_HIP_TRY(hipMemcpyAsync(&hb, b->d_bounds, sizeof(hb), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipEventRecord(b->ev[1], st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    b->preprocess_us = elapsed_us(b->ev[0], b->ev[1]);
    if (hb.bad) { set_error("lio_bev: a pixel coordinate left the %u x %u image (the key would alias another pixel)", w, h); return LIO_E_CAPACITY; }
    b->info.n_pixels = npix;
    b->have_points = b->have_pixels = 1;
    return LIO_OK;
}

template <typename T>
int64_t download(lio_bev* b, const T* src, uint64_t n, T* out, uint64_t cap) {
    return prims::download("lio_bev", b->device, b->stream, src, n, out, cap);
}

}  // namespace

extern "C" {

void lio_bev_grey_table(uint16_t out[65536]) {
    if (!out) return;
    const double step = 1.0 / 65535.0;
    for (int i = 0; i < 65536; i++) {
        const double t = i == 65535 ? 1.0 : (double)i * step;
        out[i] = (uint16_t)(t * 65535.0);
    }
}

lio_bev* lio_bev_create(int device) {
    lio_bev* b = new lio_bev();
    memset(b, 0, sizeof(*b));
    b->device = device;
    if (!open_device("lio_bev_create", device, &b->stream, b->ev, 5)) {
        delete b;
        return nullptr;
    }
    bool ok = alloc(&b->d_bounds, 1) && alloc(&b->d_word, 16) && alloc(&b->d_grey, 65536);
    if (ok) {
        std::vector<uint16_t> g(65536);
        lio_bev_grey_table(g.data());
        ok = hipMemcpy(b->d_grey, g.data(), 65536 * sizeof(uint16_t), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        set_error("lio_bev_create: stream / event / table allocation failed");
        lio_bev_destroy(b);
        return nullptr;
    }
    return b;
}

void lio_bev_destroy(lio_bev* b) {
    if (!b) return;
    hipSetDevice(b->device);
    if (b->stream) hipStreamSynchronize(b->stream);
    free_points(b);
    void* all[] = {b->d_bounds, b->d_word, b->d_grey, b->rows, b->ncount, b->nstep, b->nclip, b->ncdf, b->nslope, b->image};
    for (void* p : all)
        if (p) (void)hipFree(p);
    for (int i = 0; i < 5; i++)
        if (b->ev[i]) hipEventDestroy(b->ev[i]);
    if (b->stream) hipStreamDestroy(b->stream);
    delete b;
}

int lio_bev_preprocess_host(lio_bev* b, const float* xyzi, uint64_t n, double pixel_per_meter) {
    if (!b || (!xyzi && n) || !ppm_ok(pixel_per_meter)) return LIO_E_INVALID;
    hipSetDevice(b->device);
    const int rc = reserve(b, n);
    if (rc != LIO_OK) return rc;
    if (n) LIO_HIP_TRY(hipMemcpyAsync(b->stage, xyzi, n * sizeof(float4), hipMemcpyHostToDevice, b->stream));
    return preprocess(b, b->stage, (uint32_t)n, pixel_per_meter);
}

int lio_bev_preprocess_cloud(lio_bev* b, lio_cloud* c, double pixel_per_meter) {
    if (!b || !c || !ppm_ok(pixel_per_meter)) return LIO_E_INVALID;
    const cloud::CloudView v = cloud::cloud_view(c);
    if (v.device != b->device) { set_error("lio_bev_preprocess_cloud: the cloud lives on device %d, the image on %d", v.device, b->device); return LIO_E_INVALID; }
    hipSetDevice(b->device);
    const int rc = reserve(b, v.n);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipEventRecord(b->ev[4], v.stream));  // the cloud's appends and voxel grid first
    LIO_HIP_TRY(hipStreamWaitEvent(b->stream, b->ev[4], 0));
    return preprocess(b, v.pts, (uint32_t)v.n, pixel_per_meter);
}

int lio_bev_upload_pixels(lio_bev* b, const uint32_t* keys, const float* intensity, const float* z, uint64_t n, uint32_t image_w, uint32_t image_h) {
    if (!b || (n && (!keys || !intensity))) return LIO_E_INVALID;
    if (image_w == 0 || image_h == 0 || (uint64_t)image_w * image_h > 0xFFFFFFFFull) {
        set_error("lio_bev_upload_pixels: %u x %u pixels do not fit the 32-bit pixel key", image_w, image_h);
        return LIO_E_CAPACITY;
    }
    for (uint64_t i = 0; i < n; i++)
        if ((i && keys[i] <= keys[i - 1]) || keys[i] >= (uint64_t)image_w * image_h) {
            set_error("lio_bev_upload_pixels: the keys must ascend strictly and lie inside the image (entry %llu)", (unsigned long long)i);
            return LIO_E_INVALID;
        }
    hipSetDevice(b->device);
    const int rc = reserve(b, n);
    if (rc != LIO_OK) return rc;
    b->have_pixels = b->have_points = b->have_image = 0;
    memset(&b->info, 0, sizeof(b->info));
    if (n) {
        LIO_HIP_TRY(hipMemcpyAsync(b->pkey, keys, n * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
        LIO_HIP_TRY(hipMemcpyAsync(b->pI, intensity, n * sizeof(float), hipMemcpyHostToDevice, b->stream));
        if (z) LIO_HIP_TRY(hipMemcpyAsync(b->pz, z, n * sizeof(float), hipMemcpyHostToDevice, b->stream));
        else LIO_HIP_TRY(hipMemsetAsync(b->pz, 0, n * sizeof(float), b->stream));
        LIO_HIP_TRY(hipStreamSynchronize(b->stream));
    }
    b->info.image_w = image_w;
    b->info.image_h = image_h;
    b->info.n_pixels = (uint32_t)n;
    b->have_pixels = 1;
    return LIO_OK;
}

int lio_bev_convert(lio_bev* b, double window, double pixel_per_meter) {
    if (!b) return LIO_E_INVALID;
    if (!b->have_pixels) { set_error("lio_bev_convert: no pixel list (call lio_bev_preprocess_* or lio_bev_upload_pixels first)"); return LIO_E_STATE; }
    if (!ppm_ok(pixel_per_meter)) return LIO_E_INVALID;
    const double pd = window * pixel_per_meter;
    if (!(pd >= 2.0) || pd > 1048576.0) { set_error("lio_bev_convert: a patch of %g pixels (window x pixel_per_meter) must lie in [2, 2^20]", pd); return LIO_E_INVALID; }
    hipSetDevice(b->device);
    hipStream_t st = b->stream;
    b->have_image = 0;
    Geo g;
    g.w = b->info.image_w;
    g.h = b->info.image_h;
    g.P = (int32_t)pd;
    g.hp = (int32_t)((double)g.P / 2.0);
    g.q = (int32_t)((double)g.hp / 2.0);
    const uint64_t W = ((uint64_t)g.w + g.hp) / g.hp * g.hp, H = ((uint64_t)g.h + g.hp) / g.hp * g.hp;
    if (W * H > 0xFFFFFFFFull) { set_error("lio_bev_convert: the padded image of %llu x %llu pixels is too large", (unsigned long long)W, (unsigned long long)H); return LIO_E_CAPACITY; }
    g.W = (uint32_t)W;
    g.H = (uint32_t)H;
    g.nx = g.W / g.hp + 1;
    g.ny = g.H / g.hp + 1;
    const uint64_t nodes = (uint64_t)g.nx * g.ny;
    const uint32_t npix = b->info.n_pixels;
    b->geo = g;
    b->info.padded_w = g.W; b->info.padded_h = g.H;
    b->info.patch = g.P; b->info.half_patch = g.hp; b->info.quarter_patch = g.q;
    b->info.nodes_x = g.nx; b->info.nodes_y = g.ny;
    int rc = grow("lio_bev", &b->rows, &b->rows_cap, (uint64_t)g.h * g.nx * 2, st);
    if (rc == LIO_OK) rc = grow("lio_bev", &b->ncount, &b->ncap[0], nodes, st);
    if (rc == LIO_OK) rc = grow("lio_bev", &b->nstep, &b->ncap[1], nodes, st);
    if (rc == LIO_OK) rc = grow("lio_bev", &b->nclip, &b->ncap[2], nodes, st);
    if (rc == LIO_OK) rc = grow("lio_bev", &b->ncdf, &b->ncap[3], nodes * kBins, st);
    if (rc == LIO_OK) rc = grow("lio_bev", &b->nslope, &b->ncap[4], nodes * kBins, st);
    if (rc == LIO_OK) rc = grow("lio_bev", &b->image, &b->image_cap, W * H, st);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipEventRecord(b->ev[2], st));
    LIO_HIP_TRY(hipMemsetAsync(b->image, 0, W * H * sizeof(uint16_t), st));
    const NodeOut out = {b->ncount, b->nstep, b->nclip, b->ncdf, b->nslope};
    bv_rows<<<dim3(blocks_of((uint64_t)g.h * g.nx)), dim3(kThreads), 0, st>>>(b->pkey, npix, g, b->rows);
    bv_node<<<dim3((uint32_t)nodes), dim3(kThreads), 0, st>>>(b->pI, b->rows, g, out);
    if (npix) bv_render<<<dim3(blocks_of(npix)), dim3(kThreads), 0, st>>>(b->pkey, b->pI, npix, g, out, b->d_grey, b->eq, b->image);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(b->ev[3], st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    b->convert_us = elapsed_us(b->ev[2], b->ev[3]);
    b->have_image = 1;
    return LIO_OK;
}

int lio_bev_get_info(lio_bev* b, lio_bev_info* out) {
    if (!b || !out) return LIO_E_INVALID;
    *out = b->info;
    return LIO_OK;
}

int64_t lio_bev_download_pixel_coords(lio_bev* b, int32_t* xy, uint64_t cap) {
    if (!b) return LIO_E_INVALID;
    const uint64_t n = b->have_points ? b->info.n_in : 0;
    if (n > cap) return -(int64_t)n;
    const int64_t rc = download(b, reinterpret_cast<const int32_t*>(b->xy), 2 * n, xy, 2 * n);
    return rc < 0 ? rc : (int64_t)n;
}

int64_t lio_bev_download_kept(lio_bev* b, uint32_t* idx, uint64_t cap) {
    if (!b) return LIO_E_INVALID;
    return download(b, b->kept, b->have_points ? b->info.n_kept : 0, idx, cap);
}

int64_t lio_bev_download_pixels(lio_bev* b, uint32_t* keys, float* intensity, float* z, uint64_t cap) {
    if (!b) return LIO_E_INVALID;
    const uint64_t n = b->have_pixels ? b->info.n_pixels : 0;
    if (n > cap) return -(int64_t)n;
    int64_t rc = (int64_t)n;
    if (keys && rc >= 0) rc = download(b, b->pkey, n, keys, cap);
    if (intensity && rc >= 0) rc = download(b, b->pI, n, intensity, cap);
    if (z && rc >= 0) rc = download(b, b->pz, n, z, cap);
    return rc;
}

int64_t lio_bev_download_nodes(lio_bev* b, uint32_t* count, int32_t* step, double* clip, uint64_t cap) {
    if (!b) return LIO_E_INVALID;
    const uint64_t n = b->have_image ? (uint64_t)b->geo.nx * b->geo.ny : 0;
    if (n > cap) return -(int64_t)n;
    int64_t rc = (int64_t)n;
    if (count && rc >= 0) rc = download(b, b->ncount, n, count, cap);
    if (step && rc >= 0) rc = download(b, b->nstep, n, step, cap);
    if (clip && rc >= 0) rc = download(b, b->nclip, n, clip, cap);
    return rc;
}

int64_t lio_bev_download_equalised(lio_bev* b, float* out, uint64_t cap) {
    if (!b) return LIO_E_INVALID;
    return download(b, b->eq, b->have_image ? b->info.n_pixels : 0, out, cap);
}

int64_t lio_bev_download_image(lio_bev* b, uint16_t* out, uint64_t cap) {
    if (!b) return LIO_E_INVALID;
    return download(b, b->image, b->have_image ? (uint64_t)b->geo.W * b->geo.H : 0, out, cap);
}

int lio_bev_last_times(lio_bev* b, double* preprocess_us, double* convert_us) {
    if (!b) return LIO_E_INVALID;
    if (preprocess_us) *preprocess_us = b->preprocess_us;
    if (convert_us) *convert_us = b->convert_us;
    return LIO_OK;
}

}  // extern "C"
