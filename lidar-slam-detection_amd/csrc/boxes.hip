// boxes.hip -- the geometry around the reference's detection network on gfx950 (wave64): the rotated bird's-eye overlap of two boxes, the area
// of their convex hull, BEV IoU and GIoU3D (sensor_driver/inference/iou3d_nms/iou3d_cpu.cpp, iou3d_nms_kernel.cu, iou3d_nms.py), rotated NMS
// with its greedy sweep on the device, and the detector's post-process (sensor_inference/utils/model_nms_utils.py) as one call.
// include/lio_hip.h states every rule; box_overlap, box_union and iou_bev are restated statement for statement in f32 (-ffp-contract=off).
//
//   prepare    one lane per box: the rotated corners, cosf / sinf of -heading for check_in_box2d, the half extents with its margin, dx * dy,
//              the z extent, the volume and the axis-aligned extents of nms_cpu's gate.  The pair kernels do no trigonometry but the
//              polygon sort's atan2f keys
//   pairwise   one lane per pair, the row box uniform in the workgroup; any of overlap, hull, IoU and GIoU3D in one pass over the pair
//   nms_mask   64 x 64 tiles, the column tile's boxes in LDS, tiles with col_block >= row_block only
//   nms_sweep  one workgroup, lane w owns removal word w in a register; the rows of the next step (half a 64-row block) are loaded before the
//              current step is resolved (rows do not depend on decisions), the owner of the diagonal word resolves the in-block decisions
//              on it, then every lane ORs the kept rows into its word: N / 32 dependent steps, not N dependent loads
//   filter     score >= thresh[label], device_prims.h's stable compaction;  order: a rank by counting over order-preserving keys, ties to
//              the smaller original index;  gather: kept boxes, scores and labels behind the count in one buffer, one download
//
// The point list of a pair (at most 16 points) and the hull's stack live in LDS, one column per lane: nothing is indexed at run time in
// private memory, and no kernel here uses scratch.  One stream; no host synchronisation between the upload and the download of a result.
#include <algorithm>
#include <cstring>

#include "device_prims.h"

namespace lio {
namespace boxes {

using namespace prims;

constexpr int kLanes = 64;          // the pair kernels: one wave per workgroup
constexpr int kMaxPts = 16;         // 8 intersections and 8 corners
constexpr float kEps = 1e-8f;       // EPS of iou3d_cpu.cpp
constexpr float kMargin = 1e-2f;    // MARGIN of check_in_box2d
constexpr uint32_t kMaxBoxes = 16384;  // the sweep owns one removal word per lane: 256 lanes x 64 boxes
constexpr int kSweepThreads = 256;
constexpr int kSweepRows = 32;        // rows per step of the sweep: two register buffers of this many words per lane
constexpr int kOrderThreads = 256;
static_assert(kMaxBoxes == kSweepThreads * 64, "one removal word per lane of the sweep");

struct P2 {
    float x, y;
};

// what the pair kernels need of a box: 24 floats, read as six float4
struct __attribute__((aligned(16))) Prep {
    float x0, y0, x1, y1, x2, y2, x3, y3;  // the corners, rotated about the centre
    float cx, cy, hx, hy;                  // centre; dx / 2 + MARGIN, dy / 2 + MARGIN
    float cn, sn, area, vol;               // cosf(-heading), sinf(-heading); dx * dy; dx * dy * dz
    float zmin, zmax, ax0, ax1;            // z -+ dz / 2; x -+ dx / 2 (nms_cpu's gate)
    float ay0, ay1, pad0, pad1;            // y -+ dy / 2
};
static_assert(sizeof(Prep) == 96, "six float4");

// the LDS of one lane: element k of an array is at [k * kLanes]
struct Lds {
    float* px;
    float* py;
    float* key;
    uint8_t* idx;
};

__device__ __forceinline__ float fmin_ref(float a, float b) { return a > b ? b : a; }  // iou3d_cpu.cpp:12-18
__device__ __forceinline__ float fmax_ref(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float cross2(P2 a, P2 b) { return a.x * b.y - a.y * b.x; }
__device__ __forceinline__ float cross3(P2 p1, P2 p2, P2 p0) { return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y); }

__device__ __forceinline__ bool rect_cross(P2 p1, P2 p2, P2 q1, P2 q2) {
    return fmin_ref(p1.x, p2.x) <= fmax_ref(q1.x, q2.x) && fmin_ref(q1.x, q2.x) <= fmax_ref(p1.x, p2.x) &&
           fmin_ref(p1.y, p2.y) <= fmax_ref(q1.y, q2.y) && fmin_ref(q1.y, q2.y) <= fmax_ref(p1.y, p2.y);
}

// intersection() of iou3d_cpu.cpp:77-106
__device__ __forceinline__ bool intersection(P2 p1, P2 p0, P2 q1, P2 q0, P2& ans) {
    if (!rect_cross(p0, p1, q0, q1)) return false;
    const float s1 = cross3(q0, p1, p0);
    const float s2 = cross3(p1, q1, p0);
    const float s3 = cross3(p0, q1, q0);
    const float s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0.f && s3 * s4 > 0.f)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > kEps) {
        ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        ans.x = (b0 * c1 - b1 * c0) / D;
        ans.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

// check_in_box2d() of iou3d_cpu.cpp:65-75 over the prepared cosf(-heading), sinf(-heading) and half extents
__device__ __forceinline__ bool in_box2d(const Prep& b, P2 p) {
    const float rot_x = (p.x - b.cx) * b.cn + (p.y - b.cy) * (-b.sn);
    const float rot_y = (p.x - b.cx) * b.sn + (p.y - b.cy) * b.cn;
    return fabsf(rot_x) < b.hx && fabsf(rot_y) < b.hy;
}

__device__ __forceinline__ void push(const Lds& l, int& cnt, P2& sum, P2 p) {
    if (cnt < kMaxPts) {  // more than 16 cannot occur (the reference's array holds 16)
        l.px[cnt * kLanes] = p.x;
        l.py[cnt * kLanes] = p.y;
    }
    sum.x = sum.x + p.x;
    sum.y = sum.y + p.y;
    cnt++;
}

// box_overlap() of iou3d_cpu.cpp:118-210
__device__ float box_overlap(const Prep& a, const Prep& b, const Lds& l) {
    const P2 A[5] = {{a.x0, a.y0}, {a.x1, a.y1}, {a.x2, a.y2}, {a.x3, a.y3}, {a.x0, a.y0}};
    const P2 B[5] = {{b.x0, b.y0}, {b.x1, b.y1}, {b.x2, b.y2}, {b.x3, b.y3}, {b.x0, b.y0}};
    int cnt = 0;
    P2 sum = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            P2 ans;
            if (intersection(A[i + 1], A[i], B[j + 1], B[j], ans)) push(l, cnt, sum, ans);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (in_box2d(a, B[k])) push(l, cnt, sum, B[k]);
        if (in_box2d(b, A[k])) push(l, cnt, sum, A[k]);
    }
    if (cnt == 0) return 0.f;  // the reference's loops do not run and its 0 / 0 centre is never used
    cnt = cnt < kMaxPts ? cnt : kMaxPts;
    const float cx = sum.x / (float)cnt, cy = sum.y / (float)cnt;
    for (int k = 0; k < cnt; k++) l.key[k * kLanes] = atan2f(l.py[k * kLanes] - cy, l.px[k * kLanes] - cx);
    // the stable ascending order of the keys (the reference's bubble sort swaps on `>` only): idx[rank] = point
    for (int i = 0; i < cnt; i++) {
        const float ki = l.key[i * kLanes];
        int rank = 0;
        for (int j = 0; j < cnt; j++) {
            const float kj = l.key[j * kLanes];
            rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
        }
        l.idx[rank * kLanes] = (uint8_t)i;
    }
    const int i0 = l.idx[0] & (kMaxPts - 1);
    const P2 p0 = {l.px[i0 * kLanes], l.py[i0 * kLanes]};
    float area = 0.f;
    P2 prev = {0.f, 0.f};  // point 0 - point 0
    for (int k = 1; k < cnt; k++) {
        const int ik = l.idx[k * kLanes] & (kMaxPts - 1);
        const P2 d = {l.px[ik * kLanes] - p0.x, l.py[ik * kLanes] - p0.y};
        area += cross2(prev, d);
        prev = d;
    }
    return fabsf(area) * 0.5f;
}

// Point::operator< of iou3d_cpu.cpp:41-46: descending x then descending y, `>=` lets equal points swap
__device__ __forceinline__ bool point_lt(P2 a, P2 b) { return (a.x == b.x) ? (a.y >= b.y) : (a.x >= b.x); }

// box_union() of iou3d_cpu.cpp:212-303: the area of the convex hull of the eight corners
__device__ float box_union(const Prep& a, const Prep& b, const Lds& l) {
    P2 T[8] = {{a.x0, a.y0}, {a.x1, a.y1}, {a.x2, a.y2}, {a.x3, a.y3}, {b.x0, b.y0}, {b.x1, b.y1}, {b.x2, b.y2}, {b.x3, b.y3}};
    // the bubble sort's exact passes: a fixed network of 28 compare-exchanges
#pragma unroll
    for (int k = 0; k < 8; k++) {
#pragma unroll
        for (int i = 0; i < 8 - k - 1; i++) {
            const bool sw = point_lt(T[i], T[i + 1]);
            const P2 lo = sw ? T[i + 1] : T[i], hi = sw ? T[i] : T[i + 1];
            T[i] = lo;
            T[i + 1] = hi;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        l.px[k * kLanes] = T[k].x;
        l.py[k * kLanes] = T[k].y;
    }
    auto pt = [&](int i) { return P2{l.px[(i & 7) * kLanes], l.py[(i & 7) * kLanes]}; };
    auto hull = [&](int i) { return (int)l.idx[(i & (kMaxPts - 1)) * kLanes]; };
    int pos = 1;
    uint32_t used = 0;
    l.idx[0] = 0;
    for (int k = 1; k < 8; k++) {
        const P2 pk = pt(k);
        while (pos > 1 && cross3(pt(hull(pos - 1)), pk, pt(hull(pos - 2))) <= 0.f) {
            used &= ~(1u << hull(pos - 1));
            pos--;
        }
        used |= 1u << k;
        l.idx[(pos & (kMaxPts - 1)) * kLanes] = (uint8_t)k;
        pos++;
    }
    const int m = pos;
    for (int k = 8 - 2; k >= 0; k--) {
        if (!((used >> k) & 1u)) {
            const P2 pk = pt(k);
            while (pos > m && cross3(pt(hull(pos - 1)), pk, pt(hull(pos - 2))) <= 0.f) {
                used &= ~(1u << hull(pos - 1));
                pos--;
            }
            used |= 1u << k;
            l.idx[(pos & (kMaxPts - 1)) * kLanes] = (uint8_t)k;
            pos++;
        }
    }
    pos--;
    const P2 p0 = pt(hull(0));
    float area = 0.f;
    P2 prev = {0.f, 0.f};
    for (int k = 1; k < pos; k++) {
        const P2 q = pt(hull(k));
        const P2 d = {q.x - p0.x, q.y - p0.y};
        area += cross2(prev, d);
        prev = d;
    }
    return fabsf(area) * 0.5f;
}

// iou_bev() of iou3d_cpu.cpp:305-312 from the overlap
__device__ __forceinline__ float iou_of(const Prep& a, const Prep& b, float overlap) { return overlap / fmaxf(a.area + b.area - overlap, kEps); }

// boxes_giou3d_gpu of iou3d_nms.py:20-62, operation for operation in f32; np.clip(v, lo, None) is np.maximum(v, lo)
__device__ __forceinline__ float clip_lo(float v, float lo) { return (v >= lo || v != v) ? v : lo; }
__device__ __forceinline__ float giou3d_of(const Prep& a, const Prep& b, float overlap, float hull) {
    const float max_of_min = fmax_ref(a.zmin, b.zmin), min_of_max = fmin_ref(a.zmax, b.zmax);
    const float overlaps_h = clip_lo(min_of_max - max_of_min, 0.f);
    const float min_of_min = fmin_ref(a.zmin, b.zmin), max_of_max = fmax_ref(a.zmax, b.zmax);
    const float unions_h = clip_lo(max_of_max - min_of_min, 0.f);
    const float overlaps_3d = overlap * overlaps_h;
    const float convexhull_3d = clip_lo(hull * unions_h, 1e-6f);
    const float unions_3d = clip_lo(a.vol + b.vol - overlaps_3d, 1e-6f);
    return overlaps_3d / unions_3d - (convexhull_3d - unions_3d) / convexhull_3d;
}

__device__ __forceinline__ Prep load_prep(const Prep* __restrict__ p) {
    const float4* q = reinterpret_cast<const float4*>(p);
    const float4 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4], f = q[5];
    Prep r;
    r.x0 = a.x; r.y0 = a.y; r.x1 = a.z; r.y1 = a.w;
    r.x2 = b.x; r.y2 = b.y; r.x3 = b.z; r.y3 = b.w;
    r.cx = c.x; r.cy = c.y; r.hx = c.z; r.hy = c.w;
    r.cn = d.x; r.sn = d.y; r.area = d.z; r.vol = d.w;
    r.zmin = e.x; r.zmax = e.y; r.ax0 = e.z; r.ax1 = e.w;
    r.ay0 = f.x; r.ay1 = f.y; r.pad0 = 0.f; r.pad1 = 0.f;
    return r;
}

#define LIO_BOXES_LDS(l)                                                                \
    __shared__ float s_px[kMaxPts * kLanes], s_py[kMaxPts * kLanes], s_key[kMaxPts * kLanes]; \
    __shared__ uint8_t s_idx[kMaxPts * kLanes];                                          \
    const Lds l = {s_px + (threadIdx.x & 63), s_py + (threadIdx.x & 63), s_key + (threadIdx.x & 63), s_idx + (threadIdx.x & 63)}

// the number of items a kernel works on: a device word where an earlier kernel of the same call decided it, else the host's
__device__ __forceinline__ uint32_t count_of(const uint32_t* __restrict__ d_m, uint32_t m_host) { return d_m ? min(*d_m, m_host) : m_host; }

// ---- prepare ---------------------------------------------------------------------------------------------------------------------------------
// box k of the output is row order[k] of `boxes` (order NULL: row k)
__global__ __launch_bounds__(kThreads) void boxes_prepare(const float* __restrict__ boxes, const uint32_t* __restrict__ order, uint32_t m_host,
                                                          const uint32_t* __restrict__ d_m, Prep* __restrict__ out) {
    const uint32_t m = count_of(d_m, m_host);
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= m) return;
    const float* b = boxes + (uint64_t)(order ? order[k] : k) * 7;
    const float x = b[0], y = b[1], z = b[2], dx = b[3], dy = b[4], dz = b[5], h = b[6];
    const float dxh = dx / 2, dyh = dy / 2;
    const float x1 = x - dxh, y1 = y - dyh, x2 = x + dxh, y2 = y + dyh;
    const float c = cosf(h), s = sinf(h);
    // rotate_around_center(), iou3d_cpu.cpp:108-112
    auto rot = [&](float px, float py, float& ox, float& oy) {
        ox = (px - x) * c + (py - y) * (-s) + x;
        oy = (px - x) * s + (py - y) * c + y;
    };
    Prep p;
    rot(x1, y1, p.x0, p.y0);
    rot(x2, y1, p.x1, p.y1);
    rot(x2, y2, p.x2, p.y2);
    rot(x1, y2, p.x3, p.y3);
    p.cx = x;
    p.cy = y;
    p.hx = dxh + kMargin;
    p.hy = dyh + kMargin;
    p.cn = cosf(-h);
    p.sn = sinf(-h);
    p.area = dx * dy;
    p.vol = dx * dy * dz;
    const float dzh = dz / 2;
    p.zmin = z - dzh;
    p.zmax = z + dzh;
    p.ax0 = x1;
    p.ax1 = x2;
    p.ay0 = y1;
    p.ay1 = y2;
    p.pad0 = p.pad1 = 0.f;
    float4* q = reinterpret_cast<float4*>(out + k);
    q[0] = make_float4(p.x0, p.y0, p.x1, p.y1);
    q[1] = make_float4(p.x2, p.y2, p.x3, p.y3);
    q[2] = make_float4(p.cx, p.cy, p.hx, p.hy);
    q[3] = make_float4(p.cn, p.sn, p.area, p.vol);
    q[4] = make_float4(p.zmin, p.zmax, p.ax0, p.ax1);
    q[5] = make_float4(p.ay0, p.ay1, 0.f, 0.f);
}

// ---- pairwise --------------------------------------------------------------------------------------------------------------------------------
// row blockIdx.y of A against 64 columns of B; each of the four outputs may be NULL
__global__ __launch_bounds__(kLanes) void boxes_pairwise(const Prep* __restrict__ A, uint32_t na, const Prep* __restrict__ B, uint32_t nb,
                                                         float* __restrict__ o_overlap, float* __restrict__ o_hull, float* __restrict__ o_iou,
                                                         float* __restrict__ o_giou) {
    LIO_BOXES_LDS(l);
    const uint32_t i = blockIdx.y, j = blockIdx.x * kLanes + threadIdx.x;
    if (i >= na || j >= nb) return;
    const Prep a = load_prep(A + i), b = load_prep(B + j);
    const uint64_t o = (uint64_t)i * nb + j;
    float overlap = 0.f, hull = 0.f;
    if (o_overlap || o_iou || o_giou) overlap = box_overlap(a, b, l);
    if (o_hull || o_giou) hull = box_union(a, b, l);
    if (o_overlap) o_overlap[o] = overlap;
    if (o_hull) o_hull[o] = hull;
    if (o_iou) o_iou[o] = iou_of(a, b, overlap);
    if (o_giou) o_giou[o] = giou3d_of(a, b, overlap, hull);
}

// ---- NMS mask --------------------------------------------------------------------------------------------------------------------------------
// nms_cpu's gate (iou3d_nms.py:95-120): the axis-aligned extents overlap strictly in x, y and z
__device__ __forceinline__ bool aabb_gate(const Prep& a, const Prep& b) {
    return fmin_ref(b.ax1, a.ax1) > fmax_ref(b.ax0, a.ax0) && fmin_ref(b.ay1, a.ay1) > fmax_ref(b.ay0, a.ay0) &&
           fmin_ref(b.zmax, a.zmax) > fmax_ref(b.zmin, a.zmin);
}

// bit i of mask[row * cb + col_block] = iou_bev(row box, box col_block * 64 + i) > thresh (nms_kernel of iou3d_nms_kernel.cu); on the diagonal
// tile only i > lane; tiles left of the diagonal are not computed (the sweep never reads them)
__global__ __launch_bounds__(kLanes) void boxes_nms_mask(const Prep* __restrict__ P, uint32_t n_host, const uint32_t* __restrict__ d_n, float thresh,
                                                         int mode, uint32_t cb, unsigned long long* __restrict__ mask) {
    LIO_BOXES_LDS(l);
    __shared__ float4 s_col[kLanes * 6];
    const uint32_t n = count_of(d_n, n_host);
    const uint32_t rb = blockIdx.y, cblk = blockIdx.x;
    if (cblk < rb) return;
    const uint32_t row0 = rb * kLanes, col0 = cblk * kLanes;
    if (row0 >= n || col0 >= n) return;
    const uint32_t lane = threadIdx.x;
    if (col0 + lane < n) {
        const float4* q = reinterpret_cast<const float4*>(P + col0 + lane);
#pragma unroll
        for (int k = 0; k < 6; k++) s_col[lane * 6 + k] = q[k];
    }
    __syncthreads();
    const uint32_t row = row0 + lane;
    if (row >= n) return;
    const Prep a = load_prep(P + row);
    const uint32_t ncol = min((uint32_t)kLanes, n - col0);
    const uint32_t start = (rb == cblk) ? lane + 1 : 0;
    unsigned long long bits = 0;
    for (uint32_t i = 0; i < ncol; i++) {
        if (i < start) continue;
        const Prep b = load_prep(reinterpret_cast<const Prep*>(s_col + i * 6));
        if (mode != 0 && !aabb_gate(a, b)) continue;
        if (iou_of(a, b, box_overlap(a, b, l)) > thresh) bits |= 1ull << i;
    }
    mask[(uint64_t)row * cb + cblk] = bits;
}

// ---- NMS sweep -------------------------------------------------------------------------------------------------------------------------------
// the greedy sweep of nms_gpu (iou3d_nms_api.cpp): box i is kept when bit i of the running removal words is clear, and then its row is ORed
// into them.  keep[k] = order[row] (order NULL: row) of the k-th kept row, at most max_out of them; count[0] = how many, count[1] = 0.
__global__ __launch_bounds__(kSweepThreads) void boxes_nms_sweep(const unsigned long long* __restrict__ mask, uint32_t n_host,
                                                                 const uint32_t* __restrict__ d_n, uint32_t cb, uint32_t max_out,
                                                                 const uint32_t* __restrict__ order, uint32_t* __restrict__ count_out,
                                                                 long long* __restrict__ keep) {
    __shared__ unsigned long long s_kept;
    const uint32_t n = count_of(d_n, n_host);
    const uint32_t nblk = (n + 63) / 64;
    const uint32_t nstep = (n + kSweepRows - 1) / kSweepRows;
    const uint32_t w = threadIdx.x;
    unsigned long long remv = 0;
    uint32_t count = 0;
    unsigned long long cur[kSweepRows], nxt[kSweepRows];
    // word w of the rows of step s (half a 64-row block); the words left of the diagonal and beyond the last block do not exist
    auto load = [&](unsigned long long (&buf)[kSweepRows], uint32_t s) {
        const bool mine = w >= s * kSweepRows / 64 && w < nblk;
#pragma unroll
        for (int r = 0; r < kSweepRows; r++) {
            const uint32_t row = s * kSweepRows + r;
            buf[r] = (mine && row < n) ? mask[(uint64_t)row * cb + w] : 0ull;
        }
    };
    load(cur, 0);
    for (uint32_t s = 0; s < nstep && count < max_out; s++) {
        load(nxt, s + 1);  // ahead of the decisions of step s: rows do not depend on them
        const uint32_t rb = s * kSweepRows / 64, bit0 = s * kSweepRows % 64;
        if (w == rb) {
            unsigned long long c = remv, kept = 0;
            uint32_t cnt = count;
#pragma unroll
            for (int r = 0; r < kSweepRows; r++) {
                const uint32_t row = s * kSweepRows + r;
                if (row < n && !((c >> (bit0 + r)) & 1ull) && cnt < max_out) {
                    kept |= 1ull << r;
                    c |= cur[r];
                    keep[cnt] = order ? (long long)order[row] : (long long)row;
                    cnt++;
                }
            }
            s_kept = kept;
        }
        __syncthreads();
        const unsigned long long kept = s_kept;
        if (w >= rb) {  // the owner too: the second half of its block reads what the first half removed
#pragma unroll
            for (int r = 0; r < kSweepRows; r++) remv |= ((kept >> r) & 1ull) ? cur[r] : 0ull;
        }
        count += (uint32_t)__popcll(kept);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kSweepRows; r++) cur[r] = nxt[r];
    }
    if (w == 0) {
        count_out[0] = count;
        count_out[1] = 0;
    }
}

// ---- filter, order, gather -------------------------------------------------------------------------------------------------------------------
// class_agnostic_nms's mask (model_nms_utils.py:5-8): label c (1-based) has the entry thresh[c - 1] >= 0 and score >= it; NaN never passes
__device__ __forceinline__ bool passes(float score, int label, const float* __restrict__ thresh, int n_class) {
    if (label < 1 || label > n_class) return false;
    const float t = thresh[label - 1];
    return t >= 0.f && score >= t;
}

__global__ __launch_bounds__(kThreads) void boxes_filter_count(const float* __restrict__ scores, const int* __restrict__ labels, uint32_t n,
                                                               const float* __restrict__ thresh, int n_class, uint8_t* __restrict__ flags,
                                                               uint32_t* __restrict__ counts) {
    const uint32_t base = blockIdx.x * kTile;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        if (i < n) {
            const bool in = passes(scores[i], labels[i], thresh, n_class);
            flags[i] = in ? 1 : 0;
            c += in ? 1u : 0u;
        }
    }
    compact_tile_count(c, counts);
}

__global__ __launch_bounds__(kThreads) void boxes_filter_write(uint32_t n, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ offs,
                                                               uint32_t* __restrict__ cidx) {
    const uint32_t base = blockIdx.x * kTile;
    bool keep[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        keep[r] = i < n && flags[i] != 0;
    }
    compact_tile_write(keep, offs, [&](int r, uint32_t o) { cidx[o] = base + r * kThreads + threadIdx.x; });
}

// the key whose unsigned order is np.argsort(-scores, kind="stable")'s: ascending -score, -0 and +0 equal, NaN last
__device__ __forceinline__ uint32_t order_key(float score) {
    if (score != score) return 0xFFFFFFFFu;
    const float v = -score;
    return f2ord(v == 0.f ? 0.f : v);
}

// order[rank] = the original index of item i, rank = the items before it: a smaller key, or an equal key and a smaller position (positions
// ascend with the original index: the compaction is stable)
__global__ __launch_bounds__(kOrderThreads) void boxes_order(const float* __restrict__ scores, const uint32_t* __restrict__ cidx, uint32_t m_host,
                                                             const uint32_t* __restrict__ d_m, uint32_t* __restrict__ order) {
    __shared__ uint32_t s_key[kOrderThreads];
    const uint32_t m = count_of(d_m, m_host);
    if (blockIdx.x * kOrderThreads >= m) return;
    const uint32_t i = blockIdx.x * kOrderThreads + threadIdx.x;
    const uint32_t src = (i < m) ? (cidx ? cidx[i] : i) : 0;
    const uint32_t ki = (i < m) ? order_key(scores[src]) : 0u;
    uint32_t rank = 0;
    for (uint32_t base = 0; base < m; base += kOrderThreads) {
        const uint32_t j = base + threadIdx.x;
        __syncthreads();
        s_key[threadIdx.x] = (j < m) ? order_key(scores[cidx ? cidx[j] : j]) : 0xFFFFFFFFu;
        __syncthreads();
        const uint32_t lim = min((uint32_t)kOrderThreads, m - base);
        for (uint32_t t = 0; t < lim; t++) {
            const uint32_t kj = s_key[t];
            rank += (kj < ki || (kj == ki && base + t < i)) ? 1u : 0u;
        }
    }
    if (i < m) order[rank] = src;
}

// res: [count, 0, 0, 0][post_max x 7 boxes][post_max scores][post_max labels][post_max original indices]
__global__ __launch_bounds__(kThreads) void boxes_gather(const float* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ labels,
                                                         const long long* __restrict__ keep, uint32_t post_max, uint32_t* __restrict__ res) {
    const uint32_t count = min(res[0], post_max);
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= count) return;
    const uint64_t i = (uint64_t)keep[k];
    float* ob = reinterpret_cast<float*>(res + 4) + (uint64_t)k * 7;
#pragma unroll
    for (int c = 0; c < 7; c++) ob[c] = boxes[i * 7 + c];
    reinterpret_cast<float*>(res + 4)[(uint64_t)post_max * 7 + k] = scores[i];
    reinterpret_cast<int*>(res + 4)[(uint64_t)post_max * 8 + k] = labels[i];
    res[4 + (uint64_t)post_max * 9 + k] = (uint32_t)i;
}

}  // namespace boxes
}  // namespace lio

using namespace lio;
using namespace lio::boxes;

struct lio_boxes {
    int device;
    hipStream_t stream;
    hipEvent_t ev[5];  // begin, ordered, mask written, swept, gathered
    uint32_t max_boxes;
    int gate;  // lio_boxes_set_gate: the mode of the fused post-process
    float* d_a;  // raw rows, max_boxes x 7 each
    float* d_b;
    float* d_scores;
    int* d_labels;
    float* d_thresh;
    uint64_t thresh_cap;
    Prep* prep_a;
    Prep* prep_b;
    uint8_t* flags;
    uint32_t* cidx;
    uint32_t* order;
    uint32_t* aux;  // the compaction's scratch
    unsigned long long* mask;
    uint64_t mask_cap;
    long long* d_keep;  // [count][max_boxes indices]
    uint32_t* d_res;    // the post-process's result
    uint64_t res_cap;
    float* mats[4];
    uint64_t mats_cap[4];
    void* h_stage;  // pinned: the keep list or the post-process's result
    uint32_t post_count, post_room;  // the last post-process's kept count and post_max: its indices are still in h_stage
    uint64_t stage_bytes;
    double order_us, mask_us, sweep_us, total_us;
};

namespace {

uint64_t res_words(uint32_t post_max) { return 4 + (uint64_t)post_max * 10; }

bool rows_ok(const char* who, lio_boxes* h, const void* p, uint64_t n) {
    if (!p && n) { set_error("%s: %llu boxes without a pointer", who, (unsigned long long)n); return false; }
    if (n > h->max_boxes) { set_error("%s: %llu boxes exceed the handle's max_boxes %u", who, (unsigned long long)n, h->max_boxes); return false; }
    return true;
}

void read_times(lio_boxes* h) {
    h->order_us = elapsed_us(h->ev[0], h->ev[1]);
    h->mask_us = elapsed_us(h->ev[1], h->ev[2]);
    h->sweep_us = elapsed_us(h->ev[2], h->ev[3]);
    h->total_us = elapsed_us(h->ev[0], h->ev[4]);
}

// prepare (in `order`, or row order when NULL), mask and sweep over m boxes (m_host bounds it; d_m, when given, holds it on the device):
// the keep list lands in h->d_keep + 1, the count in count_out
int mask_and_sweep(lio_boxes* h, const float* d_boxes, const uint32_t* order, uint32_t m_host, const uint32_t* d_m, float thresh, int mode,
                   uint32_t max_out, uint32_t* count_out) {
    hipStream_t st = h->stream;
    const uint32_t cb = (m_host + 63) / 64;
    int rc = grow("lio_boxes", &h->mask, &h->mask_cap, (uint64_t)m_host * cb, st);
    if (rc != LIO_OK) return rc;
    boxes_prepare<<<dim3(blocks_of(m_host)), dim3(kThreads), 0, st>>>(d_boxes, order, m_host, d_m, h->prep_a);
    boxes_nms_mask<<<dim3(cb, cb), dim3(kLanes), 0, st>>>(h->prep_a, m_host, d_m, thresh, mode, cb, h->mask);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(h->ev[2], st));
    boxes_nms_sweep<<<dim3(1), dim3(kSweepThreads), 0, st>>>(h->mask, m_host, d_m, cb, max_out, order, count_out, h->d_keep + 1);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(h->ev[3], st));
    return LIO_OK;
}

// the fused post-process over device inputs
int64_t postprocess_on_device(const char* who, lio_boxes* h, const float* d_boxes, const float* d_scores, const int* d_labels, uint32_t n,
                              const float* class_thresh, int n_class, float nms_thresh, uint32_t post_max, float* out_boxes, float* out_scores,
                              int* out_labels) {
    hipStream_t st = h->stream;
    if (post_max == 0 || post_max > n) post_max = n;
    h->post_count = 0;
    if (n == 0) return 0;
    int rc = grow("lio_boxes", &h->d_thresh, &h->thresh_cap, (uint64_t)n_class, st);
    if (rc != LIO_OK) return rc;
    rc = grow("lio_boxes", &h->d_res, &h->res_cap, res_words(post_max), st);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipMemcpyAsync(h->d_thresh, class_thresh, (size_t)n_class * sizeof(float), hipMemcpyHostToDevice, st));
    LIO_HIP_TRY(hipEventRecord(h->ev[0], st));
    const uint32_t ntiles = tiles_of(n);
    boxes_filter_count<<<dim3(ntiles), dim3(kThreads), 0, st>>>(d_scores, d_labels, n, h->d_thresh, n_class, h->flags, h->aux);
    const uint32_t* d_m = compact_finish(st, h->aux, n);
    if (!d_m) return LIO_E_DEVICE;
    boxes_filter_write<<<dim3(ntiles), dim3(kThreads), 0, st>>>(n, h->flags, h->aux, h->cidx);
    boxes_order<<<dim3((n + kOrderThreads - 1) / kOrderThreads), dim3(kOrderThreads), 0, st>>>(d_scores, h->cidx, n, d_m, h->order);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(h->ev[1], st));
    rc = mask_and_sweep(h, d_boxes, h->order, n, d_m, nms_thresh, h->gate, post_max, h->d_res);
    if (rc != LIO_OK) return rc;
    boxes_gather<<<dim3(blocks_of(post_max)), dim3(kThreads), 0, st>>>(d_boxes, d_scores, d_labels, h->d_keep + 1, post_max, h->d_res);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(h->ev[4], st));
    const uint64_t bytes = res_words(post_max) * sizeof(uint32_t);
    LIO_HIP_TRY(hipMemcpyAsync(h->h_stage, h->d_res, bytes, hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    read_times(h);
    const uint32_t* w = static_cast<const uint32_t*>(h->h_stage);
    const uint32_t count = std::min(w[0], post_max);
    if (count > 0 && (!out_boxes || !out_scores || !out_labels)) {
        set_error("%s: %u boxes are kept and an output pointer is NULL", who, count);
        return LIO_E_INVALID;
    }
    if (count > 0) {
        memcpy(out_boxes, w + 4, (size_t)count * 7 * sizeof(float));
        memcpy(out_scores, w + 4 + (uint64_t)post_max * 7, (size_t)count * sizeof(float));
        memcpy(out_labels, w + 4 + (uint64_t)post_max * 8, (size_t)count * sizeof(int));
    }
    h->post_count = count;
    h->post_room = post_max;
    return (int64_t)count;
}

bool post_args_ok(const char* who, lio_boxes* h, const void* boxes, const void* scores, const void* labels, uint32_t n, const float* class_thresh,
                  int n_class) {
    if (!rows_ok(who, h, boxes, n)) return false;
    if (n && (!scores || !labels)) { set_error("%s: scores and labels are required", who); return false; }
    if (n_class < 1 || n_class > 65536 || !class_thresh) { set_error("%s: 1 to 65536 class thresholds are required (%d given)", who, n_class); return false; }
    return true;
}

}  // namespace

extern "C" {

lio_boxes* lio_boxes_create(int device, uint32_t max_boxes) {
    if (max_boxes == 0 || max_boxes > kMaxBoxes) {
        set_error("lio_boxes_create: max_boxes in [1, %u] is required (%u given)", kMaxBoxes, max_boxes);
        return nullptr;
    }
    lio_boxes* h = new lio_boxes();
    memset(h, 0, sizeof(*h));
    h->device = device;
    h->max_boxes = max_boxes;
    if (!open_device("lio_boxes_create", device, &h->stream, h->ev, 5)) {
        delete h;
        return nullptr;
    }
    const uint64_t m = max_boxes;
    h->stage_bytes = std::max<uint64_t>((m + 1) * sizeof(long long), res_words(max_boxes) * sizeof(uint32_t));
    const bool ok = alloc(&h->d_a, m * 7) && alloc(&h->d_b, m * 7) && alloc(&h->d_scores, m) && alloc(&h->d_labels, m) && alloc(&h->prep_a, m) &&
                    alloc(&h->prep_b, m) && alloc(&h->flags, m) && alloc(&h->cidx, m) && alloc(&h->order, m) && alloc(&h->aux, compact_words(m)) &&
                    alloc(&h->d_keep, m + 1) && hipHostMalloc(&h->h_stage, h->stage_bytes) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        set_error("lio_boxes_create: buffers for %u boxes not available", max_boxes);
        lio_boxes_destroy(h);
        return nullptr;
    }
    return h;
}

void lio_boxes_destroy(lio_boxes* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    void* all[] = {h->d_a, h->d_b, h->d_scores, h->d_labels, h->d_thresh, h->prep_a, h->prep_b, h->flags, h->cidx, h->order, h->aux, h->mask, h->d_keep,
                   h->d_res, h->mats[0], h->mats[1], h->mats[2], h->mats[3]};
    for (void* p : all)
        if (p) (void)hipFree(p);
    if (h->h_stage) hipHostFree(h->h_stage);
    for (int i = 0; i < 5; i++)
        if (h->ev[i]) hipEventDestroy(h->ev[i]);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

int lio_boxes_pairwise(lio_boxes* h, const float* a, uint32_t na, const float* b, uint32_t nb, float* overlap, float* hull, float* iou_bev,
                       float* giou3d) {
    if (!h) return LIO_E_INVALID;
    if (!rows_ok("lio_boxes_pairwise", h, a, na) || !rows_ok("lio_boxes_pairwise", h, b, nb)) return LIO_E_INVALID;
    if (na == 0 || nb == 0) return LIO_OK;
    hipSetDevice(h->device);
    hipStream_t st = h->stream;
    float* out[4] = {overlap, hull, iou_bev, giou3d};
    const uint64_t cells = (uint64_t)na * nb;
    for (int k = 0; k < 4; k++) {
        if (!out[k]) continue;
        const int rc = grow("lio_boxes_pairwise", &h->mats[k], &h->mats_cap[k], cells, st);
        if (rc != LIO_OK) return rc;
    }
    LIO_HIP_TRY(hipMemcpyAsync(h->d_a, a, (size_t)na * 7 * sizeof(float), hipMemcpyHostToDevice, st));
    LIO_HIP_TRY(hipMemcpyAsync(h->d_b, b, (size_t)nb * 7 * sizeof(float), hipMemcpyHostToDevice, st));
    LIO_HIP_TRY(hipEventRecord(h->ev[0], st));
    boxes_prepare<<<dim3(blocks_of(na)), dim3(kThreads), 0, st>>>(h->d_a, nullptr, na, nullptr, h->prep_a);
    boxes_prepare<<<dim3(blocks_of(nb)), dim3(kThreads), 0, st>>>(h->d_b, nullptr, nb, nullptr, h->prep_b);
    boxes_pairwise<<<dim3((nb + kLanes - 1) / kLanes, na), dim3(kLanes), 0, st>>>(h->prep_a, na, h->prep_b, nb, overlap ? h->mats[0] : nullptr,
                                                                                 hull ? h->mats[1] : nullptr, iou_bev ? h->mats[2] : nullptr,
                                                                                 giou3d ? h->mats[3] : nullptr);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(h->ev[4], st));
    for (int k = 0; k < 4; k++)
        if (out[k]) LIO_HIP_TRY(hipMemcpyAsync(out[k], h->mats[k], cells * sizeof(float), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    h->order_us = h->mask_us = h->sweep_us = 0;
    h->total_us = elapsed_us(h->ev[0], h->ev[4]);
    return LIO_OK;
}

int64_t lio_boxes_nms(lio_boxes* h, const float* boxes, const float* scores, uint32_t n, float thresh, int mode, uint32_t max_out, int64_t* keep) {
    if (!h) return LIO_E_INVALID;
    if (!rows_ok("lio_boxes_nms", h, boxes, n)) return LIO_E_INVALID;
    if (mode != LIO_BOXES_NMS_ROTATED && mode != LIO_BOXES_NMS_AABB_GATE) { set_error("lio_boxes_nms: mode %d is not one of the two", mode); return LIO_E_INVALID; }
    if (n && !keep) { set_error("lio_boxes_nms: keep is required"); return LIO_E_INVALID; }
    if (n == 0) return 0;
    if (max_out == 0 || max_out > n) max_out = n;
    h->post_count = 0;  // the staging is about to hold the keep list
    hipSetDevice(h->device);
    hipStream_t st = h->stream;
    LIO_HIP_TRY(hipMemcpyAsync(h->d_a, boxes, (size_t)n * 7 * sizeof(float), hipMemcpyHostToDevice, st));
    if (scores) LIO_HIP_TRY(hipMemcpyAsync(h->d_scores, scores, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    LIO_HIP_TRY(hipEventRecord(h->ev[0], st));
    if (scores) boxes_order<<<dim3((n + kOrderThreads - 1) / kOrderThreads), dim3(kOrderThreads), 0, st>>>(h->d_scores, nullptr, n, nullptr, h->order);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(h->ev[1], st));
    const int rc = mask_and_sweep(h, h->d_a, scores ? h->order : nullptr, n, nullptr, thresh, mode, max_out, reinterpret_cast<uint32_t*>(h->d_keep));
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipEventRecord(h->ev[4], st));
    LIO_HIP_TRY(hipMemcpyAsync(h->h_stage, h->d_keep, ((size_t)max_out + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    read_times(h);
    const long long* w = static_cast<const long long*>(h->h_stage);
    const uint32_t count = (uint32_t)std::min<long long>(w[0], max_out);
    for (uint32_t k = 0; k < count; k++) keep[k] = (int64_t)w[1 + k];
    return (int64_t)count;
}

int lio_boxes_set_gate(lio_boxes* h, int mode) {
    if (!h || (mode != LIO_BOXES_NMS_ROTATED && mode != LIO_BOXES_NMS_AABB_GATE)) return LIO_E_INVALID;
    h->gate = mode;
    return LIO_OK;
}

int64_t lio_boxes_postprocess(lio_boxes* h, const float* boxes, const float* scores, const int32_t* labels, uint32_t n, const float* class_thresh,
                              int n_class, float nms_thresh, uint32_t post_max, float* out_boxes, float* out_scores, int32_t* out_labels) {
    if (!h) return LIO_E_INVALID;
    if (!post_args_ok("lio_boxes_postprocess", h, boxes, scores, labels, n, class_thresh, n_class)) return LIO_E_INVALID;
    h->post_count = 0;
    if (n == 0) return 0;
    hipSetDevice(h->device);
    hipStream_t st = h->stream;
    LIO_HIP_TRY(hipMemcpyAsync(h->d_a, boxes, (size_t)n * 7 * sizeof(float), hipMemcpyHostToDevice, st));
    LIO_HIP_TRY(hipMemcpyAsync(h->d_scores, scores, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    LIO_HIP_TRY(hipMemcpyAsync(h->d_labels, labels, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    return postprocess_on_device("lio_boxes_postprocess", h, h->d_a, h->d_scores, h->d_labels, n, class_thresh, n_class, nms_thresh, post_max, out_boxes,
                                 out_scores, out_labels);
}

int64_t lio_boxes_postprocess_device(lio_boxes* h, const float* d_boxes, const float* d_scores, const int32_t* d_labels, uint32_t n,
                                     const float* class_thresh, int n_class, float nms_thresh, uint32_t post_max, float* out_boxes, float* out_scores,
                                     int32_t* out_labels) {
    if (!h) return LIO_E_INVALID;
    if (!post_args_ok("lio_boxes_postprocess_device", h, d_boxes, d_scores, d_labels, n, class_thresh, n_class)) return LIO_E_INVALID;
    h->post_count = 0;
    if (n == 0) return 0;
    hipSetDevice(h->device);
    return postprocess_on_device("lio_boxes_postprocess_device", h, d_boxes, d_scores, d_labels, n, class_thresh, n_class, nms_thresh, post_max,
                                 out_boxes, out_scores, out_labels);
}

int64_t lio_boxes_last_indices(lio_boxes* h, uint32_t* out, uint64_t cap) {
    if (!h) return LIO_E_INVALID;
    if (h->post_count > cap) return -(int64_t)h->post_count;
    if (h->post_count == 0) return 0;
    if (!out) return LIO_E_INVALID;
    memcpy(out, static_cast<const uint32_t*>(h->h_stage) + 4 + (uint64_t)h->post_room * 9, (size_t)h->post_count * sizeof(uint32_t));
    return (int64_t)h->post_count;
}

int lio_boxes_last_times(lio_boxes* h, double* order_us, double* mask_us, double* sweep_us, double* total_us) {
    if (!h) return LIO_E_INVALID;
    if (order_us) *order_us = h->order_us;
    if (mask_us) *mask_us = h->mask_us;
    if (sweep_us) *sweep_us = h->sweep_us;
    if (total_us) *total_us = h->total_us;
    return LIO_OK;
}

}  // extern "C"
