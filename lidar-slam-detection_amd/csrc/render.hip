// render.hip -- the road-surface colour map on gfx950 (wave64): MapRender of slam/localization/map_render/ (map_render.cpp, render_common.h,
// image_render.hpp's ImageRenderCpu, camera_model.{h,cpp}), rule by rule.  include/lio_hip.h states every rule; tests/render_cases.py restates
// them in numpy.
//
//   insert    world transform, voxel and key of every frame point; the voxel hash (hashgrid.h's brick probing over the box triple) and the
//             (voxel, key) hash are probed and tentatively filled, the smallest input index claims each new voxel and each new key (atomicMin)
//   number    device_prims.h's stable compaction, twice: voxel creators and stored points in input order -> voxel numbers and point serials
//   decide    one lane: the frame fits (voxels, points, hash tables) or it does not.  Every later kernel reads that word: a frame that does not
//             fit commits nothing and its tentative hash entries are taken back (they were the last to enter, so the tables are as before)
//   hits      one lane per touched voxel: hits + 1, its point list grown, the voxel put on the hit list
//   link      stored points appended to their voxel's list
//   gate      (per image) one lane per hit voxel: the centre must project, be available and lie in (2, 80) m -- the survivors are queued
//   project   one wave per queued voxel: every stored point projected, the (u, v) bounding box by wave reduction, the 10-pixel mask, then
//             the 64-bit atomicMin of (f32 depth bits, serial) into the image-sized buffer
//   resolve   one lane per pixel: an owned pixel runs the 9 x 9 depth test straight from the buffer, then score, sample and blend
//   finish    the frame's scratch words reset, the roll-back when the frame did not fit
//
// Point lists.  A voxel's stored points are a contiguous run of serials in a pool; a run that is outgrown moves to one of twice the size
// (bump allocation, the old run is left behind: at most 4 words per point and 8 per voxel in all).  A wave reads a run with consecutive
// lanes on consecutive words; chunked lists would chase a pointer every chunk, and a per-frame sort would touch every stored point of every
// hit voxel once more per frame.  The order inside a run is the order of arrival and nothing reads it: the bounding box is a min / max, the
// z-buffer an atomicMin, the blend per point.
// Window test.  Owned pixels are sparse (one per visible point, a few ten thousand in two million), so a staged tile with its halo would
// load whole tiles for a handful of owners; the 81 reads go to the buffer, which L2 / MALL hold.
// Sample.  Only a valid winner needs its colour, so score and sample are taken in resolve, not for every projected point.
//
// One stream, no host round trip between the images of a frame, one wait at the frame's end (the ground detector, when asked for, waits
// for its own RANSAC before that).
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "device_prims.h"
#include "hashgrid.h"

namespace lio {
namespace render {

using namespace prims;

constexpr double kPointRes = 0.02, kInvPointRes = 1.0 / kPointRes, kVoxelRes = 0.2, kInvVoxelRes = 1.0 / kVoxelRes;
constexpr double kMinDepth = 2.0, kMaxDepth = 80.0, kMargin = 0.005;
constexpr int kBoxLimit = 1 << 20;          // |box| below this: pack_key's 21 bits per axis
constexpr uint32_t kKeyBias = 1024;         // offset key + bias lies in [0, 4096)
constexpr unsigned long long kNoOwner = 0xFFFFFFFFFFFFFFFFull;
constexpr uint32_t kProjectBlocks = 4096;

struct Status {
    uint32_t n_voxels, n_points;   // committed
    uint32_t base_v, base_p;       // ... before this frame
    uint32_t new_voxels, new_points, n_hits, overflow, ok, dropped;
    unsigned long long pool_top;
};

struct Tables {
    unsigned long long* vkeys;  // voxel hash: pack_key of the box triple
    uint32_t vmask;
    uint32_t *slot_vid, *slot_first, *slot_new;
    unsigned long long* pkeys;  // (voxel slot, offset key) hash
    uint32_t pmask;
    uint32_t *ent_serial, *ent_claim;
};

struct Voxels {
    int4* box;
    uint32_t *hits, *cnt, *ptr, *cap;
};

struct Points {
    float4* pos;   // x, y, z, voxel number
    float4* col;   // r, g, b, score
    float* depth;  // m_depth
};

struct Mat34 {
    double m[12];
};

struct Camera {  // camera from world, intrinsics, image
    double R[9], t[3], fx, fy, cx, cy;
    int cols, rows;
};

struct Proj {
    double u, v, z;
};

__device__ __forceinline__ bool project(const Camera& c, double x, double y, double z, Proj& o) {
    const double px = ((c.R[0] * x + c.R[1] * y) + c.R[2] * z) + c.t[0];
    const double py = ((c.R[3] * x + c.R[4] * y) + c.R[5] * z) + c.t[1];
    const double pz = ((c.R[6] * x + c.R[7] * y) + c.R[8] * z) + c.t[2];
    if (pz < 0.001 || !(pz == pz)) return false;
    o.u = px * c.fx / pz + c.cx;
    o.v = py * c.fy / pz + c.cy;
    o.z = pz;
    return true;
}

__device__ __forceinline__ bool available(const Camera& c, double u, double v) {
    return u >= (kMargin * c.cols + 1) && ceil(u) < ((1 - kMargin) * c.cols) && v >= (kMargin * c.rows + 1) && ceil(v) < ((1 - kMargin) * c.rows);
}

__device__ __forceinline__ int unpack21(unsigned long long k, int shift) {
    const uint32_t v = (uint32_t)(k >> shift) & 0x1FFFFFu;
    return (int)(v << 11) >> 11;
}

__device__ __forceinline__ uint32_t hash64(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)k;
}

// ---- insert ----
__global__ __launch_bounds__(kThreads) void rd_insert(const float4* __restrict__ in, uint32_t n, Mat34 T, float4* __restrict__ world,
                                                      uint32_t* __restrict__ slot_of, uint32_t* __restrict__ ent_of, Tables tb, Status* __restrict__ st) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float4 p = in[i];
    const double x = p.x, y = p.y, z = p.z;
    float4 w;
    w.x = (float)(((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3]);
    w.y = (float)(((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7]);
    w.z = (float)(((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11]);
    w.w = p.w;
    world[i] = w;
    uint32_t slot = kNoIdx, ent = kNoIdx;
    const double bx = round((double)w.x * kInvVoxelRes), by = round((double)w.y * kInvVoxelRes), bz = round((double)w.z * kInvVoxelRes);
    const bool in_range = fabs(bx) < (double)kBoxLimit && fabs(by) < (double)kBoxLimit && fabs(bz) < (double)kBoxLimit;  // (false for NaN)
    if (!in_range) {
        atomicAdd(&st->dropped, 1u);
    } else {
        const int ix = (int)bx, iy = (int)by, iz = (int)bz;
        const unsigned long long want = pack_key(ix, iy, iz);
        BrickProbe bp = brick_probe(ix, iy, iz);
        for (uint32_t probe = 0; probe <= (tb.vmask >> 6); probe++) {
            const uint32_t s = brick_slot(bp, tb.vmask);
            unsigned long long k = __hip_atomic_load(&tb.vkeys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k == kEmptyKey) k = atomicCAS(&tb.vkeys[s], kEmptyKey, want);
            if (k == kEmptyKey || k == want) { slot = s; break; }
            brick_next(bp);
        }
        if (slot != kNoIdx) {
            atomicMin(&tb.slot_first[slot], i);
            const long long cx = (long long)(((double)ix * kVoxelRes) * kInvPointRes), cy = (long long)(((double)iy * kVoxelRes) * kInvPointRes),
                            cz = (long long)(((double)iz * kVoxelRes) * kInvPointRes);
            const int ox = (int)((long long)((double)w.x * kInvPointRes) - cx + 5), oy = (int)((long long)((double)w.y * kInvPointRes) - cy + 5),
                      oz = (int)((long long)((double)w.z * kInvPointRes) - cz + 5);
            const int key = ox * 100 + oy * 10 + oz;
            const unsigned long long pk = ((unsigned long long)slot << 12) | (uint32_t)((key + (int)kKeyBias) & 4095);
            uint32_t e = hash64(pk) & tb.pmask;
            for (uint32_t probe = 0; probe <= tb.pmask; probe++) {
                unsigned long long k = __hip_atomic_load(&tb.pkeys[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (k == kEmptyKey) k = atomicCAS(&tb.pkeys[e], kEmptyKey, pk);
                if (k == kEmptyKey || k == pk) { ent = e; break; }
                e = (e + 1u) & tb.pmask;
            }
            if (ent != kNoIdx) {
                // an entry of an earlier frame has its serial; the others are this frame's and the smallest input index takes them
                if (tb.ent_serial[ent] == kNoIdx) atomicMin(&tb.ent_claim[ent], i);
            }
        }
        if (slot == kNoIdx || ent == kNoIdx) atomicOr(&st->overflow, 1u);
    }
    slot_of[i] = slot;
    ent_of[i] = ent;
}

// which = 0: point i creates its voxel; 1: point i is stored
__device__ __forceinline__ bool numbered(int which, uint32_t i, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ ent_of, const Tables& tb) {
    if (which == 0) {
        const uint32_t s = slot_of[i];
        return s != kNoIdx && tb.slot_first[s] == i && tb.slot_vid[s] == kNoIdx;
    }
    const uint32_t e = ent_of[i];
    return e != kNoIdx && tb.ent_claim[e] == i && tb.ent_serial[e] == kNoIdx;
}

__global__ __launch_bounds__(kThreads) void rd_count(int which, uint32_t n, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ ent_of, Tables tb,
                                                     uint32_t* __restrict__ counts) {
    const uint32_t base = blockIdx.x * kTile;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        c += (i < n && numbered(which, i, slot_of, ent_of, tb)) ? 1u : 0u;
    }
    compact_tile_count(c, counts);
}

__global__ void rd_decide(const uint32_t* __restrict__ tot_v, const uint32_t* __restrict__ tot_p, uint32_t max_voxels, uint32_t max_points, Status* __restrict__ st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t nv = *tot_v, np = *tot_p;
    const bool ok = !st->overflow && (uint64_t)st->n_voxels + nv <= max_voxels && (uint64_t)st->n_points + np <= max_points;
    st->base_v = st->n_voxels;
    st->base_p = st->n_points;
    st->new_voxels = nv;
    st->new_points = np;
    st->n_hits = 0;
    st->ok = ok ? 1u : 0u;
    if (ok) {
        st->n_voxels += nv;
        st->n_points += np;
    }
}

__global__ __launch_bounds__(kThreads) void rd_number_voxels(uint32_t n, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ ent_of, Tables tb,
                                                             const uint32_t* __restrict__ offs, Voxels vx, const Status* __restrict__ st) {
    if (!st->ok) return;
    const uint32_t base = blockIdx.x * kTile, base_v = st->base_v;
    bool keep[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        keep[r] = i < n && numbered(0, i, slot_of, ent_of, tb);
    }
    compact_tile_write(keep, offs, [&](int r, uint32_t o) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        const uint32_t s = slot_of[i], v = base_v + o;
        const unsigned long long k = tb.vkeys[s];
        tb.slot_vid[s] = v;
        vx.box[v] = make_int4(unpack21(k, 0), unpack21(k, 21), unpack21(k, 42), 0);
        vx.hits[v] = 0;
        vx.cnt[v] = 0;
        vx.ptr[v] = 0;
        vx.cap[v] = 0;
    });
}

__global__ __launch_bounds__(kThreads) void rd_number_points(uint32_t n, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ ent_of, Tables tb,
                                                             const uint32_t* __restrict__ offs, const float4* __restrict__ world, Points pt,
                                                             uint32_t* __restrict__ stored, const Status* __restrict__ st) {
    if (!st->ok) return;
    const uint32_t base = blockIdx.x * kTile, base_p = st->base_p;
    bool keep[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        keep[r] = i < n && numbered(1, i, slot_of, ent_of, tb);
    }
    compact_tile_write(keep, offs, [&](int r, uint32_t o) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        const uint32_t e = ent_of[i], s = slot_of[i], q = base_p + o;
        const float4 w = world[i];
        tb.ent_serial[e] = q;
        pt.pos[q] = make_float4(w.x, w.y, w.z, 0.f);
        pt.col[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        pt.depth[q] = 100.0f;
        stored[i] = q;
        atomicAdd(&tb.slot_new[s], 1u);
    });
}

// one lane per touched voxel (the frame's first point in it): hits, room for the new points, the hit list
__global__ __launch_bounds__(kThreads) void rd_hits(uint32_t n, const uint32_t* __restrict__ slot_of, Tables tb, Voxels vx, uint32_t* __restrict__ pool,
                                                    uint64_t pool_cap, uint32_t* __restrict__ hitlist, Status* __restrict__ st) {
    if (!st->ok) return;
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t s = i < n ? slot_of[i] : kNoIdx;
    const bool head = s != kNoIdx && tb.slot_first[s] == i;
    uint32_t v = 0;
    if (head) {
        v = tb.slot_vid[s];
        vx.hits[v] += 1u;
        const uint32_t have = vx.cnt[v], need = have + tb.slot_new[s];
        if (need > vx.cap[v]) {
            uint32_t nc = 8;
            while (nc < need) nc <<= 1;
            const unsigned long long to = atomicAdd(&st->pool_top, (unsigned long long)nc);
            const uint32_t from = vx.ptr[v];
            if (to + nc <= pool_cap) {  // (always: the pool holds 4 words per point and 8 per voxel, more than the runs can add up to)
                for (uint32_t k = 0; k < have; k++) pool[to + k] = pool[from + k];
                vx.ptr[v] = (uint32_t)to;
                vx.cap[v] = nc;
            }
        }
    }
    const unsigned long long hm = __ballot(head);
    if (hm) {
        const int lane = threadIdx.x & 63, leader = __ffsll((long long)hm) - 1;
        uint32_t qb = 0;
        if (lane == leader) qb = atomicAdd(&st->n_hits, (uint32_t)__popcll(hm));
        qb = __shfl(qb, leader);
        if (head) hitlist[qb + __popcll(hm & ((1ull << lane) - 1ull))] = v;
    }
}

__global__ __launch_bounds__(kThreads) void rd_link(uint32_t n, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ stored, Tables tb, Voxels vx,
                                                    Points pt, uint32_t* __restrict__ pool, const Status* __restrict__ st) {
    if (!st->ok) return;
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t q = stored[i];
    if (q == kNoIdx) return;
    const uint32_t v = tb.slot_vid[slot_of[i]];
    const uint32_t j = atomicAdd(&vx.cnt[v], 1u);
    if (j < vx.cap[v]) pool[vx.ptr[v] + j] = q;
    pt.pos[q].w = __uint_as_float(v);
}

// ---- per image ----
__global__ __launch_bounds__(kThreads) void rd_gate(const uint32_t* __restrict__ hitlist, Voxels vx, Camera cam, uint32_t* __restrict__ passlist,
                                                    double2* __restrict__ passuv, uint32_t* __restrict__ n_pass, const Status* __restrict__ st) {
    if (!st->ok) return;
    const uint32_t h = blockIdx.x * kThreads + threadIdx.x;
    bool pass = false;
    uint32_t v = 0;
    Proj c = {0, 0, 0};
    if (h < st->n_hits) {
        v = hitlist[h];
        const int4 b = vx.box[v];
        const long long cx = (long long)(((double)b.x * kVoxelRes) * kInvPointRes), cy = (long long)(((double)b.y * kVoxelRes) * kInvPointRes),
                        cz = (long long)(((double)b.z * kVoxelRes) * kInvPointRes);
        pass = project(cam, (double)cx * kPointRes, (double)cy * kPointRes, (double)cz * kPointRes, c) && available(cam, c.u, c.v) && !(c.z <= kMinDepth) &&
               !(c.z >= kMaxDepth);
    }
    const unsigned long long pm = __ballot(pass);
    if (pm) {
        const int lane = threadIdx.x & 63, leader = __ffsll((long long)pm) - 1;
        uint32_t qb = 0;
        if (lane == leader) qb = atomicAdd(n_pass, (uint32_t)__popcll(pm));
        qb = __shfl(qb, leader);
        if (pass) {
            const uint32_t o = qb + __popcll(pm & ((1ull << lane) - 1ull));
            passlist[o] = v;
            passuv[o] = make_double2(c.u, c.v);
        }
    }
}

__device__ __forceinline__ double wave_min(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmin(x, __shfl_xor(x, off));
    return x;
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off));
    return x;
}

__global__ __launch_bounds__(kThreads) void rd_project(const uint32_t* __restrict__ passlist, const double2* __restrict__ passuv, const uint32_t* __restrict__ n_pass,
                                                       Voxels vx, Points pt, const uint32_t* __restrict__ pool, Camera cam, Proj* __restrict__ scr,
                                                       unsigned long long* __restrict__ zbuf, const Status* __restrict__ st) {
    if (!st->ok) return;
    const int lane = threadIdx.x & 63;
    const uint32_t np = *n_pass;
    for (uint32_t w = blockIdx.x * kWaves + (threadIdx.x >> 6); w < np; w += gridDim.x * kWaves) {
        const uint32_t v = passlist[w];
        const double2 cuv = passuv[w];
        const uint32_t cnt = min(vx.cnt[v], vx.cap[v]), ptr = vx.ptr[v];
        double ulo = cuv.x, uhi = cuv.x, vlo = cuv.y, vhi = cuv.y;
        for (uint32_t k = lane; k < cnt; k += 64) {
            const uint32_t q = pool[ptr + k];
            const float4 p = pt.pos[q];
            Proj o;
            const bool kept = project(cam, (double)p.x, (double)p.y, (double)p.z, o) && available(cam, o.u, o.v);
            if (kept) {
                ulo = fmin(ulo, o.u); uhi = fmax(uhi, o.u);
                vlo = fmin(vlo, o.v); vhi = fmax(vhi, o.v);
            } else {
                o.u = 0; o.v = 0; o.z = -1.0;
            }
            scr[q] = o;
        }
        ulo = wave_min(ulo); uhi = wave_max(uhi);
        vlo = wave_min(vlo); vhi = wave_max(vhi);
        if ((uhi - ulo) <= 10.0 && (vhi - vlo) <= 10.0) continue;  // the voxel covers too little of this image
        for (uint32_t k = lane; k < cnt; k += 64) {
            const uint32_t q = pool[ptr + k];
            const Proj o = scr[q];  // (this lane's own store)
            if (!(o.z > 0)) continue;
            const int pu = (int)round(o.u), pv = (int)round(o.v);
            if (pu < 0 || pu >= cam.cols || pv < 0 || pv >= cam.rows) continue;  // (cannot happen for an available point)
            atomicMin(&zbuf[(uint64_t)pv * cam.cols + pu], ((unsigned long long)__float_as_uint((float)o.z) << 32) | q);
        }
    }
}

__device__ __forceinline__ uint32_t u8_term(double w, uint32_t pix) {
    const double r = rint(w * (double)pix);  // ties to even, as cvRound
    return r <= 0.0 ? 0u : (r >= 255.0 ? 255u : (uint32_t)r);
}

__global__ __launch_bounds__(kThreads) void rd_resolve(const unsigned long long* __restrict__ zbuf, const Proj* __restrict__ scr, const uint8_t* __restrict__ img,
                                                       Camera cam, Points pt, uint8_t* __restrict__ valid, const Status* __restrict__ st) {
    if (!st->ok) return;
    const uint64_t pix = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const int cols = cam.cols, rows = cam.rows;
    if (pix >= (uint64_t)cols * rows) return;
    const unsigned long long own = zbuf[pix];
    if (own == kNoOwner) { valid[pix] = 0; return; }
    const uint32_t q = (uint32_t)own;
    const Proj o = scr[q];
    float dmin = (float)o.z, dmax = (float)o.z;
    for (int i = -4; i <= 4; i++) {
        for (int j = -4; j <= 4; j++) {
            const int iu = (int)(o.u + i), jv = (int)(o.v + j);
            if (iu < 0 || iu >= cols || jv < 0 || jv >= rows) continue;
            const unsigned long long k = zbuf[(uint64_t)jv * cols + iu];
            if (k == kNoOwner) continue;
            const float d = __uint_as_float((uint32_t)(k >> 32));
            dmin = fminf(dmin, d);
            dmax = fmaxf(dmax, d);
        }
    }
    const bool ok = !((double)(dmax - dmin) > 2.0);
    valid[pix] = ok ? 1 : 0;
    if (!ok) return;
    // update_voxel_rgb
    const float score = (float)(1.0 - fabs(o.u - cols / 2.0) / (cols / 2.0));
    if ((double)score < 0.1) return;
    const float md = pt.depth[q];
    if (o.z > (double)md * 1.5) return;
    if (o.z < (double)md) pt.depth[q] = (float)o.z;
    // getSubPixel<cv::Vec3b>(image, v, u)
    const int fr = (int)floor(o.v), fc = (int)floor(o.u);
    const double ar = o.v - fr, ac = o.u - fc;
    const double wt[4] = {(1.0 - ar) * (1.0 - ac), ar * (1.0 - ac), (1.0 - ar) * ac, ar * ac};
    const int tr[4] = {fr, fr + 1, fr, fr + 1}, tc[4] = {fc, fc, fc + 1, fc + 1};
    uint32_t bgr[3] = {0, 0, 0};
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (wt[t] == 0.0 || tr[t] < 0 || tr[t] >= rows || tc[t] < 0 || tc[t] >= cols) continue;  // a tap of weight zero is not read
        const uint8_t* px = img + ((uint64_t)tr[t] * cols + tc[t]) * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) bgr[c] = min(bgr[c] + u8_term(wt[t], px[c]), 255u);
    }
    const float4 old = pt.col[q];
    const double s1 = (double)old.w, s2 = (double)score;
    float4 nw;
    nw.x = (float)(((double)old.x * s1 + (double)bgr[2] * s2) / (s1 + s2));
    nw.y = (float)(((double)old.y * s1 + (double)bgr[1] * s2) / (s1 + s2));
    nw.z = (float)(((double)old.z * s1 + (double)bgr[0] * s2) / (s1 + s2));
    nw.w = (float)fmax(s1, s2);
    pt.col[q] = nw;
}

// the frame's scratch words back to their rest values; a frame that did not fit takes its hash entries back
__global__ __launch_bounds__(kThreads) void rd_finish(uint32_t n, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ ent_of, Tables tb,
                                                      const Status* __restrict__ st) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const bool undo = !st->ok;
    const uint32_t s = slot_of[i], e = ent_of[i];
    if (s != kNoIdx) {
        tb.slot_first[s] = kNoIdx;
        tb.slot_new[s] = 0;
        if (undo && tb.slot_vid[s] == kNoIdx) tb.vkeys[s] = kEmptyKey;
    }
    if (e != kNoIdx) {
        tb.ent_claim[e] = kNoIdx;
        if (undo && tb.ent_serial[e] == kNoIdx) tb.pkeys[e] = kEmptyKey;
    }
}

// ---- export ----
__device__ __forceinline__ bool exported(uint32_t q, const Voxels& vx, const Points& pt) {
    const uint32_t v = __float_as_uint(pt.pos[q].w);
    return vx.hits[v] > 2u && !((double)pt.col[q].w < 0.1);
}

__global__ __launch_bounds__(kThreads) void rd_export_count(uint32_t n, Voxels vx, Points pt, uint32_t* __restrict__ counts) {
    const uint32_t base = blockIdx.x * kTile;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t q = base + r * kThreads + threadIdx.x;
        c += (q < n && exported(q, vx, pt)) ? 1u : 0u;
    }
    compact_tile_count(c, counts);
}

__global__ __launch_bounds__(kThreads) void rd_export_write(uint32_t n, Voxels vx, Points pt, const uint32_t* __restrict__ offs, uint32_t* __restrict__ keys,
                                                            uint32_t* __restrict__ vals) {
    const uint32_t base = blockIdx.x * kTile;
    bool keep[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t q = base + r * kThreads + threadIdx.x;
        keep[r] = q < n && exported(q, vx, pt);
    }
    compact_tile_write(keep, offs, [&](int r, uint32_t o) {
        const uint32_t q = base + r * kThreads + threadIdx.x;
        keys[o] = __float_as_uint(pt.pos[q].w);
        vals[o] = q;
    });
}

__device__ __forceinline__ uint32_t channel(float c) { return (uint32_t)(uint8_t)(int)c; }

__global__ __launch_bounds__(kThreads) void rd_export_gather(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ d_n, Points pt, float4* __restrict__ out) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= *d_n) return;
    const uint32_t q = vals[j];
    const float4 p = pt.pos[q], c = pt.col[q];
    out[j] = make_float4(p.x, p.y, p.z, __uint_as_float((channel(c.x) << 16) | (channel(c.y) << 8) | channel(c.z)));
}

}  // namespace render
}  // namespace lio

using namespace lio;
using namespace lio::render;

struct lio_render {
    int device;
    hipStream_t stream;
    hipEvent_t ev[6];  // frame begin, insert end, images end, frame end, export begin / end
    uint64_t max_voxels, max_points;
    Tables tb;
    Voxels vx;
    Points pt;
    uint32_t* pool;
    uint64_t pool_cap;
    Proj* scr;
    Status* d_st;
    Status* h_st;  // pinned
    lio_ground* ground;
    // per-frame scratch (frame_cap points)
    uint64_t frame_cap;
    float4 *stage, *world;
    uint32_t *slot_of, *ent_of, *stored, *hitlist, *passlist, *aux;
    double2* passuv;
    uint64_t region;
    uint32_t* d_npass;
    // images
    uint8_t* img;
    uint64_t img_cap;
    unsigned long long* zbuf;
    uint8_t* valid;
    uint64_t zbuf_cap, valid_cap;
    int last_cols, last_rows;
    // export scratch
    uint32_t *ka, *kb, *va, *vb, *radix, *eaux;
    float4* eout;
    uint64_t exp_cap;
    // cameras
    std::vector<std::string>* names;
    std::vector<double>* intr;   // 4 per camera
    std::vector<double>* ext;    // 12 per camera: R, t of static_trans^-1
    int active;
    double last_pose[16];
    double insert_us, image_us, finish_us;
};

namespace {

void mul3(const double* a, const double* b, double* c) {  // c = a b, every sum left to right
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}
void mulv(const double* a, const double* v, double* o) {
    for (int i = 0; i < 3; i++) o[i] = (a[3 * i] * v[0] + a[3 * i + 1] * v[1]) + a[3 * i + 2] * v[2];
}
void split(const double* T, double* R, double* t) {
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[3 * i + j] = T[4 * i + j];
        t[i] = T[4 * i + 3];
    }
}
// the inverse of a rigid transform: R^T, -(R^T t)
void rigid_inverse(const double* R, const double* t, double* Ri, double* ti) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Ri[3 * i + j] = R[3 * j + i];
    double v[3];
    mulv(Ri, t, v);
    for (int i = 0; i < 3; i++) ti[i] = -v[i];
}

void free_frame(lio_render* r) {
    void* all[] = {r->stage, r->world, r->slot_of, r->ent_of, r->stored, r->hitlist, r->passlist, r->aux, r->passuv};
    for (void* p : all)
        if (p) (void)hipFree(p);
    r->stage = r->world = nullptr;
    r->slot_of = r->ent_of = r->stored = r->hitlist = r->passlist = r->aux = nullptr;
    r->passuv = nullptr;
    r->frame_cap = 0;
}

int reserve_frame(lio_render* r, uint64_t n) {
    if (n <= r->frame_cap) return LIO_OK;
    const uint64_t want = std::max<uint64_t>(n, std::max<uint64_t>(2 * r->frame_cap, 1ull << 14));
    LIO_HIP_TRY(hipStreamSynchronize(r->stream));
    free_frame(r);
    r->region = compact_words(want);
    const bool ok = alloc(&r->stage, want) && alloc(&r->world, want) && alloc(&r->slot_of, want) && alloc(&r->ent_of, want) && alloc(&r->stored, want) &&
                    alloc(&r->hitlist, want) && alloc(&r->passlist, want) && alloc(&r->passuv, want) && alloc(&r->aux, 2 * r->region);
    if (!ok) {
        (void)hipGetLastError();
        free_frame(r);
        set_error("lio_render: device scratch for a frame of %llu points not available", (unsigned long long)want);
        return LIO_E_DEVICE;
    }
    r->frame_cap = want;
    return LIO_OK;
}

uint32_t pow2_at_least(uint64_t x) {
    uint64_t p = 64;
    while (p < x) p <<= 1;
    return (uint32_t)p;
}

int reset_map(lio_render* r) {
    hipStream_t st = r->stream;
    LIO_HIP_TRY(hipMemsetAsync(r->tb.vkeys, 0xFF, ((uint64_t)r->tb.vmask + 1) * sizeof(unsigned long long), st));
    LIO_HIP_TRY(hipMemsetAsync(r->tb.slot_vid, 0xFF, ((uint64_t)r->tb.vmask + 1) * sizeof(uint32_t), st));
    LIO_HIP_TRY(hipMemsetAsync(r->tb.slot_first, 0xFF, ((uint64_t)r->tb.vmask + 1) * sizeof(uint32_t), st));
    LIO_HIP_TRY(hipMemsetAsync(r->tb.slot_new, 0, ((uint64_t)r->tb.vmask + 1) * sizeof(uint32_t), st));
    LIO_HIP_TRY(hipMemsetAsync(r->tb.pkeys, 0xFF, ((uint64_t)r->tb.pmask + 1) * sizeof(unsigned long long), st));
    LIO_HIP_TRY(hipMemsetAsync(r->tb.ent_serial, 0xFF, ((uint64_t)r->tb.pmask + 1) * sizeof(uint32_t), st));
    LIO_HIP_TRY(hipMemsetAsync(r->tb.ent_claim, 0xFF, ((uint64_t)r->tb.pmask + 1) * sizeof(uint32_t), st));
    LIO_HIP_TRY(hipMemsetAsync(r->d_st, 0, sizeof(Status), st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    memset(r->h_st, 0, sizeof(Status));
    r->last_cols = r->last_rows = 0;
    return LIO_OK;
}

void identity(double* T) {
    for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

template <typename T>
int64_t fetch(lio_render* r, const T* src, uint64_t n, T* out, uint64_t cap) {
    return prims::download("lio_render", r->device, r->stream, src, n, out, cap);
}

}  // namespace

extern "C" {

lio_render* lio_render_create(int device, uint64_t max_voxels, uint64_t max_points) {
    if (max_voxels == 0 || max_points == 0 || max_voxels > 0x7FFFFFFFull || max_points > 0x7FFFFFFFull ||
        4 * max_points + 8 * max_voxels > 0xFFFFFFFFull) {
        set_error("lio_render_create: max_voxels and max_points must be positive and 4 max_points + 8 max_voxels below 2^32");
        return nullptr;
    }
    lio_render* r = new lio_render();
    memset((void*)r, 0, sizeof(*r));
    r->device = device;
    if (!open_device("lio_render_create", device, &r->stream, r->ev, 6)) {
        delete r;
        return nullptr;
    }
    r->names = new std::vector<std::string>();
    r->intr = new std::vector<double>();
    r->ext = new std::vector<double>();
    r->max_voxels = max_voxels;
    r->max_points = max_points;
    identity(r->last_pose);
    const uint64_t vcap = pow2_at_least(2 * max_voxels), pcap = pow2_at_least(2 * max_points);
    r->tb.vmask = (uint32_t)(vcap - 1);
    r->tb.pmask = (uint32_t)(pcap - 1);
    r->pool_cap = 4 * max_points + 8 * max_voxels;
    bool ok = alloc(&r->tb.vkeys, vcap) && alloc(&r->tb.slot_vid, vcap) && alloc(&r->tb.slot_first, vcap) && alloc(&r->tb.slot_new, vcap) &&
              alloc(&r->tb.pkeys, pcap) && alloc(&r->tb.ent_serial, pcap) && alloc(&r->tb.ent_claim, pcap) && alloc(&r->vx.box, max_voxels) &&
              alloc(&r->vx.hits, max_voxels) && alloc(&r->vx.cnt, max_voxels) && alloc(&r->vx.ptr, max_voxels) && alloc(&r->vx.cap, max_voxels) &&
              alloc(&r->pt.pos, max_points) && alloc(&r->pt.col, max_points) && alloc(&r->pt.depth, max_points) && alloc(&r->pool, r->pool_cap) &&
              alloc(&r->scr, max_points) && alloc(&r->d_st, 1) && alloc(&r->d_npass, 16) &&
              hipHostMalloc((void**)&r->h_st, sizeof(Status), hipHostMallocDefault) == hipSuccess;
    if (ok) ok = reset_map(r) == LIO_OK;
    if (ok) {
        r->ground = lio_ground_create(device);
        ok = r->ground != nullptr;
    }
    if (!ok) {
        (void)hipGetLastError();
        const char* e = lio_last_error();
        const std::string why = e ? e : "";
        lio_render_destroy(r);
        set_error("lio_render_create: device memory for %llu voxels and %llu points not available (%s)", (unsigned long long)max_voxels,
                  (unsigned long long)max_points, why.c_str());
        return nullptr;
    }
    return r;
}

void lio_render_destroy(lio_render* r) {
    if (!r) return;
    hipSetDevice(r->device);
    if (r->stream) hipStreamSynchronize(r->stream);
    if (r->ground) lio_ground_destroy(r->ground);
    free_frame(r);
    void* all[] = {r->tb.vkeys, r->tb.slot_vid, r->tb.slot_first, r->tb.slot_new, r->tb.pkeys, r->tb.ent_serial, r->tb.ent_claim, r->vx.box, r->vx.hits,
                   r->vx.cnt, r->vx.ptr, r->vx.cap, r->pt.pos, r->pt.col, r->pt.depth, r->pool, r->scr, r->d_st, r->d_npass, r->img, r->zbuf, r->valid,
                   r->ka, r->kb, r->va, r->vb, r->radix, r->eaux, r->eout};
    for (void* p : all)
        if (p) (void)hipFree(p);
    if (r->h_st) (void)hipHostFree(r->h_st);
    for (int i = 0; i < 6; i++)
        if (r->ev[i]) hipEventDestroy(r->ev[i]);
    if (r->stream) hipStreamDestroy(r->stream);
    delete r->names;
    delete r->intr;
    delete r->ext;
    delete r;
}

int lio_render_clear(lio_render* r) {
    if (!r) return LIO_E_INVALID;
    hipSetDevice(r->device);
    return reset_map(r);
}

int lio_render_set_cameras(lio_render* r, int n, const char* const* names, const double* intrinsics, const double* extrinsics, const double* lidar_static) {
    if (!r || n < 0 || (n && (!names || !intrinsics || !extrinsics))) return LIO_E_INVALID;
    double Rl[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tl[3] = {0, 0, 0};
    if (lidar_static) split(lidar_static, Rl, tl);
    double Rli[9], tli[3];
    rigid_inverse(Rl, tl, Rli, tli);
    std::vector<std::string> nm;
    std::vector<double> in, ex;
    for (int c = 0; c < n; c++) {
        if (!names[c]) return LIO_E_INVALID;
        for (int k = 0; k < c; k++)
            if (nm[k] == names[c]) { set_error("lio_render_set_cameras: the name %s is given twice", names[c]); return LIO_E_INVALID; }
        nm.push_back(names[c]);
        for (int k = 0; k < 4; k++) in.push_back((double)(float)intrinsics[4 * c + k]);  // K is read as f32
        // static_trans = camera_extrinsic * lidar_static^-1 (setParameter), ext = static_trans^-1
        double Re[9], te[3], Rs[9], ts[3], v[3], Rx[9], tx[3];
        split(extrinsics + 16 * c, Re, te);
        mul3(Re, Rli, Rs);
        mulv(Re, tli, v);
        for (int k = 0; k < 3; k++) ts[k] = v[k] + te[k];
        rigid_inverse(Rs, ts, Rx, tx);
        ex.insert(ex.end(), Rx, Rx + 9);
        ex.insert(ex.end(), tx, tx + 3);
    }
    *r->names = nm;
    *r->intr = in;
    *r->ext = ex;
    return LIO_OK;
}

int lio_render_set_active(lio_render* r, int active) {
    if (!r) return LIO_E_INVALID;
    r->active = active != 0;
    return LIO_OK;
}

int lio_render_frame(lio_render* r, const float* xyzi, uint64_t n, const double pose[16], int use_ground, uint32_t seed, const lio_render_image* images,
                     int n_images) {
    if (!r || !pose || (n && !xyzi) || n_images < 0 || (n_images && !images)) return LIO_E_INVALID;
    if (n > 0x7FFFFFFFull) { set_error("lio_render_frame: %llu points exceed the int index range", (unsigned long long)n); return LIO_E_CAPACITY; }
    for (int i = 0; i < 16; i++)
        if (!std::isfinite(pose[i])) { set_error("lio_render_frame: the pose is not finite"); return LIO_E_INVALID; }
    // the images in ascending name order (std::map), each checked before anything happens
    std::vector<int> order;
    for (int m = 0; m < n_images; m++) {
        const lio_render_image& im = images[m];
        if (im.camera < 0 || im.camera >= (int)r->names->size() || !im.bgr || im.rows <= 0 || im.cols <= 0 || (uint64_t)im.rows * im.cols > 0x7FFFFFFFull) {
            set_error("lio_render_frame: image %d names camera %d of %d, or is empty", m, im.camera, (int)r->names->size());
            return LIO_E_INVALID;
        }
        for (int k : order)
            if (images[k].camera == im.camera) { set_error("lio_render_frame: two images of camera %s", (*r->names)[im.camera].c_str()); return LIO_E_INVALID; }
        order.push_back(m);
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return (*r->names)[images[a].camera] < (*r->names)[images[b].camera]; });
    if (!r->active) return LIO_RENDER_SKIPPED;
    // movement: the translation of last_pose^-1 pose
    {
        double Rl[9], tl[3], Rli[9], tli[3], tp[3] = {pose[3], pose[7], pose[11]}, v[3];
        split(r->last_pose, Rl, tl);
        rigid_inverse(Rl, tl, Rli, tli);
        mulv(Rli, tp, v);
        const double dx = v[0] + tli[0], dy = v[1] + tli[1], dz = v[2] + tli[2];
        if (std::sqrt((dx * dx + dy * dy) + dz * dz) < 0.1) return LIO_RENDER_SKIPPED;
    }
    memcpy(r->last_pose, pose, sizeof(r->last_pose));
    hipSetDevice(r->device);
    hipStream_t st = r->stream;
    const float4* src = nullptr;
    uint32_t np = (uint32_t)n;
    if (use_ground) {
        lio_ground_params gp;
        lio_ground_default_params(&gp, 0);
        gp.distance_threshold = 0.2;
        gp.seed = seed;
        int found = 0;
        float co[4];
        const int rc = lio_ground_detect_host(r->ground, xyzi, n, &gp, &found, co, nullptr, nullptr, nullptr);
        if (rc != LIO_OK) return rc;
        if (!found) return LIO_RENDER_NO_FLOOR;
        src = ground::inliers_view(r->ground, &np);  // (the detector's stream is idle on return)
    }
    int rc = reserve_frame(r, std::max(np, 1u));
    if (rc != LIO_OK) return rc;
    uint64_t img_bytes = 0, max_pix = 1;
    for (int m : order) {
        img_bytes += ((uint64_t)images[m].rows * images[m].cols * 3 + 255) & ~255ull;
        max_pix = std::max<uint64_t>(max_pix, (uint64_t)images[m].rows * images[m].cols);
    }
    rc = grow("lio_render", &r->img, &r->img_cap, img_bytes, st);
    if (rc == LIO_OK) rc = grow("lio_render", &r->zbuf, &r->zbuf_cap, max_pix, st);
    if (rc == LIO_OK) rc = grow("lio_render", &r->valid, &r->valid_cap, max_pix, st);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipEventRecord(r->ev[0], st));
    if (!use_ground) {
        if (np) LIO_HIP_TRY(hipMemcpyAsync(r->stage, xyzi, (uint64_t)np * sizeof(float4), hipMemcpyHostToDevice, st));
        src = r->stage;
    }
    {
        uint64_t off = 0;
        for (int m : order) {
            const uint64_t bytes = (uint64_t)images[m].rows * images[m].cols * 3;
            LIO_HIP_TRY(hipMemcpyAsync(r->img + off, images[m].bgr, bytes, hipMemcpyHostToDevice, st));
            off += (bytes + 255) & ~255ull;
        }
    }
    Mat34 T;
    for (int i = 0; i < 12; i++) T.m[i] = pose[i];
    const uint32_t nb = std::max(blocks_of(np), 1u), ntiles = std::max(tiles_of(np), 1u);
    uint32_t *cnt_v = r->aux, *cnt_p = r->aux + r->region;
    LIO_HIP_TRY(hipMemsetAsync(r->stored, 0xFF, std::max<uint64_t>(np, 1) * sizeof(uint32_t), st));
    LIO_HIP_TRY(hipMemsetAsync(&r->d_st->overflow, 0, 3 * sizeof(uint32_t), st));  // overflow, ok, dropped
    rd_insert<<<dim3(nb), dim3(kThreads), 0, st>>>(src, np, T, r->world, r->slot_of, r->ent_of, r->tb, r->d_st);
    rd_count<<<dim3(ntiles), dim3(kThreads), 0, st>>>(0, np, r->slot_of, r->ent_of, r->tb, cnt_v);
    rd_count<<<dim3(ntiles), dim3(kThreads), 0, st>>>(1, np, r->slot_of, r->ent_of, r->tb, cnt_p);
    const uint32_t* tot_v = compact_finish(st, cnt_v, std::max(np, 1u));
    const uint32_t* tot_p = compact_finish(st, cnt_p, std::max(np, 1u));
    if (!tot_v || !tot_p) return LIO_E_DEVICE;
    rd_decide<<<dim3(1), dim3(64), 0, st>>>(tot_v, tot_p, (uint32_t)r->max_voxels, (uint32_t)r->max_points, r->d_st);
    rd_number_voxels<<<dim3(ntiles), dim3(kThreads), 0, st>>>(np, r->slot_of, r->ent_of, r->tb, cnt_v, r->vx, r->d_st);
    rd_number_points<<<dim3(ntiles), dim3(kThreads), 0, st>>>(np, r->slot_of, r->ent_of, r->tb, cnt_p, r->world, r->pt, r->stored, r->d_st);
    rd_hits<<<dim3(nb), dim3(kThreads), 0, st>>>(np, r->slot_of, r->tb, r->vx, r->pool, r->pool_cap, r->hitlist, r->d_st);
    rd_link<<<dim3(nb), dim3(kThreads), 0, st>>>(np, r->slot_of, r->stored, r->tb, r->vx, r->pt, r->pool, r->d_st);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(r->ev[1], st));
    {
        uint64_t off = 0;
        for (int m : order) {
            const lio_render_image& im = images[m];
            Camera cam;
            const double* in = r->intr->data() + 4 * im.camera;
            const double* ex = r->ext->data() + 12 * im.camera;
            cam.fx = in[0]; cam.fy = in[1]; cam.cx = in[2]; cam.cy = in[3];
            cam.cols = im.cols; cam.rows = im.rows;
            // ImageRender::setPose: R_w2c = R_pose R_ext, t_w2c = R_pose t_ext + t_pose; camera from world: R = R_w2c^T, t = -(R t_w2c)
            double Rp[9], tp[3], Rw[9], tw[3], v[3];
            split(im.pose, Rp, tp);
            mul3(Rp, ex, Rw);
            mulv(Rp, ex + 9, v);
            for (int k = 0; k < 3; k++) tw[k] = v[k] + tp[k];
            rigid_inverse(Rw, tw, cam.R, cam.t);
            const uint64_t npix = (uint64_t)im.rows * im.cols;
            LIO_HIP_TRY(hipMemsetAsync(r->zbuf, 0xFF, npix * sizeof(unsigned long long), st));
            LIO_HIP_TRY(hipMemsetAsync(r->d_npass, 0, sizeof(uint32_t), st));
            rd_gate<<<dim3(nb), dim3(kThreads), 0, st>>>(r->hitlist, r->vx, cam, r->passlist, r->passuv, r->d_npass, r->d_st);
            rd_project<<<dim3(std::min<uint32_t>(std::max((np + kWaves - 1) / kWaves, 1u), kProjectBlocks)), dim3(kThreads), 0, st>>>(
                r->passlist, r->passuv, r->d_npass, r->vx, r->pt, r->pool, cam, r->scr, r->zbuf, r->d_st);
            rd_resolve<<<dim3(blocks_of(npix)), dim3(kThreads), 0, st>>>(r->zbuf, r->scr, r->img + off, cam, r->pt, r->valid, r->d_st);
            LIO_HIP_TRY(hipGetLastError());
            off += (npix * 3 + 255) & ~255ull;
            r->last_cols = im.cols;
            r->last_rows = im.rows;
        }
    }
    LIO_HIP_TRY(hipEventRecord(r->ev[2], st));
    rd_finish<<<dim3(nb), dim3(kThreads), 0, st>>>(np, r->slot_of, r->ent_of, r->tb, r->d_st);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipMemcpyAsync(r->h_st, r->d_st, sizeof(Status), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipEventRecord(r->ev[3], st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    r->insert_us = elapsed_us(r->ev[0], r->ev[1]);
    r->image_us = elapsed_us(r->ev[1], r->ev[2]);
    r->finish_us = elapsed_us(r->ev[2], r->ev[3]);
    if (!r->h_st->ok) {
        r->last_cols = r->last_rows = 0;
        set_error("lio_render_frame: the frame does not fit (%u + %u of %llu voxels, %u + %u of %llu points%s); the map is unchanged", r->h_st->n_voxels,
                  r->h_st->new_voxels, (unsigned long long)r->max_voxels, r->h_st->n_points, r->h_st->new_points, (unsigned long long)r->max_points,
                  r->h_st->overflow ? ", a hash table full" : "");
        return LIO_E_CAPACITY;
    }
    if (n_images == 0) r->last_cols = r->last_rows = 0;
    return LIO_RENDER_DONE;
}

int lio_render_size(lio_render* r, uint64_t* n_voxels, uint64_t* n_points) {
    if (!r) return LIO_E_INVALID;
    if (n_voxels) *n_voxels = r->h_st->n_voxels;
    if (n_points) *n_points = r->h_st->n_points;
    return LIO_OK;
}

int64_t lio_render_download(lio_render* r, float* xyzrgb, uint64_t cap) {
    if (!r) return LIO_E_INVALID;
    hipSetDevice(r->device);
    hipStream_t st = r->stream;
    const uint32_t n = r->h_st->n_points, nv = r->h_st->n_voxels;
    if (n == 0) return 0;
    if (n > r->exp_cap) {
        LIO_HIP_TRY(hipStreamSynchronize(st));
        void* all[] = {r->ka, r->kb, r->va, r->vb, r->radix, r->eaux, r->eout};
        for (void* p : all)
            if (p) (void)hipFree(p);
        r->ka = r->kb = r->va = r->vb = r->radix = r->eaux = nullptr;
        r->eout = nullptr;
        r->exp_cap = 0;
        const uint64_t want = std::max<uint64_t>(n, 1ull << 14);
        if (!(alloc(&r->ka, want) && alloc(&r->kb, want) && alloc(&r->va, want) && alloc(&r->vb, want) && alloc(&r->radix, cloud::radix_scratch_words(want)) &&
              alloc(&r->eaux, compact_words(want)) && alloc(&r->eout, want))) {
            (void)hipGetLastError();
            set_error("lio_render_download: device scratch for %llu points not available", (unsigned long long)want);
            return LIO_E_DEVICE;
        }
        r->exp_cap = want;
    }
    const uint32_t ntiles = tiles_of(n);
    LIO_HIP_TRY(hipEventRecord(r->ev[4], st));
    rd_export_count<<<dim3(ntiles), dim3(kThreads), 0, st>>>(n, r->vx, r->pt, r->eaux);
    const uint32_t* d_m = compact_finish(st, r->eaux, n);
    if (!d_m) return LIO_E_DEVICE;
    rd_export_write<<<dim3(ntiles), dim3(kThreads), 0, st>>>(n, r->vx, r->pt, r->eaux, r->ka, r->va);
    LIO_HIP_TRY(hipGetLastError());
    uint32_t m = 0;
    LIO_HIP_TRY(hipMemcpyAsync(&m, d_m, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    if (m > cap) return -(int64_t)m;
    if (m == 0) return 0;
    if (!xyzrgb) return LIO_E_INVALID;
    // ascending voxel number, then serial: the kept points are in serial order, a stable sort by the voxel number does the rest
    uint32_t *ki = r->ka, *vi = r->va, *ko = r->kb, *vo = r->vb;
    for (int shift = 0; shift < 32 && ((uint64_t)(nv - 1) >> shift) != 0; shift += 8) {
        const int rc = cloud::radix_pass(st, ki, vi, ko, vo, m, shift, r->radix);
        if (rc != LIO_OK) return rc;
        std::swap(ki, ko);
        std::swap(vi, vo);
    }
    rd_export_gather<<<dim3(blocks_of(m)), dim3(kThreads), 0, st>>>(vi, d_m, r->pt, r->eout);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(r->ev[5], st));
    return fetch(r, reinterpret_cast<const float*>(r->eout), 4ull * m, xyzrgb, 4ull * m) < 0 ? LIO_E_DEVICE : (int64_t)m;
}

int64_t lio_render_download_voxels(lio_render* r, int32_t* box, uint32_t* hits, uint32_t* counts, uint64_t cap) {
    if (!r) return LIO_E_INVALID;
    const uint64_t n = r->h_st->n_voxels;
    if (n > cap) return -(int64_t)n;
    if (n == 0) return 0;
    int64_t rc = (int64_t)n;
    if (box) {
        std::vector<int4> tmp(n);
        rc = fetch(r, r->vx.box, n, tmp.data(), n);
        for (uint64_t i = 0; rc >= 0 && i < n; i++) { box[3 * i] = tmp[i].x; box[3 * i + 1] = tmp[i].y; box[3 * i + 2] = tmp[i].z; }
    }
    if (hits && rc >= 0) rc = fetch(r, r->vx.hits, n, hits, cap);
    if (counts && rc >= 0) rc = fetch(r, r->vx.cnt, n, counts, cap);
    return rc;
}

int64_t lio_render_download_points(lio_render* r, float* xyz, uint32_t* voxel, float* rgb, float* score, float* depth, uint64_t cap) {
    if (!r) return LIO_E_INVALID;
    const uint64_t n = r->h_st->n_points;
    if (n > cap) return -(int64_t)n;
    if (n == 0) return 0;
    std::vector<float4> pos(n), col(n);
    int64_t rc = fetch(r, r->pt.pos, n, pos.data(), n);
    if (rc >= 0) rc = fetch(r, r->pt.col, n, col.data(), n);
    if (rc >= 0 && depth) rc = fetch(r, r->pt.depth, n, depth, cap);
    if (rc < 0) return rc;
    for (uint64_t i = 0; i < n; i++) {
        if (xyz) { xyz[3 * i] = pos[i].x; xyz[3 * i + 1] = pos[i].y; xyz[3 * i + 2] = pos[i].z; }
        if (voxel) memcpy(&voxel[i], &pos[i].w, sizeof(uint32_t));
        if (rgb) { rgb[3 * i] = col[i].x; rgb[3 * i + 1] = col[i].y; rgb[3 * i + 2] = col[i].z; }
        if (score) score[i] = col[i].w;
    }
    return (int64_t)n;
}

int64_t lio_render_download_last_image(lio_render* r, float* depth, int32_t* owner, uint8_t* valid, uint64_t cap, int* rows, int* cols) {
    if (!r) return LIO_E_INVALID;
    if (rows) *rows = r->last_rows;
    if (cols) *cols = r->last_cols;
    const uint64_t n = (uint64_t)r->last_rows * r->last_cols;
    if (n > cap) return -(int64_t)n;
    if (n == 0) return 0;
    std::vector<unsigned long long> z(n);
    int64_t rc = fetch(r, r->zbuf, n, z.data(), n);
    if (rc >= 0 && valid) rc = fetch(r, r->valid, n, valid, cap);
    if (rc < 0) return rc;
    for (uint64_t i = 0; i < n; i++) {
        const bool own = z[i] != kNoOwner;
        const uint32_t bits = (uint32_t)(z[i] >> 32);
        float d = -1.0f;
        if (own) memcpy(&d, &bits, sizeof(float));
        if (depth) depth[i] = d;
        if (owner) owner[i] = own ? (int32_t)(uint32_t)z[i] : -1;
    }
    return (int64_t)n;
}

int lio_render_last_times(lio_render* r, double* insert_us, double* image_us, double* finish_us) {
    if (!r) return LIO_E_INVALID;
    if (insert_us) *insert_us = r->insert_us;
    if (image_us) *image_us = r->image_us;
    if (finish_us) *finish_us = r->finish_us;
    return LIO_OK;
}

}  // extern "C"
