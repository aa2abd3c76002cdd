// localmap.hip -- local-map assembly for localisation, resident on the device: Localization::runUpdateLocalMap
// (/root/reference/slam/localization/src/localization.cpp:303-373).  The reference keeps every key frame's world-frame cloud on
// the host, and every 10 m of travel concatenates the key frames within 30 m of the pose (nearest first, thinned by
// key_frame_distance, until 200 000 points), runs a VoxelGrid over the result and hands it to the matcher as its new target
// (a host -> device upload of up to 200 k points each time).  Here the key-frame clouds live in one HBM buffer; an update is
// a handful of device-to-device segment copies into a scan buffer, the VoxelGrid kernels (voxelgrid.hip) and the NDT target
// build (ndt.hip) -- nothing crosses PCIe.  Key-frame selection (tens of candidates) stays on the host.
//
// The operator's hint (GlobalLocalization::getEstimatePose, /root/reference/slam/localization/src/global_localization.cpp:196-262) uses the same
// store: the five key frames nearest the hint are gathered into one buffer by ONE launch (which also sums z), handed to the FAST_VGICP matcher
// as its target without leaving HBM, and the latest scan -- already on the device -- is its source.
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "lio_common.h"

using namespace lio;

namespace lio {

constexpr int kGatherMaxIds = 16;
struct GatherSegs {
    uint64_t src[kGatherMaxIds];  // first point of the key frame in the store
    uint32_t end[kGatherMaxIds];  // one past its last point in the output
    int n;
};

// The z sum's rule (include/lio_hip.h, "the chunked z sum"): lane j of a chunk of 256 consecutive points holds (double)z of its point, 0 past
// the end; the chunk's sum is the tree x[j] += x[j + s], s = 128, 64, ..., 1.  Returns the sum in every lane.
__device__ __forceinline__ double chunk_z_sum(double* x, double z) {
    const int j = threadIdx.x;
    x[j] = z;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (j < s) x[j] += x[j + s];
        __syncthreads();
    }
    return x[0];
}

// the named key frames back to back, in the order given: one lane per output point, one block per chunk of the z sum
__global__ void __launch_bounds__(256) localmap_gather_kernel(const float4* __restrict__ store, GatherSegs g, uint32_t total, float4* __restrict__ out,
                                                              double* __restrict__ partial) {
    __shared__ double x[256];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    double z = 0.0;
    if (i < total) {
        int f = 0;
        while (f < g.n - 1 && i >= g.end[f]) f++;  // (empty frames have end[f] == end[f - 1] and are passed over)
        const uint32_t begin = f ? g.end[f - 1] : 0u;
        const float4 p = store[g.src[f] + (i - begin)];
        out[i] = p;
        z = (double)p.z;
    }
    const double s = chunk_z_sum(x, z);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// the chunk sums of a cloud that stays where it is (the source's mean z)
__global__ void __launch_bounds__(256) localmap_zsum_kernel(const float4* __restrict__ pts, uint32_t n, double* __restrict__ partial) {
    __shared__ double x[256];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const double s = chunk_z_sum(x, i < n ? (double)pts[i].z : 0.0);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// the chunk sums added in rising chunk order by one thread; the block only brings them into LDS 256 at a time
__global__ void __launch_bounds__(256) localmap_zfinish_kernel(const double* __restrict__ partial, uint32_t n_chunks, double* __restrict__ out) {
    __shared__ double x[256];
    double s = 0.0;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += 256u) {
        const uint32_t m = n_chunks - c0 < 256u ? n_chunks - c0 : 256u;
        if (threadIdx.x < m) x[threadIdx.x] = partial[c0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (uint32_t j = 0; j < m; j++) s += x[j];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s;
}

}  // namespace lio

struct lio_localmap {
    int device;
    float4* pts;  // all key-frame clouds, back to back
    uint64_t cap, used;
    std::vector<uint64_t> off;
    std::vector<uint32_t> cnt;
    std::vector<std::array<float, 3>> pos;
    lio_scan* scan;  // assembly + VoxelGrid buffers
    uint32_t max_local;
    bool have_last;
    double last[3];
    bool have_map;
    // get_estimate_pose: the gathered key frames, the z sum's scratch, two kept frames (0 the latest scan, 1 the matched one), the stage events;
    // all made when first needed
    float4* gather = nullptr;
    uint32_t gather_cap = 0, n_gather = 0;
    double* zpartial = nullptr;
    uint32_t zpartial_cap = 0;
    double* zsum = nullptr;
    float4* frame[2] = {nullptr, nullptr};
    uint32_t frame_cap[2] = {0, 0}, frame_n[2] = {0, 0};
    hipEvent_t ev[8] = {};
    bool have_ev = false;
};

namespace {

// chunk sums -> sum -> mean, the second half of the z rule; `chunks` partial sums lie in lm->zpartial
int localmap_finish_z(lio_localmap* lm, uint32_t chunks, uint32_t n, double* z_mean) {
    hipStream_t st = lm->scan->stream;
    hipLaunchKernelGGL(localmap_zfinish_kernel, 1, 256, 0, st, lm->zpartial, chunks, lm->zsum);
    LIO_HIP_TRY(hipGetLastError());
    double sum = 0.0;
    LIO_HIP_TRY(hipMemcpyAsync(&sum, lm->zsum, sizeof(double), hipMemcpyDeviceToHost, st));
    LIO_HIP_TRY(hipStreamSynchronize(st));
    if (z_mean) *z_mean = sum / (double)n;
    return LIO_OK;
}

int localmap_z_scratch(lio_localmap* lm, uint32_t chunks) {
    if (!lm->zsum) LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&lm->zsum), sizeof(double)));
    if (chunks > lm->zpartial_cap) {
        double* p = nullptr;
        LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), (size_t)chunks * sizeof(double)));
        if (lm->zpartial) hipFree(lm->zpartial);
        lm->zpartial = p;
        lm->zpartial_cap = chunks;
    }
    return LIO_OK;
}

double us_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace

extern "C" {

lio_localmap* lio_localmap_create(int device, uint64_t max_total_points, uint32_t max_local_points, uint32_t max_keyframe_points) {
    if (max_total_points == 0 || max_local_points == 0 || max_keyframe_points == 0) { set_error("lio_localmap_create: bad argument"); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { set_error("lio_localmap_create: no HIP device %d (this library has no CPU fallback)", device); return nullptr; }
    lio_localmap* lm = new lio_localmap();
    lm->device = device;
    lm->cap = max_total_points;
    lm->used = 0;
    lm->max_local = max_local_points;
    lm->have_last = lm->have_map = false;
    lm->pts = nullptr;
    // the concatenation stops AFTER the key frame that crosses max_local_points (localization.cpp:345-347)
    lm->scan = lio_scan_create(device, max_local_points + max_keyframe_points, max_local_points + max_keyframe_points);
    if (!lm->scan || hipMalloc(reinterpret_cast<void**>(&lm->pts), max_total_points * sizeof(float4)) != hipSuccess) {
        if (lm->scan) lio_scan_destroy(lm->scan);
        set_error("lio_localmap_create: allocation failed");
        delete lm;
        return nullptr;
    }
    return lm;
}

void lio_localmap_destroy(lio_localmap* lm) {
    if (!lm) return;
    hipSetDevice(lm->device);
    lio_scan_destroy(lm->scan);
    hipFree(lm->pts);
    if (lm->gather) hipFree(lm->gather);
    if (lm->zpartial) hipFree(lm->zpartial);
    if (lm->zsum) hipFree(lm->zsum);
    for (float4* f : lm->frame) if (f) hipFree(f);
    if (lm->have_ev) for (hipEvent_t e : lm->ev) hipEventDestroy(e);
    delete lm;
}

// one key frame: its cloud already transformed to the map frame (KeyFrame::mTransfromPoints) and its position (the graph kd-tree's point)
int lio_localmap_add_keyframe(lio_localmap* lm, const float* world_xyzi, uint32_t n, const float position[3]) {
    if (!lm || (!world_xyzi && n) || !position) return LIO_E_INVALID;
    if (lm->used + n > lm->cap) { set_error("key-frame store full (%llu + %u > %llu points)", (unsigned long long)lm->used, n, (unsigned long long)lm->cap); return LIO_E_CAPACITY; }
    if (n > lm->scan->max_raw - lm->max_local) { set_error("key frame of %u points exceeds max_keyframe_points", n); return LIO_E_CAPACITY; }
    hipSetDevice(lm->device);
    if (n) LIO_HIP_TRY(hipMemcpy(lm->pts + lm->used, world_xyzi, (size_t)n * sizeof(float4), hipMemcpyHostToDevice));
    lm->off.push_back(lm->used);
    lm->cnt.push_back(n);
    lm->pos.push_back({position[0], position[1], position[2]});
    lm->used += n;
    return (int)lm->off.size() - 1;
}

int lio_localmap_num_keyframes(lio_localmap* lm) { return lm ? (int)lm->off.size() : LIO_E_INVALID; }

// One pass of runUpdateLocalMap's loop body.  Returns 0: pose within update_distance of the last update, nothing done;
// 1: target replaced; 2: no key frame within `radius` (target dropped, "out of map"); 3: nearest key frame >= 20 m away (target
// dropped).  n_keyframes / n_points report what went into the target (after the VoxelGrid).
int lio_localmap_update(lio_localmap* lm, lio_ndt* ndt, const double pose_xyz[3], double update_distance, double radius, double key_frame_distance,
                        float leaf, int* n_keyframes, uint32_t* n_points) {
    if (!lm || !ndt || !pose_xyz || !(leaf > 0.f)) return LIO_E_INVALID;
    if (n_keyframes) *n_keyframes = 0;
    if (n_points) *n_points = 0;
    if (lm->have_map && lm->have_last) {
        const double dx = pose_xyz[0] - lm->last[0], dy = pose_xyz[1] - lm->last[1], dz = pose_xyz[2] - lm->last[2];
        if (!(std::sqrt(dx * dx + dy * dy + dz * dz) > update_distance)) return 0;
    }
    hipSetDevice(lm->device);
    // mGraphKDTree->radiusSearch(searchPoint, radius): key frames within the radius, nearest first (f32 like pcl::PointXYZ)
    const float sx = (float)pose_xyz[0], sy = (float)pose_xyz[1], sz = (float)pose_xyz[2];
    std::vector<std::pair<float, int>> hits;
    for (size_t i = 0; i < lm->pos.size(); i++) {
        const float dx = lm->pos[i][0] - sx, dy = lm->pos[i][1] - sy, dz = lm->pos[i][2] - sz;
        const float d2 = dx * dx + dy * dy + dz * dz;
        if (d2 <= (float)(radius * radius)) hits.push_back({d2, (int)i});
    }
    if (hits.empty()) {
        lm->have_map = false;
        lio_ndt_set_target_device(ndt, nullptr, 0);
        return 2;
    }
    std::stable_sort(hits.begin(), hits.end(), [](const std::pair<float, int>& a, const std::pair<float, int>& b) { return a.first < b.first; });
    for (int i = 0; i < 3; i++) lm->last[i] = pose_xyz[i];
    lm->have_last = true;
    lio_scan* s = lm->scan;
    uint32_t total = 0;
    int used = 0;
    float accum = 0.f;
    for (const auto& h : hits) {
        const float distance = std::sqrt(h.first);
        if (total != 0 && (double)(distance - accum) < key_frame_distance) continue;
        accum = distance;
        const uint32_t c = lm->cnt[h.second];
        if (c) LIO_HIP_TRY(hipMemcpyAsync(s->raw_own + total, lm->pts + lm->off[h.second], (size_t)c * sizeof(float4), hipMemcpyDeviceToDevice, s->stream));
        total += c;
        used++;
        if (total >= lm->max_local) break;
    }
    s->raw = s->raw_own;
    s->n_raw = total;
    uint32_t n_ds = 0;
    int rc = lio_scan_voxel_downsample(s, leaf, 1, &n_ds);
    if (rc != LIO_OK) return rc;
    if (n_keyframes) *n_keyframes = used;
    if (n_points) *n_points = n_ds;
    if (hits[0].first >= 400.f) {  // nearest key frame 20 m away or more
        lm->have_map = false;
        lio_ndt_set_target_device(ndt, nullptr, 0);
        return 3;
    }
    rc = lio_ndt_set_target_device(ndt, s->ds_body, n_ds);
    if (rc != LIO_OK) return rc;
    lm->have_map = true;
    return 1;
}

// the assembled, downsampled local map of the last update (test visibility)
int lio_localmap_download(lio_localmap* lm, float* out_xyzi, uint32_t cap) { return (!lm || !out_xyzi) ? LIO_E_INVALID : lio_scan_download_ds(lm->scan, out_xyzi, cap); }


// ---- the operator's hint ----------------------------------------------------------------------------------------------------------------

// mGraphKDTree->nearestKSearch over the key-frame positions with z = 0 on both sides (buildGraphKDTree): host, like lio_localmap_update's selection
int lio_localmap_nearest(lio_localmap* lm, const double xy[2], uint32_t k, int32_t* ids, float* d2) {
    if (!lm || !xy || (k && !ids) || !std::isfinite(xy[0]) || !std::isfinite(xy[1])) return LIO_E_INVALID;
    const float sx = (float)xy[0], sy = (float)xy[1];
    std::vector<std::pair<float, int>> all(lm->pos.size());
    for (size_t i = 0; i < lm->pos.size(); i++) {
        const float dx = lm->pos[i][0] - sx, dy = lm->pos[i][1] - sy;
        all[i] = {dx * dx + dy * dy, (int)i};
    }
    std::sort(all.begin(), all.end());  // (d2, id): equal distances go to the smaller id
    const uint32_t n = (uint32_t)std::min<size_t>(k, all.size());
    for (uint32_t i = 0; i < n; i++) {
        ids[i] = all[i].second;
        if (d2) d2[i] = all[i].first;
    }
    return (int)n;
}

int lio_localmap_gather(lio_localmap* lm, const int32_t* ids, uint32_t n_ids, uint32_t* n_points, double* z_mean) {
    if (!lm || (!ids && n_ids) || n_ids > (uint32_t)kGatherMaxIds) { set_error("lio_localmap_gather: bad argument (at most %d ids)", kGatherMaxIds); return LIO_E_INVALID; }
    GatherSegs g;
    std::memset(&g, 0, sizeof(g));
    g.n = (int)n_ids;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_ids; i++) {
        if (ids[i] < 0 || (size_t)ids[i] >= lm->off.size()) { set_error("lio_localmap_gather: no key frame %d", ids[i]); return LIO_E_INVALID; }
        total += lm->cnt[ids[i]];
        g.src[i] = lm->off[ids[i]];
        g.end[i] = (uint32_t)std::min<uint64_t>(total, 0xFFFFFFFFull);
    }
    // the buffer holds what five of the largest key frames come to, and no less than a local map
    const uint64_t cap = std::max<uint64_t>((uint64_t)lm->scan->max_raw, 5ull * (lm->scan->max_raw - lm->max_local));
    if (total > cap || total > 0x7FFFFFFFull) { set_error("lio_localmap_gather: %llu points exceed the buffer of %llu", (unsigned long long)total, (unsigned long long)cap); return LIO_E_CAPACITY; }
    if (total == 0) { set_error("lio_localmap_gather: the named key frames hold no point"); return LIO_E_INVALID; }
    hipSetDevice(lm->device);
    if (!lm->gather) {
        LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&lm->gather), (size_t)cap * sizeof(float4)));
        lm->gather_cap = (uint32_t)cap;
    }
    const uint32_t n = (uint32_t)total, chunks = (n + 255u) / 256u;
    int rc = localmap_z_scratch(lm, chunks);
    if (rc != LIO_OK) return rc;
    hipLaunchKernelGGL(localmap_gather_kernel, chunks, 256, 0, lm->scan->stream, lm->pts, g, n, lm->gather, lm->zpartial);
    LIO_HIP_TRY(hipGetLastError());
    lm->n_gather = n;
    if (n_points) *n_points = n;
    return localmap_finish_z(lm, chunks, n, z_mean);
}

// the mean z of any cloud in HBM by the gather's rule (the source of the hint)
int lio_localmap_z_mean(lio_localmap* lm, const void* d_xyzi, uint32_t n, double* z_mean) {
    if (!lm || !d_xyzi || n == 0 || !z_mean) return LIO_E_INVALID;
    hipSetDevice(lm->device);
    const uint32_t chunks = (n + 255u) / 256u;
    const int rc = localmap_z_scratch(lm, chunks);
    if (rc != LIO_OK) return rc;
    hipLaunchKernelGGL(localmap_zsum_kernel, chunks, 256, 0, lm->scan->stream, static_cast<const float4*>(d_xyzi), n, lm->zpartial);
    LIO_HIP_TRY(hipGetLastError());
    return localmap_finish_z(lm, chunks, n, z_mean);
}

int lio_localmap_download_gather(lio_localmap* lm, float* out_xyzi, uint32_t cap) {
    if (!lm || !out_xyzi) return LIO_E_INVALID;
    if (lm->n_gather > cap) return LIO_E_CAPACITY;
    hipSetDevice(lm->device);
    if (lm->n_gather) LIO_HIP_TRY(hipMemcpy(out_xyzi, lm->gather, (size_t)lm->n_gather * sizeof(float4), hipMemcpyDeviceToHost));
    return (int)lm->n_gather;
}

const void* lio_localmap_gather_device(lio_localmap* lm, uint32_t* n) {
    if (n) *n = lm ? lm->n_gather : 0;
    return lm && lm->n_gather ? lm->gather : nullptr;
}

// a device copy of a cloud kept with the local map (slot 0: the latest scan, 1: the frame a hint was matched with); n = 0 empties the slot
int lio_localmap_store_frame(lio_localmap* lm, int slot, const void* d_xyzi, uint32_t n) {
    if (!lm || slot < 0 || slot > 1 || (!d_xyzi && n)) return LIO_E_INVALID;
    hipSetDevice(lm->device);
    if (n > lm->frame_cap[slot]) {
        float4* p = nullptr;
        const uint32_t cap = std::max<uint32_t>(n, 1u << 16);
        LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p), (size_t)cap * sizeof(float4)));
        if (lm->frame[slot]) hipFree(lm->frame[slot]);
        lm->frame[slot] = p;
        lm->frame_cap[slot] = cap;
    }
    if (n && d_xyzi != lm->frame[slot]) LIO_HIP_TRY(hipMemcpy(lm->frame[slot], d_xyzi, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice));
    lm->frame_n[slot] = n;
    return LIO_OK;
}

const void* lio_localmap_frame(lio_localmap* lm, int slot, uint32_t* n) {
    const bool ok = lm && slot >= 0 && slot <= 1;
    if (n) *n = ok ? lm->frame_n[slot] : 0;
    return ok && lm->frame_n[slot] ? lm->frame[slot] : nullptr;
}

// the matcher as GlobalLocalization's mRegistration is configured: select_registration_method("FAST_VGICP"), the loop detector's coarse form
void lio_estimate_matcher_params(lio_ndt_params* p) {
    if (!p) return;
    lio_loop_params lp;
    lio_loop_default_params(&lp);
    lio_ndt_default_params(p);
    p->rotation_epsilon_deg = lp.coarse_rotation_epsilon_deg;
    p->transformation_epsilon = lp.coarse_translation_epsilon;
    p->max_iterations = lp.max_iterations;
    p->max_process_time_ms = -1;
}

int lio_localmap_estimate_pose(lio_localmap* lm, lio_gicp* gicp, const void* d_source_xyzi, uint32_t n_source, const double hint[16], lio_estimate_report* report,
                               double out_T[16]) {
    if (!lm || !gicp || !hint || !out_T || (!d_source_xyzi && n_source)) return LIO_E_INVALID;
    for (int a = 0; a < 12; a++)
        if (!std::isfinite(hint[a])) { set_error("lio_localmap_estimate_pose: the hint is not finite"); return LIO_E_INVALID; }
    lio_estimate_report r;
    std::memset(&r, 0, sizeof(r));
    r.n_source = n_source;
    std::memcpy(out_T, hint, 16 * sizeof(double));
    std::memcpy(r.guess, hint, 16 * sizeof(double));
    auto done = [&](int rc) { if (report) *report = r; return rc; };
    hipSetDevice(lm->device);
    if (!lm->have_ev) {
        for (hipEvent_t& e : lm->ev) LIO_HIP_TRY(hipEventCreate(&e));
        lm->have_ev = true;
    }
    hipStream_t st = lm->scan->stream;
    // 1. the 5 nearest key frames, nearest first, up to the first one more than 20 m away
    auto t0 = std::chrono::steady_clock::now();
    const double xy[2] = {hint[3], hint[7]};
    int32_t ids[LIO_ESTIMATE_K];
    float d2[LIO_ESTIMATE_K];
    const int nn = lio_localmap_nearest(lm, xy, LIO_ESTIMATE_K, ids, d2);
    if (nn < 0) return done(nn);
    uint64_t total = 0;
    for (int i = 0; i < nn; i++) {
        if (d2[i] > 400.f) break;
        r.ids[r.n_ids++] = ids[i];
        total += lm->cnt[ids[i]];
    }
    r.nearest_us = us_since(t0);
    if (total == 0 || n_source == 0) return done(LIO_OK);  // "getEstimatePose: data is empty": result 0, the hint untouched
    // 2. the target without leaving HBM, the source from where it lies
    int rc;
    LIO_HIP_TRY(hipEventRecord(lm->ev[0], st));
    if ((rc = lio_localmap_gather(lm, r.ids, (uint32_t)r.n_ids, &r.n_target, &r.z_mean_target)) != LIO_OK) return done(rc);
    LIO_HIP_TRY(hipEventRecord(lm->ev[1], st));
    if ((rc = lio_gicp_set_target_device(gicp, lm->gather, r.n_target)) != LIO_OK) return done(rc);
    LIO_HIP_TRY(hipEventRecord(lm->ev[2], st));
    if ((rc = lio_gicp_set_source_device(gicp, d_source_xyzi, n_source)) != LIO_OK) return done(rc);
    LIO_HIP_TRY(hipEventRecord(lm->ev[3], st));
    // 3. the hint's height: the difference of the two clouds' mean z
    if ((rc = lio_localmap_z_mean(lm, d_source_xyzi, n_source, &r.z_mean_source)) != LIO_OK) return done(rc);
    LIO_HIP_TRY(hipEventRecord(lm->ev[4], st));
    out_T[11] = r.z_mean_target - r.z_mean_source;
    // 4. align(*aligned, t.cast<float>())
    for (int a = 0; a < 16; a++) r.guess[a] = (double)(float)out_T[a];
    // 5. FAST_VGICP
    lio_ndt_params p;
    lio_estimate_matcher_params(&p);
    lio_loop_params lp;
    lio_loop_default_params(&lp);
    double T[16];
    int it = 0, conv = 0;
    if ((rc = lio_gicp_align(gicp, r.guess, &p, 1.0, T, &it, &conv)) != LIO_OK) return done(rc);
    LIO_HIP_TRY(hipEventRecord(lm->ev[5], st));
    r.iterations = it;
    r.converged = conv;
    bool scored = false;
    if (conv) {  // 7. getFitnessScore(fitness_score_max_range)
        if ((rc = lio_gicp_fitness_score(gicp, T, lp.fitness_score_max_range, &r.score, nullptr)) != LIO_OK) return done(rc);
        scored = true;
        if (r.score < 5.0) {
            for (int a = 0; a < 12; a++) out_T[a] = (double)(float)T[a];
            out_T[12] = out_T[13] = out_T[14] = 0.0;
            out_T[15] = 1.0;
            r.pose_replaced = 1;
        }
        if (r.score < 0.5) r.result = 1;
    }
    LIO_HIP_TRY(hipEventRecord(lm->ev[6], st));
    LIO_HIP_TRY(hipEventSynchronize(lm->ev[6]));
    double* us[6] = {&r.gather_us, &r.set_target_us, &r.set_source_us, &r.z_source_us, &r.align_us, &r.fitness_us};
    for (int k = 0; k < 6; k++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, lm->ev[k], lm->ev[k + 1]) == hipSuccess) *us[k] = (double)ms * 1000.0;
    }
    if (!scored) r.fitness_us = 0.0;
    return done(LIO_OK);
}

}  // extern "C"
