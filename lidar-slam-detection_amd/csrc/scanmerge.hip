// scanmerge.hip -- several lidars into one frame on gfx950 (wave64): mergePoints (slam/common/slam_utils.cpp:249-273) followed by
// preprocessPoints (slam/common/slam_base.h:83-85) as RTKM::feedPointData calls them (slam/mapping/rtkm/src/rtkm.cpp:105-109), in one pass
// over HBM.
//
//   input     L <= 16 clouds laid end to end in one flat index space, cloud 0 the base: float4 (x, y, z, intensity) and a uint32 stamp (us since
//             the cloud's header) per point
//   keep      the base ungated; a point of cloud l > 0 iff 0 <= double(stamp) + time_shift_l <= double(scan_period_us), its stamp then
//             uint32_t(that sum); time_shift_l = double(header_l) - double(header_0) comes from the host
//   count     sm_count: kept points per tile of 2048 (device_prims.h's stable compaction), and per cloud the kept / early / late totals
//             (LDS counters, one global atomic per cloud a tile touched -- integer sums, the same whatever the order)
//   write     sm_write: the kept points in input order -- base first, then the clouds as given -- each through the Matrix4d rule
//             (prims::xform, the function lio_cloud_append_* applies), intensity as it is, float4 + uint32 out
//
// The offsets and shifts of the clouds are staged in LDS once per workgroup (a kernel argument indexed per lane would go through scratch);
// a point finds its cloud by a four-step search over them.  Non-finite points are neither dropped nor counted apart: mergePoints has no such test.
#include <algorithm>

#include "device_prims.h"

namespace lio {
namespace scanmerge {

using namespace prims;

constexpr uint32_t kMaxClouds = 16;

struct MergeArgs {
    XformArgs x;
    double shift[kMaxClouds];       // time_shift of every cloud ([0] is not read)
    double period;                  // double(scan_period_us)
    uint32_t start[kMaxClouds];     // first flat index of every cloud; 0xFFFFFFFF from n_clouds on
    uint32_t n;                     // points of all clouds
};

struct Staged {
    uint32_t start[kMaxClouds];
    double shift[kMaxClouds];
};

__device__ __forceinline__ void stage(const MergeArgs& a, Staged& s) {
    if (threadIdx.x < kMaxClouds) {
        s.start[threadIdx.x] = a.start[threadIdx.x];
        s.shift[threadIdx.x] = a.shift[threadIdx.x];
    }
    __syncthreads();
}

// the largest l with start[l] <= i (start is ascending, start[0] = 0, the tail 0xFFFFFFFF > every i): empty clouds own no index
__device__ __forceinline__ uint32_t cloud_of(const Staged& s, uint32_t i) {
    uint32_t l = 0;
#pragma unroll
    for (uint32_t step = kMaxClouds / 2; step > 0; step >>= 1)
        if (s.start[l + step] <= i) l += step;
    return l;
}

// mergePoints' test for a point of cloud l: 0 kept, 1 early, 2 late; *stamp becomes uint32_t(stamp + shift) when kept
__device__ __forceinline__ int gate(const Staged& s, uint32_t l, double period, uint32_t* stamp) {
    if (l == 0) return 0;
    const double t = (double)*stamp + s.shift[l];
    if (!(t >= 0)) return 1;
    if (!(t <= period)) return 2;
    *stamp = (uint32_t)t;
    return 0;
}

__global__ __launch_bounds__(kThreads) void sm_count(const uint32_t* __restrict__ stamps, MergeArgs a, uint32_t* __restrict__ counts,
                                                     uint32_t* __restrict__ stats) {
    __shared__ Staged s;
    __shared__ uint32_t tally[3 * kMaxClouds];
    if (threadIdx.x < 3 * kMaxClouds) tally[threadIdx.x] = 0;
    stage(a, s);
    const uint32_t base = blockIdx.x * kTile;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        if (i < a.n) {
            const uint32_t l = cloud_of(s, i);
            uint32_t st = stamps[i];
            const int g = gate(s, l, a.period, &st);
            c += g == 0 ? 1u : 0u;
            if (l) atomicAdd(&tally[3 * l + g], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 * kMaxClouds && tally[threadIdx.x]) atomicAdd(&stats[threadIdx.x], tally[threadIdx.x]);
    compact_tile_count(c, counts);
}

__global__ __launch_bounds__(kThreads) void sm_write(const float4* __restrict__ in, const uint32_t* __restrict__ stamps, MergeArgs a,
                                                     const uint32_t* __restrict__ offs, float4* __restrict__ out, uint32_t* __restrict__ out_stamps) {
    __shared__ Staged s;
    stage(a, s);
    const uint32_t base = blockIdx.x * kTile;
    float4 p[kItems];
    uint32_t st[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        const uint32_t j = i < a.n ? i : a.n - 1u;
        p[r] = in[j];
        st[r] = stamps[j];
    }
    bool keep[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        keep[r] = i < a.n && gate(s, cloud_of(s, i < a.n ? i : a.n - 1u), a.period, &st[r]) == 0;
    }
    compact_tile_write(keep, offs, [&](int r, uint32_t o) {
        out[o] = xform(p[r], a.x);
        out_stamps[o] = st[r];
    });
}

}  // namespace scanmerge
}  // namespace lio

using namespace lio;
using namespace lio::scanmerge;

struct lio_scan_merge {
    int device;
    hipStream_t stream;
    hipEvent_t ev[3];      // upload begin, merge begin, merge end
    uint32_t max_clouds;
    uint64_t max_points;
    float4 *in, *out;
    uint32_t *in_stamps, *out_stamps;
    uint32_t* aux;         // the compaction's scratch, then 3 x 16 words of per-cloud tallies
    uint64_t aux_words;
    double T[16];
    uint64_t n_out;
    double upload_us, merge_us;
};

extern "C" {

lio_scan_merge* lio_scan_merge_create(int device, uint32_t max_clouds, uint64_t max_points) {
    if (max_clouds < 1 || max_clouds > kMaxClouds || max_points < 1 || max_points > 0x7FFFFFFFull) {
        set_error("lio_scan_merge_create: 1 <= max_clouds <= 16 and 1 <= max_points <= 2^31 - 1 (%u, %llu)", max_clouds, (unsigned long long)max_points);
        return nullptr;
    }
    lio_scan_merge* h = new lio_scan_merge();
    memset(h, 0, sizeof(*h));
    h->device = device;
    h->max_clouds = max_clouds;
    h->max_points = max_points;
    for (int i = 0; i < 16; i++) h->T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    if (!open_device("lio_scan_merge_create", device, &h->stream, h->ev, 3)) {
        delete h;
        return nullptr;
    }
    h->aux_words = compact_words(max_points);
    if (!alloc(&h->in, max_points) || !alloc(&h->out, max_points) || !alloc(&h->in_stamps, max_points) || !alloc(&h->out_stamps, max_points) ||
        !alloc(&h->aux, h->aux_words + 3 * kMaxClouds)) {
        (void)hipGetLastError();
        set_error("lio_scan_merge_create: device memory for %llu points not available", (unsigned long long)max_points);
        lio_scan_merge_destroy(h);
        return nullptr;
    }
    return h;
}

void lio_scan_merge_destroy(lio_scan_merge* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->in) hipFree(h->in);
    if (h->out) hipFree(h->out);
    if (h->in_stamps) hipFree(h->in_stamps);
    if (h->out_stamps) hipFree(h->out_stamps);
    if (h->aux) hipFree(h->aux);
    for (int i = 0; i < 3; i++)
        if (h->ev[i]) hipEventDestroy(h->ev[i]);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

int lio_scan_merge_set_transform(lio_scan_merge* h, const double T[16]) {
    if (!h || !T) return LIO_E_INVALID;
    for (int i = 0; i < 16; i++) h->T[i] = T[i];
    return LIO_OK;
}

int lio_scan_merge_run_host(lio_scan_merge* h, uint32_t n_clouds, const float* const* xyzi, const uint32_t* const* stamps, const uint32_t* n_points,
                            const uint64_t* header_us, uint64_t scan_period_us, uint32_t* kept, uint32_t* early, uint32_t* late, uint64_t* n_out) {
    if (!h || !xyzi || !stamps || !n_points || !header_us) return LIO_E_INVALID;
    if (n_clouds < 1 || n_clouds > h->max_clouds) {
        set_error("lio_scan_merge_run_host: %u clouds, the handle takes 1 .. %u", n_clouds, h->max_clouds);
        return LIO_E_INVALID;
    }
    if (scan_period_us > 0xFFFFFFFFull) {
        set_error("lio_scan_merge_run_host: a scan period of %llu us does not fit a point's 32-bit stamp", (unsigned long long)scan_period_us);
        return LIO_E_INVALID;
    }
    uint64_t n = 0;
    for (uint32_t l = 0; l < n_clouds; l++) {
        if (n_points[l] && (!xyzi[l] || !stamps[l])) return LIO_E_INVALID;
        n += n_points[l];
    }
    if (n > h->max_points) {
        set_error("lio_scan_merge_run_host: %llu points, the handle holds %llu", (unsigned long long)n, (unsigned long long)h->max_points);
        return LIO_E_CAPACITY;
    }
    hipSetDevice(h->device);
    MergeArgs a;
    for (int i = 0; i < 12; i++) a.x.m[i] = h->T[i];
    a.x.zmin = a.x.zmax = 0.0;
    a.x.scale = 1.0f;
    a.x.band = 0;
    a.period = (double)scan_period_us;
    a.n = (uint32_t)n;
    uint64_t at = 0;
    LIO_HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    for (uint32_t l = 0; l < kMaxClouds; l++) {
        a.start[l] = l < n_clouds ? (uint32_t)at : 0xFFFFFFFFu;
        a.shift[l] = l < n_clouds ? (double)header_us[l] - (double)header_us[0] : 0.0;
        if (l < n_clouds && n_points[l]) {
            LIO_HIP_TRY(hipMemcpyAsync(h->in + at, xyzi[l], (uint64_t)n_points[l] * sizeof(float4), hipMemcpyHostToDevice, h->stream));
            LIO_HIP_TRY(hipMemcpyAsync(h->in_stamps + at, stamps[l], (uint64_t)n_points[l] * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
            at += n_points[l];
        }
    }
    uint32_t tally[3 * kMaxClouds] = {};
    uint32_t total = 0;
    LIO_HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    if (n > 0) {
        const uint32_t ntiles = tiles_of(n);
        uint32_t* stats = h->aux + h->aux_words;
        LIO_HIP_TRY(hipMemsetAsync(stats, 0, sizeof(tally), h->stream));
        sm_count<<<dim3(ntiles), dim3(kThreads), 0, h->stream>>>(h->in_stamps, a, h->aux, stats);
        const uint32_t* d_total = compact_finish(h->stream, h->aux, n);
        if (!d_total) return LIO_E_DEVICE;
        sm_write<<<dim3(ntiles), dim3(kThreads), 0, h->stream>>>(h->in, h->in_stamps, a, h->aux, h->out, h->out_stamps);
        LIO_HIP_TRY(hipGetLastError());
        LIO_HIP_TRY(hipMemcpyAsync(&total, d_total, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        LIO_HIP_TRY(hipMemcpyAsync(tally, stats, sizeof(tally), hipMemcpyDeviceToHost, h->stream));
    }
    LIO_HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    LIO_HIP_TRY(hipStreamSynchronize(h->stream));
    h->upload_us = elapsed_us(h->ev[0], h->ev[1]);
    h->merge_us = elapsed_us(h->ev[1], h->ev[2]);
    h->n_out = total;
    for (uint32_t l = 0; l < n_clouds; l++) {
        if (kept) kept[l] = l == 0 ? n_points[0] : tally[3 * l];
        if (early) early[l] = tally[3 * l + 1];
        if (late) late[l] = tally[3 * l + 2];
    }
    if (n_out) *n_out = total;
    return LIO_OK;
}

int64_t lio_scan_merge_download(lio_scan_merge* h, float* xyzi, uint32_t* stamps, uint64_t cap) {
    if (!h) return LIO_E_INVALID;
    if (h->n_out > cap) return -(int64_t)h->n_out;
    if (h->n_out && (!xyzi || !stamps)) return LIO_E_INVALID;
    const int64_t a = download("lio_scan_merge_download", h->device, h->stream, reinterpret_cast<const float*>(h->out), 4 * h->n_out, xyzi, 4 * cap);
    if (a < 0) return a;
    const int64_t b = download("lio_scan_merge_download", h->device, h->stream, h->out_stamps, h->n_out, stamps, cap);
    return b < 0 ? b : (int64_t)h->n_out;
}

const void* lio_scan_merge_device(lio_scan_merge* h, const uint32_t** d_stamps, uint64_t* n) {
    if (!h) return nullptr;
    if (d_stamps) *d_stamps = h->out_stamps;
    if (n) *n = h->n_out;
    return h->out;
}

int lio_scan_merge_last_times(lio_scan_merge* h, double* upload_us, double* merge_us) {
    if (!h) return LIO_E_INVALID;
    if (upload_us) *upload_us = h->upload_us;
    if (merge_us) *merge_us = h->merge_us;
    return LIO_OK;
}

}  // extern "C"
