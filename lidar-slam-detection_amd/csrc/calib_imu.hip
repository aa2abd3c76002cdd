// calib_imu.hip -- the device half of the lidar-IMU calibration on gfx950 (wave64): the odometry of the reference's CalibLidarImu
// (sensor_driver/calibration/lidar_imu/src/calib_lidar_imu.cpp: get_lidar_T_R:29-75, addLidarData:77-105) with its local map resident in HBM,
// around the host half of calib_imu_host.cpp.  The C entry points and their contract are in include/lio_hip.h (lio_calib_imu_*, ABI 27).
//
//   lidar_pose   upload the rows -> ci_stage (strided rows to float4, the points that are not finite counted: one word comes back)
//                -> cloud::voxel_filter at 0.2 into the source buffer -> first call: the raw scan becomes the map and the target
//                -> later: lio_gicp_set_source_device, lio_gicp_align from the last pose (f32), the result rounded to f32
//   add_frame    ci_stage -> ci_xform (the Matrix4d rule of device_prims.h, f64) into a scratch -> voxel_filter at 0.2 in place -> the
//                filtered frame copied behind the map -> voxel_filter of the WHOLE map out of place into the target staging
//                -> lio_gicp_set_target_device.  The map's length moves only when all of that held.
//
// The filter is cloud.hip's chain (device_prims.h: voxel_filter) over a scratch allocated once for the larger of the two capacities; the
// matcher is one lio_gicp in voxel mode.  Between the upload of the rows and the 16 doubles of the pose no cloud crosses the link; the host
// reads back words: the finite count, the filter's grid and voxel count, the matcher's round records.
#include <cmath>
#include <new>

#include "calib_imu_host.h"
#include "device_prims.h"

namespace lio {
namespace calib_imu {

using namespace prims;

constexpr float kLeaf = 0.2f;  // downer_.setLeafSize(0.2, 0.2, 0.2)

// rows of `stride` floats (x y z intensity first) to float4; *bad += the points whose x, y or z is not finite, one atomic per wave.
// Item r of thread tid is point blockIdx.x * kTile + r * kThreads + tid: a wave's 64 lanes write 1 KiB in a row.
__global__ __launch_bounds__(kThreads) void ci_stage(const float* __restrict__ rows, uint32_t n, uint32_t stride, float4* __restrict__ out,
                                                     uint32_t* __restrict__ bad) {
    const uint32_t base = blockIdx.x * kTile;
    float4 p[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        const float* q = rows + (size_t)(i < n ? i : n - 1u) * stride;
        p[r] = make_float4(q[0], q[1], q[2], q[3]);
    }
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        if (i < n) {
            out[i] = p[r];
            c += finite3(p[r].x, p[r].y, p[r].z) ? 0u : 1u;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(bad, c);
}

// pcl::transformPointCloud(in, out, Matrix4d) into another buffer (the append of cloud.hip writes behind a cloud; here the filter reads the result)
__global__ __launch_bounds__(kThreads) void ci_xform(const float4* __restrict__ in, uint32_t n, XformArgs a, float4* __restrict__ out) {
    const uint32_t base = blockIdx.x * kTile;
    float4 p[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        p[r] = in[i < n ? i : n - 1u];
    }
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        if (i < n) out[i] = xform(p[r], a);
    }
}

}  // namespace calib_imu
}  // namespace lio

using namespace lio;
using namespace lio::calib_imu;

struct lio_calib_imu {
    Host host;
    int device = 0;
    uint32_t max_scan = 0, max_map = 0;
    bool open = false;      // the device half exists
    bool no_rtk = false;    // no_rtk_flag
    bool have_map = false;  // local_map_ != nullptr
    double last_pose[16];
    int max_iterations = 64;
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // stage begin / end = filter begin, filter end = align begin, align end; map update begin / end
    float* rows = nullptr;  // the uploaded rows as they came
    uint64_t rows_cap = 0;
    float4* scan = nullptr;     // the staged frame (max_scan)
    float4* work = nullptr;     // the filtered frame (the source) or the moved key frame (max_scan)
    float4* map = nullptr;      // the local map, append only (max_map)
    float4* target = nullptr;   // the whole map filtered (max_map)
    uint32_t* scratch = nullptr;  // the filter's, for max(max_scan, max_map) points
    uint32_t* bad = nullptr;
    uint32_t map_n = 0, target_n = 0;
    lio_gicp* gicp = nullptr;
    double stage_us = 0, filter_us = 0, align_us = 0, map_us = 0;
};

namespace {

void eye16(double* T) {
    for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

void close_device(lio_calib_imu* h) {
    if (h->stream || h->gicp || h->scan) hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->gicp) lio_gicp_destroy(h->gicp);
    void* bufs[] = {h->rows, h->scan, h->work, h->map, h->target, h->scratch, h->bad};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    for (hipEvent_t& e : h->ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    h->stream = nullptr;
    h->gicp = nullptr;
    h->rows = nullptr; h->scan = h->work = h->map = h->target = nullptr; h->scratch = h->bad = nullptr;
    h->rows_cap = 0;
    h->open = false;
}

// the first call that handles a cloud opens the device: buffers, stream, events, the matcher (FAST_VGICP: 20 neighbours, voxels of 1.0, DIRECT1)
int ensure_device(lio_calib_imu* h) {
    if (h->open) { hipSetDevice(h->device); return LIO_OK; }
    if (!open_device("lio_calib_imu", h->device, &h->stream, h->ev, 6)) return LIO_E_DEVICE;
    const uint64_t big = std::max(h->max_scan, h->max_map);
    lio_loop_params lp;
    lio_loop_default_params(&lp);
    bool ok = alloc(&h->scan, h->max_scan) && alloc(&h->work, h->max_scan) && alloc(&h->map, h->max_map) && alloc(&h->target, h->max_map) &&
              alloc(&h->scratch, cloud::voxel_filter_words(big)) && alloc(&h->bad, 1);
    if (!ok) {
        (void)hipGetLastError();
        set_error("lio_calib_imu: device memory for %u scan and %u map points not available", h->max_scan, h->max_map);
        close_device(h);
        return LIO_E_DEVICE;
    }
    h->gicp = lio_gicp_create(h->device, lp.grid_resolution, (uint32_t)big, lp.k_correspondences);
    if (!h->gicp || lio_gicp_set_voxel_mode(h->gicp, lp.voxel_resolution, 1) != LIO_OK) {
        close_device(h);
        return LIO_E_DEVICE;
    }
    h->open = true;
    return LIO_OK;
}

// the rows to h->scan on the stream; LIO_E_INVALID when a point is not finite (waits for the one word)
int stage_rows(lio_calib_imu* h, const float* rows, uint32_t n, uint32_t stride) {
    const uint64_t words = (uint64_t)n * stride;
    int rc = grow("lio_calib_imu", &h->rows, &h->rows_cap, words, h->stream);
    if (rc != LIO_OK) return rc;
    uint32_t bad = 0;
    LIO_HIP_TRY(hipMemcpyAsync(h->rows, rows, words * sizeof(float), hipMemcpyHostToDevice, h->stream));
    LIO_HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    LIO_HIP_TRY(hipMemsetAsync(h->bad, 0, sizeof(uint32_t), h->stream));
    ci_stage<<<dim3(tiles_of(n)), dim3(kThreads), 0, h->stream>>>(h->rows, n, stride, h->scan, h->bad);
    LIO_HIP_TRY(hipGetLastError());
    LIO_HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    LIO_HIP_TRY(hipMemcpyAsync(&bad, h->bad, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    LIO_HIP_TRY(hipStreamSynchronize(h->stream));
    if (bad) {
        set_error("lio_calib_imu: %u of %u points are not finite", bad, n);
        return LIO_E_INVALID;
    }
    return LIO_OK;
}

int check_rows(const char* who, lio_calib_imu* h, const float* rows, uint32_t n, uint32_t stride) {
    if (!rows || stride < 4) { set_error("%s: rows of at least 4 floats (x y z intensity) are expected", who); return LIO_E_INVALID; }
    if (n > h->max_scan) { set_error("%s: %u points, the handle takes %u per frame", who, n, h->max_scan); return LIO_E_CAPACITY; }
    return LIO_OK;
}

}  // namespace

extern "C" {

lio_calib_imu* lio_calib_imu_create(int device, uint32_t max_scan_points, uint32_t max_map_points) {
    if (device < 0 || max_scan_points == 0 || max_map_points == 0 || max_scan_points > 0x7FFFFFFFu || max_map_points > 0x7FFFFFFFu) {
        set_error("lio_calib_imu_create: bad argument");
        return nullptr;
    }
    lio_calib_imu* h = new (std::nothrow) lio_calib_imu();
    if (!h) return nullptr;
    h->device = device;
    h->max_scan = max_scan_points;
    h->max_map = max_map_points;
    eye16(h->last_pose);
    return h;
}

void lio_calib_imu_destroy(lio_calib_imu* h) {
    if (!h) return;
    close_device(h);
    delete h;
}

// caliber.reset(new CalibLidarImu()): the buffers of the device half are kept, their contents forgotten
int lio_calib_imu_reset(lio_calib_imu* h) {
    if (!h) return LIO_E_INVALID;
    h->host.reset();
    h->no_rtk = false;
    h->have_map = false;
    h->map_n = h->target_n = 0;
    h->max_iterations = 64;
    eye16(h->last_pose);
    h->stage_us = h->filter_us = h->align_us = h->map_us = 0;
    return LIO_OK;
}

int lio_calib_imu_add_imu(lio_calib_imu* h, const double* rows7, uint32_t n) {
    if (!h || (n && !rows7)) return LIO_E_INVALID;
    h->host.add_imu(rows7, n);
    return LIO_OK;
}

int lio_calib_imu_set_max_iterations(lio_calib_imu* h, int max_iterations) {
    if (!h || max_iterations < 1) return LIO_E_INVALID;
    h->max_iterations = max_iterations;
    return LIO_OK;
}

int lio_calib_imu_lidar_pose(lio_calib_imu* h, const float* rows, uint32_t n, uint32_t stride_floats, double out_T[16]) {
    if (!h || !out_T) return LIO_E_INVALID;
    if (n == 0) {  // "no cloud in lidar data"
        h->no_rtk = true;
        eye16(out_T);
        return LIO_OK;
    }
    int rc = check_rows("lio_calib_imu_lidar_pose", h, rows, n, stride_floats);
    if (rc != LIO_OK) return rc;
    if (!h->have_map && n > h->max_map) { set_error("lio_calib_imu_lidar_pose: %u points, the map takes %u", n, h->max_map); return LIO_E_CAPACITY; }
    if ((rc = ensure_device(h)) != LIO_OK) return rc;
    if ((rc = stage_rows(h, rows, n, stride_floats)) != LIO_OK) return rc;
    // downer_.filter(*downed_cloud)
    uint64_t n_ds = 0;
    if ((rc = cloud::voxel_filter(h->stream, h->scan, n, kLeaf, h->work, h->scratch, &n_ds)) != LIO_OK) return rc;
    LIO_HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    LIO_HIP_TRY(hipStreamSynchronize(h->stream));
    h->stage_us = elapsed_us(h->ev[0], h->ev[1]);
    h->filter_us = elapsed_us(h->ev[1], h->ev[2]);
    h->align_us = 0;
    if (!h->have_map) {  // the map and the target are the RAW scan
        if ((rc = lio_gicp_set_target_device(h->gicp, h->scan, n)) != LIO_OK) return rc;
        LIO_HIP_TRY(hipMemcpyAsync(h->map, h->scan, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
        LIO_HIP_TRY(hipStreamSynchronize(h->stream));
        h->map_n = h->target_n = n;
        h->have_map = true;
        h->no_rtk = true;
        eye16(h->last_pose);
        eye16(out_T);
        return LIO_OK;
    }
    if ((rc = lio_gicp_set_source_device(h->gicp, h->work, (uint32_t)n_ds)) != LIO_OK) return rc;
    h->no_rtk = true;
    double guess[16], T[16];
    for (int a = 0; a < 16; a++) guess[a] = (double)(float)h->last_pose[a];  // last_frame_pose_.cast<float>()
    lio_ndt_params p;
    lio_estimate_matcher_params(&p);
    p.max_iterations = h->max_iterations;
    int it = 0, conv = 0;
    if ((rc = lio_gicp_align(h->gicp, guess, &p, 1.0, T, &it, &conv)) != LIO_OK) return rc;
    LIO_HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    LIO_HIP_TRY(hipEventSynchronize(h->ev[3]));
    h->align_us = elapsed_us(h->ev[2], h->ev[3]);
    if (!conv) {  // "register cant converge": I, the last pose stays
        set_warning("lio_calib_imu_lidar_pose: the matcher did not converge in %d iterations", it);
        eye16(out_T);
        return LIO_OK;
    }
    for (int a = 0; a < 16; a++) out_T[a] = h->last_pose[a] = (double)(float)T[a];  // getFinalTransformation() is a Matrix4f
    return LIO_OK;
}

int lio_calib_imu_add_frame(lio_calib_imu* h, uint64_t stamp_us, const float* rows, uint32_t n, uint32_t stride_floats, const double global_T[16],
                            const double delta_T[16]) {
    if (!h || !global_T || !delta_T) return LIO_E_INVALID;
    if (h->host.frames.size() >= kMaxFrames) return LIO_OK;  // calib_wrapper.cpp:142
    if (!h->no_rtk) {  // the RTK path: the frame alone
        h->host.add_frame(stamp_us, global_T, delta_T);
        return LIO_OK;
    }
    if (!h->have_map) { set_error("lio_calib_imu_add_frame: the flag is set and there is no map yet"); return LIO_E_STATE; }
    for (int a = 0; a < 12; a++)
        if (!std::isfinite(global_T[a])) { set_error("lio_calib_imu_add_frame: global_T is not finite"); return LIO_E_INVALID; }
    int rc;
    uint64_t n_key = 0;
    if (n && (rc = check_rows("lio_calib_imu_add_frame", h, rows, n, stride_floats)) != LIO_OK) return rc;
    if ((rc = ensure_device(h)) != LIO_OK) return rc;
    if (n) {
        if ((rc = stage_rows(h, rows, n, stride_floats)) != LIO_OK) return rc;
        LIO_HIP_TRY(hipEventRecord(h->ev[4], h->stream));
        XformArgs a;
        for (int i = 0; i < 12; i++) a.m[i] = global_T[i];
        a.zmin = a.zmax = 0.0;
        a.scale = 1.0f;
        a.band = 0;
        ci_xform<<<dim3(tiles_of(n)), dim3(kThreads), 0, h->stream>>>(h->scan, n, a, h->work);
        LIO_HIP_TRY(hipGetLastError());
        if ((rc = cloud::voxel_filter(h->stream, h->work, n, kLeaf, h->work, h->scratch, &n_key)) != LIO_OK) return rc;
    } else {
        LIO_HIP_TRY(hipEventRecord(h->ev[4], h->stream));
    }
    const uint64_t grown = (uint64_t)h->map_n + n_key;
    if (grown > h->max_map) {
        (void)hipStreamSynchronize(h->stream);
        set_error("lio_calib_imu_add_frame: the map would hold %llu points, the handle takes %u", (unsigned long long)grown, h->max_map);
        return LIO_E_CAPACITY;
    }
    // *local_map_ += *key_lidar_frame behind the map's end; the length moves when the target is set
    if (n_key) LIO_HIP_TRY(hipMemcpyAsync(h->map + h->map_n, h->work, (size_t)n_key * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
    uint64_t n_target = 0;
    if ((rc = cloud::voxel_filter(h->stream, h->map, (uint32_t)grown, kLeaf, h->target, h->scratch, &n_target)) != LIO_OK) return rc;
    LIO_HIP_TRY(hipStreamSynchronize(h->stream));
    if ((rc = lio_gicp_set_target_device(h->gicp, h->target, (uint32_t)n_target)) != LIO_OK) return rc;
    LIO_HIP_TRY(hipEventRecord(h->ev[5], h->stream));
    LIO_HIP_TRY(hipEventSynchronize(h->ev[5]));
    h->map_us = elapsed_us(h->ev[4], h->ev[5]);
    h->map_n = (uint32_t)grown;
    h->target_n = (uint32_t)n_target;
    h->host.add_frame(stamp_us, global_T, delta_T);
    return LIO_OK;
}

int lio_calib_imu_calibrate(lio_calib_imu* h, double R[9]) {
    if (!h || !R) return LIO_E_INVALID;
    double out[9];
    const int rc = h->host.calibrate(out);
    if (rc != LIO_OK) {
        set_error("lio_calib_imu_calibrate: no IMU sample, or no frame stamped at or after the first one");
        return rc;
    }
    memcpy(R, out, sizeof(out));
    return LIO_OK;
}

int64_t lio_calib_imu_lidar_poses(lio_calib_imu* h, double* out, uint64_t cap) {
    if (!h) return LIO_E_INVALID;
    const uint64_t n = h->host.n_poses();
    if (n > cap) return -(int64_t)n;
    if (n && !out) return LIO_E_INVALID;
    h->host.lidar_poses(out);
    return (int64_t)n;
}

int64_t lio_calib_imu_imu_poses(lio_calib_imu* h, double* out, uint64_t cap) {
    if (!h) return LIO_E_INVALID;
    const uint64_t n = h->host.n_poses();
    if (n > cap) return -(int64_t)n;
    if (n && !out) return LIO_E_INVALID;
    h->host.imu_poses(out);
    return (int64_t)n;
}

int64_t lio_calib_imu_map_download(lio_calib_imu* h, float* xyzi, uint64_t cap) {
    if (!h) return LIO_E_INVALID;
    if (!h->open || !h->have_map) return 0;
    return download("lio_calib_imu_map_download", h->device, h->stream, reinterpret_cast<const float*>(h->map), 4ull * h->map_n, xyzi, 4 * cap) / 4;
}

int64_t lio_calib_imu_target_download(lio_calib_imu* h, float* xyzi, uint64_t cap) {
    if (!h) return LIO_E_INVALID;
    if (!h->open || !h->have_map) return 0;
    if (h->target_n > cap) return -(int64_t)h->target_n;
    if (!xyzi) return LIO_E_INVALID;
    const int rc = lio_gicp_download(h->gicp, 0, xyzi, nullptr, (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFFFull));
    return rc;
}

int lio_calib_imu_counts(lio_calib_imu* h, uint32_t* frames, uint32_t* imus, uint32_t* aligned, uint32_t* map_points, uint32_t* target_points, int* no_rtk) {
    if (!h) return LIO_E_INVALID;
    if (frames) *frames = (uint32_t)h->host.frames.size();
    if (imus) *imus = (uint32_t)h->host.imu_stamp.size();
    if (aligned) *aligned = (uint32_t)h->host.aligned.size();
    if (map_points) *map_points = h->have_map ? h->map_n : 0u;
    if (target_points) *target_points = h->have_map ? h->target_n : 0u;
    if (no_rtk) *no_rtk = h->no_rtk ? 1 : 0;
    return LIO_OK;
}

int lio_calib_imu_last_times(lio_calib_imu* h, double* stage_us, double* filter_us, double* align_us, double* map_update_us) {
    if (!h) return LIO_E_INVALID;
    if (stage_us) *stage_us = h->stage_us;
    if (filter_us) *filter_us = h->filter_us;
    if (align_us) *align_us = h->align_us;
    if (map_update_us) *map_update_us = h->map_us;
    return LIO_OK;
}

}  // extern "C"
