// slam_wrapper.cpp -- the reference's OUTER boundary: the pybind11 module `slam_wrapper` that slam/slam.py and slam/map_manager.py
// import (/root/reference/slam/src/slam_wrapper.cpp:192-324: same function names, argument names and order, return types), in C++
// over the C ABI of liblio_hip.so.
//
// On the hot path (mapping mode, FastLIO): init_slam / set_ins_external_param / set_imu_external_param / setup_slam / process /
// deinit_slam do what the reference does between Python and the filter --
//   numpy_to_imu            slam/src/py_utils.cpp:244-258   deg/s -> rad/s, g -> m/s^2, us -> s
//   pydict_to_cloud         slam/src/py_utils.cpp:149-181   N x 4 f32 + N x 2 attr (col 0 = per-point offset in us)
//   preprocessPoints        slam/common/slam_base.h:83-85   lidar -> INS static transform (pcl::transformPointCloud with a Matrix4d)
//   HDL_FastLIO::init / setSensors / feedImuData / feedPointData / runLio / getPose   slam/mapping/fastlio/src/fastlio.cpp:119-277
//   SLAM::run               slam/src/slam.cpp:273-367       pose fields, heading / pitch / roll from the odometry
// -- except that the cloud goes numpy -> pinned staging buffer -> HBM in ONE pass (lio_fastlio_pcl_stage / _commit): the static
// transform and the stamp conversion are applied while copying, the 48-byte PointXYZINormal inflation and the two intermediate
// PCL clouds of the reference never exist.
// The dense-map export (set_export_map_config / export_points / dump_map_points, accumulate_cloud / save_accumulate_cloud,
// save_undistortion_cloud: graph_utils.cpp:160-200, 384-446) runs on the device over lio_cloud_* (csrc/cloud.hip), texture_mesh
// (graph_utils.cpp:449-501) over lio_knn_index_* (csrc/knn_index.hip).
// The GNSS side of mapping mode (SLAM::run's GNSS lines, HDL_FastLIO::setOrigin / feedInsData, the method RTKM: slam.cpp:280-292,
// fastlio.cpp:177-188, slam/mapping/rtkm/src/rtkm.cpp) runs over lio_utm_* / lio_rtk_track_* / lio_gnss_queue_* (csrc/geodesy.cpp, host) and
// lio_scan_merge_* (csrc/scanmerge.hip): set_gnss, init_slam(method = "RTKM").
// Off the hot path (what SURVEY.md section 2 and Appendix B leave out): type-correct minimal implementations -- empty dict / list,
// identity 4 x 4, stored-and-returned settings -- so that slam.py and map_manager.py run unchanged.  They are listed in INTEGRATION.md.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <charconv>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <initializer_list>
#include <iomanip>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/lio_hip.h"

namespace py = pybind11;

namespace {

constexpr double kAng2Rad = 0.01745329251994;  // the reference's truncated constant (slam/common/slam_utils.cpp:88)

struct Mat4 {
    double m[16];
    static Mat4 identity() {
        Mat4 r;
        for (int i = 0; i < 16; i++) r.m[i] = (i % 5 == 0) ? 1.0 : 0.0;
        return r;
    }
    double& operator()(int r, int c) { return m[r * 4 + c]; }
    double operator()(int r, int c) const { return m[r * 4 + c]; }
};
Mat4 mul(const Mat4& a, const Mat4& b) {
    Mat4 r;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += a(i, k) * b(k, j);
            r(i, j) = s;
        }
    return r;
}
Mat4 rigid_inverse(const Mat4& a) {  // [R t; 0 1]^-1 = [R^T  -R^T t; 0 1]
    Mat4 r = Mat4::identity();
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r(i, j) = a(j, i);
    for (int i = 0; i < 3; i++) r(i, 3) = -(r(i, 0) * a(0, 3) + r(i, 1) * a(1, 3) + r(i, 2) * a(2, 3));
    return r;
}
// getTransformFromRPYT (slam_utils.cpp:89-96): translation * Rz(yaw) * Rx(pitch) * Ry(roll), angles in degrees (the library's: csrc/geodesy.cpp)
Mat4 transform_from_rpyt(double x, double y, double z, double yaw, double pitch, double roll) {
    Mat4 T;
    lio_transform_from_rpyt(x, y, z, yaw, pitch, roll, T.m);
    return T;
}
// getRPYTfromTransformFrom (slam_utils.cpp:98-110): Eigen's MatrixBase::eulerAngles(2, 0, 1) of the rotation block (Geometry/EulerAngles.h,
// the Tait-Bryan branch with a0 = 2, a1 = 0, a2 = 1: even permutation, i = 2, j = 0, k = 1, result negated), in degrees
void rpy_from_transform(const Mat4& T, double& yaw, double& pitch, double& roll) {
    const int i = 2, j = 0, k = 1;
    double r0 = std::atan2(T(j, k), T(k, k));
    const double c2 = std::sqrt(T(i, i) * T(i, i) + T(i, j) * T(i, j));
    double r1;
    if (r0 > 0.0) {  // (!odd && res[0] > 0)
        r0 -= M_PI;
        r1 = std::atan2(-T(i, k), -c2);
    } else {
        r1 = std::atan2(-T(i, k), c2);
    }
    const double s1 = std::sin(r0), c1 = std::cos(r0);
    const double r2 = std::atan2(s1 * T(k, i) - c1 * T(j, i), c1 * T(j, j) - s1 * T(k, j));
    yaw = -r0 / kAng2Rad;
    pitch = -r1 / kAng2Rad;
    roll = -r2 / kAng2Rad;
}

// ---- localisation mode (slam/localization): the state of Locate::Localization + the hdl_localization nodelet, over the C ABI ----
struct KeyFrameDisk {  // one directory of <map>/graph: `data` (KeyFrame::save, slam/common/keyframe.cpp:118-133) + `cloud.pcd`
    uint64_t stamp = 0;
    int id = 0;
    Mat4 odom = Mat4::identity();
    std::vector<float> xyzi;   // in the map frame (KeyFrame::mTransfromPoints)
    std::vector<float> local;  // as stored (KeyFrame::mPoints): what get_graph_map hands to map_manager.py
};
struct Loc {
    std::vector<KeyFrameDisk> frames;
    lio_localmap* lm = nullptr;
    lio_ndt* ndt = nullptr;
    lio_scan* scan = nullptr;
    lio_pose_estimator* pe = nullptr;
    lio_ndt_params par;
    double resolution = 0.2, key_frame_distance = 1.0;
    bool have_init_pose = false, initialized = false, have_map = false;
    Mat4 init_pose = Mat4::identity(), last_odom = Mat4::identity();
    uint64_t init_stamp = 0;
    int age = 0, failures = 0;          // mLocalizationAge / mFailureCounter (localization.cpp:235-275)
    std::deque<std::pair<uint64_t, Mat4>> pose_data;  // HdlLocalizationNodelet::pose_data (<= 10)
    struct Imu { double stamp; float acc[3], gyr[3]; };
    std::vector<Imu> imu_data;
    std::vector<uint32_t> stamps;
    std::vector<float> staged;
    // merge_map: the merged pose graph as a host record (key-frame ids; read from the loaded map's graph.g2o by the first merge, extended by every
    // merge that succeeds -- the device graph is built from it for the length of a call), the bank of both maps' key frames and the overlap
    // detector over it; key-frame id -> bank frame
    struct MergeEdge { int a, b, kernel; double M[16], info[36]; };
    std::vector<MergeEdge> medges;
    // under set_gnss the GNSS priors of both maps' graph.g2o (EDGE_SE3_PRIORXYZ / _PRIORQUAT with their kernels) belong to the record too
    struct MergePrior { int kf, type, kernel; double m[4], info[9], delta; };
    std::vector<MergePrior> mpriors;
    std::set<int> mfixed;
    bool have_mgraph = false;
    lio_loop* mbank = nullptr;
    lio_overlap* moverlap = nullptr;
    std::map<int, int> bank_of_kf;
    uint32_t bank_max_points = 0, ndt_biggest = 0;
    struct MergeReport { std::vector<std::array<int, 2>> overlaps; std::vector<double> scores; std::vector<int> reasons, new_ids; int fragments = 0, skipped_tags = 0, priors = 0;
                         bool origin_updated = false; } merge_report;
    // global relocalisation (GlobalLocalization::globalSearch + registrationAlign, global_localization.cpp:387-413, 456-482): off unless
    // set_global_localization(true) / LSD_AMD_RELOC=1.  The bank holds the descriptors of the key frames' local clouds, frame k = key frame k
    bool reloc = false;
    lio_sc* sc = nullptr;
    lio_gicp* reloc_gicp = nullptr;
    std::vector<float> reloc_ds;
    struct Reloc { bool searched = false, accepted = false, local = false; int match_id = -1, converged = 0, n_examined = 0; double score = 0, fitness = 0, dx = 0, da = 0;
                   float yaw = 0; Mat4 guess = Mat4::identity(); } last_reloc;
    int reloc_searches = 0;  // searches run since init_slam
    // GNSS in localisation mode (set_gnss; Localization::feedInsData, localization.cpp:199-209): a valid fix of a map with an origin, with its pose
    // T = computeRTKTransform(projector, fix, zero_utm).  Not initialised: the latest one, which the next search consumes (runSearchPose drains its
    // queue and keeps the newest, global_localization.cpp:288-296).  Initialised: the localiser's ins_data (ins_callback: at most 10, the oldest
    // leaves first) and what the bracket rule made of it for the last located frame
    struct Ins { lio_rtk_fix f = lio_rtk_fix(); Mat4 T = Mat4::identity(); };
    bool have_latest_ins = false;
    Ins latest_ins;
    std::deque<Ins> ins_data;
    struct GpsUse { bool used = false; Mat4 T = Mat4::identity(); double precision = 0, ratio = 0; int dimension = 0; } last_gps;
    double sc_dist_thres = 0.30;  // 0.25 under set_gnss (the sensor-fusion configuration, global_localization.cpp:25-35)
    // the operator's hint (GlobalLocalization::getEstimatePose / setInitPose's mLastFrame / initializePose's pose * delta).  The last frame is
    // the downsampled cloud in `scan` (have_last_frame: the scan holds the reduced cloud of the most recent non-empty frame); an accepted hint
    // keeps its pose and a device copy of that frame (slot 1 of the local map) until the next non-empty frame hands over to the filter
    lio_gicp* est_gicp = nullptr;
    bool have_last_frame = false, est_pending = false;
    Mat4 est_pose = Mat4::identity();
    struct Est { bool called = false, handover = false, delta_ran = false; int rc = 0, delta_converged = 0, delta_iterations = 0; lio_estimate_report rep = lio_estimate_report();
                 Mat4 hint = Mat4::identity(), out = Mat4::identity(), delta = Mat4::identity(); } last_est;
    ~Loc() {
        if (est_gicp) lio_gicp_destroy(est_gicp);
        if (reloc_gicp) lio_gicp_destroy(reloc_gicp);
        if (sc) lio_sc_destroy(sc);
        if (moverlap) lio_overlap_destroy(moverlap);
        if (mbank) lio_loop_destroy(mbank);
        if (pe) lio_pose_estimator_destroy(pe);
        if (lm) lio_localmap_destroy(lm);
        if (ndt) lio_ndt_destroy(ndt);
        if (scan) lio_scan_destroy(scan);
    }
};

struct Slam {
    std::unique_ptr<Loc> loc;
    std::string map_path;
    std::string mode, method;
    std::vector<std::string> sensors;
    std::string lidar;
    bool use_imu = false, use_gps = false;
    Mat4 T_static = Mat4::identity();      // lidar -> INS   (set_ins_external_param)
    Mat4 T_imu = Mat4::identity();         // IMU extrinsic  (set_imu_external_param)
    Mat4 T_imu_ins = Mat4::identity(), T_imu_ins_inv = Mat4::identity();
    double scan_period = 0.1;
    lio_engine* engine = nullptr;
    // HDL_FastLIO::runLio + mOdomQueue
    std::thread lio_thread;
    std::atomic<bool> running{false};
    std::mutex mtx;
    std::condition_variable cv;
    std::deque<std::pair<Mat4, Mat4>> odom_queue;
    // settings the off-path calls store and return
    double origin[6] = {0, 0, 0, 0, 0, 0};
    bool origin_set = false;
    bool ground_constraint = false, loop_closure = false, gravity_constraint = false, colouration = false;
    // SLAM::setInsConfig / preprocessInsData (slam.cpp:196-268): the GNSS status configurations in priority order, the state of the status filter
    struct InsCfg { std::string name; int status = 0, priority = -1; double stable_time = 0, precision = 0; };
    std::vector<InsCfg> ins_cfg;
    int last_ins_priority = -1;
    double last_ins_timestamp = 0;
    double init_pose[6] = {0, 0, 0, 0, 0, 0};
    std::string dest;
    int dest_port = 0;
    uint64_t max_points = 8000000, max_voxels = 1u << 21;
    // key-frame output (SLAM::setParams, slam.cpp:96-108): off unless set_keyframe_output(true) / LSD_AMD_KEYFRAMES=1
    double resolution = 0.2, key_frame_distance = 1.0, key_frame_degree = 10.0, key_frame_range = 50.0;
    bool keyframe_output = false;
    lio_keyframer* keyframer = nullptr;
    std::mutex kf_mtx;
    std::vector<float> kf_points;       // the T_static-transformed cloud and stamps of the frame in flight
    std::vector<uint32_t> kf_stamps;
    Mat4 last_odom_start = Mat4::identity(), last_odom_end = Mat4::identity();  // the odometry pair of the last process() call
    // loop detection over the key frames update_odom() hands out (hdl_graph_slam::LoopDetector, lio_loop_*): off unless
    // set_loop_detection(true) / LSD_AMD_LOOP=1; guarded by kf_mtx
    bool loop_detection = false;
    lio_loop* loop = nullptr;
    lio_loop_params loop_par;
    std::atomic<bool> loop_detected{false};  // graph_loop_detected: sticky; read by get_graph_status() without the mutex
    std::vector<lio_loop_edge> loop_edges;
    // the pose graph over the key frames (hdl_graph_slam_nodelet.cpp:293-334, 600-651; lio_graph_*): off unless set_pose_graph(true) /
    // LSD_AMD_GRAPH=1; guarded by kf_mtx.  Key frame k is node k of the graph and frame k of the detector's bank.
    bool pose_graph = false;
    lio_graph* graph = nullptr;
    std::vector<Mat4> graph_odom;         // keyframe->odom of every key frame in the graph
    std::vector<Mat4> graph_pose;         // keyframe->node->estimate() after the last optimisation
    Mat4 odom2map = Mat4::identity();     // trans_odom2map (the values of a Matrix4f)
    bool graph_updated = false;
    size_t graph_loops = 0;               // loop edges of loop_edges already in the graph
    // the graph's priors (flush_floor_queue, flush_gps_queue: hdl_graph_slam_nodelet.cpp:358-460, 536-594); guarded by kf_mtx
    bool fix_first_node = true;           // the reference's flag: the first floor or GNSS edge releases node 0
    lio_ground* floor_ground = nullptr;   // the floor detector of the key frames (a handle of its own: update_odom runs without the GIL)
    bool floor_plane = false;             // floor_plane_node exists
    double floor_world[4] = {0, 0, 1, 0}; // its (fixed) estimate
    double floor_last_distance = 0;       // floor_last_update_distance
    double gnss_last[3] = {0, 0, 0};      // gps_last_update_pose
    std::vector<uint8_t> graph_has_gnss;  // keyframe->utm_coord is set
    std::vector<uint8_t> graph_gone;      // del_graph_vertex took the key frame out (its node is removed, its bank frame retired; ids stay)
    // every key frame the bank took, by bank id (= node id with a graph): what get_graph_map needs beside the bank's cloud; guarded by kf_mtx
    std::vector<uint64_t> bank_stamp;
    std::vector<Mat4> bank_odom;
    // HDL_FastLIO::mOdometrys (fastlio.cpp:242-250) in mapping mode, MapLoader::mOdometrys (map_loader.cpp:223-253, 141-142) in localisation mode:
    // what dump_odometry writes; guarded by mtx
    std::vector<std::pair<uint64_t, Mat4>> odometrys;
    struct InjectedKeyFrame { std::vector<float> pts; Mat4 pose; uint64_t stamp; double accum; };
    std::deque<InjectedKeyFrame> injected;  // test visibility: key frames handed to update_odom() without the front end (_push_keyframe)
    // the colour map of the localisation mode (MapLoader::mRender, map_render.cpp; lio_render_*): cameras from set_camera_param, switched by
    // set_map_colouration, painted by process() after a stable localisation; guarded by mtx
    struct CamCfg { std::string name; double K[4]; Mat4 ext; };
    std::vector<CamCfg> cameras;
    lio_render* painter = nullptr;
    bool painter_stale = true;            // the cameras or the static transform changed since the painter got them
    uint32_t colour_seed = 0;             // of the ground test's draws (lio_ground)
    // the GNSS side of mapping mode (SLAM::run, slam.cpp:280-292; HDL_FastLIO::setOrigin / feedInsData, fastlio.cpp:177-188): off unless
    // set_gnss(true) / LSD_AMD_GNSS=1.  On: the first valid fix sets the map origin, every valid fix goes to the graph's GNSS queue, and
    // update_odom() flushes the queue against the graph's key frames into priors.  The queue is guarded by kf_mtx
    bool gnss = false;
    // the GNSS moment stage of run_robust_graph_optimization("mapping") (hdl_graph_slam_nodelet.cpp:1037-1081): off unless set_gnss_moment(true) /
    // LSD_AMD_GNSS_MOMENT=1.  What the last stage found, for _last_gnss_moment(); guarded by kf_mtx
    bool gnss_moment = false, moment_ran = false;
    double moment_last[3] = {0, 0, 0};
    int moment_priors = 0;
    lio_graph_report moment_report{};
    int ins_dim = 2;                      // SLAM::mInsDim (set_ins_config's ins_type)
    lio_gnss_queue* gnss_queue = nullptr;
    // method = "RTKM" (slam/mapping/rtkm/src/rtkm.cpp): poses straight from the RTK track, the lidars merged into one frame on the device;
    // no FastLIO engine.  Guarded by mtx
    bool rtkm = false, rtkm_ready = false;
    lio_rtk_track* track = nullptr;
    lio_scan_merge* merger = nullptr;
    uint64_t merger_cap = 0;
    Mat4 rtkm_last_odom = Mat4::identity();  // mLastOdom
    std::vector<float> merged_pts;           // the last merged frame (INS frame) and its stamps
    std::vector<uint32_t> merged_stamps;
    // localisation mode: SLAM::mProjector and mZeroUtm (slam.cpp:159-166) of a loaded map that has an origin
    lio_utm* utm = nullptr;
    bool have_zero_utm = false;
    double zero_utm[3] = {0, 0, 0};
};
std::unique_ptr<Slam> g;  // one global instance per process, like the reference's slam_ptr (slam_wrapper.cpp:4)

void require(bool ok, const char* what) {
    if (!ok) throw std::runtime_error(std::string("slam_wrapper: ") + what + (lio_last_error()[0] ? std::string(": ") + lio_last_error() : std::string()));
}

// ---- the GNSS side shared by both mapping methods ---------------------------------------------------------------------------------------------
// pydict_to_rtk (py_utils.cpp:214-242), as far as the GNSS side reads it; a missing key is 0 (the reference throws)
struct Fix {
    lio_rtk_fix f = lio_rtk_fix();
    int status = 0;
    bool has_stamp = false;
    std::string sensor;
};
Fix fix_of(py::dict& rtk_dict) {
    Fix x;
    auto num = [&](const char* k) { return rtk_dict.contains(k) ? py::cast<double>(rtk_dict[k]) : 0.0; };
    x.f.latitude = num("latitude"); x.f.longitude = num("longitude"); x.f.altitude = num("altitude");
    x.f.heading = num("heading"); x.f.pitch = num("pitch"); x.f.roll = num("roll");
    x.f.dimension = 2; x.f.precision = 100.0;  // RTKType's defaults (mapping_types.h:107-108)
    if (rtk_dict.contains("Status")) x.status = py::cast<int>(rtk_dict["Status"]);
    if (rtk_dict.contains("timestamp")) { x.f.stamp_us = py::cast<uint64_t>(rtk_dict["timestamp"]); x.has_stamp = true; }
    if (rtk_dict.contains("Sensor")) x.sensor = py::cast<std::string>(rtk_dict["Sensor"]);
    return x;
}
// SLAM::preprocessInsData (slam.cpp:194-271): the validity filter; a valid fix leaves with the configured dimension and its status' precision
bool preprocess_ins(Slam* s, uint64_t timestamp, Fix& x) {
    if (x.status == 0 && std::fabs(x.f.longitude) < 1e-4 && std::fabs(x.f.latitude) < 1e-4) {
        const double lost = timestamp / 1000000.0 - s->last_ins_timestamp;
        if (s->last_ins_priority != -1 && lost >= 1.0) s->last_ins_priority = -1;
        return false;
    }
    if (s->rtkm) return true;  // "don't check the status when doing RTK Mapping"
    const Slam::InsCfg* match = nullptr;
    for (const auto& c : s->ins_cfg) if (c.status == x.status) { match = &c; break; }
    if (!match) for (const auto& c : s->ins_cfg) if (c.status == -1) { match = &c; break; }
    const int mp = match ? match->priority : -1;
    const double now = x.f.stamp_us / 1000000.0;
    int priority = -1;
    if (mp == s->last_ins_priority) { priority = mp; s->last_ins_timestamp = now; }
    else if (mp < s->last_ins_priority) { priority = mp; s->last_ins_priority = mp; s->last_ins_timestamp = now; }
    else {
        const double keep = now - s->last_ins_timestamp;
        if (keep >= match->stable_time) { priority = mp; s->last_ins_priority = mp; s->last_ins_timestamp = now; }
        else priority = s->last_ins_priority;
    }
    if (priority < 0) return false;
    x.f.dimension = s->ins_dim;
    for (const auto& c : s->ins_cfg) if (c.priority == priority) x.f.precision = c.precision;
    return true;
}
// SLAM::setOrigin -> mSlam->setOrigin (HDL_FastLIO::setOrigin, fastlio.cpp:177-183: graph_set_origin; RTKM::setOrigin, rtkm.cpp:37-54): the
// first one wins, whether it comes from a fix or from set_map_origin.  Called with the GIL held and no mutex
void slam_set_origin(Slam* s, const lio_rtk_fix& f) {
    if (s->origin_set) return;
    const double v[6] = {f.latitude, f.longitude, f.altitude, f.heading, f.pitch, f.roll};
    std::memcpy(s->origin, v, sizeof(v));
    s->origin_set = true;
    if (s->rtkm) {
        std::lock_guard<std::mutex> lk(s->mtx);
        if (!s->track) s->track = lio_rtk_track_create();
        require(lio_rtk_track_set_origin(s->track, &f, s->rtkm_last_odom.m) >= 0, "set origin: lio_rtk_track_set_origin failed");
    } else if (s->gnss && !s->loc) {
        py::gil_scoped_release rel;
        std::lock_guard<std::mutex> kl(s->kf_mtx);
        if (!s->gnss_queue) s->gnss_queue = lio_gnss_queue_create();
        // set_origin (hdl_graph_slam_nodelet.cpp:141-156): the altitude less the z of the last key frame's estimate
        int last = (int)s->graph_pose.size() - 1;
        while (last >= 0 && s->graph_gone[(size_t)last]) last--;
        require(lio_gnss_queue_set_origin(s->gnss_queue, &f, last >= 0, last >= 0 ? s->graph_pose[(size_t)last](2, 3) : 0.0, nullptr) == LIO_OK,
                "set origin: lio_gnss_queue_set_origin failed");
    }
}
// SLAM::run's GNSS lines (slam.cpp:280-292) for one fix: the validity filter, the origin, feedInsData of the method.  With the switch off and
// FastLIO only the filter runs (as before); its answer goes back to the caller for the velocity hand-over
bool feed_gnss(Slam* s, uint64_t timestamp, Fix& x) {
    const bool valid = preprocess_ins(s, timestamp, x);
    if (!s->rtkm && !s->gnss) return valid;
    if (valid && !s->origin_set) slam_set_origin(s, x.f);
    if (s->rtkm) {  // RTKM::feedInsData (rtkm.cpp:91-95); nothing goes to the graph's queue
        std::lock_guard<std::mutex> lk(s->mtx);
        if (!s->track) s->track = lio_rtk_track_create();
        require(lio_rtk_track_feed(s->track, valid ? 1 : 0, &x.f) >= 0, "lio_rtk_track_feed failed");
    } else if (valid) {  // enqueue_graph_gps (hdl_graph_slam_nodelet.cpp:800-804)
        py::gil_scoped_release rel;
        std::lock_guard<std::mutex> kl(s->kf_mtx);
        if (!s->gnss_queue) s->gnss_queue = lio_gnss_queue_create();
        require(lio_gnss_queue_push(s->gnss_queue, &x.f) == LIO_OK, "lio_gnss_queue_push failed");
    }
    return valid;
}


// ---- the map on disk: <map>/graph/<n>/{data, cloud.pcd} as KeyFrame::save writes them (slam/common/keyframe.cpp:118-133; the cloud through
// pcl::io::savePCDFileBinary for PointXYZI: FIELDS x y z intensity, 16 bytes per point) -------------------------------------------------
bool write_pcd_binary(const std::string& path, const float* xyzi, size_t n) {
    std::ofstream f(path, std::ios::binary);
    if (!f) return false;
    f << "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH " << n
      << "\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS " << n << "\nDATA binary\n";
    f.write(reinterpret_cast<const char*>(xyzi), (std::streamsize)(n * 16));
    return (bool)f;
}
// reads the x, y, z, intensity fields of an ascii or binary PCD (any field order / extra fields of 4-byte scalars)
bool read_pcd(const std::string& path, std::vector<float>& xyzi) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::vector<std::string> fields;
    std::vector<int> sizes, counts;
    size_t points = 0;
    std::string data_kind, line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ls(line);
        std::string key;
        ls >> key;
        if (key == "FIELDS") { std::string v; while (ls >> v) fields.push_back(v); }
        else if (key == "SIZE") { int v; while (ls >> v) sizes.push_back(v); }
        else if (key == "COUNT") { int v; while (ls >> v) counts.push_back(v); }
        else if (key == "POINTS") ls >> points;
        else if (key == "DATA") { ls >> data_kind; break; }
    }
    if (fields.empty() || sizes.size() != fields.size()) return false;
    if (counts.empty()) counts.assign(fields.size(), 1);
    int off[4] = {-1, -1, -1, -1}, stride = 0, col[4] = {-1, -1, -1, -1}, ncol = 0;
    for (size_t i = 0; i < fields.size(); i++) {
        const int k = fields[i] == "x" ? 0 : fields[i] == "y" ? 1 : fields[i] == "z" ? 2 : fields[i] == "intensity" ? 3 : -1;
        if (k >= 0) { if (sizes[i] != 4) return false; off[k] = stride; col[k] = ncol; }
        stride += sizes[i] * counts[i];
        ncol += counts[i];
    }
    if (off[0] < 0 || off[1] < 0 || off[2] < 0) return false;
    xyzi.assign(points * 4, 0.f);
    if (data_kind == "binary") {
        std::vector<char> rec(stride);
        for (size_t i = 0; i < points; i++) {
            if (!f.read(rec.data(), stride)) return false;
            for (int k = 0; k < 4; k++)
                if (off[k] >= 0) std::memcpy(&xyzi[4 * i + k], rec.data() + off[k], 4);
        }
    } else if (data_kind == "ascii") {
        std::vector<double> row(ncol);
        for (size_t i = 0; i < points; i++) {
            for (int c = 0; c < ncol; c++) if (!(f >> row[c])) return false;
            for (int k = 0; k < 4; k++) if (col[k] >= 0) xyzi[4 * i + k] = (float)row[col[k]];
        }
    } else {
        return false;  // (binary_compressed: not written by the reference)
    }
    return true;
}
bool write_keyframe_data(const std::string& dir, uint64_t stamp_us, int id, const Mat4& odom) {  // KeyFrame::save (keyframe.cpp:122-132)
    std::ofstream ofs(dir + "/data");
    if (!ofs) return false;
    auto mat = [&](std::ostream& o) {
        for (int r = 0; r < 4; r++) { for (int c = 0; c < 4; c++) o << (c ? " " : "") << odom(r, c); o << "\n"; }  // (Eigen's operator<<: 6 significant digits)
    };
    ofs << "stamp " << stamp_us / 1000000ULL << " " << stamp_us % 1000000ULL * 1000 << std::endl;
    ofs << "estimate" << std::endl; mat(ofs);
    ofs << "odom " << std::endl; mat(ofs);
    ofs << "id " << id << std::endl;
    return (bool)ofs;
}
bool read_keyframe_data(const std::string& dir, KeyFrameDisk& kf) {  // KeyFrame::loadOdom, graph form (keyframe.cpp:41-64)
    std::ifstream ifs(dir + "/data");
    if (!ifs) return false;
    bool have = false;
    while (!ifs.eof()) {
        std::string token;
        ifs >> token;
        if (token == "stamp") { uint64_t sec = 0, nsec = 0; ifs >> sec >> nsec; kf.stamp = sec * 1000000ULL + nsec / 1000ULL; }
        else if (token == "estimate") { for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) ifs >> kf.odom(i, j); have = true; }
        else if (token == "id") ifs >> kf.id;
    }
    return have;
}
// MapLoader::getKeyframeFiles + loadGraphMap (map_loader.cpp:255-300): every sub-directory of <map>/graph holding `data` and `cloud.pcd`, sorted by
// name, then by id; clouds moved into the map frame by their pose (KeyFrame::transformPoints: pcl::transformPointCloud with a Matrix4d)
bool load_keyframes(const std::string& map_path, std::vector<KeyFrameDisk>& out) {
    const std::string graph = map_path + "/graph";
    DIR* d = opendir(graph.c_str());
    if (!d) return false;
    std::vector<std::string> dirs;
    while (dirent* e = readdir(d)) {
        const std::string name = e->d_name;
        if (name == "." || name == "..") continue;
        const std::string p = graph + "/" + name;
        struct stat st;
        if (stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode) && stat((p + "/data").c_str(), &st) == 0 && stat((p + "/cloud.pcd").c_str(), &st) == 0) dirs.push_back(p);
    }
    closedir(d);
    std::sort(dirs.begin(), dirs.end());
    for (const std::string& p : dirs) {
        KeyFrameDisk kf;
        if (!read_keyframe_data(p, kf) || !read_pcd(p + "/cloud.pcd", kf.xyzi)) { out.clear(); return false; }
        kf.local = kf.xyzi;
        const size_t n = kf.xyzi.size() / 4;
        for (size_t i = 0; i < n; i++) {
            const double x = kf.xyzi[4 * i], y = kf.xyzi[4 * i + 1], z = kf.xyzi[4 * i + 2];
            for (int r = 0; r < 3; r++) kf.xyzi[4 * i + r] = (float)(kf.odom(r, 0) * x + kf.odom(r, 1) * y + kf.odom(r, 2) * z + kf.odom(r, 3));
        }
        out.push_back(std::move(kf));
    }
    std::stable_sort(out.begin(), out.end(), [](const KeyFrameDisk& a, const KeyFrameDisk& b) { return a.id < b.id; });
    return !out.empty();
}

// GlobalLocalization::feedInitData -> KeyFrame::computeDescriptor for every key frame (keyframe.cpp:163-168), PoseRange(+-10000): the descriptors
// of the key frames' local clouds into a bank on the device, 64 frames a call; every frame is searched
bool loc_fill_sc(Loc& L) {
    if (L.sc) { lio_sc_destroy(L.sc); L.sc = nullptr; }
    uint32_t biggest = 0;
    for (const KeyFrameDisk& kf : L.frames) biggest = std::max<uint32_t>(biggest, (uint32_t)(kf.local.size() / 4));
    L.sc = lio_sc_create(0, (uint32_t)L.frames.size(), std::max<uint32_t>(biggest, 1u << 20));
    if (!L.sc) return false;
    std::vector<float> buf;
    std::vector<uint64_t> off;
    for (size_t k0 = 0; k0 < L.frames.size(); k0 += 64) {
        const size_t k1 = std::min(L.frames.size(), k0 + 64);
        buf.clear();
        off.assign(1, 0);
        for (size_t k = k0; k < k1; k++) {
            buf.insert(buf.end(), L.frames[k].local.begin(), L.frames[k].local.end());
            off.push_back(buf.size() / 4);
        }
        if (lio_sc_add_frames_host(L.sc, buf.data(), off.data(), (uint32_t)(k1 - k0)) != (int)k0) return false;
    }
    // mGraphKDTree (feedInitData): every key frame's position, for the INS-aided search
    std::vector<float> pos;
    for (const KeyFrameDisk& kf : L.frames) for (int a = 0; a < 3; a++) pos.push_back((float)kf.odom(a, 3));
    return lio_sc_set_positions(L.sc, pos.data(), (uint32_t)L.frames.size()) == LIO_OK;
}

// yaw2matrix (Scancontext.cpp:68-75): cos / sin of the f32 angle
Mat4 yaw_matrix_f32(float y) {
    Mat4 m = Mat4::identity();
    m(0, 0) = (double)std::cos(y); m(0, 1) = (double)-std::sin(y);
    m(1, 0) = (double)std::sin(y); m(1, 1) = (double)std::cos(y);
    return m;
}

// GlobalLocalization::downsample of the cloud in L.staged: the VoxelGrid of the localizer's resolution, into L.scan.  The reduced cloud stays in
// HBM as the last frame (mLastFrame) a hint is matched with
bool loc_reduce_staged(Loc& L, uint32_t n, uint32_t& n_ds) {
    L.have_last_frame = false;
    if (lio_scan_upload(L.scan, L.staged.data(), n) != LIO_OK) return false;
    n_ds = n;
    if (L.resolution >= 0.1) { if (lio_scan_voxel_downsample(L.scan, (float)L.resolution, 1, &n_ds) != LIO_OK) return false; }
    else if (lio_scan_set_ds(L.scan, L.staged.data(), n) != LIO_OK) return false;
    L.have_last_frame = n_ds > 0;
    return true;
}

// GlobalLocalization::globalSearch + registrationAlign with the cloud in L.staged: true when an initial pose was accepted into L.init_pose.
// DEVIATION: synchronous, on every uninitialised frame (the reference's search thread drops the frames that arrive while it is busy and
// registers the next one against the frame it searched with); the image search is not built.  With a fix held (set_gnss) localSearch runs instead
bool loc_relocalize(Loc& L, uint32_t n) {
    Loc::Reloc& r = L.last_reloc;
    r = Loc::Reloc();
    if (!L.sc || n == 0) return false;
    uint32_t n_ds = n;
    if (!loc_reduce_staged(L, n, n_ds)) return false;
    if (L.resolution >= 0.1) {
        L.reloc_ds.resize(4 * (size_t)n_ds);
        if (n_ds && lio_scan_download_ds(L.scan, L.reloc_ds.data(), n_ds) < 0) return false;
    } else {
        L.reloc_ds.assign(L.staged.begin(), L.staged.begin() + 4 * (size_t)n);
    }
    r.searched = true;
    L.reloc_searches++;
    int32_t id = -1;
    // runSearchPose (global_localization.cpp:311-323): with an INS fix held the local search runs INSTEAD of the global one -- no fallback on this
    // frame -- and the fix is consumed
    const bool local = L.have_latest_ins;
    const Loc::Ins ins = L.latest_ins;
    L.have_latest_ins = false;
    r.local = local;
    if (local) {
        const double xyz[3] = {ins.T(0, 3), ins.T(1, 3), ins.T(2, 3)};
        int32_t ne = 0;
        if (lio_sc_local_search(L.sc, L.reloc_ds.data(), n_ds, xyz, ins.f.precision, &id, &r.yaw, &r.score, &ne) != LIO_OK) return false;
        r.n_examined = ne;
    } else if (lio_sc_global_search_host(L.sc, L.reloc_ds.data(), n_ds, L.sc_dist_thres, &id, &r.yaw, &r.score, nullptr) != LIO_OK) return false;
    r.match_id = id;
    if (id < 0 || (size_t)id >= L.frames.size()) return false;
    // select_registration_method("FAST_VGICP"): the loop detector's coarse configuration
    lio_loop_params lp;
    lio_loop_default_params(&lp);
    const KeyFrameDisk& kf = L.frames[id];
    const uint32_t nt = (uint32_t)(kf.local.size() / 4);
    if ((int)nt < lp.k_correspondences || (int)n_ds < lp.k_correspondences) return false;
    if (!L.reloc_gicp) {
        uint32_t biggest = 1u << 18;
        for (const KeyFrameDisk& f : L.frames) biggest = std::max<uint32_t>(biggest, (uint32_t)(f.local.size() / 4));
        L.reloc_gicp = lio_gicp_create(0, lp.grid_resolution, biggest, lp.k_correspondences);
        if (!L.reloc_gicp || lio_gicp_set_voxel_mode(L.reloc_gicp, lp.voxel_resolution, 1) != LIO_OK) return false;
    }
    if (lio_gicp_set_target(L.reloc_gicp, kf.local.data(), nt) != LIO_OK || lio_gicp_set_source(L.reloc_gicp, L.reloc_ds.data(), n_ds) != LIO_OK) return false;
    Mat4 guess = yaw_matrix_f32(-r.yaw);
    if (local && ins.f.dimension == 6) {
        // :313-315: kf.odom.cast<float>().inverse() * ins.T.cast<float>() in f32 (the inverse taken as a rigid one), the height set to 0
        float K[16], I[16], G[16];
        for (int i = 0; i < 16; i++) { K[i] = (float)kf.odom.m[i]; I[i] = (float)ins.T.m[i]; }
        float Ki[16] = {K[0], K[4], K[8], 0.f, K[1], K[5], K[9], 0.f, K[2], K[6], K[10], 0.f, 0.f, 0.f, 0.f, 1.f};
        for (int a = 0; a < 3; a++) Ki[4 * a + 3] = -(Ki[4 * a] * K[3] + Ki[4 * a + 1] * K[7] + Ki[4 * a + 2] * K[11]);
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) {
                float v = 0.f;
                for (int c = 0; c < 4; c++) v += Ki[4 * a + c] * I[4 * c + b];
                G[4 * a + b] = v;
            }
        for (int i = 0; i < 16; i++) guess.m[i] = (double)G[i];
        guess(2, 3) = 0.0;
    }
    r.guess = guess;
    lio_ndt_params p;
    lio_ndt_default_params(&p);
    p.rotation_epsilon_deg = lp.coarse_rotation_epsilon_deg;
    p.transformation_epsilon = lp.coarse_translation_epsilon;
    p.max_iterations = lp.max_iterations;
    p.max_process_time_ms = -1;
    double T[16];
    int it = 0, conv = 0;
    if (lio_gicp_align(L.reloc_gicp, guess.m, &p, 1.0, T, &it, &conv) != LIO_OK) return false;
    r.converged = conv;
    if (!conv) return false;
    if (lio_gicp_fitness_score(L.reloc_gicp, T, lp.fitness_score_max_range, &r.fitness, nullptr) != LIO_OK) return false;
    // :468-473: delta = getFinalTransformation() (f32), deltadelta = guess^-1 * delta, its translation norm and rotation angle
    Mat4 delta;
    for (int i = 0; i < 16; i++) delta.m[i] = (double)(float)T[i];
    delta(3, 0) = delta(3, 1) = delta(3, 2) = 0.0; delta(3, 3) = 1.0;
    const Mat4 dd = mul(rigid_inverse(guess), delta);
    r.dx = std::sqrt(dd(0, 3) * dd(0, 3) + dd(1, 3) * dd(1, 3) + dd(2, 3) * dd(2, 3));
    const double c = std::max(-1.0, std::min(1.0, (dd(0, 0) + dd(1, 1) + dd(2, 2) - 1.0) * 0.5));
    r.da = std::acos(c) / M_PI * 180.0;
    if (!(r.fitness < 1.5 && r.dx < 10.0 && r.da < 30.0)) return false;
    L.init_pose = mul(kf.odom, delta);
    L.have_init_pose = true;
    r.accepted = true;
    return true;
}

// GlobalLocalization::getEstimatePose for the hint (a pose on the ground, z = 0): ends the current localisation, matches the last frame against the
// key frames near the hint on the device (lio_localmap_estimate_pose) and, when the match is good, keeps the pose and the frame for the hand-over.
// `out` is the pose to answer with.  Returns the reference's result
int loc_estimate_pose(Loc& L, const Mat4& hint, Mat4& out) {
    Loc::Est& e = L.last_est;
    e = Loc::Est();
    e.called = true;
    e.hint = hint;
    out = hint;
    L.initialized = false;     // Localization::getEstimatePose: mInitialized = false, whatever follows
    L.have_init_pose = false;  // (a pose from set_init_pose that no frame has taken up yet is replaced by the hint)
    L.est_pending = false;
    lio_loop_params lp;
    lio_loop_default_params(&lp);
    if (!L.est_gicp) {  // select_registration_method("FAST_VGICP"); room for five of the largest key frames
        L.est_gicp = lio_gicp_create(0, lp.grid_resolution, std::max<uint32_t>(1u << 18, 5u * L.ndt_biggest), lp.k_correspondences);
        if (!L.est_gicp || lio_gicp_set_voxel_mode(L.est_gicp, lp.voxel_resolution, 1) != LIO_OK) { e.rc = LIO_E_DEVICE; return 0; }
    }
    uint32_t ns = 0;
    const void* src = L.have_last_frame ? lio_scan_ds_device(L.scan, &ns) : nullptr;
    e.rc = lio_localmap_estimate_pose(L.lm, L.est_gicp, src, src ? ns : 0, hint.m, &e.rep, out.m);
    e.out = out;
    if (e.rc != LIO_OK || e.rep.result != 1) return 0;
    // mInitialized = true; setInputTarget(mLastFrame); mPoseQueue.enqueue(t)
    require(lio_localmap_store_frame(L.lm, 1, src, ns) == LIO_OK, "get_estimate_pose: keeping the matched frame failed");
    L.est_pose = out;
    L.est_pending = true;
    return 1;
}

// initializePose's second branch (global_localization.cpp:85-91): the new frame (reduced, in L.scan) aligned to the frame the hint was matched with,
// from the identity, by the same matcher; delta = getFinalTransformation() (f32).  The identity when the matcher cannot run (a cloud below k points)
Mat4 loc_handover_delta(Loc& L) {
    Loc::Est& e = L.last_est;
    e.handover = true;
    e.delta = Mat4::identity();
    lio_loop_params lp;
    lio_loop_default_params(&lp);
    uint32_t nt = 0, ns = 0;
    const void* tgt = lio_localmap_frame(L.lm, 1, &nt);
    const void* src = lio_scan_ds_device(L.scan, &ns);
    if (!L.est_gicp || !tgt || !src || (int)nt < lp.k_correspondences || (int)ns < lp.k_correspondences) return e.delta;
    if (lio_gicp_set_target_device(L.est_gicp, tgt, nt) != LIO_OK || lio_gicp_set_source_device(L.est_gicp, src, ns) != LIO_OK) return e.delta;
    lio_ndt_params p;
    lio_estimate_matcher_params(&p);
    const Mat4 I = Mat4::identity();
    double T[16];
    if (lio_gicp_align(L.est_gicp, I.m, &p, 1.0, T, &e.delta_iterations, &e.delta_converged) != LIO_OK) return e.delta;
    e.delta_ran = true;
    for (int i = 0; i < 12; i++) e.delta.m[i] = (double)(float)T[i];
    return e.delta;
}

// Localization::init (localization.cpp:91-131) without the graph back end: the key frames of the map go to HBM once
bool loc_setup(Slam* s) {
    Loc& L = *s->loc;
    if (L.frames.empty()) return false;  // "Map Loader: error to load map" (setup_slam read the key frames from disk)
    uint64_t total = 0;
    uint32_t biggest = 0;
    for (const KeyFrameDisk& kf : L.frames) { total += kf.xyzi.size() / 4; biggest = std::max<uint32_t>(biggest, (uint32_t)(kf.xyzi.size() / 4)); }
    L.lm = lio_localmap_create(0, total + 16, 200000, std::max<uint32_t>(biggest, 1024));
    L.ndt = lio_ndt_create(0, 1.0f, 7, 200000ull + biggest + 1024, 400000, 262144);
    L.ndt_biggest = biggest;
    L.scan = lio_scan_create(0, 1u << 18, 1u << 18);
    if (!L.lm || !L.ndt || !L.scan) return false;
    lio_ndt_default_params(&L.par);
    L.par.max_process_time_ms = 50000;  // select_registration_method("NDT_CUDA", 50000) (hdl_localization_nodelet.cpp:47)
    for (const KeyFrameDisk& kf : L.frames) {
        const float pos[3] = {(float)kf.odom(0, 3), (float)kf.odom(1, 3), (float)kf.odom(2, 3)};
        if (lio_localmap_add_keyframe(L.lm, kf.xyzi.data(), (uint32_t)(kf.xyzi.size() / 4), pos) < 0) return false;
    }
    if (L.reloc && !loc_fill_sc(L)) return false;
    return true;
}

// the resident map made again from the key-frame list (a re-initialisation, and merge_map once the list has grown and its poses moved)
bool loc_refill_local_map(Loc& L) {
    lio_localmap_destroy(L.lm);
    L.lm = nullptr;
    uint64_t total = 0;
    uint32_t biggest = 0;
    for (const KeyFrameDisk& kf : L.frames) { total += kf.xyzi.size() / 4; biggest = std::max<uint32_t>(biggest, (uint32_t)(kf.xyzi.size() / 4)); }
    L.lm = lio_localmap_create(0, total + 16, 200000, std::max<uint32_t>(biggest, 1024));
    if (!L.lm) return false;
    for (const KeyFrameDisk& kf : L.frames) {
        const float kp[3] = {(float)kf.odom(0, 3), (float)kf.odom(1, 3), (float)kf.odom(2, 3)};
        lio_localmap_add_keyframe(L.lm, kf.xyzi.data(), (uint32_t)(kf.xyzi.size() / 4), kp);
    }
    return true;
}

// one loop turn of Localization::runUpdateLocalMap for the pose just located (localization.cpp:303-373) -- synchronous: the key frames are
// resident in HBM, an update is a millisecond of device-to-device copies + VoxelGrid + target build, not a thread's worth of work
void loc_update_local_map(Loc& L, const Mat4& pose) {
    const double p[3] = {pose(0, 3), pose(1, 3), pose(2, 3)};
    int nk = 0;
    uint32_t npts = 0;
    const int rc = lio_localmap_update(L.lm, L.ndt, p, 10.0, 30.0, L.key_frame_distance, (float)std::max(L.resolution, 0.1), &nk, &npts);
    if (rc == 1) L.have_map = true;
    else if (rc == 2 || rc == 3) L.have_map = false;  // out of map / nearest key frame too far: the localizer is handed a null map
}

// HdlLocalizationNodelet::get_timed_pose(stamp) (hdl_localization_nodelet.cpp:108-155) for the two stamps the undistortion asks for
bool loc_timed_pose(Loc& L, uint64_t stamp, Mat4& out) {
    if (L.pose_data.empty()) return false;
    if (stamp < L.pose_data.front().first) return false;
    if (stamp > L.pose_data.back().first) {
        if (stamp - L.pose_data.back().first > 1000000) return false;
        if (!L.pe) return false;
        return lio_pose_estimator_predict_nostate(L.pe, stamp, out.m) >= 0;
    }
    if (L.pose_data.size() < 2) return false;
    out = L.pose_data.back().second;  // (a stamp inside the stored history: not reached by frame_callback, whose stamps are the newest)
    return true;
}

// HdlLocalizationNodelet::frame_callback (hdl_localization_nodelet.cpp:166-275) + Localization::feedPointData's bookkeeping (localization.cpp:235-275).
// The cloud (INS frame) is in L.staged / L.stamps.  Returns true when the pose is a localised one.
bool loc_localize(Slam* s, uint32_t n, uint64_t stamp, Mat4& pose_out) {
    Loc& L = *s->loc;
    if (!L.initialized) {
        if (L.est_pending) {  // an accepted hint: the next non-empty frame hands over, the filter starts from pose * delta
            uint32_t m = 0;
            if (n == 0 || !loc_reduce_staged(L, n, m)) return false;
            L.init_pose = mul(L.est_pose, loc_handover_delta(L));
            L.have_init_pose = true;
            L.est_pending = false;
        } else if (!L.have_init_pose) {
            // no pose from set_init_pose: the global locator (scan context + FAST_VGICP) looks for one when it is switched on.  Either way the
            // frame is reduced and stays on the device: it is what a hint would be matched with
            bool found = false;
            uint32_t m = 0;
            if (L.reloc) found = loc_relocalize(L, n);
            else if (n) loc_reduce_staged(L, n, m);
            if (!found) return false;
        }
        // Localization::initLocalizer -> initialpose_callback (hdl_localization_nodelet.cpp:304-317): normalised quaternion of the pose, cool time 0.2 s
        float ext[16];
        for (int i = 0; i < 16; i++) ext[i] = (float)s->T_imu.m[i];
        const Mat4& T = L.init_pose;
        double q[4];  // w x y z, Eigen's matrix -> quaternion
        {
            const double t = T(0, 0) + T(1, 1) + T(2, 2);
            if (t > 0) { const double r = std::sqrt(t + 1.0); q[0] = 0.5 * r; const double k = 0.5 / r; q[1] = (T(2, 1) - T(1, 2)) * k; q[2] = (T(0, 2) - T(2, 0)) * k; q[3] = (T(1, 0) - T(0, 1)) * k; }
            else {
                int i = 0;
                if (T(1, 1) > T(0, 0)) i = 1;
                if (T(2, 2) > T(i, i)) i = 2;
                const int j = (i + 1) % 3, k = (j + 1) % 3;
                const double r = std::sqrt(T(i, i) - T(j, j) - T(k, k) + 1.0);
                q[1 + i] = 0.5 * r;
                const double kk = 0.5 / r;
                q[0] = (T(k, j) - T(j, k)) * kk; q[1 + j] = (T(j, i) + T(i, j)) * kk; q[1 + k] = (T(k, i) + T(i, k)) * kk;
            }
            const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            for (double& v : q) v /= nq;
        }
        const float pos[3] = {(float)T(0, 3), (float)T(1, 3), (float)T(2, 3)};
        const float qf[4] = {(float)q[0], (float)q[1], (float)q[2], (float)q[3]};
        if (L.pe) lio_pose_estimator_destroy(L.pe);
        L.pe = lio_pose_estimator_create(ext, stamp, pos, qf, 0.2);
        if (!L.pe) return false;
        L.init_stamp = stamp;
        L.pose_data.clear();
        L.imu_data.clear();
        L.ins_data.clear();  // a fresh localiser
        L.last_gps = Loc::GpsUse();
        L.last_odom = T;
        L.initialized = true;
        L.age = 0;
        L.failures = 0;
        if (!loc_refill_local_map(L)) return false;  // a fresh local-map thread state: the first pose always builds a map
        loc_update_local_map(L, T);  // mPoseQueue.enqueue(mLastOdom)
    }
    if (n == 0) {  // "cloud is empty!!": the nodelet returns LocType::OTHER, which Localization::feedPointData counts like any failed frame
                   // (localization.cpp:245-254)
        L.failures++;
        if (L.failures >= 5) { L.initialized = false; L.have_init_pose = false; }
        return false;
    }
    // imu process: mean of the samples up to the frame's stamp
    float acc[3] = {0, 0, 0}, gyr[3] = {0, 0, 0};
    size_t used = 0;
    for (; used < L.imu_data.size(); used++) {
        if (stamp < (uint64_t)(L.imu_data[used].stamp * 1000000.0)) break;
        for (int a = 0; a < 3; a++) { acc[a] = acc[a] + L.imu_data[used].acc[a]; gyr[a] = gyr[a] + L.imu_data[used].gyr[a]; }
    }
    const bool use_imu = used != 0;
    if (use_imu) for (int a = 0; a < 3; a++) { acc[a] = acc[a] / (float)(int)used; gyr[a] = gyr[a] / (float)(int)used; }
    L.imu_data.erase(L.imu_data.begin(), L.imu_data.begin() + used);
    lio_pose_estimator_predict(L.pe, stamp, use_imu ? acc : nullptr, use_imu ? gyr : nullptr);
    // undistortion over the filter's step, then the downsample, on the device
    if (lio_scan_upload(L.scan, L.staged.data(), n) != LIO_OK) return false;
    Mat4 a, b;
    if (loc_timed_pose(L, stamp, a) && loc_timed_pose(L, stamp + lio_pose_estimator_get_dt(L.pe), b)) {
        const Mat4 d = mul(rigid_inverse(a), b);
        float df[16];
        for (int i = 0; i < 16; i++) df[i] = (float)d.m[i];
        lio_scan_undistort_delta(L.scan, L.stamps.data(), 0, df, s->scan_period);
    }
    uint32_t n_ds = 0;
    L.have_last_frame = false;
    if (L.resolution >= 0.1) { if (lio_scan_voxel_downsample(L.scan, (float)L.resolution, 1, &n_ds) != LIO_OK) return false; }
    else { std::vector<float> raw(4 * (size_t)n); lio_scan_download_raw(L.scan, raw.data(), n); lio_scan_set_ds(L.scan, raw.data(), n); n_ds = n; }
    L.have_last_frame = n_ds > 0;  // DEVIATION: mLastFrame is refreshed while localising too (the reference matches a hint against a stale scan)
    // ins process (hdl_localization_nodelet.cpp:231-261), statement for statement: the pair of fixes around the scan's stamp
    lio_gps_observation gps_obs;
    const lio_gps_observation* gps = nullptr;
    L.last_gps = Loc::GpsUse();
    if (!L.ins_data.empty()) {
        if (stamp > L.ins_data.back().f.stamp_us) {
            L.ins_data.clear();
        } else if (stamp >= L.ins_data.front().f.stamp_us) {
            bool gps_data_valid = false;
            size_t first_ins = 0, second_ins = 0;
            for (; second_ins != L.ins_data.size(); second_ins++) {
                const double dt = (L.ins_data[first_ins].f.stamp_us - double(stamp)) / 1000000.0;
                const double dt2 = (L.ins_data[second_ins].f.stamp_us - double(stamp)) / 1000000.0;
                if (dt <= 0 && dt2 >= 0 && (dt2 - dt) < 0.2) { gps_data_valid = true; break; }
                first_ins = second_ins;
            }
            if (gps_data_valid) {
                const Loc::Ins &a1 = L.ins_data[first_ins], &a2 = L.ins_data[second_ins];
                const double t_diff_ratio = static_cast<double>(stamp - a1.f.stamp_us) / static_cast<double>(a2.f.stamp_us - a1.f.stamp_us + 1);
                L.last_gps.used = true;
                L.last_gps.precision = a1.f.precision;
                L.last_gps.dimension = a1.f.dimension;
                L.last_gps.ratio = t_diff_ratio;
                lio_interpolate_transform(a1.T.m, a2.T.m, t_diff_ratio, L.last_gps.T.m);
                std::memcpy(gps_obs.T, L.last_gps.T.m, sizeof(gps_obs.T));
                gps_obs.precision = a1.f.precision;
                gps_obs.dimension = a1.f.dimension;
                gps = &gps_obs;
            }
        }
    }
    // correct
    float obs[7], cov[49];
    bool result = false;
    double fitness = 0.0;
    if (L.have_map) {
        int it = 0;
        const int rc = lio_pose_estimator_match_gps(L.pe, L.ndt, L.scan, &L.par, gps, obs, cov, &it);
        result = rc == 1;
        if (stamp - L.init_stamp < 10000000) {  // WARM_UP_TIME: getFitnessScore(25) of the alignment (pose_estimator.cpp:254-264)
            double T[16] = {0, 0, 0, obs[0], 0, 0, 0, obs[1], 0, 0, 0, obs[2], 0, 0, 0, 1};
            const double w = obs[3], x = obs[4], y = obs[5], z = obs[6];
            T[0] = 1 - 2 * (y * y + z * z); T[1] = 2 * (x * y - z * w); T[2] = 2 * (x * z + y * w);
            T[4] = 2 * (x * y + z * w); T[5] = 1 - 2 * (x * x + z * z); T[6] = 2 * (y * z - x * w);
            T[8] = 2 * (x * z - y * w); T[9] = 2 * (y * z + x * w); T[10] = 1 - 2 * (x * x + y * y);
            uint32_t n_in = 0;
            lio_ndt_fitness_score(L.ndt, L.scan, T, 25.0, &fitness, &n_in);
        }
    } else {
        result = lio_pose_estimator_match_gps_only(L.pe, gps, obs, cov) == 1;
    }
    lio_pose_estimator_correct(L.pe, stamp, obs);
    float M[16];
    lio_pose_estimator_matrix(L.pe, M);
    for (int i = 0; i < 16; i++) pose_out.m[i] = (double)M[i];
    while (L.pose_data.size() >= 10) L.pose_data.pop_front();
    L.pose_data.emplace_back(stamp, pose_out);
    if (fitness > 1.0) result = false;  // "localization fitness score is too large"
    L.last_odom = pose_out;
    // Localization::feedPointData (localization.cpp:252-274)
    if (result) {
        L.age++;
        L.failures = 0;
        loc_update_local_map(L, pose_out);  // mPoseQueue.enqueue(mLastOdom)
    } else {
        L.failures++;
    }
    if (L.failures >= 5) {  // "failed to localize, fallback to initializing": back to waiting for an initial pose
        L.initialized = false;
        L.have_init_pose = false;
    }
    return true;
}

// HDL_FastLIO::runLio (fastlio.cpp:262-276)
void run_lio(Slam* s) {
    while (s->running.load()) {
        const int rc = lio_fastlio_main(s->engine);
        if (rc != LIO_MAIN_IDLE && rc >= 0) {
            double os[16], oe[16];
            lio_fastlio_odometry(s->engine, os, oe);
            Mat4 a, b;
            std::memcpy(a.m, os, sizeof(os));
            std::memcpy(b.m, oe, sizeof(oe));
            a = mul(mul(s->T_imu_ins_inv, a), s->T_imu_ins);
            b = mul(mul(s->T_imu_ins_inv, b), s->T_imu_ins);
            {
                std::lock_guard<std::mutex> lk(s->mtx);
                s->odom_queue.emplace_back(a, b);
            }
            s->cv.notify_all();
            continue;  // more may be queued
        }
        std::this_thread::sleep_for(std::chrono::microseconds(rc == LIO_MAIN_IDLE ? 200 : 2000));
    }
}

py::array_t<float> mat4_to_numpy_f32(const Mat4& T) {  // eigen_to_numpy(Matrix4d) -> float32 4 x 4 (py_utils.cpp:4-11)
    py::array_t<float> a({4, 4});
    auto r = a.mutable_unchecked<2>();
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) r(i, j) = (float)T(i, j);
    return a;
}

}  // namespace

// ---- hot path ---------------------------------------------------------------------------------------------------------------
py::list init_slam(const std::string mode, const std::string map_path, const std::string method, py::list& sensor_input, double resolution,
                   float dist_threshold, float degree_threshold, float frame_range) {
    // slam.py hands in method = "Localization" when the mode is not "mapping" (slam/slam.py:12); SLAM::SLAM then builds Locate::Localization
    const bool localization = mode == "localization" || method == "Localization";
    if (!localization && method != "FastLIO" && method != "RTKM")
        throw std::runtime_error("slam_wrapper: only the FastLIO and RTKM mapping methods and the localisation mode are built on the device (method=" + method + ")");
    g.reset(new Slam());
    g->rtkm = !localization && method == "RTKM";
    const char* gnss_env = std::getenv("LSD_AMD_GNSS");
    g->gnss = gnss_env && gnss_env[0] == '1';
    const char* moment_env = std::getenv("LSD_AMD_GNSS_MOMENT");
    g->gnss_moment = moment_env && moment_env[0] == '1';
    g->mode = localization ? "localization" : mode;
    g->method = method;
    g->map_path = map_path;
    g->resolution = resolution;                 // SLAM::setParams (slam.cpp:96-103)
    g->key_frame_distance = dist_threshold;
    g->key_frame_degree = degree_threshold;
    g->key_frame_range = frame_range;
    const char* kf_env = std::getenv("LSD_AMD_KEYFRAMES");
    g->keyframe_output = kf_env && kf_env[0] == '1';
    lio_loop_default_params(&g->loop_par);
    const char* loop_env = std::getenv("LSD_AMD_LOOP");
    g->loop_detection = loop_env && loop_env[0] == '1';
    const char* graph_env = std::getenv("LSD_AMD_GRAPH");
    g->pose_graph = graph_env && graph_env[0] == '1';
    if (g->pose_graph) g->loop_detection = true;       // the graph consumes the loops
    if (g->loop_detection) g->keyframe_output = true;  // the detector consumes the key frames
    std::vector<std::string> in;
    for (auto h : sensor_input) in.push_back(py::cast<std::string>(h));
    if (localization) {
        g->loc.reset(new Loc());
        const char* reloc_env = std::getenv("LSD_AMD_RELOC");
        g->loc->reloc = reloc_env && reloc_env[0] == '1';
        g->loc->resolution = resolution;
        g->loc->key_frame_distance = dist_threshold;
        // Localization::setSensors (localization.cpp:154-182): RTK / IMU as they come, the first "n-" name is the lidar, the first other one the camera
        bool cam = false;
        for (auto& s : in) {
            g->sensors.push_back(s);
            if (s == "RTK") g->use_gps = true;
            else if (s == "IMU") g->use_imu = true;
            else if (s.length() < 2 || s[1] != '-') cam = cam || true;
            else if (g->lidar.empty()) g->lidar = s;
        }
        return py::cast(g->sensors);
    }
    if (g->rtkm) {
        // RTKM::setSensors (rtkm.cpp:56-89): RTK and IMU first; without RTK nothing else (no lidar); camera names pass; the first "n-" name is
        // the base lidar
        for (auto& s : in) {
            if (s == "RTK") { g->sensors.push_back(s); g->use_gps = true; }
            else if (s == "IMU") { g->sensors.push_back(s); g->use_imu = true; }
        }
        if (g->use_gps)
            for (auto& s : in) {
                if (s == "RTK" || s == "IMU") continue;
                g->sensors.push_back(s);
                if (!(s.length() < 2 || s[1] != '-') && g->lidar.empty()) g->lidar = s;
            }
        return py::cast(g->sensors);
    }
    // HDL_FastLIO::setSensors (fastlio.cpp:119-151): RTK and IMU first; without an IMU nothing else; the first "n-" name is the lidar
    bool imu = false;
    for (auto& s : in) {
        if (s == "RTK") { g->sensors.push_back(s); g->use_gps = true; }
        else if (s == "IMU") { g->sensors.push_back(s); imu = true; }
    }
    g->use_imu = imu;
    if (imu)
        for (auto& s : in) {
            if (s == "RTK" || s == "IMU") continue;
            g->sensors.push_back(s);
            if (!(s.length() < 2 || s[1] != '-') && g->lidar.empty()) g->lidar = s;
        }
    return py::cast(g->sensors);
}

void set_ins_external_param(double x, double y, double z, double yaw, double pitch, double roll) {
    require((bool)g, "init_slam first");
    g->T_static = transform_from_rpyt(x, y, z, yaw, pitch, roll);
    g->painter_stale = true;
}
void set_imu_external_param(double x, double y, double z, double yaw, double pitch, double roll) {
    require((bool)g, "init_slam first");
    g->T_imu = transform_from_rpyt(x, y, z, yaw, pitch, roll);
}

// MapLoader::loadOdometry (map_loader.cpp:223-253): <map>/graph/odometrys.txt, one `stamp x y z qx qy qz qw` a line; the stamp goes to whole
// microseconds, the quaternion through toRotationMatrix as it stands.  A missing file adds nothing
void read_odometrys(const std::string& map_path, std::vector<std::pair<uint64_t, Mat4>>& out) {
    std::ifstream fs(map_path + "/graph/odometrys.txt");
    if (!fs) return;
    double stamp, v[7];
    while (fs >> stamp >> v[0] >> v[1] >> v[2] >> v[3] >> v[4] >> v[5] >> v[6]) {
        const double x = v[3], y = v[4], z = v[5], w = v[6];
        Mat4 T = Mat4::identity();
        T(0, 0) = 1 - 2 * (y * y + z * z); T(0, 1) = 2 * (x * y - z * w); T(0, 2) = 2 * (x * z + y * w);
        T(1, 0) = 2 * (x * y + z * w); T(1, 1) = 1 - 2 * (x * x + z * z); T(1, 2) = 2 * (y * z - x * w);
        T(2, 0) = 2 * (x * z - y * w); T(2, 1) = 2 * (y * z + x * w); T(2, 2) = 1 - 2 * (x * x + y * y);
        T(0, 3) = v[0]; T(1, 3) = v[1]; T(2, 3) = v[2];
        out.emplace_back((uint64_t)(stamp * 1000000), T);
    }
}

namespace {
struct MapInfo { double origin[6] = {0, 0, 0, 0, 0, 0}; int coordinate = 0; bool origin_set = false; };
bool read_map_info(const std::string& map_path, MapInfo& mi) {  // MapLoader::loadMapOrigin (map_loader.cpp:180-221)
    std::ifstream fs(map_path + "/graph/map_info.txt");
    if (!fs) return false;
    for (int i = 0; i < 6; i++) fs >> mi.origin[i];
    double c = 0;
    fs >> c;
    mi.coordinate = (int)c;
    mi.origin_set = false;
    for (int i = 0; i < 6; i++) mi.origin_set = mi.origin_set || !(std::fabs(mi.origin[i]) < 1e-4);
    return true;
}
}  // namespace

bool setup_slam() {
    require((bool)g, "init_slam first");
    if (g->loc) load_keyframes(g->map_path, g->loc->frames);  // host side of MapLoader: get_graph_map serves the key frames whatever follows
    if (g->loc) {
        std::lock_guard<std::mutex> lk(g->mtx);
        g->odometrys.clear();
        read_odometrys(g->map_path, g->odometrys);
    }
    if (lio_device_count() < 1) return false;  // the reference logs and returns false from setup() when the back end cannot start
    if (g->loc) {
        // SLAM::setup (slam.cpp:159-166): the loaded map's origin, projected once, is mZeroUtm
        MapInfo mi;
        if (read_map_info(g->map_path, mi) && mi.origin_set) {
            if (!g->utm) g->utm = lio_utm_create(6);
            require(g->utm != nullptr && lio_utm_forward(g->utm, mi.origin[0], mi.origin[1], &g->zero_utm[0], &g->zero_utm[1]) == LIO_OK, "setup_slam: the map origin's projection failed");
            g->zero_utm[2] = mi.origin[2];
            g->have_zero_utm = true;
        }
        return loc_setup(g.get());
    }
    if (g->rtkm) {  // RTKM::init (rtkm.cpp:22-31): mLastOdom = identity; no FastLIO engine.  The merge handle is made at the first frame
        std::lock_guard<std::mutex> lk(g->mtx);
        if (!g->track) g->track = lio_rtk_track_create();
        g->rtkm_ready = g->track != nullptr;
        return g->rtkm_ready;
    }
    // HDL_FastLIO::init (fastlio.cpp:153-171): T_imu_ins = T_imu * T_static^-1 is the (INS-frame cloud) -> IMU extrinsic
    g->T_imu_ins = mul(g->T_imu, rigid_inverse(g->T_static));
    g->T_imu_ins_inv = rigid_inverse(g->T_imu_ins);
    g->engine = lio_engine_create(0, 0.5f, 75, g->max_points, g->max_voxels, 1u << 18, 100000);
    if (!g->engine) return false;
    const double extT[3] = {g->T_imu_ins(0, 3), g->T_imu_ins(1, 3), g->T_imu_ins(2, 3)};
    double extR[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) extR[i * 3 + j] = g->T_imu_ins(i, j);
    if (lio_fastlio_init(g->engine, extT, extR, 1, -1, g->scan_period, 1) != LIO_OK) return false;
    g->running.store(true);
    g->lio_thread = std::thread(run_lio, g.get());
    return true;
}

void deinit_slam() {
    if (!g) return;
    if (g->running.exchange(false) && g->lio_thread.joinable()) g->lio_thread.join();
    if (g->engine) lio_engine_destroy(g->engine);
    if (g->keyframer) lio_keyframer_destroy(g->keyframer);
    if (g->loop) lio_loop_destroy(g->loop);
    if (g->graph) lio_graph_destroy(g->graph);
    if (g->floor_ground) lio_ground_destroy(g->floor_ground);
    if (g->painter) lio_render_destroy(g->painter);
    if (g->gnss_queue) lio_gnss_queue_destroy(g->gnss_queue);
    if (g->track) lio_rtk_track_destroy(g->track);
    if (g->merger) lio_scan_merge_destroy(g->merger);
    if (g->utm) lio_utm_destroy(g->utm);
    g->loc.reset(nullptr);
    g.reset(nullptr);
}


// ---- the colour map (slam/localization/map_render; csrc/render.hip) ---------------------------------------------------------------------------
using CamCfg = Slam::CamCfg;
constexpr uint64_t kColourVoxels = 1ull << 20, kColourPoints = 1ull << 25;  // 0.2 m voxels and 0.02 m cells: about 3.5 GB of HBM

// pylist_to_camera_config (py_utils.cpp:329-358): K entries cast to float, the extrinsic through getTransformFromRPYT(e0, e1, e2, e5, e4, e3)
std::vector<CamCfg> camera_config(py::list& cameras) {
    std::vector<CamCfg> out;
    for (py::handle obj : cameras) {
        py::dict cam = obj.cast<py::dict>();
        CamCfg c;
        c.name = py::cast<std::string>(cam["name"]);
        py::list in = py::cast<py::list>(cam["intrinsic_parameters"]), ex = py::cast<py::list>(cam["extrinsic_parameters"]);
        if (py::len(in) < 4 || py::len(ex) < 6) throw std::invalid_argument("slam_wrapper: camera '" + c.name + "': 4 intrinsic and 6 extrinsic parameters are needed");
        c.K[0] = (double)py::cast<float>(in[0]);  // fx
        c.K[1] = (double)py::cast<float>(in[1]);  // fy
        c.K[2] = (double)py::cast<float>(in[2]);  // cx
        c.K[3] = (double)py::cast<float>(in[3]);  // cy
        c.ext = transform_from_rpyt(py::cast<double>(ex[0]), py::cast<double>(ex[1]), py::cast<double>(ex[2]), py::cast<double>(ex[5]), py::cast<double>(ex[4]),
                                    py::cast<double>(ex[3]));
        bool seen = false;
        for (CamCfg& o : out)
            if (o.name == c.name) { o = c; seen = true; }  // (a std::map in the reference: the later entry of a name wins)
        if (!seen) out.push_back(c);
    }
    return out;
}

// a fresh painter with these cameras (MapRender::setParameter); throws without a device
lio_render* make_painter(const std::vector<CamCfg>& cams, const Mat4& lidar_static, const char* what) {
    lio_render* r = lio_render_create(0, kColourVoxels, kColourPoints);
    if (!r) throw std::runtime_error(std::string("slam_wrapper: ") + what + ": the colour map needs a HIP device (there is no CPU fallback): " + lio_last_error());
    std::vector<const char*> names;
    std::vector<double> in, ex;
    for (const CamCfg& c : cams) {
        names.push_back(c.name.c_str());
        in.insert(in.end(), c.K, c.K + 4);
        ex.insert(ex.end(), c.ext.m, c.ext.m + 16);
    }
    if (lio_render_set_cameras(r, (int)cams.size(), names.data(), in.data(), ex.data(), lidar_static.m) != LIO_OK) {
        lio_render_destroy(r);
        require(false, what);
    }
    return r;
}

// pydict_to_image (py_utils.cpp:198-212) for the cameras that are configured: BGR rows x cols x 3 u8 and the stamp of image_param[name].  A 2-D
// (I420) image raises ValueError: imageCvtColor's conversion is out of scope.
struct FrameImage { int camera; uint64_t stamp; int rows, cols; std::vector<uint8_t> bgr; Mat4 pose; };
std::vector<FrameImage> frame_images(py::dict& image_dict, py::dict& image_param, const std::vector<CamCfg>& cams, const char* what) {
    std::vector<FrameImage> out;
    for (auto item : image_dict) {
        const std::string name = py::cast<std::string>(item.first);
        py::array ar = py::cast<py::array>(item.second);
        if (ar.ndim() != 3 || ar.shape(2) != 3)
            throw std::invalid_argument(std::string("slam_wrapper: ") + what + ": image '" + name + "' must be rows x cols x 3 (BGR); an I420 image is not converted");
        int cam = -1;
        for (size_t k = 0; k < cams.size(); k++)
            if (cams[k].name == name) cam = (int)k;
        if (cam < 0 || !image_param.contains(name.c_str())) continue;  // (no camera of that name: nothing to paint with)
        auto a = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>::ensure(ar);
        if (!a) throw std::invalid_argument(std::string("slam_wrapper: ") + what + ": image '" + name + "' is not a uint8 array");
        FrameImage im;
        im.camera = cam;
        im.stamp = py::cast<uint64_t>(py::cast<py::dict>(image_param[name.c_str()])["timestamp"]);
        im.rows = (int)a.shape(0);
        im.cols = (int)a.shape(1);
        im.bgr.assign(a.data(), a.data() + (size_t)a.size());
        im.pose = Mat4::identity();
        out.push_back(std::move(im));
    }
    return out;
}

// MapRender::render over the images that have a pose; LIO_RENDER_* or a negative error
int paint_frame(lio_render* r, const float* xyzi, size_t n, const Mat4& pose, uint32_t seed, const std::vector<FrameImage>& imgs) {
    std::vector<lio_render_image> li(imgs.size());
    for (size_t k = 0; k < imgs.size(); k++) {
        li[k].camera = imgs[k].camera;
        li[k].rows = imgs[k].rows;
        li[k].cols = imgs[k].cols;
        li[k].reserved = 0;
        li[k].bgr = imgs[k].bgr.data();
        std::memcpy(li[k].pose, imgs[k].pose.m, sizeof(li[k].pose));
    }
    return lio_render_frame(r, xyzi, n, pose.m, 1, seed, li.data(), (int)li.size());
}

// getColorMap as pointcloud_to_numpy(PointCloudRGB) packs it (py_utils.cpp:118-129): N x 4; nothing painted: the empty array this module has
// always returned
std::vector<float> colour_map_points(lio_render* r) {
    std::vector<float> out;
    if (!r) return out;
    const int64_t n = -lio_render_download(r, nullptr, 0);
    if (n <= 0) return out;
    out.resize(4 * (size_t)n);
    require(lio_render_download(r, out.data(), (uint64_t)n) == n, "get_color_map: download failed");
    return out;
}

// the live painter as the cameras and the static transform stand (Localization::init: mMap->setParameter(mStaticTrans, mCameraParams))
lio_render* live_painter(Slam* s) {
    if (s->painter && !s->painter_stale) return s->painter;
    if (s->painter) lio_render_destroy(s->painter);
    s->painter = nullptr;
    s->painter = make_painter(s->cameras, s->T_static, "process");
    lio_render_set_active(s->painter, 1);
    s->painter_stale = false;
    return s->painter;
}

// what process() does with a fix in localisation mode under set_gnss (_push_gnss calls it too): preprocessInsData's validity test, then
// Localization::feedInsData (localization.cpp:199-209) -- dropped unless valid and the map has an origin; T = computeRTKTransform(projector, fix,
// zero_utm); the global locator keeps the newest, the localiser a list of ten (ins_callback).  Returns rtk_valid
bool loc_feed_fix(Slam* s, py::dict& rtk_dict, uint64_t timestamp) {
    Fix fix = fix_of(rtk_dict);
    const bool rtk_valid = fix.has_stamp && preprocess_ins(s, timestamp, fix);
    if (!rtk_valid || !s->have_zero_utm) return rtk_valid;
    Loc& L = *s->loc;
    Loc::Ins ins;
    ins.f = fix.f;
    std::lock_guard<std::mutex> lk(s->mtx);
    require(lio_rtk_transform_utm(s->utm, &fix.f, s->zero_utm, ins.T.m) == LIO_OK, "process: the fix's projection failed");
    if (!L.initialized) { L.latest_ins = ins; L.have_latest_ins = true; }
    else {
        if (L.ins_data.size() >= 10) L.ins_data.pop_front();
        L.ins_data.push_back(ins);
    }
    return rtk_valid;
}

// SLAM::run, localisation branch (slam.cpp:273-367) over Localization::feedImuData / feedPointData / getPose
py::dict process_localization(Slam* s, py::dict& points, py::dict& points_attr, py::dict& image_dict, py::dict& image_param, py::dict& rtk_dict,
                              py::array_t<double>& imu_list, uint64_t timestamp) {
    Loc& L = *s->loc;
    // with colouration off the images are not looked at
    std::vector<FrameImage> images;
    if (s->colouration && !s->cameras.empty()) images = frame_images(image_dict, image_param, s->cameras, "process");
    int status = 0;
    if (rtk_dict.contains("Status")) status = py::cast<int>(rtk_dict["Status"]);
    std::string name = s->lidar;
    if (name.empty() || !points.contains(name.c_str())) {
        require(py::len(points) > 0, "process: no point cloud");
        name = py::cast<std::string>((*points.begin()).first);
    }
    py::array_t<float, py::array::c_style | py::array::forcecast> cloud = py::cast<py::array>(points[name.c_str()]);
    py::dict attr = py::cast<py::dict>(points_attr[name.c_str()]);
    py::array_t<float, py::array::c_style | py::array::forcecast> pattr = py::cast<py::array>(attr["points_attr"]);
    const uint64_t header_stamp = py::cast<uint64_t>(attr["timestamp"]);
    require(cloud.ndim() == 2 && cloud.shape(1) >= 4 && pattr.ndim() == 2 && pattr.shape(1) >= 1 && pattr.shape(0) == cloud.shape(0),
            "process: points must be N x 4 float32 with an N x 2 attribute array");
    const uint32_t n = (uint32_t)cloud.shape(0);
    const float* src = cloud.data();
    const float* asrc = pattr.data();
    const py::ssize_t cs = cloud.shape(1), as = pattr.shape(1);
    std::vector<Loc::Imu> imu_in;
    if (s->use_imu && imu_list.ndim() == 2 && imu_list.shape(1) >= 7) {  // numpy_to_imu (py_utils.cpp:244-258)
        auto ref = imu_list.unchecked<2>();
        for (py::ssize_t i = 0; i < ref.shape(0); i++) {
            Loc::Imu m;
            m.stamp = ref(i, 0) / 1000000.0;
            for (int a = 0; a < 3; a++) { m.gyr[a] = (float)(ref(i, 1 + a) / 180.0 * M_PI); m.acc[a] = (float)(ref(i, 4 + a) * 9.81); }
            imu_in.push_back(m);
        }
    }
    // SLAM::run's GNSS lines (slam.cpp:280-292) in localisation mode, behind set_gnss: the validity filter mapping mode uses; with the switch off
    // the fix is not looked at
    const bool gnss_side = s->gnss && s->use_gps;
    const bool rtk_valid = gnss_side && loc_feed_fix(s, rtk_dict, timestamp);
    Mat4 out_pose = Mat4::identity();
    bool located = false, inited = false;
    {
        py::gil_scoped_release release;
        std::lock_guard<std::mutex> lk(s->mtx);
        L.sc_dist_thres = gnss_side ? 0.25 : 0.30;  // like everything of the switch here: only with RTK among the sensors
        if (L.initialized) L.imu_data.insert(L.imu_data.end(), imu_in.begin(), imu_in.end());  // Localization::feedImuData: dropped while not initialised
        // preprocessPoints (slam_base.h:83-85) straight into the staging vector
        L.staged.resize(4 * (size_t)n + 4);
        L.stamps.resize((size_t)n + 1);
        const Mat4& M = s->T_static;
        for (uint32_t i = 0; i < n; i++) {
            const double x = src[i * cs], y = src[i * cs + 1], z = src[i * cs + 2];
            L.staged[4 * i + 0] = (float)(M(0, 0) * x + M(0, 1) * y + M(0, 2) * z + M(0, 3));
            L.staged[4 * i + 1] = (float)(M(1, 0) * x + M(1, 1) * y + M(1, 2) * z + M(1, 3));
            L.staged[4 * i + 2] = (float)(M(2, 0) * x + M(2, 1) * y + M(2, 2) * z + M(2, 3));
            L.staged[4 * i + 3] = src[i * cs + 3];
            L.stamps[i] = (uint32_t)asrc[i * as];
        }
        located = loc_localize(s, n, header_stamp, out_pose);
        if (!located) out_pose = L.last_odom;
        inited = L.initialized && L.age >= 10;  // Localization::isInited: mInitialized && isStable()
        // Localization::feedPointData, localization.cpp:237-244: a located frame of a stable localisation is painted (renderMap, :22-30: the
        // images whose stamp getTimedPose answers), with the frame as the localiser left it (undistorted, INS frame)
        if (located && inited && s->colouration && !s->cameras.empty()) {
            lio_render* r = live_painter(s);
            std::vector<FrameImage> posed;
            for (FrameImage& im : images)
                if (loc_timed_pose(L, im.stamp, im.pose)) posed.push_back(std::move(im));
            std::vector<float> frame(4 * (size_t)n + 4);
            const int m = lio_scan_download_raw(L.scan, frame.data(), n);
            // (a frame that does not fit leaves the map as it is: the drive goes on without it)
            if (m > 0) (void)paint_frame(r, frame.data(), (size_t)m, out_pose, s->colour_seed, posed);
        }
    }
    double heading, pitch, roll;
    rpy_from_transform(out_pose, heading, pitch, roll);
    if (std::fabs(roll) >= 90.0 || std::fabs(pitch) >= 90.0) {
        const Mat4 o2 = transform_from_rpyt(out_pose(0, 3), out_pose(1, 3), out_pose(2, 3), -heading, pitch, roll);
        rpy_from_transform(o2, heading, pitch, roll);
    } else {
        heading = -heading;
    }
    if (heading < 0) heading += 360;
    // slam.cpp:335-342: the inverse projection of zero_utm + odom once the localiser is inited and the map has an origin; zeros otherwise
    double lat = 0.0, lon = 0.0, alt = 0.0;
    if (inited && s->have_zero_utm) {
        require(lio_utm_inverse(s->utm, s->zero_utm[0] + out_pose(0, 3), s->zero_utm[1] + out_pose(1, 3), &lat, &lon) == LIO_OK, "process: the inverse projection failed");
        alt = s->zero_utm[2] + out_pose(2, 3);
    }
    py::dict pose;
    pose["latitude"] = lat;
    pose["longitude"] = lon;
    pose["altitude"] = alt;
    pose["heading"] = heading;
    pose["pitch"] = pitch;
    pose["roll"] = roll;
    pose["Ve"] = 0;
    pose["Vn"] = 0;
    pose["Vu"] = 0;
    pose["Status"] = status;
    pose["state"] = inited ? ((gnss_side && rtk_valid) ? "Localizing(L+G)" : "Localizing(L)") : "Initializing";  // slam.cpp:324-332
    pose["timestamp"] = header_stamp;
    pose["odom_matrix"] = mat4_to_numpy_f32(out_pose);
    py::dict data;
    data["frame_start_timestamp"] = timestamp;
    data["pose"] = pose;
    data["slam_valid"] = true;
    return data;
}

// what process() does with a fix in mapping mode, and nothing else (_push_gnss calls it too).
// SLAM::run (slam.cpp:283-296): preprocessInsData's validity test, the origin and the method's feedInsData (feed_gnss), then for FastLIO
// fastlio_ins_enqueue (fastlio.cpp:185-187, laserMapping.cpp:417-441): the INS velocity, ENU -> ego -> IMU, third component zeroed -- IMU
// initialisation seeds the state's velocity from it (IMU_Processing.hpp:201-204), the wheel-speed rows read it
void feed_fix(Slam* s, py::dict& rtk_dict, Fix& fix, uint64_t timestamp) {
    if (!s->use_gps || !fix.has_stamp) return;
    const bool gnss_side = s->rtkm || s->gnss;
    if (!rtk_dict.contains("Ve") && !gnss_side) return;
    const bool valid = feed_gnss(s, timestamp, fix);
    if (s->rtkm || !s->engine || !rtk_dict.contains("Ve")) return;
    if (valid || fix.sensor.find("Wheel") != std::string::npos) {
        const double hd = fix.f.heading, pt = fix.f.pitch, rl = fix.f.roll;
        const double ve[3] = {py::cast<double>(rtk_dict["Ve"]), rtk_dict.contains("Vn") ? py::cast<double>(rtk_dict["Vn"]) : 0.0,
                              rtk_dict.contains("Vu") ? py::cast<double>(rtk_dict["Vu"]) : 0.0};
        const Mat4 Tve = rigid_inverse(transform_from_rpyt(0, 0, 0, -hd, pt, rl));
        double ego[3], vi[3];
        for (int r = 0; r < 3; r++) ego[r] = Tve(r, 0) * ve[0] + Tve(r, 1) * ve[1] + Tve(r, 2) * ve[2];
        for (int r = 0; r < 3; r++) vi[r] = s->T_imu_ins(r, 0) * ego[0] + s->T_imu_ins(r, 1) * ego[1] + s->T_imu_ins(r, 2) * ego[2];
        vi[2] = 0.0;  // "body up speed of INS is not accurate"
        lio_fastlio_ins_enqueue(s->engine, fix.f.stamp_us / 1000000.0, vi);
    }
}

// the frame of process() into the key-frame selector (SLAM::runMappingThread -> enqueue_graph -> cloud_callback, slam.cpp:398-411,
// hdl_graph_slam_nodelet.cpp:163-246) with its odometry pose and its delta; no pose list (the delta branch).  kf_mtx is held
void push_frame_locked(Slam* s, const float* pts, const uint32_t* stamps, uint32_t n, uint64_t header_stamp, const Mat4& pose, const Mat4& delta) {
    if (!s->keyframer) {
        lio_keyframer_params kp;
        lio_keyframer_default_params(&kp);
        kp.key_frame_distance = s->key_frame_distance;
        kp.key_frame_degree = s->key_frame_degree;
        kp.resolution = s->resolution;
        kp.key_frame_range = s->key_frame_range;
        kp.scan_period = s->scan_period;
        s->keyframer = lio_keyframer_create(0, &kp);
        require(s->keyframer != nullptr, "process: lio_keyframer_create failed");
    }
    require(lio_keyframer_push_host(s->keyframer, pts, stamps, n, header_stamp, pose.m, delta.m, nullptr, nullptr, 0, nullptr) == LIO_OK,
            "process: key-frame push failed");
}

py::dict mapping_pose_dict(const Mat4& out_pose, double lat, double lon, double alt, int status, uint64_t header_stamp, uint64_t timestamp);
py::dict process_rtkm(Slam* s, py::dict& points, py::dict& points_attr, py::dict& rtk_dict, uint64_t timestamp);

py::dict process(py::dict& points, py::dict& points_attr, py::dict& image_dict, py::dict& image_stream_dict, py::dict& image_param,
                 py::dict& rtk_dict, py::array_t<double>& imu_list, uint64_t timestamp) {
    (void)image_stream_dict;
    require(g && (g->engine || g->rtkm_ready || (g->loc && g->loc->scan)), "init_slam / setup_slam first");
    Slam* s = g.get();
    if (s->loc) return process_localization(s, points, points_attr, image_dict, image_param, rtk_dict, imu_list, timestamp);
    if (s->rtkm) return process_rtkm(s, points, points_attr, rtk_dict, timestamp);
    // pydict_to_rtk; SLAM::run copies latitude / longitude / altitude / status into the pose in mapping mode (slam.cpp:344-348)
    Fix fix = fix_of(rtk_dict);
    const double lat = fix.f.latitude, lon = fix.f.longitude, alt = fix.f.altitude;
    const int status = fix.status;
    feed_fix(s, rtk_dict, fix, timestamp);
    // numpy_to_imu + HDL_FastLIO::feedImuData
    if (s->use_imu && imu_list.ndim() == 2 && imu_list.shape(1) >= 7) {
        auto ref = imu_list.unchecked<2>();
        for (py::ssize_t i = 0; i < ref.shape(0); i++) {
            const double gyr[3] = {ref(i, 1) / 180.0 * M_PI, ref(i, 2) / 180.0 * M_PI, ref(i, 3) / 180.0 * M_PI};
            const double acc[3] = {ref(i, 4) * 9.81, ref(i, 5) * 9.81, ref(i, 6) * 9.81};
            lio_fastlio_imu_enqueue(s->engine, ref(i, 0) / 1000000.0, gyr, acc);
        }
    }
    // pydict_to_cloud + feedPointData: the lidar's cloud (fastlio.cpp:204-210 takes points[mLidarName])
    std::string name = s->lidar;
    if (name.empty() || !points.contains(name.c_str())) {
        require(py::len(points) > 0, "process: no point cloud");
        name = py::cast<std::string>((*points.begin()).first);
    }
    py::array_t<float, py::array::c_style | py::array::forcecast> cloud = py::cast<py::array>(points[name.c_str()]);
    py::dict attr = py::cast<py::dict>(points_attr[name.c_str()]);
    py::array_t<float, py::array::c_style | py::array::forcecast> pattr = py::cast<py::array>(attr["points_attr"]);
    const uint64_t header_stamp = py::cast<uint64_t>(attr["timestamp"]);
    require(cloud.ndim() == 2 && cloud.shape(1) >= 4 && pattr.ndim() == 2 && pattr.shape(1) >= 1 && pattr.shape(0) == cloud.shape(0),
            "process: points must be N x 4 float32 with an N x 2 attribute array");
    const uint32_t n = (uint32_t)cloud.shape(0);
    const float* src = cloud.data();
    const float* asrc = pattr.data();
    const py::ssize_t cs = cloud.shape(1), as = pattr.shape(1);
    Mat4 out_pose = Mat4::identity();
    bool got = false;
    {
        py::gil_scoped_release release;
        float* dst = nullptr;
        uint32_t* dstamp = nullptr;
        require(lio_fastlio_pcl_stage(s->engine, n, &dst, &dstamp) == LIO_OK, "process: staging failed");
        // pcl::transformPointCloud(in, out, Matrix4d): per point in double, terms left to right, cast to float (PCL 1.9.1 transforms.hpp)
        const Mat4& M = s->T_static;
        for (uint32_t i = 0; i < n; i++) {
            const double x = src[i * cs], y = src[i * cs + 1], z = src[i * cs + 2];
            dst[4 * i + 0] = (float)(M(0, 0) * x + M(0, 1) * y + M(0, 2) * z + M(0, 3));
            dst[4 * i + 1] = (float)(M(1, 0) * x + M(1, 1) * y + M(1, 2) * z + M(1, 3));
            dst[4 * i + 2] = (float)(M(2, 0) * x + M(2, 1) * y + M(2, 2) * z + M(2, 3));
            dst[4 * i + 3] = src[i * cs + 3];
            dstamp[i] = (uint32_t)asrc[i * as];  // pointcloud_attr[i].stamp = ref_attr(i, 0): float -> uint32_t
        }
        const bool keyframes = s->keyframe_output;
        if (keyframes) {  // the staging buffers are the engine's after the commit
            s->kf_points.assign(dst, dst + 4 * (size_t)n);
            s->kf_stamps.assign(dstamp, dstamp + n);
        }
        require(lio_fastlio_pcl_commit(s->engine, n, (double)header_stamp / 1000000.0) == LIO_OK, "process: enqueue failed");
        // HDL_FastLIO::getPose: wait for the LIO thread's odometry (10 s), then get_odom2map() (identity without a graph back end) * odom.first
        std::unique_lock<std::mutex> lk(s->mtx);
        got = s->cv.wait_for(lk, std::chrono::seconds(10), [&] { return !s->odom_queue.empty(); });
        Mat4 odom_end = Mat4::identity();
        if (got) {
            out_pose = s->odom_queue.front().first;
            odom_end = s->odom_queue.front().second;
            s->odom_queue.pop_front();
            s->last_odom_start = out_pose;
            s->last_odom_end = odom_end;
            // mOdometrys (fastlio.cpp:242-250): the reference pushes the IMU-predicted poses inside the frame; here the frame's end-of-scan pose
            // at the end-of-scan stamp, and a stamp that does not exceed the last is dropped as there
            const uint64_t end_stamp = header_stamp + (uint64_t)std::llround(s->scan_period * 1e6);
            if (s->odometrys.empty() || s->odometrys.back().first < end_stamp) s->odometrys.emplace_back(end_stamp, odom_end);
        }
        lk.unlock();
        // SLAM::runMappingThread -> enqueue_graph -> cloud_callback (slam.cpp:398-411, hdl_graph_slam_nodelet.cpp:163-246): the frame with its
        // odometry pose and delta = first^-1 * second; the IMU pose list of HDL_FastLIO::prediction is not fed (the delta branch)
        if (got && keyframes) {
            std::lock_guard<std::mutex> kl(s->kf_mtx);
            const Mat4 delta = mul(rigid_inverse(out_pose), odom_end);
            push_frame_locked(s, s->kf_points.data(), s->kf_stamps.data(), n, header_stamp, out_pose, delta);
        }
        if (got && s->pose_graph) {  // HDL_FastLIO::getPose: get_odom2map() * odom.first (the key frame above carries the odometry itself)
            std::lock_guard<std::mutex> kl(s->kf_mtx);
            out_pose = mul(s->odom2map, out_pose);
        }
    }
    return mapping_pose_dict(out_pose, lat, lon, alt, status, header_stamp, timestamp);
}

// SLAM::run, mapping branch (slam.cpp:344-364)
py::dict mapping_pose_dict(const Mat4& out_pose, double lat, double lon, double alt, int status, uint64_t header_stamp, uint64_t timestamp) {
    double heading, pitch, roll;
    rpy_from_transform(out_pose, heading, pitch, roll);
    if (std::fabs(roll) >= 90.0 || std::fabs(pitch) >= 90.0) {
        // (the reference rebuilds a LOCAL copy of the odometry here; pose.T was assigned before and keeps the filter's matrix)
        const Mat4 o2 = transform_from_rpyt(out_pose(0, 3), out_pose(1, 3), out_pose(2, 3), -heading, pitch, roll);
        rpy_from_transform(o2, heading, pitch, roll);
    } else {
        heading = -heading;
    }
    if (heading < 0) heading += 360;
    py::dict pose;
    pose["latitude"] = lat;
    pose["longitude"] = lon;
    pose["altitude"] = alt;
    pose["heading"] = heading;
    pose["pitch"] = pitch;
    pose["roll"] = roll;
    pose["Ve"] = 0;
    pose["Vn"] = 0;
    pose["Vu"] = 0;
    pose["Status"] = status;
    pose["state"] = "Mapping";
    pose["timestamp"] = header_stamp;
    pose["odom_matrix"] = mat4_to_numpy_f32(out_pose);
    py::dict data;
    data["frame_start_timestamp"] = timestamp;
    data["pose"] = pose;
    data["slam_valid"] = true;
    return data;
}

// SLAM::run over RTKM (rtkm.cpp): the fix to the track, the lidars merged into one frame on the device, the pose from the track at the merged
// header stamp (mLastOdom when the track refuses), delta = mLastOdom^-1 * odom
py::dict process_rtkm(Slam* s, py::dict& points, py::dict& points_attr, py::dict& rtk_dict, uint64_t timestamp) {
    Fix fix = fix_of(rtk_dict);
    feed_fix(s, rtk_dict, fix, timestamp);
    // pydict_to_cloud into std::map order; mergePoints (slam_utils.cpp:249-273): without the base lidar the frame is empty
    std::map<std::string, int> order;
    std::vector<py::array_t<float, py::array::c_style | py::array::forcecast>> clouds, attrs;
    std::vector<uint64_t> headers;
    for (auto item : points) {
        const std::string name = py::cast<std::string>(item.first);
        py::dict attr = py::cast<py::dict>(points_attr[name.c_str()]);
        order[name] = (int)clouds.size();
        clouds.push_back(py::cast<py::array>(item.second));
        attrs.push_back(py::cast<py::array>(attr["points_attr"]));
        headers.push_back(py::cast<uint64_t>(attr["timestamp"]));
        const auto& c = clouds.back();
        const auto& a = attrs.back();
        require(c.ndim() == 2 && c.shape(1) >= 4 && a.ndim() == 2 && a.shape(1) >= 1 && a.shape(0) == c.shape(0),
                "process: points must be N x 4 float32 with an N x 2 attribute array");
    }
    std::vector<int> take;  // the base, then the others by name
    if (order.count(s->lidar)) {
        take.push_back(order[s->lidar]);
        for (const auto& kv : order)
            if (kv.first != s->lidar) take.push_back(kv.second);
    }
    require(take.size() <= 16, "process: RTKM merges at most 16 lidars");
    std::vector<std::vector<float>> xyzi(take.size());
    std::vector<std::vector<uint32_t>> stamps(take.size());
    std::vector<const float*> pp(take.size());
    std::vector<const uint32_t*> sp(take.size());
    std::vector<uint32_t> np_(take.size());
    std::vector<uint64_t> hd(take.size());
    uint64_t total = 0;
    for (size_t l = 0; l < take.size(); l++) {
        const auto& c = clouds[(size_t)take[l]];
        const auto& a = attrs[(size_t)take[l]];
        const size_t n = (size_t)c.shape(0);
        const py::ssize_t cs = c.shape(1), as = a.shape(1);
        xyzi[l].resize(4 * n + 4);
        stamps[l].resize(n + 1);
        const float* src = c.data();
        const float* asrc = a.data();
        for (size_t i = 0; i < n; i++) {
            for (int k = 0; k < 4; k++) xyzi[l][4 * i + k] = src[i * cs + k];
            stamps[l][i] = (uint32_t)asrc[i * as];  // pointcloud_attr[i].stamp = ref_attr(i, 0): float -> uint32_t
        }
        pp[l] = xyzi[l].data(); sp[l] = stamps[l].data(); np_[l] = (uint32_t)n; hd[l] = headers[(size_t)take[l]];
        total += n;
    }
    const uint64_t header_stamp = take.empty() ? 0 : hd[0];
    Mat4 odom = Mat4::identity();
    {
        py::gil_scoped_release release;
        std::unique_lock<std::mutex> lk(s->mtx);
        uint64_t n_out = 0;
        if (!take.empty()) {
            if (!s->merger || total > s->merger_cap) {
                if (s->merger) lio_scan_merge_destroy(s->merger);
                s->merger_cap = std::max<uint64_t>(2 * total, 1ull << 20);
                s->merger = lio_scan_merge_create(0, 16, s->merger_cap);
                require(s->merger != nullptr, "process: lio_scan_merge_create failed");
            }
            require(lio_scan_merge_set_transform(s->merger, s->T_static.m) == LIO_OK, "process: lio_scan_merge_set_transform failed");
            require(lio_scan_merge_run_host(s->merger, (uint32_t)take.size(), pp.data(), sp.data(), np_.data(), hd.data(),
                                            uint64_t(s->scan_period * 1000000.0), nullptr, nullptr, nullptr, &n_out) == LIO_OK, "process: the merge failed");
        }
        s->merged_pts.resize(4 * (size_t)n_out + 4);
        s->merged_stamps.resize((size_t)n_out + 1);
        if (n_out)
            require(lio_scan_merge_download(s->merger, s->merged_pts.data(), s->merged_stamps.data(), n_out) == (int64_t)n_out, "process: the merged frame's download failed");
        s->merged_pts.resize(4 * (size_t)n_out);
        s->merged_stamps.resize((size_t)n_out);
        // RTKM::getPose (rtkm.cpp:111-123)
        odom = s->rtkm_last_odom;
        if (s->track) (void)lio_rtk_track_interpolate(s->track, header_stamp, odom.m);
        const Mat4 delta = mul(rigid_inverse(s->rtkm_last_odom), odom);
        s->last_odom_start = s->rtkm_last_odom;  // (_last_odometry: mLastOdom before and after this frame)
        s->last_odom_end = odom;
        s->rtkm_last_odom = odom;
        const std::vector<float> pts = s->merged_pts;
        const std::vector<uint32_t> st = s->merged_stamps;
        lk.unlock();
        if (s->keyframe_output && n_out > 0) {
            std::lock_guard<std::mutex> kl(s->kf_mtx);
            push_frame_locked(s, pts.data(), st.data(), (uint32_t)n_out, header_stamp, odom, delta);
        }
    }
    return mapping_pose_dict(odom, fix.f.latitude, fix.f.longitude, fix.f.altitude, fix.status, header_stamp, timestamp);
}

// ---- off the hot path: type-correct minimal implementations -------------------------------------------
// SLAM::setCameraParameter: kept for the colour map (the painter takes them with the static transform at its next frame)
void set_camera_param(py::list& cameras) {
    if (!g) return;
    std::vector<CamCfg> cams = camera_config(cameras);
    std::lock_guard<std::mutex> lk(g->mtx);
    g->cameras = std::move(cams);
    g->painter_stale = true;
}
// pydict_to_ins_config (py_utils.cpp:295-317): ins_normal / ins_float / ins_fix entries with use, status, stable_time, precision
void set_ins_config(py::dict& dict) {
    if (!g) return;
    if (dict.contains("ins_type")) {  // pydict_to_ins_dimension (py_utils.cpp:317-327)
        const std::string dim = py::cast<std::string>(dict["ins_type"]);
        g->ins_dim = dim == "2D" ? 2 : (dim == "3D" ? 3 : (dim == "6D" ? 6 : 0));
    }
    g->ins_cfg.clear();
    int priority = 0;
    for (const char* name : {"ins_normal", "ins_float", "ins_fix"}) {
        if (!dict.contains(name)) continue;
        py::dict e = py::cast<py::dict>(dict[name]);
        if (!e.contains("use") || !py::cast<bool>(e["use"])) continue;
        Slam::InsCfg c;
        c.name = name;
        c.status = py::cast<int>(e["status"]);
        c.stable_time = py::cast<double>(e["stable_time"]);
        c.precision = py::cast<double>(e["precision"]);
        c.priority = priority++;
        g->ins_cfg.push_back(c);
    }
}
void set_init_pose(double x, double y, double z, double yaw, double pitch, double roll) {
    if (!g) return;
    const double v[6] = {x, y, z, yaw, pitch, roll};
    std::memcpy(g->init_pose, v, sizeof(v));
    if (g->loc) {  // SLAM::setInitPose (slam.cpp): getTransformFromRPYT(x, y, z, yaw, pitch, roll) -> Localization::setInitPose: mInitialized = false
        std::lock_guard<std::mutex> lk(g->mtx);
        g->loc->init_pose = transform_from_rpyt(x, y, z, yaw, pitch, roll);
        g->loc->have_init_pose = true;
        g->loc->initialized = false;
    }
}
// SLAM::getEstimatePose (slam.cpp:137-146) -> Localization::getEstimatePose, and the answer of slam_wrapper.cpp:45-56.  The hint's rotation is
// Rz(atan2(y1 - y0, x1 - x0)) (the project's rule: FromTwoVectors is ambiguous for an arrow along -x and NaN for one of zero length)
py::list get_estimate_pose(double x0, double y0, double x1, double y1) {
    const std::vector<double> none{0, 0, 0, 0, 0, 0, 0};  // x, y, z, roll, pitch, -yaw, result (0 = no estimate)
    if (!g || !g->loc || !g->loc->lm || !g->loc->scan) return py::cast(none);
    const double dx = x1 - x0, dy = y1 - y0;
    if (!(dx * dx + dy * dy > 0.0) || !std::isfinite(x0) || !std::isfinite(y0) || !std::isfinite(dx) || !std::isfinite(dy)) return py::cast(none);
    const double yaw0 = std::atan2(dy, dx);
    Mat4 hint = Mat4::identity(), out = Mat4::identity();
    hint(0, 0) = std::cos(yaw0); hint(0, 1) = -std::sin(yaw0);
    hint(1, 0) = std::sin(yaw0); hint(1, 1) = std::cos(yaw0);
    hint(0, 3) = x0; hint(1, 3) = y0;
    int result = 0;
    {
        py::gil_scoped_release release;
        std::lock_guard<std::mutex> lk(g->mtx);
        result = loc_estimate_pose(*g->loc, hint, out);
    }
    double yaw, pitch, roll;
    rpy_from_transform(out, yaw, pitch, roll);
    return py::cast(std::vector<double>{out(0, 3), out(1, 3), out(2, 3), roll, pitch, -yaw, (double)result});
}
void set_destination(bool enable, std::string dest, int port) { (void)enable; if (g) { g->dest = dest; g->dest_port = port; } }
// GraphSLAM::optimize(1024) and what optimization_timer_callback does with the result (hdl_graph_slam_nodelet.cpp:634-651): the estimates, trans_odom2map
// = last.node * last.odom^-1 through a Matrix4f, and the detector's poses.  kf_mtx is held.  false: the optimisation did not run (fewer than 10 edges)
bool graph_optimize_locked(Slam* s, const char* who) {
    (void)who;
    if (!s->graph || s->graph_odom.empty()) return false;
    const int it = lio_graph_optimize(s->graph, 1024, nullptr);
    require(it >= -1, "lio_graph_optimize failed");
    const size_t n = s->graph_odom.size();
    std::vector<double> est(16 * n);
    require(lio_graph_estimates(s->graph, est.data(), (uint32_t)n) == (int)n, "lio_graph_estimates failed");
    size_t last = n;  // the last key frame still in the graph
    for (size_t k = 0; k < n; k++) {
        if (s->graph_gone[k]) continue;
        last = k;
        std::memcpy(s->graph_pose[k].m, &est[16 * k], sizeof(double) * 16);
        if (s->loop) require(lio_loop_set_pose(s->loop, (int)k, s->graph_pose[k].m) == LIO_OK, "lio_loop_set_pose failed");
    }
    if (last == n) return false;
    const Mat4 trans = mul(s->graph_pose[last], rigid_inverse(s->graph_odom[last]));
    for (int k = 0; k < 16; k++) s->odom2map.m[k] = (double)(float)trans.m[k];
    return it >= 0;
}
// map_to_pydict (py_utils.cpp:50-56): str(id) -> 4 x 4 f64
py::dict odoms_to_pydict(const std::vector<std::pair<int, Mat4>>& odoms) {
    py::dict d;
    for (const auto& o : odoms) {
        py::array_t<double> a({4, 4});
        std::memcpy(a.mutable_data(), o.second.m, sizeof(double) * 16);
        d[std::to_string(o.first).c_str()] = a;
    }
    return d;
}
uint32_t ground_seed_now();  // the seed of set_ground_extraction (below)
// the graph starts over: so do its priors' bookkeeping
void graph_prior_state_reset(Slam* s) {
    s->fix_first_node = true;
    s->floor_plane = false;
    s->floor_last_distance = 0;
    s->gnss_last[0] = s->gnss_last[1] = s->gnss_last[2] = 0;
    s->graph_has_gnss.clear();
    s->graph_gone.clear();
}
// "Release the first node" (hdl_graph_slam_nodelet.cpp:448-455, 581-588)
void release_first_node(Slam* s, const char* who) {
    if (!s->fix_first_node) return;
    s->fix_first_node = false;
    if (lio_graph_num_nodes(s->graph) > 0) require(lio_graph_set_fixed(s->graph, 0, 0) == LIO_OK, who);
}
// what flush_gps_queue (hdl_graph_slam_nodelet.cpp:398-455) does once a fix is matched to key frame `id`, for add_graph_gnss and for the flush of
// the GNSS queue alike: the distance gate against the last accepted fix (10 / 20 / 50 m by precision), the information matrices, Huber 1.0, the
// release of node 0.  `gated`: lio_gnss_queue_flush has applied the gate and marked the key frame already.  The ids of the edges added: [] when
// the gate refuses the fix, the key frame has one already or is gone, or there is no graph.  kf_mtx is held
std::vector<int> gnss_prior_locked(Slam* s, int id, const double xyz[3], const double quat[4], double precision, int dimension, bool gated, const char* who) {
    std::vector<int> added;
    if (!s->graph || id < 0 || (size_t)id >= s->graph_has_gnss.size() || s->graph_gone[(size_t)id]) return added;
    if (!gated) {
        if (s->graph_has_gnss[(size_t)id]) return added;
        const double threshold = precision < 100.0 ? 10.0 : (precision < 1000.0 ? 20.0 : 50.0);
        const double* last = s->gnss_last;
        const double d[3] = {last[0] - xyz[0], last[1] - xyz[1], last[2] - xyz[2]};
        if (std::sqrt(last[0] * last[0] + last[1] * last[1] + last[2] * last[2]) > 0 && std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < threshold) return added;
    }
    const std::string failed = std::string(who) + ": lio_graph_add_prior failed";
    double info[9] = {1.0 / precision, 0, 0, 0, 1.0 / precision, 0, 0, 0, 1.0 / precision};
    if (dimension == 2) {
        const double n2 = xyz[0] * xyz[0] + xyz[1] * xyz[1] + xyz[2] * xyz[2];
        if (gated && !(n2 > 0)) {  // (the reference divides by zero here: the fix is left out and the key frame stays open for the next one)
            s->graph_has_gnss[(size_t)id] = 0;
            return added;
        }
        require(n2 > 0, "add_graph_gnss: a 2-D fix at the origin has no information for z");
        info[8] = 1.0 / n2;  // 1 / (xyz.norm() * xyz.norm())
    }
    const double m[4] = {xyz[0], xyz[1], xyz[2], 0.0};
    int e = lio_graph_add_prior(s->graph, id, LIO_GRAPH_PRIOR_XYZ, m, nullptr, info, LIO_GRAPH_KERNEL_HUBER, 1.0);
    require(e >= 0, failed.c_str());
    added.push_back(e);
    if (dimension == 6) {
        const double r = 1.0 / (precision * 10.0);  // gps_rot_stddev
        const double rinfo[9] = {r, 0, 0, 0, r, 0, 0, 0, r};
        e = lio_graph_add_prior(s->graph, id, LIO_GRAPH_PRIOR_QUAT, quat, nullptr, rinfo, LIO_GRAPH_KERNEL_HUBER, 1.0);
        require(e >= 0, failed.c_str());
        added.push_back(e);
    }
    s->graph_has_gnss[(size_t)id] = 1;
    for (int k = 0; k < 3; k++) s->gnss_last[k] = xyz[k];
    release_first_node(s, (std::string(who) + ": lio_graph_set_fixed failed").c_str());
    return added;
}
// flush_gps_queue (hdl_graph_slam_nodelet.cpp:358-460) against the key frames the graph held BEFORE this pass (`keyframes`, not `new_keyframes`:
// optimization_timer_callback appends the new ones after the flush, :604-624): the live key frames below n_before with their stamps and fix
// flags go to lio_gnss_queue_flush, the matches become priors.  true: a prior was added.  kf_mtx is held
bool gnss_flush_locked(Slam* s, size_t n_before) {
    if (!s->gnss || !s->gnss_queue || !s->graph) return false;
    std::vector<int> ids;
    std::vector<uint64_t> stamps;
    std::vector<uint8_t> has;
    for (size_t k = 0; k < n_before && k < s->graph_gone.size(); k++)
        if (!s->graph_gone[k]) { ids.push_back((int)k); stamps.push_back(s->bank_stamp[k]); has.push_back(s->graph_has_gnss[k]); }
    if (ids.empty()) return false;
    std::vector<lio_gnss_match> matches(ids.size());
    const int n = lio_gnss_queue_flush(s->gnss_queue, stamps.data(), has.data(), (uint32_t)ids.size(), s->gnss_last, matches.data(), (uint32_t)matches.size());
    if (n == LIO_E_STATE) return false;  // fixes without an origin cannot be (the first valid fix sets it): nothing to match against
    require(n >= 0, "update_odom: lio_gnss_queue_flush failed");
    bool updated = false;
    for (int k = 0; k < n; k++) {
        const lio_gnss_match& m = matches[(size_t)k];
        const int id = ids[(size_t)m.keyframe];
        s->graph_has_gnss[(size_t)id] = 1;
        updated = !gnss_prior_locked(s, id, m.xyz, m.quat, m.precision, m.dimension, true, "update_odom").empty() || updated;
    }
    return updated;
}
// flush_floor_queue (hdl_graph_slam_nodelet.cpp:536-594) for one key frame that has just entered the graph.  The reference's floor detector is a
// thread of its own that fills floor_coeffs_queue; here the key frame's cloud as popped goes through lio_ground_detect_host (preset 1: the floor
// detector's parameters, the seed of set_ground_extraction) at this point.  The plane vertex is always fixed in the reference (:563), so the
// edge carries the world plane and the graph has no plane vertex
void floor_constraint(Slam* s, int node, const float* pts, uint64_t n, double accum) {
    if (!s->floor_ground) {
        s->floor_ground = lio_ground_create(0);
        require(s->floor_ground != nullptr, "update_odom: lio_ground_create failed");
    }
    lio_ground_params gp;
    lio_ground_default_params(&gp, 1);
    gp.seed = ground_seed_now();
    int found = 0;
    float coeffs[4];
    require(lio_ground_detect_host(s->floor_ground, pts, n, &gp, &found, coeffs, nullptr, nullptr, nullptr) == LIO_OK, "update_odom: floor detection failed");
    if (!found) return;
    if (s->floor_plane && (accum - s->floor_last_distance) < 100.0) return;
    if (!s->floor_plane) {
        const double h = s->fix_first_node ? 0.0 : s->graph_pose[(size_t)node].m[11];  // floor_height
        s->floor_world[0] = 0; s->floor_world[1] = 0; s->floor_world[2] = 1; s->floor_world[3] = -h;
        s->floor_plane = true;
    }
    s->floor_last_distance = accum;
    const double m[4] = {coeffs[0], coeffs[1], coeffs[2], coeffs[3]};
    const double info[9] = {0.1, 0, 0, 0, 0.1, 0, 0, 0, 0.1};  // Identity / floor_edge_stddev (10.0)
    require(lio_graph_add_prior(s->graph, node, LIO_GRAPH_PRIOR_PLANE, m, s->floor_world, info, LIO_GRAPH_KERNEL_HUBER, 1.0) >= 0, "update_odom: lio_graph_add_prior failed");
    release_first_node(s, "update_odom: lio_graph_set_fixed failed");
}

// update_odom (slam_wrapper.cpp:105-130): the key frames cloud_callback elected since the last call, as keyframe_to_pydict's entries (:114-125:
// points N x 4 f32 with the intensity as stored, image {}, pose 4 x 4, stamp); "odoms" stays empty without a pose graph (odom -> map is the identity)
// Lock order: kf_mtx is only ever taken with the GIL RELEASED (process() does so too).  A thread that waited for the mutex while it held the GIL
// would keep the GIL from the thread that holds the mutex and needs the GIL back: every entry below releases first, locks second, and builds its
// Python objects after the mutex is free again.
py::dict update_odom() {
    struct Popped {
        std::vector<float> pts;
        int64_t n = 0;
        Mat4 pose;
        uint64_t stamp = 0;
    };
    std::vector<Popped> popped;
    std::vector<std::pair<int, Mat4>> odoms;
    if (g && (g->keyframer || !g->injected.empty() || g->gnss)) {
        py::gil_scoped_release rel;
        std::lock_guard<std::mutex> kl(g->kf_mtx);
        bool banked = false;
        const bool graph_on = g->pose_graph && g->loop_detection;
        const size_t n_before = g->graph_odom.size();  // `keyframes` as the GNSS flush sees it
        while ((g->keyframer && lio_keyframer_pending(g->keyframer) > 0) || !g->injected.empty()) {
            popped.emplace_back();
            Popped& f = popped.back();
            double accum = 0;
            if (g->keyframer && lio_keyframer_pending(g->keyframer) > 0) {
                f.n = -lio_keyframer_pop(g->keyframer, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
                f.pts.resize((size_t)(f.n > 0 ? f.n : 1) * 4);
                require(lio_keyframer_pop(g->keyframer, f.pts.data(), (uint64_t)f.n, f.pose.m, &f.stamp, &accum, nullptr, nullptr) == f.n,
                        "update_odom: key-frame pop failed");
            } else {
                Slam::InjectedKeyFrame& in = g->injected.front();
                f.n = (int64_t)(in.pts.size() / 4);
                f.pts = std::move(in.pts);
                f.pose = in.pose; f.stamp = in.stamp; accum = in.accum;
                g->injected.pop_front();
            }
            if (graph_on) {  // flush_keyframe_queue (hdl_graph_slam_nodelet.cpp:293-334) for this key frame
                if (!g->loop) {
                    g->loop = lio_loop_create(0, &g->loop_par);
                    require(g->loop != nullptr, "update_odom: lio_loop_create failed");
                }
                if (!g->graph) {
                    g->graph = lio_graph_create(0, nullptr);
                    require(g->graph != nullptr, "update_odom: lio_graph_create failed");
                }
                const Mat4 node_pose = mul(g->odom2map, f.pose);
                // the detector searches from the graph's estimates: the frame enters the bank with its node's pose.  A frame the bank does not take
                // (fewer than k points, lio_last_warning) stays out of the graph as well: its edges' information needs the bank's cloud
                const int id = lio_loop_add_keyframe_host(g->loop, f.pts.data(), (uint32_t)f.n, node_pose.m, accum);
                require(id >= 0 || id == LIO_E_INVALID, "update_odom: lio_loop_add_keyframe_host failed");
                if (id < 0) continue;
                banked = true;
                const int node = lio_graph_add_node(g->graph, node_pose.m);
                require(node == id && (size_t)node == g->graph_odom.size(), "update_odom: lio_graph_add_node failed");
                if (node == 0) require(lio_graph_set_fixed(g->graph, 0, 1) == LIO_OK, "update_odom: lio_graph_set_fixed failed");  // fix_first_node
                g->graph_odom.push_back(f.pose);
                g->graph_pose.push_back(node_pose);
                g->graph_has_gnss.push_back(0);
                g->graph_gone.push_back(0);
                g->bank_stamp.push_back(f.stamp);
                g->bank_odom.push_back(f.pose);
                int prev = node - 1;  // keyframes.back() (hdl_graph_slam_nodelet.cpp:318): the last key frame del_graph_vertex has left in the list
                while (prev >= 0 && g->graph_gone[(size_t)prev]) prev--;
                if (prev >= 0) {  // the edge key frame -> previous: relative_pose = odom^-1 * prev.odom, the pair's information, no kernel
                    const Mat4 relp = mul(rigid_inverse(f.pose), g->graph_odom[(size_t)prev]);
                    double info[36];
                    require(lio_loop_pair_information(g->loop, node, prev, relp.m, nullptr, nullptr, info) == LIO_OK, "update_odom: lio_loop_pair_information failed");
                    require(lio_graph_add_edge(g->graph, node, prev, relp.m, info, LIO_GRAPH_KERNEL_NONE, 1.0) >= 0, "update_odom: lio_graph_add_edge failed");
                }
                if (g->ground_constraint) floor_constraint(g.get(), node, f.pts.data(), (uint64_t)f.n, accum);
            } else if (g->loop_detection) {  // the key frame joins the detector's bank (new_keyframes); one with fewer than k points is left out (lio_last_warning)
                if (!g->loop) {
                    g->loop = lio_loop_create(0, &g->loop_par);
                    require(g->loop != nullptr, "update_odom: lio_loop_create failed");
                }
                const int id = lio_loop_add_keyframe_host(g->loop, f.pts.data(), (uint32_t)f.n, f.pose.m, accum);
                require(id >= 0 || id == LIO_E_INVALID, "update_odom: lio_loop_add_keyframe_host failed");
                banked = banked || id >= 0;
                if (id >= 0) { g->bank_stamp.push_back(f.stamp); g->bank_odom.push_back(f.pose); }
            }
        }
        // flush_gps_queue after flush_keyframe_queue and the floor (optimization_timer_callback, hdl_graph_slam_nodelet.cpp:604-606)
        const bool gnss_updated = graph_on && gnss_flush_locked(g.get(), n_before);
        if (gnss_updated && !banked && graph_optimize_locked(g.get(), "update_odom")) g->graph_updated = true;
        if (banked) {  // LoopDetector::detect over the frames just queued (optimization_timer_callback, hdl_graph_slam_nodelet.cpp:588-623)
            lio_loop_edge found[8];  // (more than 8 loops in one call come back as -(count), below every error code)
            const int n_loops = lio_loop_detect(g->loop, found, 8);
            require(n_loops >= 0 || n_loops < -8, "update_odom: lio_loop_detect failed");
            const int total = -lio_loop_edges(g->loop, nullptr, 0);
            if (total > 0) {
                g->loop_edges.resize((size_t)total);
                require(lio_loop_edges(g->loop, g->loop_edges.data(), (uint32_t)total) == total, "update_odom: lio_loop_edges failed");
                g->loop_detected = true;
            }
            if (graph_on) {  // optimization_timer_callback (hdl_graph_slam_nodelet.cpp:610-651)
                for (; g->graph_loops < g->loop_edges.size(); g->graph_loops++) {  // every new loop: key1 -> key2, Huber 1.0
                    const lio_loop_edge& e = g->loop_edges[g->graph_loops];
                    Mat4 relp;
                    for (int k = 0; k < 16; k++) relp.m[k] = (double)e.relative_pose[k];
                    double info[36];
                    require(lio_loop_pair_information(g->loop, e.key1, e.key2, relp.m, nullptr, nullptr, info) == LIO_OK, "update_odom: lio_loop_pair_information failed");
                    require(lio_graph_add_edge(g->graph, e.key1, e.key2, relp.m, info, LIO_GRAPH_KERNEL_HUBER, 1.0) >= 0, "update_odom: lio_graph_add_edge failed");
                }
                if (graph_optimize_locked(g.get(), "update_odom")) g->graph_updated = true;
            }
        }
        if (g->graph_updated) {  // graph_update_odom (hdl_graph_slam_nodelet.cpp:821-833)
            for (size_t k = 0; k < g->graph_pose.size(); k++)
                if (!g->graph_gone[k]) odoms.emplace_back((int)k, g->graph_pose[k]);
            g->graph_updated = false;
        }
    }
    py::dict d;
    d["odoms"] = odoms_to_pydict(odoms);
    py::list frames;
    for (const Popped& f : popped) {
        py::array_t<float> pts({(py::ssize_t)f.n, (py::ssize_t)4});
        if (f.n > 0) std::memcpy(pts.mutable_data(), f.pts.data(), (size_t)f.n * 4 * sizeof(float));
        py::dict e;
        e["points"] = pts;
        e["image"] = py::dict();
        e["pose"] = mat4_to_numpy_f32(f.pose);
        e["stamp"] = f.stamp;
        frames.append(e);
    }
    d["keyframes"] = frames;
    return d;
}
// not in the reference's module: key frames out of process() / update_odom() in mapping mode (off by default; LSD_AMD_KEYFRAMES=1 in the
// environment at init_slam switches it on for an unchanged slam.py)
// test visibility: the f64 odometry pair (start, end of the frame) the last process() call took from the filter
py::tuple _last_odometry() {
    require((bool)g, "init_slam first");
    py::array_t<double> a({4, 4}), b({4, 4});
    std::memcpy(a.mutable_data(), g->last_odom_start.m, sizeof(double) * 16);
    std::memcpy(b.mutable_data(), g->last_odom_end.m, sizeof(double) * 16);
    return py::make_tuple(a, b);
}
void set_keyframe_output(bool enable) {
    require((bool)g, "init_slam first");
    g->keyframe_output = enable;
}
// not in the reference's module: loop detection over the key frames (off by default; LSD_AMD_LOOP=1 at init_slam switches it on for an unchanged
// slam.py).  It consumes the key frames, so it switches their output on too.
void set_loop_detection(bool enable) {
    require((bool)g, "init_slam first");
    py::gil_scoped_release rel;
    std::lock_guard<std::mutex> kl(g->kf_mtx);
    g->loop_detection = enable;
    if (enable) g->keyframe_output = true;
}
// not in the reference's module (whose global locator always runs): global relocalisation in localisation mode, off by default; LSD_AMD_RELOC=1 at
// init_slam switches it on for an unchanged slam.py.  Switched on after setup_slam, the descriptor bank is filled here
void set_global_localization(bool enable) {
    require((bool)g && (bool)g->loc, "init_slam in localisation mode first");
    py::gil_scoped_release rel;
    std::lock_guard<std::mutex> lk(g->mtx);
    g->loc->reloc = enable;
    if (enable && !g->loc->sc && g->loc->scan) require(loc_fill_sc(*g->loc), "the scan-context bank could not be filled");
}
// test visibility: what the last search of the global locator found and why it was (not) accepted
py::dict _last_relocalization() {
    py::dict d;
    if (!g || !g->loc) return d;
    std::lock_guard<std::mutex> lk(g->mtx);
    const auto& r = g->loc->last_reloc;
    d["searched"] = r.searched;
    d["match_id"] = r.match_id;
    d["score"] = r.score;
    d["yaw"] = r.yaw;
    d["converged"] = (bool)r.converged;
    d["fitness"] = r.fitness;
    d["dx"] = r.dx;
    d["da"] = r.da;
    d["accepted"] = r.accepted;
    d["searches"] = g->loc->reloc_searches;
    d["kind"] = r.local ? "local" : "global";
    d["n_examined"] = r.n_examined;
    py::array_t<double> guess({(py::ssize_t)4, (py::ssize_t)4});
    std::memcpy(guess.mutable_data(), r.guess.m, sizeof(r.guess.m));
    d["guess"] = guess;  // what registrationAlign started from
    return d;
}
// test visibility: the report of the last get_estimate_pose call, and the delta of the hand-over once it has happened
py::dict _last_estimate_pose() {
    py::dict d;
    if (!g || !g->loc) return d;
    Loc::Est e;
    {
        std::lock_guard<std::mutex> lk(g->mtx);
        e = g->loc->last_est;
    }
    auto mat = [](const double* m) {
        py::array_t<double> a({4, 4});
        std::memcpy(a.mutable_data(), m, 16 * sizeof(double));
        return a;
    };
    const lio_estimate_report& r = e.rep;
    d["called"] = e.called;
    d["rc"] = e.rc;
    d["result"] = r.result;
    d["converged"] = (bool)r.converged;
    d["iterations"] = r.iterations;
    d["score"] = r.score;
    d["pose_replaced"] = (bool)r.pose_replaced;
    d["ids"] = std::vector<int>(r.ids, r.ids + r.n_ids);
    d["n_target"] = r.n_target;
    d["n_source"] = r.n_source;
    d["z_mean_target"] = r.z_mean_target;
    d["z_mean_source"] = r.z_mean_source;
    d["hint"] = mat(e.hint.m);
    d["guess"] = mat(r.guess);
    d["out_T"] = mat(e.out.m);
    py::dict t;
    t["nearest_us"] = r.nearest_us; t["gather_us"] = r.gather_us; t["set_target_us"] = r.set_target_us; t["set_source_us"] = r.set_source_us;
    t["z_source_us"] = r.z_source_us; t["align_us"] = r.align_us; t["fitness_us"] = r.fitness_us;
    d["times"] = t;
    d["handover"] = e.handover;
    if (e.handover) {
        d["delta"] = mat(e.delta.m);
        d["delta_ran"] = e.delta_ran;
        d["delta_converged"] = (bool)e.delta_converged;
        d["delta_iterations"] = e.delta_iterations;
    }
    return d;
}
// not in the reference's module: the pose graph over the key frames and the loops (off by default; LSD_AMD_GRAPH=1 at init_slam switches it on for
// an unchanged slam.py).  It consumes the loops and the key frames, so it switches both on too.
void set_pose_graph(bool enable) {
    require((bool)g, "init_slam first");
    py::gil_scoped_release rel;
    std::lock_guard<std::mutex> kl(g->kf_mtx);
    g->pose_graph = enable;
    if (enable) { g->loop_detection = true; g->keyframe_output = true; }
}
// not in the reference's module (whose GNSS side always runs): the GNSS side of FastLIO mapping -- the map origin from the first valid fix, the
// fixes queued for the graph and flushed into priors by update_odom() -- off by default; LSD_AMD_GNSS=1 at init_slam switches it on for an
// unchanged slam.py.  RTKM needs no switch.  In localisation mode (with "RTK" among the sensors and a map that has an origin) the same switch
// lets the fix in: a valid fix starts the relocalisation near the INS position (localSearch instead of the nine-shift global search, whose
// threshold is 0.25 under the switch), the fixes around a scan's stamp are fused by the pose filter, and the state reads "Localizing(L+G)"
void set_gnss(bool enable) {
    require((bool)g, "init_slam first");
    py::gil_scoped_release rel;
    std::lock_guard<std::mutex> kl(g->kf_mtx);
    g->gnss = enable;
}
// not in the reference's module (whose mapping mode always runs the stage): the GNSS moment stage of run_robust_graph_optimization("mapping") --
// the constant offset between the antenna and the lidar frame estimated as one shared vertex, every GNSS prior moved by it -- off by default;
// LSD_AMD_GNSS_MOMENT=1 at init_slam switches it on for an unchanged slam.py.  Off: run_robust_graph_optimization answers as it always has
void set_gnss_moment(bool enable) {
    require((bool)g, "init_slam first");
    py::gil_scoped_release rel;
    std::lock_guard<std::mutex> kl(g->kf_mtx);
    g->gnss_moment = enable;
}
// test visibility: what the moment stage of the last run_robust_graph_optimization found; {} when it did not run
py::dict _last_gnss_moment() {
    py::dict d;
    if (!g) return d;
    double m[3];
    int priors;
    bool ran;
    lio_graph_report rep;
    {
        py::gil_scoped_release rel;
        std::lock_guard<std::mutex> kl(g->kf_mtx);
        ran = g->moment_ran;
        std::memcpy(m, g->moment_last, sizeof(m));
        priors = g->moment_priors;
        rep = g->moment_report;
    }
    if (!ran) return d;
    d["moment"] = std::vector<double>{m[0], m[1], m[2]};
    d["priors"] = priors;
    d["iterations"] = rep.iterations;
    d["chi2_initial"] = rep.chi2_initial;
    d["chi2_final"] = rep.chi2_final;
    return d;
}
// test visibility: what process() does with a fix (the validity filter, the origin, the method's feedInsData, FastLIO's velocity hand-over when
// there is an engine) and nothing else; the frame's timestamp is the fix's own
void _push_gnss(py::dict rtk_dict) {
    require((bool)g, "init_slam first");
    if (g->loc) {  // localisation mode: the fix's way into the localiser, when the switch is on and RTK is a sensor
        if (g->gnss && g->use_gps) (void)loc_feed_fix(g.get(), rtk_dict, rtk_dict.contains("timestamp") ? py::cast<uint64_t>(rtk_dict["timestamp"]) : 0);
        return;
    }
    Fix fix = fix_of(rtk_dict);
    feed_fix(g.get(), rtk_dict, fix, fix.f.stamp_us);
}
// test visibility: the points (N x 4 f32, INS frame) and stamps (N u32) of the last RTKM frame
py::tuple _last_merged() {
    require((bool)g && g->rtkm, "init_slam with method RTKM first");
    std::vector<float> pts;
    std::vector<uint32_t> st;
    {
        std::lock_guard<std::mutex> lk(g->mtx);
        pts = g->merged_pts;
        st = g->merged_stamps;
    }
    py::array_t<float> a({(py::ssize_t)st.size(), (py::ssize_t)4});
    py::array_t<uint32_t> b((py::ssize_t)st.size());
    if (!st.empty()) {
        std::memcpy(a.mutable_data(), pts.data(), pts.size() * sizeof(float));
        std::memcpy(b.mutable_data(), st.data(), st.size() * sizeof(uint32_t));
    }
    return py::make_tuple(a, b);
}
// test visibility: the state of the GNSS side -- fixes queued for the graph, fixes on the RTK track
py::dict _gnss_state() {
    py::dict d;
    if (!g) return d;
    int queued = 0, tracked = 0;
    {
        py::gil_scoped_release rel;
        std::lock_guard<std::mutex> kl(g->kf_mtx);
        queued = g->gnss_queue ? lio_gnss_queue_size(g->gnss_queue) : 0;
    }
    {
        std::lock_guard<std::mutex> lk(g->mtx);
        tracked = g->track ? lio_rtk_track_size(g->track) : 0;
    }
    d["enabled"] = g->gnss;
    d["origin_set"] = g->origin_set;
    d["queued"] = queued;
    d["tracked"] = tracked;
    if (g->loc) {  // localisation mode: the localiser's list of fixes, the fix held for the next search, the observation of the last located frame
        std::lock_guard<std::mutex> lk(g->mtx);
        const Loc& L = *g->loc;
        std::vector<uint64_t> stamps;
        for (const Loc::Ins& i : L.ins_data) stamps.push_back(i.f.stamp_us);
        d["stamps"] = stamps;
        d["latest_held"] = L.have_latest_ins;
        py::dict o;
        o["used"] = L.last_gps.used;
        py::array_t<double> T({(py::ssize_t)4, (py::ssize_t)4});
        std::memcpy(T.mutable_data(), L.last_gps.T.m, sizeof(L.last_gps.T.m));
        o["T"] = T;
        o["precision"] = L.last_gps.precision;
        o["dimension"] = L.last_gps.dimension;
        o["ratio"] = L.last_gps.ratio;
        d["observation"] = o;
    }
    return d;
}
// test visibility: a key frame (points N x 4 f32, odometry pose 4 x 4 f64, stamp, accumulated distance) for the next update_odom(), as if the
// front end had elected it
void _push_keyframe(py::array_t<float, py::array::c_style | py::array::forcecast> points, py::array_t<double, py::array::c_style | py::array::forcecast> pose,
                    uint64_t stamp, double accum_distance) {
    require((bool)g, "init_slam first");
    require(points.ndim() == 2 && points.shape(1) == 4 && pose.size() == 16, "_push_keyframe: points N x 4, pose 4 x 4");
    Slam::InjectedKeyFrame in;
    in.pts.assign(points.data(), points.data() + points.size());
    std::memcpy(in.pose.m, pose.data(), sizeof(double) * 16);
    in.stamp = stamp; in.accum = accum_distance;
    py::gil_scoped_release rel;
    std::lock_guard<std::mutex> kl(g->kf_mtx);
    g->injected.push_back(std::move(in));
}
// the LoopDetector's thresholds (loop_detector.hpp:42-61) by their names.  A detector that already holds key frames starts over with the new
// values: its bank is gone and frame ids begin at 0 again, so the edges found so far, which name frames of the old bank, are dropped with it
// (get_loop_edges() is empty until the new detector finds one); get_graph_status()["loop_detected"] stays as it is -- it is sticky.
void set_loop_config(py::dict cfg) {
    require((bool)g, "init_slam first");
    const char* names[] = {"distance_thresh", "accum_distance_thresh", "distance_from_last_edge_thresh", "distance_new_keyframe_thresh",
                           "distance_keyframe_thresh", "fitness_score_max_range", "fitness_score_thresh", "fine_max_corr_dist"};
    constexpr int kKeys = (int)(sizeof(names) / sizeof(names[0]));
    bool have[kKeys] = {};
    double value[kKeys] = {};
    for (auto item : cfg) {  // read with the GIL, applied below without it
        const std::string k = py::cast<std::string>(item.first);
        bool known = false;
        for (int i = 0; i < kKeys; i++)
            if (k == names[i]) { value[i] = py::cast<double>(item.second); have[i] = true; known = true; }
        require(known, "set_loop_config: unknown key");
    }
    py::gil_scoped_release rel;
    std::lock_guard<std::mutex> kl(g->kf_mtx);
    lio_loop_params& p = g->loop_par;
    double* field[kKeys] = {&p.distance_thresh, &p.accum_distance_thresh, &p.distance_from_last_edge_thresh, &p.distance_new_keyframe_thresh,
                            &p.distance_keyframe_thresh, &p.fitness_score_max_range, &p.fitness_score_thresh, &p.fine_max_corr_dist};
    for (int i = 0; i < kKeys; i++)
        if (have[i]) *field[i] = value[i];
    if (g->loop) { lio_loop_destroy(g->loop); g->loop = nullptr; }
    g->loop_edges.clear();
    // the graph's nodes are the old bank's frames: it starts over with the detector (odom -> map keeps its value)
    if (g->graph) { lio_graph_destroy(g->graph); g->graph = nullptr; }
    g->graph_odom.clear(); g->graph_pose.clear();
    g->bank_stamp.clear(); g->bank_odom.clear();
    g->graph_loops = 0;
    g->graph_updated = false;
    graph_prior_state_reset(g.get());
}
// the loop edges found so far: what the reference hands to add_se3_edge (key1 = the new frame, key2, the relative pose, the score's information matrix)
py::list get_loop_edges() {
    py::list out;
    if (!g) return out;
    std::vector<lio_loop_edge> edges;
    {
        py::gil_scoped_release rel;
        std::lock_guard<std::mutex> kl(g->kf_mtx);
        edges = g->loop_edges;
    }
    for (const lio_loop_edge& e : edges) {
        py::dict d;
        d["key1"] = e.key1;
        d["key2"] = e.key2;
        py::array_t<float> T({4, 4});
        std::memcpy(T.mutable_data(), e.relative_pose, sizeof(e.relative_pose));
        d["relative_pose"] = T;
        d["score"] = e.score;
        py::array_t<double> I({6, 6});
        std::memcpy(I.mutable_data(), e.information, sizeof(e.information));
        d["information"] = I;
        out.append(d);
    }
    return out;
}
py::dict get_graph_status() {
    py::dict d;
    d["loop_detected"] = g ? g->loop_detected.load() : false;  // graph_loop_detected: stays true after the first loop
    return d;
}
py::array_t<double> get_map_origin() {
    py::array_t<double> a({1, 7});
    auto r = a.mutable_unchecked<2>();
    for (int i = 0; i < 6; i++) r(0, i) = g ? g->origin[i] : 0.0;
    r(0, 6) = 0;
    return a;
}
void set_map_origin(double lat, double lon, double alt, double heading, double pitch, double roll) {
    if (g && !g->origin_set) {  // SLAM::setOrigin: first one wins, against the fixes of process() as well
        lio_rtk_fix f = lio_rtk_fix();
        f.latitude = lat; f.longitude = lon; f.altitude = alt; f.heading = heading; f.pitch = pitch; f.roll = roll;
        f.dimension = 2; f.precision = 100.0;
        slam_set_origin(g.get(), f);
    }
}
// ---- merge_map (slam_wrapper.cpp:174-178 -> SLAM::mergeMap -> MapLoader::mergeMapSLAM, map_loader.cpp:82-169) ----------------------------------
// g2o's text format, as far as a map's graph/graph.g2o needs it: VERTEX_SE3:QUAT id x y z qx qy qz qw; EDGE_SE3:QUAT from to x y z qx qy qz qw and
// the 21 values of the information matrix's upper triangle, row by row; FIX id ...  Every other tag is passed over and counted.
struct G2oFile {
    struct Vertex { int id; double v[7]; };
    struct Edge { int from, to; double m[7], info[36]; };
    // a unary edge of the reference's own classes (EDGE_SE3_PRIORXYZ / EDGE_SE3_PRIORQUAT): the numbers behind the vertex id as the class's write()
    // puts them -- x y z (edge_se3_priorxyz.hpp:61-67) or w x y z (edge_se3_priorquat.hpp:68-74), then the 6 values of the information's upper triangle
    struct Prior { std::string tag; int node; std::vector<double> values; };
    struct Kernel { std::vector<int> vertices; std::string type; double delta; };  // a line of graph.g2o.kernels (robust_kernel_io.cpp:72-76)
    std::vector<Vertex> vertices;
    std::vector<Edge> edges;
    std::vector<int> fixed;
    std::vector<Prior> priors;    // counted in `skipped` as before: the graph built from the file does not take them
    std::vector<Kernel> kernels;  // of <path>.kernels when that file exists
    int skipped = 0;
};
bool pose_ok(const double v[7]) {  // x y z qx qy qz qw: finite, and a quaternion that can be normalised
    for (int k = 0; k < 7; k++)
        if (!std::isfinite(v[k])) return false;
    return std::sqrt(v[3] * v[3] + v[4] * v[4] + v[5] * v[5] + v[6] * v[6]) > 1e-9;
}
bool read_g2o(const std::string& path, G2oFile& out, std::string& err) {
    std::ifstream f(path);
    if (!f) { err = "cannot open " + path; return false; }
    std::string line;
    int ln = 0;
    while (std::getline(f, line)) {
        ln++;
        std::istringstream ls(line);
        std::string tag;
        if (!(ls >> tag) || tag[0] == '#') continue;
        if (tag == "VERTEX_SE3:QUAT") {
            G2oFile::Vertex v;
            bool ok = (bool)(ls >> v.id);
            for (int k = 0; k < 7 && ok; k++) ok = (bool)(ls >> v.v[k]);
            if (!ok) { err = path + ":" + std::to_string(ln) + ": truncated VERTEX_SE3:QUAT"; return false; }
            if (!pose_ok(v.v)) { err = path + ":" + std::to_string(ln) + ": a VERTEX_SE3:QUAT that is not finite or has a null quaternion"; return false; }
            out.vertices.push_back(v);
        } else if (tag == "EDGE_SE3:QUAT") {
            G2oFile::Edge e;
            bool ok = (bool)(ls >> e.from >> e.to);
            for (int k = 0; k < 7 && ok; k++) ok = (bool)(ls >> e.m[k]);
            for (int r = 0; r < 6 && ok; r++)
                for (int c = r; c < 6 && ok; c++) { ok = (bool)(ls >> e.info[r * 6 + c]); e.info[c * 6 + r] = e.info[r * 6 + c]; }
            if (!ok) { err = path + ":" + std::to_string(ln) + ": truncated EDGE_SE3:QUAT"; return false; }
            for (int k = 0; k < 36 && ok; k++) ok = std::isfinite(e.info[k]);
            if (!ok || !pose_ok(e.m)) { err = path + ":" + std::to_string(ln) + ": an EDGE_SE3:QUAT that is not finite or has a null quaternion"; return false; }
            out.edges.push_back(e);
        } else if (tag == "FIX") {
            int id, n = 0;
            while (ls >> id) { out.fixed.push_back(id); n++; }
            if (!n) { err = path + ":" + std::to_string(ln) + ": truncated FIX"; return false; }
        } else {
            out.skipped++;
            if (tag == "EDGE_SE3_PRIORXYZ" || tag == "EDGE_SE3_PRIORQUAT") {  // kept for the writer's sake, passed over all the same
                G2oFile::Prior p;
                p.tag = tag;
                double v;
                if (ls >> p.node) {
                    while (ls >> v) p.values.push_back(v);
                    out.priors.push_back(p);
                }
            }
        }
    }
    std::ifstream kf(path + ".kernels");
    while (kf && std::getline(kf, line)) {
        std::istringstream ls(line);
        size_t nv = 0;
        G2oFile::Kernel k;
        if (!(ls >> nv) || nv > 8) continue;
        k.vertices.resize(nv);
        bool ok = true;
        for (size_t i = 0; i < nv && ok; i++) ok = (bool)(ls >> k.vertices[i]);
        if (ok && (ls >> k.type >> k.delta)) out.kernels.push_back(k);
    }
    return true;
}
Mat4 mat_from_tq(const double v[7]) {  // x y z qx qy qz qw -> the pose, the quaternion normalised
    const double n = std::sqrt(v[3] * v[3] + v[4] * v[4] + v[5] * v[5] + v[6] * v[6]);
    const double x = v[3] / n, y = v[4] / n, z = v[5] / n, w = v[6] / n;
    Mat4 T = Mat4::identity();
    T(0, 0) = 1 - 2 * (y * y + z * z); T(0, 1) = 2 * (x * y - z * w); T(0, 2) = 2 * (x * z + y * w);
    T(1, 0) = 2 * (x * y + z * w); T(1, 1) = 1 - 2 * (x * x + z * z); T(1, 2) = 2 * (y * z - x * w);
    T(2, 0) = 2 * (x * z - y * w); T(2, 1) = 2 * (y * z + x * w); T(2, 2) = 1 - 2 * (x * x + y * y);
    T(0, 3) = v[0]; T(1, 3) = v[1]; T(2, 3) = v[2];
    return T;
}
// test visibility: _read_g2o(path) -> {vertices: {id: [x y z qx qy qz qw]}, edges: [(from, to, [7], 6 x 6)], fixed: [ids], skipped: tags passed over,
// priors: [(tag, vertex, values)] of the passed-over tags that are GNSS priors, kernels: [([vertices], type, delta)] of <path>.kernels}
py::dict _read_g2o(std::string path) {
    G2oFile gf;
    std::string err;
    if (!read_g2o(path, gf, err)) throw std::runtime_error("slam_wrapper: _read_g2o: " + err);
    py::dict d, vs;
    for (const auto& v : gf.vertices) vs[py::int_(v.id)] = py::array_t<double>(7, v.v);
    py::list es;
    for (const auto& e : gf.edges) {
        py::array_t<double> info({6, 6});
        std::memcpy(info.mutable_data(), e.info, sizeof(e.info));
        es.append(py::make_tuple(e.from, e.to, py::array_t<double>(7, e.m), info));
    }
    d["vertices"] = vs;
    d["edges"] = es;
    d["fixed"] = py::cast(gf.fixed);
    d["skipped"] = gf.skipped;
    py::list ps, ks;
    for (const auto& pr : gf.priors) ps.append(py::make_tuple(pr.tag, pr.node, py::array_t<double>((py::ssize_t)pr.values.size(), pr.values.data())));
    for (const auto& k : gf.kernels) ks.append(py::make_tuple(py::cast(k.vertices), k.type, k.delta));
    d["priors"] = ps;
    d["kernels"] = ks;
    return d;
}

namespace {
void to_map_frame(KeyFrameDisk& kf) {  // KeyFrame::transformPoints at the frame's pose (load_keyframes' loop)
    kf.xyzi = kf.local;
    const size_t n = kf.xyzi.size() / 4;
    for (size_t i = 0; i < n; i++) {
        const double x = kf.local[4 * i], y = kf.local[4 * i + 1], z = kf.local[4 * i + 2];
        for (int r = 0; r < 3; r++) kf.xyzi[4 * i + r] = (float)(kf.odom(r, 0) * x + kf.odom(r, 1) * y + kf.odom(r, 2) * z + kf.odom(r, 3));
    }
}
py::dict keyframes_to_pydict(const std::vector<KeyFrameDisk>& frames, size_t first) {  // keyframe_to_pydict (py_utils.cpp:272-293)
    py::dict d, points, images, poses, stamps;
    for (size_t k = first; k < frames.size(); k++) {
        const KeyFrameDisk& kf = frames[k];
        const std::string id = std::to_string(kf.id);
        const py::ssize_t n = (py::ssize_t)(kf.local.size() / 4);
        py::array_t<float> a({n, (py::ssize_t)4});
        if (n) std::memcpy(a.mutable_data(), kf.local.data(), kf.local.size() * sizeof(float));
        points[id.c_str()] = a;
        poses[id.c_str()] = mat4_to_numpy_f32(kf.odom);
        stamps[id.c_str()] = kf.stamp;
        images[id.c_str()] = py::dict();
    }
    d["points"] = points;
    d["images"] = images;
    d["poses"] = poses;
    d["stamps"] = stamps;
    return d;
}
// graph_load_impl (hdl_graph_slam_nodelet.cpp:1112-1148) of one map's file into the record: vertices without a key frame are dropped with their
// edges; `id_of`: file id -> key-frame id of the frames that exist
void record_take_file(std::vector<Loc::MergeEdge>& edges, std::set<int>& fixed, const G2oFile& gf, const std::map<int, int>& id_of) {
    for (int id : gf.fixed) {
        auto it = id_of.find(id);
        if (it != id_of.end()) fixed.insert(it->second);
    }
    for (const auto& e : gf.edges) {
        auto a = id_of.find(e.from), b = id_of.find(e.to);
        if (a == id_of.end() || b == id_of.end()) continue;
        Loc::MergeEdge me;
        me.a = a->second; me.b = b->second;
        me.kernel = LIO_GRAPH_KERNEL_NONE;  // (the text format carries no robust kernel: none)
        const Mat4 M = mat_from_tq(e.m);
        std::memcpy(me.M, M.m, sizeof(me.M));
        std::memcpy(me.info, e.info, sizeof(me.info));
        edges.push_back(me);
    }
}
// the GNSS priors of one map's file into the record (set_gnss): EDGE_SE3_PRIORXYZ = x y z + the information's upper triangle, EDGE_SE3_PRIORQUAT =
// w x y z + the same; a line of <file>.kernels that names the prior's vertex alone gives its kernel (one such line serves every prior of that
// vertex: the mapping side puts Huber 1.0 on both).  A prior on a vertex without a key frame, or one that is not complete, is passed over.
// Returns the number taken
int record_take_priors(std::vector<Loc::MergePrior>& priors, const G2oFile& gf, const std::map<int, int>& id_of) {
    int taken = 0;
    for (const auto& p : gf.priors) {
        auto it = id_of.find(p.node);
        const bool xyz = p.tag == "EDGE_SE3_PRIORXYZ";
        if (it == id_of.end() || p.values.size() != (xyz ? 9u : 10u)) continue;
        Loc::MergePrior mp;
        mp.kf = it->second;
        mp.type = xyz ? LIO_GRAPH_PRIOR_XYZ : LIO_GRAPH_PRIOR_QUAT;
        if (xyz) { mp.m[0] = p.values[0]; mp.m[1] = p.values[1]; mp.m[2] = p.values[2]; mp.m[3] = 0.0; }
        else { mp.m[0] = p.values[1]; mp.m[1] = p.values[2]; mp.m[2] = p.values[3]; mp.m[3] = p.values[0]; }
        const double* u = p.values.data() + (xyz ? 3 : 4);
        int at = 0;
        for (int r = 0; r < 3; r++)
            for (int c = r; c < 3; c++) { mp.info[r * 3 + c] = u[at]; mp.info[c * 3 + r] = u[at]; at++; }
        mp.kernel = LIO_GRAPH_KERNEL_NONE;
        mp.delta = 1.0;
        for (const auto& k : gf.kernels)
            if (k.vertices.size() == 1 && k.vertices[0] == p.node && k.delta > 0) {
                mp.kernel = k.type == "Huber" ? LIO_GRAPH_KERNEL_HUBER : k.type == "DCS2" ? LIO_GRAPH_KERNEL_DCS2 : LIO_GRAPH_KERNEL_NONE;
                mp.delta = k.delta;
                break;
            }
        priors.push_back(mp);
        taken++;
    }
    return taken;
}
void graph_add(lio_graph* gr, const std::map<int, int>& node_of_kf, const Loc::MergeEdge& e) {
    require(lio_graph_add_edge(gr, node_of_kf.at(e.a), node_of_kf.at(e.b), e.M, e.info, e.kernel, 1.0) >= 0, "merge_map: lio_graph_add_edge failed");
}
int bank_frame(Loc& L, const KeyFrameDisk& kf) {  // a frame of fewer than k points cannot be matched: it stays out of the bank (and of the detection)
    if (kf.local.size() / 4 < (size_t)20) return -1;
    const int id = lio_loop_add_keyframe_host(L.mbank, kf.local.data(), (uint32_t)(kf.local.size() / 4), kf.odom.m, 0.0);
    require(id >= 0, "merge_map: lio_loop_add_keyframe_host failed");
    L.bank_of_kf[kf.id] = id;
    return id;
}
void drop_bank(Loc& L) {
    if (L.moverlap) lio_overlap_destroy(L.moverlap);
    if (L.mbank) lio_loop_destroy(L.mbank);
    L.moverlap = nullptr;
    L.mbank = nullptr;
    L.bank_of_kf.clear();
}
// graph_optimize + graph_sync_pose(FROM_GRAPH) for every frame in `lists`, and the bank's poses
void optimize_and_sync(Loc& L, lio_graph* gr, const std::map<int, int>& node_of_kf, std::initializer_list<std::vector<KeyFrameDisk>*> lists) {
    const int it = lio_graph_optimize(gr, 1024, nullptr);
    require(it >= -1, "merge_map: lio_graph_optimize failed");
    const int n = lio_graph_num_nodes(gr);
    std::vector<double> est(16 * (size_t)n);
    require(lio_graph_estimates(gr, est.data(), (uint32_t)n) == n, "merge_map: lio_graph_estimates failed");
    for (auto* frames : lists)
        for (KeyFrameDisk& kf : *frames) {
            auto node = node_of_kf.find(kf.id);
            if (node == node_of_kf.end()) continue;
            std::memcpy(kf.odom.m, &est[16 * (size_t)node->second], sizeof(kf.odom.m));
            auto b = L.bank_of_kf.find(kf.id);
            if (b != L.bank_of_kf.end()) require(lio_loop_set_pose(L.mbank, b->second, kf.odom.m) == LIO_OK, "merge_map: lio_loop_set_pose failed");
        }
}
struct MergeInput {
    std::vector<KeyFrameDisk> fresh;
    G2oFile ref_g2o, new_g2o;
    bool reanchor = false;  // set_gnss and origins that differ: the new map goes under the loaded map's origin (`from` -> `to`)
    lio_rtk_fix from = lio_rtk_fix(), to = lio_rtk_fix();
};
// the merge itself, under the lock of process() and without the GIL.  It works on its own copies -- the record of the graph, a device graph of
// its own, the report -- and changes the key-frame list's poses and the bank as it goes; the caller undoes those when it throws
void merge_locked(Slam* s, MergeInput& in, std::vector<Loc::MergeEdge>& edges, std::vector<Loc::MergePrior>& priors, std::set<int>& fixed, Loc::MergeReport& report) {
    Loc& L = *s->loc;
    std::vector<KeyFrameDisk>& fresh = in.fresh;
    uint32_t biggest = 1024;
    for (const KeyFrameDisk& kf : L.frames) biggest = std::max<uint32_t>(biggest, (uint32_t)(kf.local.size() / 4));
    for (const KeyFrameDisk& kf : fresh) biggest = std::max<uint32_t>(biggest, (uint32_t)(kf.local.size() / 4));
    if (L.mbank && biggest > L.bank_max_points) drop_bank(L);  // a larger frame than the bank was made for: the bank is made again
    if (!L.have_mgraph) {
        std::map<int, int> same;
        for (const KeyFrameDisk& kf : L.frames) same[kf.id] = kf.id;
        record_take_file(edges, fixed, in.ref_g2o, same);
        report.skipped_tags = in.ref_g2o.skipped;
        if (s->gnss) report.skipped_tags -= record_take_priors(priors, in.ref_g2o, same);  // (taken, not passed over)
    }
    // graph_merge (hdl_graph_slam_nodelet.cpp:1222-1336): new vertex ids max + 1 ... in key-frame order, the new edges behind the graph's
    int max_id = 0;
    for (const KeyFrameDisk& kf : L.frames) max_id = std::max(max_id, kf.id);
    std::map<int, int> renamed;
    for (KeyFrameDisk& kf : fresh) { renamed[kf.id] = ++max_id; kf.id = max_id; }
    record_take_file(edges, fixed, in.new_g2o, renamed);
    report.skipped_tags += in.new_g2o.skipped;
    const size_t first_new_prior = priors.size();
    if (s->gnss) report.skipped_tags -= record_take_priors(priors, in.new_g2o, renamed);
    if (in.reanchor) {
        // graph_update_origin (hdl_graph_slam_nodelet.cpp:1396-1449, map_loader.cpp:104-112): the new map's poses (its vertex estimates: a node's
        // estimate is its key frame's pose) and the measurements of its EDGE_SE3_PRIORXYZ edges go under the loaded map's origin
        std::vector<double> poses(16 * fresh.size()), xyz;
        for (size_t k = 0; k < fresh.size(); k++) std::memcpy(&poses[16 * k], fresh[k].odom.m, 16 * sizeof(double));
        for (size_t k = first_new_prior; k < priors.size(); k++)
            if (priors[k].type == LIO_GRAPH_PRIOR_XYZ) xyz.insert(xyz.end(), priors[k].m, priors[k].m + 3);
        require(lio_update_origin(&in.from, &in.to, poses.data(), (uint32_t)fresh.size(), xyz.data(), (uint32_t)(xyz.size() / 3)) == LIO_OK, "merge_map: lio_update_origin failed");
        for (size_t k = 0; k < fresh.size(); k++) std::memcpy(fresh[k].odom.m, &poses[16 * k], 16 * sizeof(double));
        size_t at = 0;
        for (size_t k = first_new_prior; k < priors.size(); k++)
            if (priors[k].type == LIO_GRAPH_PRIOR_XYZ) { std::memcpy(priors[k].m, &xyz[at], 3 * sizeof(double)); at += 3; }
        report.origin_updated = true;
    }
    report.priors = (int)priors.size();
    // the device graph of this call: node estimates are the key frames' odom
    struct Graph { lio_graph* h = nullptr; ~Graph() { if (h) lio_graph_destroy(h); } } gr;
    gr.h = lio_graph_create(0, nullptr);
    require(gr.h != nullptr, "merge_map: lio_graph_create failed");
    std::map<int, int> node_of_kf;
    for (const std::vector<KeyFrameDisk>* frames : std::initializer_list<const std::vector<KeyFrameDisk>*>{&L.frames, &fresh})
        for (const KeyFrameDisk& kf : *frames) {
            const int node = lio_graph_add_node(gr.h, kf.odom.m);
            require(node >= 0, "merge_map: lio_graph_add_node failed");
            node_of_kf[kf.id] = node;
        }
    for (int id : fixed) require(lio_graph_set_fixed(gr.h, node_of_kf.at(id), 1) == LIO_OK, "merge_map: lio_graph_set_fixed failed");
    for (const Loc::MergeEdge& e : edges) graph_add(gr.h, node_of_kf, e);
    for (const Loc::MergePrior& p : priors)
        require(lio_graph_add_prior(gr.h, node_of_kf.at(p.kf), p.type, p.m, nullptr, p.info, p.kernel, p.delta) >= 0, "merge_map: lio_graph_add_prior failed");
    if (in.reanchor) optimize_and_sync(L, gr.h, node_of_kf, {&L.frames, &fresh});  // the graph_optimize at the end of graph_update_origin + the sync (map_loader.cpp:111)
    if (!L.mbank) {
        lio_loop_params lp;
        lio_loop_default_params(&lp);
        lp.max_points = biggest;
        L.bank_max_points = biggest;
        L.mbank = lio_loop_create(0, &lp);
        require(L.mbank != nullptr, "merge_map: lio_loop_create failed");
        L.moverlap = lio_overlap_create(L.mbank, nullptr);
        require(L.moverlap != nullptr, "merge_map: lio_overlap_create failed");
        for (const KeyFrameDisk& kf : L.frames) bank_frame(L, kf);
    }
    for (const KeyFrameDisk& kf : fresh) bank_frame(L, kf);
    std::vector<int32_t> ref_bank, ref_kf;
    for (const KeyFrameDisk& kf : L.frames) {
        auto b = L.bank_of_kf.find(kf.id);
        if (b != L.bank_of_kf.end()) { ref_bank.push_back(b->second); ref_kf.push_back(kf.id); }
    }
    std::map<int, int> kf_of_bank;
    for (const auto& kv : L.bank_of_kf) kf_of_bank[kv.second] = kv.first;
    // fragments of 10 (map_loader.cpp:119-137)
    const int fragment = 10, fragment_num = (int)(fresh.size() / fragment) + 1;
    report.fragments = fragment_num;
    for (int i = 0; i < fragment_num; i++) {
        const size_t b0 = (size_t)i * fragment, b1 = std::min<size_t>((size_t)(i + 1) * fragment, fresh.size());
        std::vector<int32_t> new_bank, new_kf, ea, eb;
        for (size_t k = b0; k < b1; k++) {
            auto b = L.bank_of_kf.find(fresh[k].id);
            if (b != L.bank_of_kf.end()) { new_bank.push_back(b->second); new_kf.push_back(fresh[k].id); }
        }
        for (const Loc::MergeEdge& e : edges) { ea.push_back(e.a); eb.push_back(e.b); }  // graph_get_edges, in key-frame ids
        std::vector<lio_overlap_edge> found(std::max<size_t>(new_bank.size(), 1));
        const int nf = lio_overlap_detect(L.moverlap, ref_bank.data(), ref_kf.data(), (uint32_t)ref_bank.size(), new_bank.data(), new_kf.data(), (uint32_t)new_bank.size(),
                                          ea.data(), eb.data(), (uint32_t)ea.size(), found.data(), (uint32_t)found.size());
        require(nf >= 0, "merge_map: lio_overlap_detect failed");
        for (size_t k = 0; k < new_bank.size(); k++) {
            lio_overlap_report rep;
            lio_overlap_last_report(L.moverlap, (uint32_t)k, &rep, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
            report.new_ids.push_back(new_kf[k]);
            report.reasons.push_back(rep.reason);
        }
        for (int k = 0; k < nf; k++) {  // graph_add_edge (hdl_graph_slam_nodelet.cpp:893-912): key1 -> key2, information(score), Huber 1.0
            Loc::MergeEdge me;
            me.a = kf_of_bank[found[k].key1]; me.b = kf_of_bank[found[k].key2];
            me.kernel = LIO_GRAPH_KERNEL_HUBER;
            for (int a = 0; a < 16; a++) me.M[a] = (double)found[k].relative_pose[a];
            std::memcpy(me.info, found[k].information, sizeof(me.info));
            graph_add(gr.h, node_of_kf, me);
            edges.push_back(me);
            report.overlaps.push_back({me.a, me.b});
            report.scores.push_back(found[k].score);
        }
        optimize_and_sync(L, gr.h, node_of_kf, {&L.frames, &fresh});
    }
    optimize_and_sync(L, gr.h, node_of_kf, {&L.frames, &fresh});  // OptimizeMap (map_loader.cpp:162)
    // the localiser's matcher must hold the merged map's biggest frame (the resident map itself is made again at the commit)
    uint32_t big_map = 0;
    for (const std::vector<KeyFrameDisk>* frames : std::initializer_list<const std::vector<KeyFrameDisk>*>{&L.frames, &fresh})
        for (const KeyFrameDisk& kf : *frames) big_map = std::max<uint32_t>(big_map, (uint32_t)(kf.local.size() / 4));
    if (L.ndt && big_map > L.ndt_biggest) {  // the matcher's target was sized for the loaded map's biggest frame
        lio_ndt* ndt = lio_ndt_create(0, 1.0f, 7, 200000ull + big_map + 1024, 400000, 262144);
        require(ndt != nullptr, "merge_map: lio_ndt_create failed");
        lio_ndt_destroy(L.ndt);
        L.ndt = ndt;
        L.ndt_biggest = big_map;
        L.have_map = false;
    }
}
py::dict merge_refused(const char* why) {
    std::fprintf(stderr, "slam_wrapper: merge_map: fail to merge map: %s\n", why);
    return py::dict();
}
}  // namespace

py::dict merge_map(const std::string& directory) {
    if (!g || !g->loc) return merge_refused("not in localisation mode");
    Slam* s = g.get();
    Loc& L = *s->loc;
    // process() localises under this lock with the GIL released; the merge holds it from its first look at the key-frame list to its last write
    std::lock_guard<std::mutex> lk(s->mtx);
    if (L.frames.empty()) return merge_refused("no map is loaded");
    // everything that can refuse the merge comes before any state is touched
    MapInfo ref_info, new_info;
    if (!read_map_info(s->map_path, ref_info) || !read_map_info(directory, new_info)) return merge_refused("graph/map_info.txt is missing");
    MergeInput in;
    if (!load_keyframes(directory, in.fresh)) return merge_refused("the new map has no key frames");
    std::string err;
    if (!L.have_mgraph && !read_g2o(s->map_path + "/graph/graph.g2o", in.ref_g2o, err)) return merge_refused(err.c_str());
    if (!read_g2o(directory + "/graph/graph.g2o", in.new_g2o, err)) return merge_refused(err.c_str());
    if (ref_info.coordinate != new_info.coordinate) return merge_refused("coordinate system is not consistent");
    if (!ref_info.origin_set || !new_info.origin_set) return merge_refused("a map without an origin needs global_alignment, which is not built");
    // map_loader.cpp:104-112: origins that differ (any of latitude, longitude, altitude by more than 1e-6) put the new map under the loaded map's
    // origin first -- behind set_gnss; without the switch such a pair is refused as it always was
    for (int i = 0; i < 3; i++)
        if (std::fabs(ref_info.origin[i] - new_info.origin[i]) > 1e-6) in.reanchor = true;
    if (in.reanchor && !s->gnss) return merge_refused("the origins differ: set_gnss(True) puts the new map under the loaded map's origin");
    if (in.reanchor) {
        in.from.latitude = new_info.origin[0]; in.from.longitude = new_info.origin[1]; in.from.altitude = new_info.origin[2];
        in.to.latitude = ref_info.origin[0]; in.to.longitude = ref_info.origin[1]; in.to.altitude = ref_info.origin[2];
    }
    auto vertex_ids = [](const G2oFile& gf) { std::set<int> v; for (const auto& x : gf.vertices) v.insert(x.id); return v; };
    const std::set<int> new_vertices = vertex_ids(in.new_g2o);
    for (const KeyFrameDisk& kf : in.fresh)
        if (!new_vertices.count(kf.id)) return merge_refused("a key frame of the new map has no vertex in graph.g2o");
    if (!L.have_mgraph) {
        const std::set<int> ref_vertices = vertex_ids(in.ref_g2o);
        for (const KeyFrameDisk& kf : L.frames)
            if (!ref_vertices.count(kf.id)) return merge_refused("a key frame of the loaded map has no vertex in graph.g2o");
    }
    if (lio_device_count() < 1) return merge_refused("no HIP device");
    // the work: on copies of the graph's record and of the report; what it changes in place (the poses of the list, the bank) is undone if it fails
    std::vector<Loc::MergeEdge> edges = L.medges;
    std::set<int> fixed = L.mfixed;
    std::vector<Loc::MergePrior> priors = L.mpriors;
    Loc::MergeReport report;
    std::vector<Mat4> saved;
    for (const KeyFrameDisk& kf : L.frames) saved.push_back(kf.odom);
    std::string failure;
    size_t first_new = L.frames.size();
    {
        py::gil_scoped_release release;
        try {
            merge_locked(s, in, edges, priors, fixed, report);
            // commit: the record, the key frames (map_loader.cpp:140), their map-frame clouds, the resident map
            L.medges.swap(edges);
            L.mpriors.swap(priors);
            L.mfixed.swap(fixed);
            L.have_mgraph = true;
            L.merge_report = report;
            for (KeyFrameDisk& kf : in.fresh) L.frames.push_back(std::move(kf));
            for (KeyFrameDisk& kf : L.frames) to_map_frame(kf);
            if (L.lm) {
                if (!loc_refill_local_map(L)) { L.initialized = false; L.have_map = false; }  // (no room for the merged map: the next initialisation tries again)
                else if (L.initialized) loc_update_local_map(L, L.last_odom);
            }
        } catch (const std::exception& e) {
            failure = e.what();
            for (size_t k = 0; k < saved.size(); k++) L.frames[k].odom = saved[k];
            drop_bank(L);  // (it holds the new map's frames and moved poses: made again by the next merge)
        }
    }
    if (!failure.empty()) throw std::runtime_error(failure);
    s->odometrys.emplace_back((uint64_t)0, Mat4::identity());  // "add a zero odometry as spliter", then the new map's list (map_loader.cpp:141-142)
    read_odometrys(directory, s->odometrys);
    std::fprintf(stderr, "slam_wrapper: merge_map: merge success, total %zu key frames, %zu overlaps\n", L.frames.size(), L.merge_report.overlaps.size());
    return keyframes_to_pydict(L.frames, first_new);
}
// test visibility: what the last merge_map did -- overlaps [(key1, key2, score)] in key-frame ids, the reason per matched new frame, fragments
py::dict _last_merge() {
    py::dict d;
    if (!g || !g->loc) return d;
    const auto& r = g->loc->merge_report;
    py::list ov, reasons;
    for (size_t k = 0; k < r.overlaps.size(); k++) ov.append(py::make_tuple(r.overlaps[k][0], r.overlaps[k][1], r.scores[k]));
    for (size_t k = 0; k < r.new_ids.size(); k++) reasons.append(py::make_tuple(r.new_ids[k], r.reasons[k]));
    d["overlaps"] = ov;
    d["reasons"] = reasons;
    d["fragments"] = r.fragments;
    d["skipped_tags"] = r.skipped_tags;
    d["origin_updated"] = r.origin_updated;
    d["priors"] = r.priors;
    return d;
}
// get_graph_map (slam_wrapper.cpp:180-184 -> keyframe_to_pydict, py_utils.cpp:272-293): the key frames of the loaded map in localisation mode
// (points N x 4 f32 as stored, pose 4 x 4 f32, stamp).  In mapping mode the key frames update_odom has handed out and del_graph_vertex has not
// taken back, in the same shape: the cloud as it was handed out (downloaded from the loop detector's bank, which holds every key frame in its
// own order), the pose the graph's estimate (the odometry pose without a graph), the stamp; four empty dictionaries with no key frame -- nothing
// is kept without a bank
py::dict get_graph_map() {
    py::dict d;
    py::dict points, images, poses, stamps;
    if (g && !g->loc) {
        struct Out { int id; std::vector<float> pts; Mat4 pose; uint64_t stamp; };
        std::vector<Out> frames;
        {
            py::gil_scoped_release rel;
            std::lock_guard<std::mutex> kl(g->kf_mtx);
            for (size_t k = 0; g->loop && k < g->bank_stamp.size(); k++) {
                const bool in_graph = g->graph && k < g->graph_pose.size();
                if (in_graph && g->graph_gone[k]) continue;
                Out o;
                o.id = (int)k;
                const int n = -lio_loop_download_keyframe(g->loop, (int)k, nullptr, nullptr, 0);
                require(n > 0, "get_graph_map: lio_loop_download_keyframe failed");
                o.pts.resize(4 * (size_t)n);
                require(lio_loop_download_keyframe(g->loop, (int)k, o.pts.data(), nullptr, (uint32_t)n) == n, "get_graph_map: lio_loop_download_keyframe failed");
                o.pose = in_graph ? g->graph_pose[k] : g->bank_odom[k];
                o.stamp = g->bank_stamp[k];
                frames.push_back(std::move(o));
            }
        }
        for (const Out& o : frames) {
            const std::string id = std::to_string(o.id);
            py::array_t<float> a({(py::ssize_t)(o.pts.size() / 4), (py::ssize_t)4});
            std::memcpy(a.mutable_data(), o.pts.data(), o.pts.size() * sizeof(float));
            points[id.c_str()] = a;
            poses[id.c_str()] = mat4_to_numpy_f32(o.pose);
            stamps[id.c_str()] = o.stamp;
            images[id.c_str()] = py::dict();
        }
        d["points"] = points;
        d["images"] = images;
        d["poses"] = poses;
        d["stamps"] = stamps;
        return d;
    }
    static const std::vector<KeyFrameDisk> none;
    for (const KeyFrameDisk& kf : (g && g->loc) ? g->loc->frames : none) {
        const std::string id = std::to_string(kf.id);
        const py::ssize_t n = (py::ssize_t)(kf.local.size() / 4);
        py::array_t<float> a({n, (py::ssize_t)4});
        auto r = a.mutable_unchecked<2>();
        for (py::ssize_t i = 0; i < n; i++) { r(i, 0) = kf.local[4 * i]; r(i, 1) = kf.local[4 * i + 1]; r(i, 2) = kf.local[4 * i + 2]; r(i, 3) = kf.local[4 * i + 3]; }
        points[id.c_str()] = a;
        poses[id.c_str()] = mat4_to_numpy_f32(kf.odom);
        stamps[id.c_str()] = kf.stamp;
        images[id.c_str()] = py::dict();
    }
    d["points"] = points;
    d["images"] = images;
    d["poses"] = poses;
    d["stamps"] = stamps;
    return d;
}
// get_color_map (slam_wrapper.cpp -> SLAM::getColorMap -> MapRender::getColorMap): N x 4 (x, y, z, r << 16 | g << 8 | b as f32 bits)
py::array_t<float> get_color_map() {
    std::vector<float> pts;
    if (g) {
        std::lock_guard<std::mutex> lk(g->mtx);
        pts = colour_map_points(g->painter);
    }
    if (pts.empty()) return py::array_t<float>(std::vector<py::ssize_t>{0, 6});
    py::array_t<float> a({(py::ssize_t)(pts.size() / 4), (py::ssize_t)4});
    std::memcpy(a.mutable_data(), pts.data(), pts.size() * sizeof(float));
    return a;
}
// the graph's live edges (graph_get_edges, hdl_graph_slam_nodelet.cpp:842-860; vector_to_pydict, py_utils.cpp:29-48): str(id) -> [prev, next]; {} without a graph
namespace {
struct GraphEdges { std::vector<int32_t> from, to, id; std::vector<uint8_t> fixed, live; };
GraphEdges graph_edges_snapshot() {
    GraphEdges e;
    if (!g) return e;
    py::gil_scoped_release rel;
    std::lock_guard<std::mutex> kl(g->kf_mtx);
    if (!g->graph) return e;
    const int n = -lio_graph_edges(g->graph, nullptr, nullptr, nullptr, 0);
    if (n > 0) {
        e.from.resize(n); e.to.resize(n); e.id.resize(n);
        require(lio_graph_edges(g->graph, e.from.data(), e.to.data(), e.id.data(), (uint32_t)n) == n, "lio_graph_edges failed");
        size_t k = 0;  // EdgeSE3 only (hdl_graph_slam_nodelet.cpp:849): a prior (to = -1) is not listed
        for (int i = 0; i < n; i++)
            if (e.to[i] >= 0) { e.from[k] = e.from[i]; e.to[k] = e.to[i]; e.id[k] = e.id[i]; k++; }
        e.from.resize(k); e.to.resize(k); e.id.resize(k);
    }
    const int nn = lio_graph_num_nodes(g->graph);
    if (nn > 0) {
        e.fixed.resize(nn);
        e.live.resize(nn);
        require(lio_graph_get_fixed(g->graph, e.fixed.data(), (uint32_t)nn) == nn, "lio_graph_get_fixed failed");
        require(lio_graph_node_live(g->graph, e.live.data(), (uint32_t)nn) == nn, "lio_graph_node_live failed");
    }
    return e;
}
}  // namespace
py::dict get_graph_edges() {
    const GraphEdges e = graph_edges_snapshot();
    py::dict d;
    for (size_t k = 0; k < e.id.size(); k++) d[std::to_string(e.id[k]).c_str()] = py::cast(std::vector<int>{e.from[k], e.to[k]});
    return d;
}
// graph_get_info's shape (graph_utils.cpp:70-90): vertex str(id) -> {fix, edge_num}, edge str(id) -> {vertex_num}, and -- this module's
// addition -- the edge's ends as prev / next; {} without a graph
py::dict get_graph_meta() {
    const GraphEdges e = graph_edges_snapshot();
    if (e.fixed.empty()) return py::dict();
    std::vector<int> deg(e.fixed.size(), 0);
    for (size_t k = 0; k < e.id.size(); k++) { deg[e.from[k]]++; deg[e.to[k]]++; }
    py::dict vertex, edge;
    for (size_t n = 0; n < e.fixed.size(); n++) {
        if (!e.live[n]) continue;  // a vertex del_graph_vertex removed is no vertex of the graph
        py::dict v;
        v["fix"] = (bool)e.fixed[n];
        v["edge_num"] = deg[n];
        vertex[std::to_string(n).c_str()] = v;
    }
    for (size_t k = 0; k < e.id.size(); k++) {
        py::dict v;
        v["vertex_num"] = 2;
        v["prev"] = e.from[k];
        v["next"] = e.to[k];
        edge[std::to_string(e.id[k]).c_str()] = v;
    }
    py::dict d;
    d["vertex"] = vertex;
    d["edge"] = edge;
    return d;
}
// pointcloud_align (graph_utils.cpp:20-46): Generalized-ICP of two clouds from a guess, the guess's translation reset when it is 50 m or
// more.  The reference calls PCL's GeneralizedIterativeClosestPoint (third-party, source not in the tree) with 20 neighbours, 64 iterations,
// transformation epsilon 1e-2; here the same cost on the device (lio_gicp_*, the FastGICP formulation the reference's other GICP call
// sites use) with those settings and PCL's default correspondence distance for that class (5 m).  Clouds too small for 20 neighbours, or
// a failed alignment, return the (sanitised) guess.
py::array_t<float> pointcloud_align(py::array_t<float>& source_point, py::array_t<float>& target_point, py::array_t<float>& guess) {
    py::array_t<float> out({4, 4});
    auto o = out.mutable_unchecked<2>();
    auto gi = guess.unchecked<2>();
    double G[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) G[i * 4 + j] = (double)(float)gi(i, j);
    const double d = std::sqrt(G[3] * G[3] + G[7] * G[7] + G[11] * G[11]);
    if (d >= 50.0) { G[3] = 0; G[7] = 0; G[11] = 0; }
    for (int i = 0; i < 16; i++) o(i / 4, i % 4) = (float)G[i];
    auto src = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(source_point);
    auto tgt = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(target_point);
    if (!src || !tgt || src.ndim() != 2 || tgt.ndim() != 2 || src.shape(1) != 4 || tgt.shape(1) != 4 || src.shape(0) < 20 || tgt.shape(0) < 20) return out;
    const uint32_t ns = (uint32_t)src.shape(0), nt = (uint32_t)tgt.shape(0);
    lio_gicp* m = lio_gicp_create(0, 1.0f, std::max(ns, nt), 20);
    if (!m) return out;
    double T[16];
    int it = 0, conv = 0;
    lio_ndt_params prm;
    lio_ndt_default_params(&prm);
    prm.transformation_epsilon = 1e-2;
    prm.rotation_epsilon_deg = 1e-2;
    prm.max_iterations = 64;
    prm.max_process_time_ms = -1;
    int rc;
    {
        py::gil_scoped_release nogil;
        rc = lio_gicp_set_target(m, tgt.data(), nt);
        if (rc == LIO_OK) rc = lio_gicp_set_source(m, src.data(), ns);
        if (rc == LIO_OK) rc = lio_gicp_align(m, G, &prm, 5.0, T, &it, &conv);
        lio_gicp_destroy(m);
    }
    if (rc == LIO_OK)
        for (int i = 0; i < 16; i++) o(i / 4, i % 4) = (float)T[i];
    return out;
}
// set_ground_constraint (hdl_graph_slam_nodelet.cpp:773-781): a toggle starts a new floor plane with the next floor edge
void set_mapping_ground_constraint(bool enable) {
    if (!g) return;
    py::gil_scoped_release rel;
    std::lock_guard<std::mutex> kl(g->kf_mtx);
    if (g->ground_constraint != enable) g->floor_plane = false;
    g->ground_constraint = enable;
}
bool get_mapping_ground_constraint() { return g ? g->ground_constraint : false; }
void set_mapping_constraint(bool loop_closure, bool gravity_constraint) { if (g) { g->loop_closure = loop_closure; g->gravity_constraint = gravity_constraint; } }
// Localization::setMapRender -> MapRender::setActive
void set_map_colouration(bool enable) {
    if (!g) return;
    std::lock_guard<std::mutex> lk(g->mtx);
    g->colouration = enable;
    if (g->painter) lio_render_set_active(g->painter, enable ? 1 : 0);
}
void del_graph_vertex(int id);  // with dump_graph, below
// graph_add_edge (hdl_graph_slam_nodelet.cpp:893-912) with score <= 0: calc_information_matrix(prev, next, relative) -- taken on the bank's frames
// prev_id and next_id, which hold the two clouds -- and Huber 1.0; nothing without a graph
void add_graph_edge(py::array_t<float>& prev, int prev_id, py::array_t<float>& next, int next_id, py::array_t<float>& relative) {
    if (g && relative.size() == 16) {
        py::array_t<float, py::array::c_style | py::array::forcecast> r(relative);
        Mat4 relp;
        for (int k = 0; k < 16; k++) relp.m[k] = (double)r.data()[k];
        py::gil_scoped_release rel;
        std::lock_guard<std::mutex> kl(g->kf_mtx);
        if (g->graph && g->loop) {
            double info[36];
            require(lio_loop_pair_information(g->loop, prev_id, next_id, relp.m, nullptr, nullptr, info) == LIO_OK, "add_graph_edge: lio_loop_pair_information failed");
            require(lio_graph_add_edge(g->graph, prev_id, next_id, relp.m, info, LIO_GRAPH_KERNEL_HUBER, 1.0) >= 0, "add_graph_edge: lio_graph_add_edge failed");
        }
    }
    (void)prev; (void)prev_id; (void)next; (void)next_id; (void)relative;
}
void del_graph_edge(int id) {
    if (!g) return;
    py::gil_scoped_release rel;
    std::lock_guard<std::mutex> kl(g->kf_mtx);
    if (!g->graph) return;
    const int np = -lio_graph_priors(g->graph, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
    if (np > 0) {  // EdgeSE3 only (hdl_graph_slam_nodelet.cpp:961): a prior's id is ignored
        std::vector<int32_t> ids((size_t)np);
        require(lio_graph_priors(g->graph, ids.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (uint32_t)np) == np, "del_graph_edge: lio_graph_priors failed");
        for (int32_t p : ids)
            if (p == id) return;
    }
    require(lio_graph_remove_edge(g->graph, id) == LIO_OK, "del_graph_edge: no such edge");
}
void set_graph_vertex_fix(int id, bool fix) {
    if (!g) return;
    py::gil_scoped_release rel;
    std::lock_guard<std::mutex> kl(g->kf_mtx);
    if (g->graph) require(lio_graph_set_fixed(g->graph, id, fix ? 1 : 0) == LIO_OK, "set_graph_vertex_fix: no such vertex");
}
// graph_optimize: optimize(1024), then every key frame's estimate as str(id) -> 4 x 4; {} without a graph
py::dict run_graph_optimization() {
    std::vector<std::pair<int, Mat4>> odoms;
    if (g) {
        py::gil_scoped_release rel;
        std::lock_guard<std::mutex> kl(g->kf_mtx);
        if (g->graph && !g->graph_odom.empty()) {
            graph_optimize_locked(g.get(), "run_graph_optimization");
            for (size_t k = 0; k < g->graph_pose.size(); k++)
                if (!g->graph_gone[k]) odoms.emplace_back((int)k, g->graph_pose[k]);
        }
    }
    return odoms_to_pydict(odoms);
}
// robust_graph_optimize (hdl_graph_slam_nodelet.cpp:1000-1038): the GNSS outlier stage at 1.0 m (DCS2 on every GNSS prior, optimise, drop the
// priors whose scale fell below 0.1, optimise), then what run_graph_optimization does; {} without a graph.  The "GNSS moment" stage of mode
// "mapping" (:1037-1081, lio_graph_estimate_gnss_moment) runs after it under set_gnss_moment(true) and never in mode "localization"; a graph
// below min_edges, which the outlier stage left untouched, skips it as well
py::dict run_robust_graph_optimization(std::string mode) {
    std::vector<std::pair<int, Mat4>> odoms;
    if (g) {
        py::gil_scoped_release rel;
        std::lock_guard<std::mutex> kl(g->kf_mtx);
        g->moment_ran = false;
        if (g->graph && !g->graph_odom.empty()) {
            const int removed = lio_graph_remove_gnss_outliers(g->graph, 1.0, 1024, nullptr, 0, nullptr);
            require(removed >= -1, "run_robust_graph_optimization: lio_graph_remove_gnss_outliers failed");
            if (g->gnss_moment && mode == "mapping" && removed >= 0) {
                const int n = lio_graph_estimate_gnss_moment(g->graph, 1.0, 1024, nullptr, g->moment_last, &g->moment_report);
                require(n >= 0, "run_robust_graph_optimization: lio_graph_estimate_gnss_moment failed");
                if (n > 0) { g->moment_ran = true; g->moment_priors = n; }
            }
            graph_optimize_locked(g.get(), "run_robust_graph_optimization");
            for (size_t k = 0; k < g->graph_pose.size(); k++)
                if (!g->graph_gone[k]) odoms.emplace_back((int)k, g->graph_pose[k]);
        }
    }
    return odoms_to_pydict(odoms);
}
// not in the reference's module: one GNSS fix for key frame `id`, what flush_gps_queue (hdl_graph_slam_nodelet.cpp:398-455) does once it has
// matched a fix to a key frame -- xyz (metres, already in the map's projection; z ignored for dimension 2), the fix's precision and dimension
// (2, 3 or 6), for dimension 6 the orientation as a quaternion (x, y, z, w).  The distance gate against the last accepted fix (10 / 20 / 50 m by
// precision), the information matrices, Huber 1.0, the release of node 0: gnss_prior_locked, which the flush of the GNSS queue calls as well
// (set_gnss: the UTM projection, the queue and the interpolation between two fixes in time, lio_gnss_queue_*).  The ids of the edges added: []
// when the gate refuses the fix, the key frame has one already, or there is no graph
std::vector<int> add_graph_gnss(int id, py::array_t<double, py::array::c_style | py::array::forcecast> xyz_in, double precision, int dimension, py::object orientation) {
    std::vector<int> added;
    if (!g) return added;
    require(xyz_in.size() == 3, "add_graph_gnss: xyz has 3 entries");
    require(dimension == 2 || dimension == 3 || dimension == 6, "add_graph_gnss: dimension is 2, 3 or 6");
    require(precision > 0, "add_graph_gnss: precision must be positive");
    double xyz[3] = {xyz_in.data()[0], xyz_in.data()[1], dimension == 2 ? 0.0 : xyz_in.data()[2]};
    double quat[4] = {0, 0, 0, 1};
    if (dimension == 6) {
        require(!orientation.is_none(), "add_graph_gnss: dimension 6 needs an orientation (x, y, z, w)");
        auto q = py::cast<py::array_t<double, py::array::c_style | py::array::forcecast>>(orientation);
        require(q.size() == 4, "add_graph_gnss: the orientation is a quaternion (x, y, z, w)");
        for (int k = 0; k < 4; k++) quat[k] = q.data()[k];
    }
    py::gil_scoped_release rel;
    std::lock_guard<std::mutex> kl(g->kf_mtx);
    return gnss_prior_locked(g.get(), id, xyz, quat, precision, dimension, false, "add_graph_gnss");
}
// test visibility: the graph's live priors as lio_graph_priors returns them
py::list _graph_priors() {
    std::vector<int32_t> id, node, type, kernel;
    std::vector<double> m, plane, info, delta;
    int n = 0;
    if (g) {
        py::gil_scoped_release rel;
        std::lock_guard<std::mutex> kl(g->kf_mtx);
        if (g->graph) {
            n = -lio_graph_priors(g->graph, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
            if (n > 0) {
                id.resize(n); node.resize(n); type.resize(n); kernel.resize(n); delta.resize(n);
                m.resize(4 * (size_t)n); plane.resize(4 * (size_t)n); info.resize(9 * (size_t)n);
                require(lio_graph_priors(g->graph, id.data(), node.data(), type.data(), m.data(), plane.data(), info.data(), kernel.data(), delta.data(), (uint32_t)n) == n,
                        "_graph_priors: lio_graph_priors failed");
            }
        }
    }
    py::list out;
    for (int k = 0; k < n; k++) {
        py::dict d;
        d["id"] = id[k]; d["node"] = node[k]; d["type"] = type[k]; d["kernel"] = kernel[k]; d["delta"] = delta[k];
        d["measurement"] = py::array_t<double>(4, &m[4 * (size_t)k]);
        d["plane"] = py::array_t<double>(4, &plane[4 * (size_t)k]);
        d["information"] = py::array_t<double>(std::vector<py::ssize_t>{3, 3}, &info[9 * (size_t)k]);
        out.append(d);
    }
    return out;
}
// dump_keyframe (graph_utils.cpp:123-131): KeyFrame(stamp, id, pose, numpy_to_pointcloud(points, 255.0)).save(directory) -- `data` + `cloud.pcd`,
// the files the localisation mode loads its map from
void dump_keyframe(const std::string& directory, uint64_t stamp, int id, py::array_t<float>& points_input, py::array_t<float>& pose_input) {
    auto pts = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(points_input);
    auto pose = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(pose_input);
    if (!pts || !pose || pts.ndim() != 2 || pts.shape(1) < 4 || pose.size() != 16) return;
    const size_t n = (size_t)pts.shape(0);
    std::vector<float> xyzi(4 * n + 4);
    const float* src = pts.data();
    const py::ssize_t cs = pts.shape(1);
    for (size_t i = 0; i < n; i++) { xyzi[4 * i] = src[i * cs]; xyzi[4 * i + 1] = src[i * cs + 1]; xyzi[4 * i + 2] = src[i * cs + 2]; xyzi[4 * i + 3] = src[i * cs + 3] * 255.0f; }
    Mat4 T;
    for (int i = 0; i < 16; i++) T.m[i] = (double)pose.data()[i];
    write_pcd_binary(directory + "/cloud.pcd", xyzi.data(), n);
    write_keyframe_data(directory, stamp, id, T);
}
void dump_odometry(const std::string& directory);  // with dump_graph, below
// ---- dense-map export (graph_utils.cpp:160-200 and 384-446) over lio_cloud: the frames go to the device, are moved into the world frame there
// and, for save_accumulate_cloud, filtered as one cloud by the device-wide VoxelGrid ----
// set_export_map_config / export_points / dump_map_points: the reference keeps g_map_config (a static, independent of the SLAM instance).
// export_points only keeps host copies of (points, odom): it needs no device, and dump_map_points moves every deferred key frame in one pass.
struct ExportCfg {
    double z_min = 0, z_max = 0;  // (zero-initialised static storage in the reference until the first set_export_map_config)
    std::string color;
    std::vector<std::vector<float>> points;  // N x 4 as given
    std::vector<Mat4> odom;
};
ExportCfg g_export;
// accumulate_cloud / save_accumulate_cloud: the reference's static g_accumulate_cloud (graph_utils.cpp:410)
struct Accumulate {
    lio_cloud* cloud = nullptr;
    lio_scan* scan = nullptr;  // the frame being undistorted
    uint32_t scan_cap = 0;
    lio_ground* ground = nullptr;  // detect_ground on the device, once set_ground_extraction enabled it
    bool ground_on = false;
    uint32_t ground_seed = 0;
};
Accumulate g_acc;

// numpy N x (>= 4) f32 -> xyzi
std::vector<float> xyzi_of(py::array_t<float>& input, const char* what) {
    auto a = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(input);
    if (!a || a.ndim() != 2 || a.shape(1) < 4) throw std::invalid_argument(std::string("slam_wrapper: ") + what + ": points must be N x 4 float32");
    const size_t n = (size_t)a.shape(0), cs = (size_t)a.shape(1);
    std::vector<float> out(4 * n);
    const float* src = a.data();
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 4; k++) out[4 * i + k] = src[i * cs + k];
    return out;
}

// a general 4 x 4 inverse (adjugate / determinant, f64): odometrys[0].T.inverse() of undistortion_cloud, graph_utils.cpp:391-393
Mat4 inverse4(const Mat4& A) {
    const double* m = A.m;
    double inv[16];
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    Mat4 r;
    for (int i = 0; i < 16; i++) r.m[i] = inv[i] / det;
    return r;
}

// numpy_to_odometry (py_utils.cpp:260-270): TUM rows (stamp us, x, y, z, qx, qy, qz, qw); rotation = Eigen::Quaterniond(w, x, y, z) =
// (col 7, 4, 5, 6), toRotationMatrix as Eigen writes it (Quaternion.h, not normalised)
struct TumPose {
    uint64_t stamp;
    Mat4 T;
};
std::vector<TumPose> tum_poses(py::array_t<double>& poses_in) {
    auto a = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(poses_in);
    if (!a || a.ndim() != 2 || a.shape(1) < 8) throw std::invalid_argument("slam_wrapper: poses must be N x 8 TUM rows (stamp, x, y, z, qx, qy, qz, qw)");
    auto r = a.unchecked<2>();
    std::vector<TumPose> out;
    for (py::ssize_t i = 0; i < r.shape(0); i++) {
        TumPose p;
        p.stamp = (uint64_t)r(i, 0);
        p.T = Mat4::identity();
        const double w = r(i, 7), x = r(i, 4), y = r(i, 5), z = r(i, 6);
        const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
        const double twx = tx * w, twy = ty * w, twz = tz * w;
        const double txx = tx * x, txy = ty * x, txz = tz * x;
        const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
        p.T(0, 0) = 1 - (tyy + tzz); p.T(0, 1) = txy - twz; p.T(0, 2) = txz + twy;
        p.T(1, 0) = txy + twz; p.T(1, 1) = 1 - (txx + tzz); p.T(1, 2) = tyz - twx;
        p.T(2, 0) = txz - twy; p.T(2, 1) = tyz + twx; p.T(2, 2) = 1 - (txx + tyy);
        p.T(0, 3) = r(i, 1); p.T(1, 3) = r(i, 2); p.T(2, 3) = r(i, 3);
        out.push_back(p);
    }
    return out;
}
// undistortion_cloud's relative poses (graph_utils.cpp:391-393): T_i <- T_0^-1 * T_i (f64), i = 0 included
std::vector<Mat4> relative_poses(const std::vector<TumPose>& poses) {
    std::vector<Mat4> rel;
    if (poses.empty()) return rel;
    const Mat4 inv0 = inverse4(poses[0].T);
    for (const TumPose& p : poses) rel.push_back(mul(inv0, p.T));
    return rel;
}

// undistortion_cloud (graph_utils.cpp:384-396) on the device: the frame into g_acc.scan, undistortPoints(poses, cloud) there
// (lio_scan_undistort_poses, slam_utils.cpp:193-228).  Throws on what the reference leaves undefined or this module leaves out.
void undistort_frame(py::array_t<float>& points, py::dict& points_attr, const std::vector<TumPose>& poses, const char* what) {
    if (poses.empty()) throw std::invalid_argument(std::string("slam_wrapper: ") + what + ": no poses (the reference indexes an empty pose list)");
    if (poses.size() > 64) throw std::invalid_argument(std::string("slam_wrapper: ") + what + ": more than 64 poses in one frame are not supported");
    const std::vector<float> xyzi = xyzi_of(points, what);
    const size_t n = xyzi.size() / 4;
    auto attr = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(py::cast<py::array>(points_attr["points_attr"]));
    if (!attr || attr.ndim() != 2 || attr.shape(1) < 1 || (size_t)attr.shape(0) != n)
        throw std::invalid_argument(std::string("slam_wrapper: ") + what + ": points_attr must be N x 2 with one row per point");
    const uint64_t header = py::cast<uint64_t>(points_attr["timestamp"]);
    std::vector<uint32_t> stamp(n);
    for (size_t i = 0; i < n; i++) stamp[i] = (uint32_t)attr.data()[i * attr.shape(1)];  // PointAttr::stamp = ref_attr(i, 0)
    std::vector<uint64_t> ps;
    std::vector<double> rel;
    for (const Mat4& T : relative_poses(poses)) rel.insert(rel.end(), T.m, T.m + 16);
    for (const TumPose& p : poses) ps.push_back(p.stamp);
    for (size_t i = 2; i < poses.size(); i++)
        if (ps[i] - header < ps[i - 1] - header)
            throw std::invalid_argument(std::string("slam_wrapper: ") + what + ": the pose intervals must not end earlier than their predecessors");
    if (n > 0xFFFFFFFFull) throw std::invalid_argument(std::string("slam_wrapper: ") + what + ": too many points in one frame");
    if (!g_acc.scan || g_acc.scan_cap < n) {
        if (g_acc.scan) lio_scan_destroy(g_acc.scan);
        g_acc.scan_cap = (uint32_t)std::max<size_t>(n, 1 << 17);
        g_acc.scan = lio_scan_create(0, g_acc.scan_cap, 1024);
        if (!g_acc.scan) g_acc.scan_cap = 0;
        require(g_acc.scan != nullptr, "no HIP device for the undistortion");
    }
    require(lio_scan_upload(g_acc.scan, xyzi.data(), (uint32_t)n) == LIO_OK, "frame upload failed");
    require(lio_scan_undistort_poses(g_acc.scan, stamp.data(), 0, header, ps.data(), rel.data(), (uint32_t)ps.size()) == LIO_OK, "undistortion failed");
}

void set_export_map_config(double z_min, double z_max, std::string color) {
    g_export = ExportCfg();
    g_export.z_min = z_min;
    g_export.z_max = z_max;
    g_export.color = color;
}
void export_points(py::array_t<float>& points_input, py::array_t<float>& odom_input) {
    if (g_export.color == "rgb") return;  // (graph_utils.cpp:169: the colour map comes from the painter, not from the exported frames)
    auto od = py::array_t<float, py::array::c_style | py::array::forcecast>::ensure(odom_input);
    if (!od || od.size() != 16) throw std::invalid_argument("slam_wrapper: export_points: odom must be 4 x 4");
    Mat4 T;
    for (int i = 0; i < 16; i++) T.m[i] = (double)od.data()[i];  // numpy_to_eigen(const py::array_t<float>&) -> Matrix4d
    g_export.points.push_back(xyzi_of(points_input, "export_points"));
    g_export.odom.push_back(T);
}
// savePCDFileBinary of a PointXYZRGB cloud: FIELDS x y z rgb, the colour word with PCL's alpha of 255 on top
bool write_pcd_rgb(const std::string& path, const float* xyzrgb, size_t n) {
    std::ofstream f(path, std::ios::binary);
    if (!f) return false;
    f << "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH " << n
      << "\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS " << n << "\nDATA binary\n";
    std::vector<float> rows(xyzrgb, xyzrgb + 4 * n);
    for (size_t i = 0; i < n; i++) {
        uint32_t w;
        std::memcpy(&w, &rows[4 * i + 3], 4);
        w |= 0xFF000000u;
        std::memcpy(&rows[4 * i + 3], &w, 4);
    }
    f.write(reinterpret_cast<const char*>(rows.data()), (std::streamsize)(n * 16));
    return (bool)f;
}
void dump_map_points(std::string file) {
    if (g_export.color == "rgb") {  // graph_utils.cpp:189-203: the colour map between z_min and z_max; an empty cloud is not written
        std::vector<float> pts, kept;
        if (g) {
            std::lock_guard<std::mutex> lk(g->mtx);
            pts = colour_map_points(g->painter);
        }
        for (size_t i = 0; i + 3 < pts.size(); i += 4)
            if ((double)pts[i + 2] >= g_export.z_min && (double)pts[i + 2] <= g_export.z_max) kept.insert(kept.end(), pts.begin() + i, pts.begin() + i + 4);
        if (kept.empty()) return;
        require(write_pcd_rgb(file, kept.data(), kept.size() / 4), "dump_map_points: cannot write the file");
        return;
    }
    uint64_t total = 0;
    for (const auto& p : g_export.points) total += p.size() / 4;
    if (total == 0) return;
    lio_cloud* c = lio_cloud_create(0, total);
    require(c != nullptr, "dump_map_points: no HIP device");
    std::vector<float> out;
    int64_t m = 0;
    for (size_t k = 0; k < g_export.points.size() && m >= 0; k++) {
        const auto& p = g_export.points[k];
        if (lio_cloud_append_host(c, p.data(), p.size() / 4, g_export.odom[k].m, 255.0f, 1, g_export.z_min, g_export.z_max) != LIO_OK) m = -1;
    }
    uint64_t n = 0;
    if (m >= 0 && lio_cloud_size(c, &n) == LIO_OK) {
        out.resize(4 * n + 4);
        m = lio_cloud_download(c, out.data(), n);
    } else {
        m = -1;
    }
    lio_cloud_destroy(c);
    require(m >= 0, "dump_map_points: the device pass failed");
    if (m == 0) return;
    require(write_pcd_binary(file, out.data(), (size_t)m), "dump_map_points: cannot write the file");
}
py::list dump_graph(const std::string& directory);  // below, with the rest of the map's way to disk
py::list align_pose(double stamp1, double stamp2, py::array_t<double>& estimate1_py, py::array_t<double>& estimate2_py, py::array_t<double>& poses_stamp,
                    py::list& poses_py);
void save_undistortion_cloud(std::string file, py::array_t<float>& points, py::dict& points_attr, py::array_t<double>& poses) {
    const std::vector<TumPose> tum = tum_poses(poses);
    undistort_frame(points, points_attr, tum, "save_undistortion_cloud");
    std::vector<float> out(4 * (size_t)g_acc.scan_cap + 4);
    const int n = lio_scan_download_raw(g_acc.scan, out.data(), g_acc.scan_cap);
    require(n >= 0, "save_undistortion_cloud: download failed");
    if (n == 0) return;  // (savePCDFileBinary refuses an empty cloud)
    require(write_pcd_binary(file, out.data(), (size_t)n), "save_undistortion_cloud: cannot write the file");
}
// the detector of accumulate_cloud(extract_ground=True) and _detect_ground; throws when there is no device
void need_ground(const char* what) {
    if (g_acc.ground) return;
    g_acc.ground = lio_ground_create(0);
    if (!g_acc.ground) throw std::runtime_error(std::string("slam_wrapper: ") + what + ": ground extraction needs a HIP device (there is no CPU fallback): " + lio_last_error());
}
// Turns accumulate_cloud(extract_ground=True) on or off (off by default: the call then raises ValueError as before).  The stage is
// detect_ground of graph_utils.cpp:329-382 on the device (include/lio_hip.h: lio_ground_*); the RANSAC's draws are THIS MODULE'S, a
// counter-based generator of (seed, draw number), not PCL's random shuffle: the same frames and seed give the same cloud on every run,
// and a different plane hypothesis sequence than the reference's on any run.
void set_ground_extraction(bool enable, uint32_t seed) {
    g_acc.ground_on = enable;
    g_acc.ground_seed = seed;
}
uint32_t ground_seed_now() { return g_acc.ground_seed; }
void accumulate_cloud(py::array_t<float>& points, py::dict& points_attr, py::array_t<double>& poses, std::string odometry_type, bool extract_ground) {
    if (odometry_type != "TUM")
        throw std::invalid_argument("slam_wrapper: accumulate_cloud: odometry_type '" + odometry_type + "' is not supported (only \"TUM\"; the reference indexes an empty pose list)");
    if (extract_ground && !g_acc.ground_on)
        throw std::invalid_argument("slam_wrapper: accumulate_cloud: extract_ground=True is off by default (detect_ground runs on the device with this "
                                    "module's own RANSAC draws, not PCL's: enable it with set_ground_extraction(True, seed))");
    if (extract_ground) need_ground("accumulate_cloud");  // (before the frame touches the device: nothing changes when there is none)
    const std::vector<TumPose> tum = tum_poses(poses);
    undistort_frame(points, points_attr, tum, "accumulate_cloud");
    if (extract_ground) {
        // detect_ground(cloud->cloud) in the sensor frame, graph_utils.cpp:421-423: no floor, no append; else the cloud is the inlier cloud
        lio_ground_params gp;
        lio_ground_default_params(&gp, 0);
        gp.seed = g_acc.ground_seed;
        int found = 0;
        float coeffs[4];
        require(lio_ground_detect_scan(g_acc.ground, g_acc.scan, &gp, 1, &found, coeffs, nullptr, nullptr, nullptr) == LIO_OK, "accumulate_cloud: ground detection failed");
        if (!found) return;
    }
    if (!g_acc.cloud) {
        g_acc.cloud = lio_cloud_create(0, 0);
        require(g_acc.cloud != nullptr, "accumulate_cloud: no HIP device");
    }
    // pcl::transformPointCloud(*cloud, *transformed, odometrys[0].T) with the absolute pose, then *g_accumulate_cloud += *transformed
    require(lio_cloud_append_scan(g_acc.cloud, g_acc.scan, tum[0].T.m, 1.0f, 0, 0.0, 0.0) == LIO_OK, "accumulate_cloud: append failed");
}
void save_accumulate_cloud(std::string file, double resolution) {
    uint64_t n = 0;
    if (!g_acc.cloud || lio_cloud_size(g_acc.cloud, &n) != LIO_OK || n == 0) return;
    if (resolution > 0.0) require(lio_cloud_voxel_downsample(g_acc.cloud, (float)resolution, &n) == LIO_OK, "save_accumulate_cloud: voxel grid failed");
    std::vector<float> out(4 * (size_t)n + 4);
    const int64_t m = lio_cloud_download(g_acc.cloud, out.data(), n);
    require(m >= 0, "save_accumulate_cloud: download failed");
    lio_cloud_clear(g_acc.cloud);
    if (m > 0) require(write_pcd_binary(file, out.data(), (size_t)m), "save_accumulate_cloud: cannot write the file");
}
// ---- texture_mesh (graph_utils.cpp:449-501): a coloured PCD, an OBJ mesh, every vertex coloured by its 3 nearest cloud points -----------------
// The readers and the writer are the module's own (PCL is not linked): every refusal raises ValueError naming the reason.
[[noreturn]] void refuse(const char* who, const std::string& why) { throw std::invalid_argument(std::string("slam_wrapper: ") + who + ": " + why); }

bool slurp(const std::string& path, std::string& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    f.seekg(0, std::ios::end);
    const std::streamoff sz = f.tellg();
    if (sz < 0) return false;
    out.resize((size_t)sz);
    f.seekg(0);
    return sz == 0 || (bool)f.read(&out[0], sz);
}

bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }

// the next whitespace-separated token of [p, end)
bool next_token(const char*& p, const char* end, const char*& a, const char*& b) {
    while (p < end && is_space(*p)) p++;
    if (p >= end) return false;
    a = p;
    while (p < end && !is_space(*p)) p++;
    b = p;
    return true;
}

// correctly rounded decimal -> f32 (as lexical_cast<float> / strtof); "nan", "inf" accepted; subnormal results through strtof (from_chars
// reports them out of range)
bool parse_f32(const char* a, const char* b, float& v) {
    if (a < b && *a == '+') a++;
    const auto r = std::from_chars(a, b, v);
    if (r.ec == std::errc() && r.ptr == b) return true;
    if (r.ec != std::errc::result_out_of_range) return false;
    const std::string t(a, b);
    char* e = nullptr;
    v = std::strtof(t.c_str(), &e);
    return e == t.c_str() + t.size();
}

template <typename T>
bool parse_int(const char* a, const char* b, T& v) {
    if (a < b && *a == '+') a++;
    const auto r = std::from_chars(a, b, v);
    return r.ec == std::errc() && r.ptr == b;
}

// a PointXYZRGB cloud: x y z (4-byte floats) and the 32-bit pattern of `rgb` / `rgba` (r = bits 16-23, g = 8-15, b = 0-7), other fields of any
// SIZE / COUNT skipped; DATA ascii or binary; WIDTH * HEIGHT points (POINTS when given)
void read_rgb_pcd(const std::string& path, std::vector<float>& xyz, std::vector<uint32_t>& rgb, const char* who) {
    std::string buf;
    if (!slurp(path, buf)) refuse(who, "cannot read the cloud '" + path + "'");
    std::vector<std::string> fields, types;
    std::vector<int> sizes, counts;
    long long width = -1, height = 1, points = -1;
    std::string data;
    size_t pos = 0;
    while (pos < buf.size() && data.empty()) {
        size_t e = buf.find('\n', pos);
        if (e == std::string::npos) e = buf.size();
        std::string line = buf.substr(pos, e - pos);
        pos = e + 1;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ls(line);
        std::string key;
        ls >> key;
        bool ok = true;
        if (key == "FIELDS") { std::string v; while (ls >> v) fields.push_back(v); }
        else if (key == "SIZE") { int v; while (ls >> v) sizes.push_back(v); ok = ls.eof(); }
        else if (key == "TYPE") { std::string v; while (ls >> v) types.push_back(v); }
        else if (key == "COUNT") { int v; while (ls >> v) counts.push_back(v); ok = ls.eof(); }
        else if (key == "WIDTH") ok = (bool)(ls >> width);
        else if (key == "HEIGHT") ok = (bool)(ls >> height);
        else if (key == "POINTS") ok = (bool)(ls >> points);
        else if (key == "DATA") { ls >> data; if (data.empty()) ok = false; }
        if (!ok) refuse(who, "malformed PCD header line '" + line + "' in '" + path + "'");
    }
    if (data.empty()) refuse(who, "no DATA line in '" + path + "'");
    if (data == "binary_compressed") refuse(who, "DATA binary_compressed is not supported ('" + path + "')");
    if (data != "ascii" && data != "binary") refuse(who, "unknown DATA kind '" + data + "' in '" + path + "'");
    if (counts.empty()) counts.assign(fields.size(), 1);
    if (fields.empty() || sizes.size() != fields.size() || types.size() != fields.size() || counts.size() != fields.size())
        refuse(who, "malformed PCD header (FIELDS / SIZE / TYPE / COUNT disagree) in '" + path + "'");
    if (points < 0) points = width * height;
    if (width < 0 || height < 0 || points < 0) refuse(who, "malformed PCD header (no WIDTH) in '" + path + "'");
    int xyz_f[3] = {-1, -1, -1}, col_f = -1;
    for (size_t i = 0; i < fields.size(); i++) {
        if (sizes[i] <= 0 || counts[i] <= 0) refuse(who, "malformed PCD header (SIZE / COUNT) in '" + path + "'");
        const int k = fields[i] == "x" ? 0 : fields[i] == "y" ? 1 : fields[i] == "z" ? 2 : -1;
        if (k >= 0 && xyz_f[k] < 0) xyz_f[k] = (int)i;
        if ((fields[i] == "rgb" || fields[i] == "rgba") && col_f < 0) col_f = (int)i;
    }
    for (int k = 0; k < 3; k++)
        if (xyz_f[k] < 0 || sizes[xyz_f[k]] != 4 || types[xyz_f[k]] != "F") refuse(who, "the cloud needs x, y and z as 4-byte floats ('" + path + "')");
    if (col_f < 0) refuse(who, "the cloud has no rgb / rgba field ('" + path + "'): nothing to colour the mesh with");
    if (sizes[col_f] != 4 || (types[col_f] != "F" && types[col_f] != "U" && types[col_f] != "I"))
        refuse(who, "the cloud's " + fields[col_f] + " field is not a 4-byte word ('" + path + "')");
    const size_t n = (size_t)points;
    xyz.assign(3 * n, 0.f);
    rgb.assign(n, 0u);
    if (data == "binary") {
        size_t stride = 0;
        std::vector<size_t> off(fields.size());
        for (size_t i = 0; i < fields.size(); i++) { off[i] = stride; stride += (size_t)sizes[i] * counts[i]; }
        if (stride == 0 || (buf.size() - std::min(pos, buf.size())) / stride < n) refuse(who, "the binary data of '" + path + "' is shorter than its header says");
        const char* d = buf.data() + pos;
        for (size_t i = 0; i < n; i++, d += stride) {
            for (int k = 0; k < 3; k++) std::memcpy(&xyz[3 * i + k], d + off[xyz_f[k]], 4);
            std::memcpy(&rgb[i], d + off[col_f], 4);
        }
    } else {
        const char* p = buf.data() + std::min(pos, buf.size());
        const char* end = buf.data() + buf.size();
        const char *a, *b;
        for (size_t i = 0; i < n; i++)
            for (size_t f = 0; f < fields.size(); f++)
                for (int c = 0; c < counts[f]; c++) {
                    if (!next_token(p, end, a, b)) refuse(who, "the ascii data of '" + path + "' ends before its header's point count");
                    if (c) continue;
                    bool ok = true;
                    if ((int)f == col_f) {
                        if (types[f] == "F") { float v; ok = parse_f32(a, b, v); std::memcpy(&rgb[i], &v, 4); }
                        else if (types[f] == "U") { uint32_t v; ok = parse_int(a, b, v); rgb[i] = v; }
                        else { int32_t v; ok = parse_int(a, b, v); rgb[i] = (uint32_t)v; }
                    } else {
                        for (int k = 0; k < 3; k++)
                            if ((int)f == xyz_f[k]) ok = parse_f32(a, b, xyz[3 * i + k]);
                    }
                    if (!ok) refuse(who, "bad value '" + std::string(a, b) + "' in the ascii data of '" + path + "'");
                }
    }
}

// an OBJ mesh: `v x y z [...]` (extra values ignored), `f` with i, i/t, i//n, i/t/n and negative (relative) indices, polygons of any arity;
// other statements ignored.  faces: the 0-based indices of every face in turn, face_size: their arities.
void read_obj(const std::string& path, std::vector<float>& v, std::vector<int32_t>& faces, std::vector<uint32_t>& face_size, const char* who) {
    std::string buf;
    if (!slurp(path, buf)) refuse(who, "cannot read the mesh '" + path + "'");
    v.clear();
    faces.clear();
    face_size.clear();
    const char* p = buf.data();
    const char* end = p + buf.size();
    size_t line_no = 0;
    std::vector<int64_t> raw;  // face indices as written (1-based or negative), checked once every vertex is known
    while (p < end) {
        const char* e = static_cast<const char*>(std::memchr(p, '\n', (size_t)(end - p)));
        if (!e) e = end;
        line_no++;
        const char* q = p;
        const char* le = e;
        p = e + 1;
        const char *a, *b;
        if (!next_token(q, le, a, b)) continue;
        const size_t kw = (size_t)(b - a);
        auto bad = [&](const char* what) { refuse(who, std::string(what) + " at line " + std::to_string(line_no) + " of '" + path + "'"); };
        if (kw == 1 && *a == 'v') {
            float c[3];
            for (int k = 0; k < 3; k++)
                if (!next_token(q, le, a, b) || !parse_f32(a, b, c[k])) bad("malformed vertex");
            v.insert(v.end(), c, c + 3);
        } else if (kw == 1 && *a == 'f') {
            uint32_t cnt = 0;
            const int64_t nv = (int64_t)(v.size() / 3);
            while (next_token(q, le, a, b)) {
                const char* s = static_cast<const char*>(std::memchr(a, '/', (size_t)(b - a)));
                int64_t i = 0;
                if (!parse_int(a, s ? s : b, i) || i == 0) bad("malformed face index");
                if (i < 0) {
                    i = nv + i;  // relative: -1 is the last vertex read so far
                    if (i < 0) bad("face index out of range");
                    raw.push_back(i);
                } else {
                    raw.push_back(i - 1);
                }
                cnt++;
            }
            if (cnt == 0) bad("face without vertices");
            if (cnt > 255) bad("face of more than 255 vertices (the PLY list count is a uchar)");
            face_size.push_back(cnt);
        }
    }
    const int64_t nv = (int64_t)(v.size() / 3);
    faces.resize(raw.size());
    for (size_t i = 0; i < raw.size(); i++) {
        if (raw[i] >= nv) refuse(who, "face index " + std::to_string(raw[i] + 1) + " out of range (" + std::to_string(nv) + " vertices) in '" + path + "'");
        faces[i] = (int32_t)raw[i];
    }
}

// the mesh as PLY, binary little endian: float x y z + uchar red green blue per vertex, `list uchar int vertex_indices` per face -- the layout
// PCL 1.9's savePLYFileBinary gives a PointXYZRGB mesh, restated (PCL is not linked)
bool write_mesh_ply(const std::string& path, const float* v, const uint8_t* rgb, size_t nv, const int32_t* faces, const uint32_t* face_size, size_t nf) {
    std::ofstream f(path, std::ios::binary);
    if (!f) return false;
    f << "ply\nformat binary_little_endian 1.0\ncomment PCL generated\nelement vertex " << nv
      << "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face " << nf
      << "\nproperty list uchar int vertex_indices\nend_header\n";
    std::vector<char> out(nv * 15);
    for (size_t i = 0; i < nv; i++) {
        std::memcpy(&out[15 * i], v + 3 * i, 12);
        std::memcpy(&out[15 * i + 12], rgb + 3 * i, 3);
    }
    f.write(out.data(), (std::streamsize)out.size());
    out.clear();
    size_t k = 0;
    for (size_t i = 0; i < nf; i++) {
        out.push_back((char)(uint8_t)face_size[i]);
        const size_t at = out.size();
        out.resize(at + 4ull * face_size[i]);
        std::memcpy(&out[at], faces + k, 4ull * face_size[i]);
        k += face_size[i];
    }
    f.write(out.data(), (std::streamsize)out.size());
    return (bool)f;
}

void texture_mesh(std::string mesh_path, std::string cloud_path, std::string output_path) {
    const char* who = "texture_mesh";
    struct stat st;
    if (stat(output_path.c_str(), &st) != 0 || !S_ISDIR(st.st_mode) || access(output_path.c_str(), W_OK | X_OK) != 0)
        refuse(who, "the output directory '" + output_path + "' cannot be written");
    std::vector<float> xyz, verts;
    std::vector<uint32_t> rgb, face_size;
    std::vector<int32_t> faces;
    read_rgb_pcd(cloud_path, xyz, rgb, who);
    size_t finite = 0;
    for (size_t i = 0; i < rgb.size(); i++) finite += std::isfinite(xyz[3 * i]) && std::isfinite(xyz[3 * i + 1]) && std::isfinite(xyz[3 * i + 2]);
    if (finite == 0) refuse(who, "the cloud '" + cloud_path + "' has no finite point");
    if (rgb.size() > 0x7FFFFFFFull) refuse(who, "the cloud '" + cloud_path + "' has more than 2^31 - 1 points");
    read_obj(mesh_path, verts, faces, face_size, who);
    const size_t nv = verts.size() / 3;
    std::vector<uint8_t> colour(3 * nv + 3);
    {
        py::gil_scoped_release nogil;
        lio_knn_index* x = lio_knn_index_create(0);
        require(x != nullptr, "texture_mesh: no HIP device");
        int rc = lio_knn_index_build(x, xyz.data(), rgb.data(), rgb.size(), nullptr);
        if (rc == LIO_OK) rc = lio_knn_index_colour(x, verts.data(), nv, 3, colour.data());  // smooth_factor = 3
        lio_knn_index_destroy(x);
        require(rc == LIO_OK, "texture_mesh: the device pass failed");
    }
    const std::string out = output_path + "/texture_mesh.ply";
    if (!write_mesh_ply(out, verts.data(), colour.data(), nv, faces.data(), face_size.data(), face_size.size())) refuse(who, "cannot write '" + out + "'");
}
// ---- the offline painter (graph_utils.cpp:503-622): set_colouration_config, set_map_odometrys, colouration_frame, save_render_cloud ----------
struct Colouration {
    lio_render* map = nullptr;
    std::vector<CamCfg> cameras;
    int odometry_idx = 0;
    std::vector<TumPose> odometrys;
    uint32_t seed = 0;
    // test visibility: what the last colouration_frame handed to the painter
    int last_outcome = -1;
    std::vector<float> last_frame;
    Mat4 last_pose = Mat4::identity();
    std::vector<std::pair<std::string, Mat4>> last_images;
};
Colouration g_col;

// Eigen's Quaterniond(Matrix3d) (w, x, y, z) and interpolateTransform (slam_utils.cpp:126-161): the library's (csrc/geodesy.cpp), which the RTK
// track and the graph's GNSS queue use as well
void quat_of(const Mat4& T, double q[4]) { lio_quat_of_transform(T.m, q); }
Mat4 interpolate_transform(const Mat4& pre, const Mat4& next, double ratio) {
    Mat4 R;
    lio_interpolate_transform(pre.m, next.m, ratio, R.m);
    return R;
}

// get_stamp_pose (graph_utils.cpp:514-544): the odometry pair around the stamp, searched from start_idx on, and the pose between them.  Its three
// refusals: no odometry, a stamp before the first or after the last, no pair found from start_idx on.
bool get_stamp_pose(uint64_t stamp, int start_idx, int& out_idx, TumPose& pose) {
    const std::vector<TumPose>& od = g_col.odometrys;
    if (od.empty()) return false;
    if (stamp < od.front().stamp) return false;
    if (stamp > od.back().stamp) return false;
    size_t first = (size_t)std::max(start_idx, 0), second = first;
    if (first >= od.size()) return false;
    for (; second != od.size(); second++) {
        const double dt = ((double)od[first].stamp - (double)stamp) / 1000000.0, dt2 = ((double)od[second].stamp - (double)stamp) / 1000000.0;
        if (dt <= 0 && dt2 >= 0) break;
        first = second;
    }
    if (first == second || second == od.size()) return false;
    out_idx = (int)first;
    const double ratio = ((double)stamp - (double)od[first].stamp) / (double)(od[second].stamp - od[first].stamp);
    pose.stamp = stamp;
    pose.T = interpolate_transform(od[first].T, od[second].T, ratio);
    return true;
}

// starts a fresh, active painter with an identity lidar transform (graph_utils.cpp:546-557)
void set_colouration_config(py::list& cameras) {
    std::vector<CamCfg> cams = camera_config(cameras);
    if (g_col.map) lio_render_destroy(g_col.map);
    g_col.map = nullptr;
    g_col.map = make_painter(cams, Mat4::identity(), "set_colouration_config");
    lio_render_set_active(g_col.map, 1);
    g_col.cameras = cams;
    g_col.last_outcome = -1;
}
void set_map_odometrys(py::array_t<double>& poses) {
    g_col.odometry_idx = 0;
    g_col.odometrys = tum_poses(poses);
}
// the seed of the ground test's draws (lio_ground; 0 unless set)
void set_colouration_seed(uint32_t seed) { g_col.seed = seed; }
void colouration_frame(std::string lidar_name, py::dict& points, py::dict& points_attr, py::dict& image_dict, py::dict& image_stream_dict, py::dict& image_param) {
    (void)image_stream_dict;
    if (!g_col.map) throw std::runtime_error("slam_wrapper: colouration_frame: set_colouration_config first (save_render_cloud releases the painter)");
    if (!points.contains(lidar_name.c_str()) || !points_attr.contains(lidar_name.c_str()))
        throw std::invalid_argument("slam_wrapper: colouration_frame: no cloud named '" + lidar_name + "'");
    std::vector<FrameImage> images = frame_images(image_dict, image_param, g_col.cameras, "colouration_frame");
    py::array_t<float> cloud = py::cast<py::array>(points[lidar_name.c_str()]);
    py::dict attr = py::cast<py::dict>(points_attr[lidar_name.c_str()]);
    const uint64_t header = py::cast<uint64_t>(attr["timestamp"]);
    g_col.last_outcome = -1;
    // the poses at the start of the scan and 100 ms later
    int start_idx = 0, end_idx = 0;
    TumPose start, end;
    if (!get_stamp_pose(header, g_col.odometry_idx, start_idx, start)) return;
    if (!get_stamp_pose(header + 100000ULL, g_col.odometry_idx, end_idx, end)) return;
    g_col.odometry_idx = start_idx;
    std::vector<TumPose> poses;
    poses.push_back(start);
    for (int i = start_idx + 1; i < end_idx; i++) poses.push_back(g_col.odometrys[(size_t)i]);
    poses.push_back(end);
    undistort_frame(cloud, attr, poses, "colouration_frame");  // (relative to the first pose, as :594-597)
    std::vector<float> frame(4 * (size_t)g_acc.scan_cap + 4);
    const int n = lio_scan_download_raw(g_acc.scan, frame.data(), g_acc.scan_cap);
    require(n >= 0, "colouration_frame: download failed");
    std::vector<FrameImage> posed;
    for (FrameImage& im : images) {
        int idx = 0;
        TumPose ip;
        if (get_stamp_pose(im.stamp, g_col.odometry_idx, idx, ip)) {
            im.pose = ip.T;
            posed.push_back(std::move(im));
        }
    }
    const int rc = paint_frame(g_col.map, frame.data(), (size_t)n, start.T, g_col.seed, posed);
    require(rc >= 0, "colouration_frame: render failed");
    g_col.last_outcome = rc;
    frame.resize(4 * (size_t)n);
    g_col.last_frame = frame;
    g_col.last_pose = start.T;
    g_col.last_images.clear();
    for (const FrameImage& im : posed) g_col.last_images.emplace_back(g_col.cameras[(size_t)im.camera].name, im.pose);
}
// the colour map as a binary PCD (x y z rgb); the painter is released; an empty cloud writes nothing, like the module's other savers
void save_render_cloud(std::string file) {
    if (!g_col.map) return;
    std::vector<float> pts = colour_map_points(g_col.map);
    lio_render_destroy(g_col.map);
    g_col.map = nullptr;
    if (pts.empty()) return;
    require(write_pcd_rgb(file, pts.data(), pts.size() / 4), "save_render_cloud: cannot write the file");
}
// test visibility: (outcome, frame N x 4, pose 4 x 4, {camera: pose}) of the last colouration_frame -- outcome -1: refused by get_stamp_pose,
// else LIO_RENDER_*; _stamp_pose(stamp, start_idx) -> (found, idx, pose) of get_stamp_pose
// ---- the map's way to disk from mapping mode: dump_graph, dump_odometry, del_graph_vertex, align_pose ---------------------------------------------
// graph.g2o as g2o's OptimizableGraph::save writes it (tag, ids, the element's own write()): every vertex in rising id, a FIX line behind a
// fixed one, then the edges.  DEVIATION: numbers go out with 17 significant digits (g2o leaves the stream at its default 6), so that a reader
// gets the same doubles back; any g2o reader takes both.  <path>.kernels in the format of robust_kernel_io.cpp:72-76 when the record has kernels
bool write_g2o(const std::string& path, const G2oFile& gf) {
    std::ofstream f(path);
    if (!f) return false;
    f << std::setprecision(17);
    std::vector<const G2oFile::Vertex*> vs;
    for (const auto& v : gf.vertices) vs.push_back(&v);
    std::stable_sort(vs.begin(), vs.end(), [](const G2oFile::Vertex* a, const G2oFile::Vertex* b) { return a->id < b->id; });
    const std::set<int> fixed(gf.fixed.begin(), gf.fixed.end());
    for (const auto* v : vs) {
        f << "VERTEX_SE3:QUAT " << v->id;
        for (int k = 0; k < 7; k++) f << " " << v->v[k];
        f << "\n";
        if (fixed.count(v->id)) f << "FIX " << v->id << "\n";
    }
    for (const auto& e : gf.edges) {
        f << "EDGE_SE3:QUAT " << e.from << " " << e.to;
        for (int k = 0; k < 7; k++) f << " " << e.m[k];
        for (int r = 0; r < 6; r++)
            for (int c = r; c < 6; c++) f << " " << e.info[r * 6 + c];
        f << "\n";
    }
    for (const auto& p : gf.priors) {
        f << p.tag << " " << p.node;
        for (double v : p.values) f << " " << v;
        f << "\n";
    }
    if (!f) return false;
    if (gf.kernels.empty()) return true;
    std::ofstream k(path + ".kernels");
    if (!k) return false;
    k << std::setprecision(17);
    for (const auto& kn : gf.kernels) {
        k << kn.vertices.size() << " ";
        for (int v : kn.vertices) k << v << " ";
        k << kn.type << " " << kn.delta << "\n";
    }
    return (bool)k;
}
// a pose as the 7 numbers of g2o's toVectorQT: x y z qx qy qz qw, the quaternion Eigen's Quaterniond(Matrix3d), normalised
void tq_of(const double T16[16], double v[7]) {
    Mat4 T;
    std::memcpy(T.m, T16, sizeof(T.m));
    double q[4];
    quat_of(T, q);
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    v[0] = T(0, 3); v[1] = T(1, 3); v[2] = T(2, 3);
    v[3] = q[1] / n; v[4] = q[2] / n; v[5] = q[3] / n; v[6] = q[0] / n;
}
const char* kernel_name(int kernel) { return kernel == LIO_GRAPH_KERNEL_HUBER ? "Huber" : kernel == LIO_GRAPH_KERNEL_DCS2 ? "DCS2" : ""; }
// test visibility: _write_g2o(path, record) -- the dictionary _read_g2o returns (skipped is not read; priors and kernels may be missing)
void _write_g2o(std::string path, py::dict rec) {
    G2oFile gf;
    for (auto item : py::cast<py::dict>(rec["vertices"])) {
        G2oFile::Vertex v;
        v.id = py::cast<int>(item.first);
        auto a = py::cast<py::array_t<double, py::array::c_style | py::array::forcecast>>(item.second);
        require(a.size() == 7, "_write_g2o: a vertex is x y z qx qy qz qw");
        std::memcpy(v.v, a.data(), sizeof(v.v));
        gf.vertices.push_back(v);
    }
    for (auto item : py::cast<py::list>(rec["edges"])) {
        py::tuple t = py::cast<py::tuple>(item);
        require(t.size() == 4, "_write_g2o: an edge is (from, to, [7], 6 x 6)");
        G2oFile::Edge e;
        e.from = py::cast<int>(t[0]); e.to = py::cast<int>(t[1]);
        auto m = py::cast<py::array_t<double, py::array::c_style | py::array::forcecast>>(t[2]);
        auto w = py::cast<py::array_t<double, py::array::c_style | py::array::forcecast>>(t[3]);
        require(m.size() == 7 && w.size() == 36, "_write_g2o: an edge is (from, to, [7], 6 x 6)");
        std::memcpy(e.m, m.data(), sizeof(e.m));
        std::memcpy(e.info, w.data(), sizeof(e.info));
        gf.edges.push_back(e);
    }
    gf.fixed = py::cast<std::vector<int>>(rec["fixed"]);
    if (rec.contains("priors"))
        for (auto item : py::cast<py::list>(rec["priors"])) {
            py::tuple t = py::cast<py::tuple>(item);
            require(t.size() == 3, "_write_g2o: a prior is (tag, vertex, values)");
            G2oFile::Prior p;
            p.tag = py::cast<std::string>(t[0]); p.node = py::cast<int>(t[1]);
            auto a = py::cast<py::array_t<double, py::array::c_style | py::array::forcecast>>(t[2]);
            p.values.assign(a.data(), a.data() + a.size());
            gf.priors.push_back(p);
        }
    if (rec.contains("kernels"))
        for (auto item : py::cast<py::list>(rec["kernels"])) {
            py::tuple t = py::cast<py::tuple>(item);
            require(t.size() == 3, "_write_g2o: a kernel is ([vertices], type, delta)");
            gf.kernels.push_back({py::cast<std::vector<int>>(t[0]), py::cast<std::string>(t[1]), py::cast<double>(t[2])});
        }
    require(write_g2o(path, gf), "_write_g2o: cannot write the file");
}
// graph_save (hdl_graph_slam_nodelet.cpp:1088-1110): graph.g2o (+ .kernels, GraphSLAM::save) and special_nodes.csv into `directory`, the ids of
// the SE3 vertices as strings.  [] and no file without a pose graph.  The floor plane is not written: its vertex and edge classes are g2o's own,
// and the plane of this graph lives in the edge, not in a vertex -- floor_node is -1.  In localisation mode after a merge the merged graph's
// host record goes out the same way
py::list dump_graph(const std::string& directory) {
    py::list out;
    if (!g) return out;
    G2oFile gf;
    bool have = false, ok = true;
    {
        py::gil_scoped_release rel;
        if (g->loc) {
            std::lock_guard<std::mutex> lk(g->mtx);
            const Loc& L = *g->loc;
            if (L.have_mgraph) {
                have = true;
                for (const KeyFrameDisk& kf : L.frames) {
                    G2oFile::Vertex v;
                    v.id = kf.id;
                    tq_of(kf.odom.m, v.v);
                    gf.vertices.push_back(v);
                }
                gf.fixed.assign(L.mfixed.begin(), L.mfixed.end());
                for (const Loc::MergeEdge& me : L.medges) {
                    G2oFile::Edge e;
                    e.from = me.a; e.to = me.b;
                    tq_of(me.M, e.m);
                    std::memcpy(e.info, me.info, sizeof(e.info));
                    gf.edges.push_back(e);
                    if (me.kernel != LIO_GRAPH_KERNEL_NONE) gf.kernels.push_back({{me.a, me.b}, kernel_name(me.kernel), 1.0});
                }
                for (const Loc::MergePrior& mp : L.mpriors) {  // (none unless the merge ran under set_gnss)
                    G2oFile::Prior p;
                    p.node = mp.kf;
                    if (mp.type == LIO_GRAPH_PRIOR_XYZ) { p.tag = "EDGE_SE3_PRIORXYZ"; p.values = {mp.m[0], mp.m[1], mp.m[2]}; }
                    else { p.tag = "EDGE_SE3_PRIORQUAT"; p.values = {mp.m[3], mp.m[0], mp.m[1], mp.m[2]}; }
                    for (int r = 0; r < 3; r++)
                        for (int c = r; c < 3; c++) p.values.push_back(mp.info[r * 3 + c]);
                    gf.priors.push_back(p);
                    if (mp.kernel != LIO_GRAPH_KERNEL_NONE) gf.kernels.push_back({{mp.kf}, kernel_name(mp.kernel), mp.delta});
                }
            }
        } else {
            std::lock_guard<std::mutex> kl(g->kf_mtx);
            if (g->graph) {
                have = true;
                lio_graph* gr = g->graph;
                const int nn = lio_graph_num_nodes(gr);
                std::vector<uint8_t> live((size_t)std::max(nn, 1)), fixed((size_t)std::max(nn, 1));
                std::vector<double> est(16 * (size_t)std::max(nn, 1));
                require(lio_graph_node_live(gr, live.data(), (uint32_t)nn) == nn && lio_graph_get_fixed(gr, fixed.data(), (uint32_t)nn) == nn &&
                            lio_graph_estimates(gr, est.data(), (uint32_t)nn) == nn, "dump_graph: reading the nodes failed");
                for (int n = 0; n < nn; n++) {
                    if (!live[(size_t)n]) continue;
                    G2oFile::Vertex v;
                    v.id = n;
                    tq_of(&est[16 * (size_t)n], v.v);
                    gf.vertices.push_back(v);
                    if (fixed[(size_t)n]) gf.fixed.push_back(n);
                }
                const int ne = -lio_graph_edge_records(gr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
                if (ne > 0) {
                    std::vector<int32_t> from((size_t)ne), to((size_t)ne), kernel((size_t)ne);
                    std::vector<double> M(16 * (size_t)ne), W(36 * (size_t)ne), delta((size_t)ne);
                    require(lio_graph_edge_records(gr, nullptr, from.data(), to.data(), M.data(), W.data(), kernel.data(), delta.data(), (uint32_t)ne) == ne,
                            "dump_graph: lio_graph_edge_records failed");
                    for (int k = 0; k < ne; k++) {
                        G2oFile::Edge e;
                        e.from = from[(size_t)k]; e.to = to[(size_t)k];
                        tq_of(&M[16 * (size_t)k], e.m);
                        std::memcpy(e.info, &W[36 * (size_t)k], sizeof(e.info));
                        gf.edges.push_back(e);
                        if (kernel[(size_t)k] != LIO_GRAPH_KERNEL_NONE) gf.kernels.push_back({{e.from, e.to}, kernel_name(kernel[(size_t)k]), delta[(size_t)k]});
                    }
                }
                const int np = -lio_graph_priors(gr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
                if (np > 0) {
                    std::vector<int32_t> node((size_t)np), type((size_t)np), kernel((size_t)np);
                    std::vector<double> m(4 * (size_t)np), W(9 * (size_t)np), delta((size_t)np);
                    require(lio_graph_priors(gr, nullptr, node.data(), type.data(), m.data(), nullptr, W.data(), kernel.data(), delta.data(), (uint32_t)np) == np,
                            "dump_graph: lio_graph_priors failed");
                    for (int k = 0; k < np; k++) {
                        if (type[(size_t)k] == LIO_GRAPH_PRIOR_PLANE) continue;
                        const double* mk = &m[4 * (size_t)k];
                        const double* Wk = &W[9 * (size_t)k];
                        G2oFile::Prior p;
                        p.node = node[(size_t)k];
                        if (type[(size_t)k] == LIO_GRAPH_PRIOR_XYZ) { p.tag = "EDGE_SE3_PRIORXYZ"; p.values = {mk[0], mk[1], mk[2]}; }
                        else { p.tag = "EDGE_SE3_PRIORQUAT"; p.values = {mk[3], mk[0], mk[1], mk[2]}; }
                        for (int r = 0; r < 3; r++)
                            for (int c = r; c < 3; c++) p.values.push_back(Wk[r * 3 + c]);
                        gf.priors.push_back(p);
                        if (kernel[(size_t)k] != LIO_GRAPH_KERNEL_NONE) gf.kernels.push_back({{p.node}, kernel_name(kernel[(size_t)k]), delta[(size_t)k]});
                    }
                }
            }
        }
        if (have) {
            ok = write_g2o(directory + "/graph.g2o", gf);
            if (ok && gf.kernels.empty()) ok = (bool)std::ofstream(directory + "/graph.g2o.kernels");  // (save_robust_kernels always makes the file)
            std::ofstream ofs(directory + "/special_nodes.csv");
            ofs << "anchor_node " << -1 << std::endl << "anchor_edge " << -1 << std::endl << "floor_node " << -1 << std::endl;
            ok = ok && (bool)ofs;
        }
    }
    require(ok, "dump_graph: cannot write into the directory");
    std::vector<int> ids;
    for (const auto& v : gf.vertices) ids.push_back(v.id);
    std::sort(ids.begin(), ids.end());
    for (int id : ids) out.append(std::to_string(id));
    return out;
}
// dump_odometry (graph_utils.cpp:133-145): odometrys.txt, `stamp x y z qx qy qz qw` a line in fixed notation with 6 decimals; an empty list
// still makes the file
void dump_odometry(const std::string& directory) {
    std::vector<std::pair<uint64_t, Mat4>> od;
    if (g) {
        std::lock_guard<std::mutex> lk(g->mtx);
        od = g->odometrys;
    }
    std::ofstream ofs(directory + "/odometrys.txt");
    for (const auto& o : od) {
        double q[4];
        quat_of(o.second, q);
        ofs << std::fixed << std::setprecision(6) << (double)o.first / 1000000.0 << " " << o.second(0, 3) << " " << o.second(1, 3) << " " << o.second(2, 3) << " " << q[1] << " "
            << q[2] << " " << q[3] << " " << q[0] << std::endl;
    }
}
// graph_del_vertex (hdl_graph_slam_nodelet.cpp:868-891): the key frame leaves the list, its vertex and every edge on it leave the graph; here its
// frame of the detector's bank is retired as well, which is what leaving `keyframes` means to LoopDetector::detect.  Nothing without a graph, a
// warning for an id the graph does not hold
void del_graph_vertex(int id) {
    if (!g) return;
    py::gil_scoped_release rel;
    std::lock_guard<std::mutex> kl(g->kf_mtx);
    if (!g->graph) return;
    if (id < 0 || (size_t)id >= g->graph_gone.size() || g->graph_gone[(size_t)id]) {
        std::fprintf(stderr, "slam_wrapper: del_graph_vertex: Vertex ID %d does not exist!!\n", id);
        return;
    }
    require(lio_graph_remove_node(g->graph, id) == LIO_OK, "del_graph_vertex: lio_graph_remove_node failed");
    if (g->loop) require(lio_loop_retire(g->loop, id) == LIO_OK, "del_graph_vertex: lio_loop_retire failed");
    g->graph_gone[(size_t)id] = 1;
    g->graph_updated = false;
}
// align_pose (graph_utils.cpp:230-282), statement for statement in f64: the poses between two aligned frames are made relative to the first
// (from the back of the list forward, so poses[0] is still the original while the others use it), the difference between the estimates' delta
// and the list's own is spread over the list by time -- with stamp2 - stamp1 as the duration, not the list's span -- as a translation and a
// rotation vector whose norm goes through a float before the 1e-8 test.  An empty list returns an empty list (the reference reads poses.back())
py::list align_pose(double stamp1, double stamp2, py::array_t<double>& estimate1_py, py::array_t<double>& estimate2_py, py::array_t<double>& poses_stamp,
                    py::list& poses_py) {
    py::list out;
    std::vector<Mat4> poses;
    auto mat_of = [](py::handle h, const char* what) {
        auto a = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(py::reinterpret_borrow<py::object>(h));
        require(a && a.size() == 16, what);
        Mat4 T;
        std::memcpy(T.m, a.data(), sizeof(T.m));
        return T;
    };
    for (auto pose : poses_py) poses.push_back(mat_of(pose, "align_pose: a pose is 4 x 4"));
    if (poses.empty()) return out;
    auto st = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(poses_stamp);
    require(st && (size_t)st.size() >= poses.size(), "align_pose: a stamp for every pose");
    const double* pose_stamp = st.data();
    const int n = (int)poses.size();
    for (int i = n - 1; i >= 0; i--) poses[(size_t)i] = mul(inverse4(poses[0]), poses[(size_t)i]);
    const Mat4 estimate1 = mat_of(estimate1_py, "align_pose: estimate1 is 4 x 4"), estimate2 = mat_of(estimate2_py, "align_pose: estimate2 is 4 x 4");
    const Mat4 delta_odom = mul(inverse4(estimate1), estimate2);
    const Mat4 dd = mul(inverse4(poses.back()), delta_odom);
    double dq[4];
    quat_of(dd, dq);
    // Eigen::AngleAxisd(q): angle = 2 atan2(|vec|, |w|), the axis vec / |vec| with the sign of w; no rotation: angle 0 about x
    double vn = std::sqrt(dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]), angle = 0, axis[3] = {1, 0, 0};
    if (vn != 0.0) {
        angle = 2.0 * std::atan2(vn, std::fabs(dq[0]));
        if (dq[0] < 0) vn = -vn;
        for (int i = 0; i < 3; i++) axis[i] = dq[1 + i] / vn;
    }
    const double duration = stamp2 - stamp1;
    for (int i = 0; i < n; i++) {
        const double ratio = (pose_stamp[i] - pose_stamp[0]) / duration;
        const double lt[3] = {ratio * dd(0, 3), ratio * dd(1, 3), ratio * dd(2, 3)};
        const double lr[3] = {ratio * (angle * axis[0]), ratio * (angle * axis[1]), ratio * (angle * axis[2])};
        const float norm = (float)std::sqrt(lr[0] * lr[0] + lr[1] * lr[1] + lr[2] * lr[2]);
        Mat4 plus = Mat4::identity();
        if (!(norm < 1e-8)) {  // Quaterniond(AngleAxisd(norm, lr / norm)).toRotationMatrix()
            const double a = (double)norm, sh = std::sin(0.5 * a), w = std::cos(0.5 * a);
            const double x = sh * (lr[0] / a), y = sh * (lr[1] / a), z = sh * (lr[2] / a);
            const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
            const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
            plus(0, 0) = 1 - (tyy + tzz); plus(0, 1) = txy - twz; plus(0, 2) = txz + twy;
            plus(1, 0) = txy + twz; plus(1, 1) = 1 - (txx + tzz); plus(1, 2) = tyz - twx;
            plus(2, 0) = txz - twy; plus(2, 1) = tyz + twx; plus(2, 2) = 1 - (txx + tyy);
        }
        for (int r = 0; r < 3; r++) plus(r, 3) = lt[r];
        poses[(size_t)i] = mul(estimate1, mul(poses[(size_t)i], plus));
    }
    for (const Mat4& T : poses) {
        py::array_t<double> a({4, 4});
        std::memcpy(a.mutable_data(), T.m, sizeof(T.m));
        out.append(a);
    }
    return out;
}

py::tuple _colouration_last() {
    auto to_np = [](const Mat4& T) {
        py::array_t<double> a({4, 4});
        std::memcpy(a.mutable_data(), T.m, sizeof(T.m));
        return a;
    };
    py::array_t<float> f({(py::ssize_t)(g_col.last_frame.size() / 4), (py::ssize_t)4});
    if (!g_col.last_frame.empty()) std::memcpy(f.mutable_data(), g_col.last_frame.data(), g_col.last_frame.size() * sizeof(float));
    py::dict im;
    for (const auto& p : g_col.last_images) im[p.first.c_str()] = to_np(p.second);
    return py::make_tuple(g_col.last_outcome, f, to_np(g_col.last_pose), im);
}
py::tuple _stamp_pose(uint64_t stamp, int start_idx) {
    int idx = -1;
    TumPose p;
    p.T = Mat4::identity();
    const bool ok = get_stamp_pose(stamp, start_idx, idx, p);
    py::array_t<double> a({4, 4});
    std::memcpy(a.mutable_data(), p.T.m, sizeof(p.T.m));
    return py::make_tuple(ok, idx, a);
}

// test visibility (not in the reference's module): the engine behind the module, so that a test can hold the C++ path against the C ABI
uintptr_t _engine_handle() { return g ? reinterpret_cast<uintptr_t>(g->engine) : 0; }
py::array_t<double> _transform_from_rpyt(double x, double y, double z, double yaw, double pitch, double roll) {  // the module's getTransformFromRPYT
    const Mat4 T = transform_from_rpyt(x, y, z, yaw, pitch, roll);
    py::array_t<double> a({4, 4});
    auto r = a.mutable_unchecked<2>();
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) r(i, j) = T(i, j);
    return a;
}
// _tum_relative_poses(poses) -> (T0, [T0^-1 * T_i]): numpy_to_odometry + undistortion_cloud's relative poses, as the module computes them
py::tuple _tum_relative_poses(py::array_t<double>& poses) {
    const std::vector<TumPose> tum = tum_poses(poses);
    auto to_np = [](const Mat4& T) {
        py::array_t<double> a({4, 4});
        auto r = a.mutable_unchecked<2>();
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) r(i, j) = T(i, j);
        return a;
    };
    py::list rel;
    for (const Mat4& T : relative_poses(tum)) rel.append(to_np(T));
    if (tum.empty()) throw std::invalid_argument("slam_wrapper: _tum_relative_poses: no poses");
    return py::make_tuple(to_np(tum[0].T), rel);
}
// texture_mesh's readers and writer without a device: _read_rgb_pcd(path) -> (xyz f32 n x 3, rgb u32 n); _read_obj(path) -> (vertices f32 m x 3,
// [faces]); _write_mesh_ply(path, vertices, rgb m x 3 uint8, faces)
py::tuple _read_rgb_pcd(std::string path) {
    std::vector<float> xyz;
    std::vector<uint32_t> rgb;
    read_rgb_pcd(path, xyz, rgb, "_read_rgb_pcd");
    py::array_t<float> a({(py::ssize_t)rgb.size(), (py::ssize_t)3});
    py::array_t<uint32_t> c((py::ssize_t)rgb.size());
    if (!rgb.empty()) {
        std::memcpy(a.mutable_data(), xyz.data(), xyz.size() * 4);
        std::memcpy(c.mutable_data(), rgb.data(), rgb.size() * 4);
    }
    return py::make_tuple(a, c);
}
py::tuple _read_obj(std::string path) {
    std::vector<float> v;
    std::vector<int32_t> faces;
    std::vector<uint32_t> fs;
    read_obj(path, v, faces, fs, "_read_obj");
    py::array_t<float> a({(py::ssize_t)(v.size() / 3), (py::ssize_t)3});
    if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * 4);
    py::list fl;
    size_t k = 0;
    for (uint32_t c : fs) {
        py::list f;
        for (uint32_t j = 0; j < c; j++) f.append(faces[k + j]);
        k += c;
        fl.append(f);
    }
    return py::make_tuple(a, fl);
}
// detect_ground (graph_utils.cpp:329-382; preset 1: the floor detector's parameters) over a host cloud: (coeffs (4,) f32 or None, inliers N x 4)
py::tuple _detect_ground(py::array_t<float>& points, int preset, uint32_t seed) {
    std::vector<float> xyzi = xyzi_of(points, "_detect_ground");
    need_ground("_detect_ground");
    lio_ground_params gp;
    lio_ground_default_params(&gp, preset);
    gp.seed = seed;
    int found = 0;
    float coeffs[4];
    uint32_t ni = 0;
    require(lio_ground_detect_host(g_acc.ground, xyzi.data(), xyzi.size() / 4, &gp, &found, coeffs, nullptr, nullptr, &ni) == LIO_OK, "_detect_ground failed");
    if (!found) return py::make_tuple(py::none(), py::array_t<float>(std::vector<py::ssize_t>{0, 4}));
    py::array_t<float> in({(py::ssize_t)ni, (py::ssize_t)4});
    require(lio_ground_download_inliers(g_acc.ground, in.mutable_data(), ni) == (int64_t)ni, "_detect_ground: download failed");
    py::array_t<float> co(4);
    std::memcpy(co.mutable_data(), coeffs, sizeof(coeffs));
    return py::make_tuple(co, in);
}
void _write_mesh_ply(std::string path, py::array_t<float, py::array::c_style | py::array::forcecast> vertices,
                     py::array_t<uint8_t, py::array::c_style | py::array::forcecast> rgb, py::list faces) {
    if (vertices.ndim() != 2 || vertices.shape(1) != 3) throw std::invalid_argument("slam_wrapper: _write_mesh_ply: vertices must be m x 3");
    const size_t nv = (size_t)vertices.shape(0);
    if (rgb.ndim() != 2 || rgb.shape(1) != 3 || (size_t)rgb.shape(0) != nv) throw std::invalid_argument("slam_wrapper: _write_mesh_ply: rgb must be m x 3");
    std::vector<int32_t> flat;
    std::vector<uint32_t> fs;
    for (py::handle f : faces) {
        const std::vector<int32_t> idx = py::cast<std::vector<int32_t>>(f);
        if (idx.empty() || idx.size() > 255) throw std::invalid_argument("slam_wrapper: _write_mesh_ply: a face has 1 to 255 vertices");
        flat.insert(flat.end(), idx.begin(), idx.end());
        fs.push_back((uint32_t)idx.size());
    }
    if (!write_mesh_ply(path, vertices.data(), rgb.data(), nv, flat.data(), fs.data(), fs.size()))
        throw std::invalid_argument("slam_wrapper: _write_mesh_ply: cannot write '" + path + "'");
}
void _set_capacity(uint64_t max_points, uint64_t max_voxels) { if (g) { g->max_points = max_points; g->max_voxels = max_voxels; } }

PYBIND11_MODULE(slam_wrapper, m) {
    m.doc() = "mapping python interface (MI355X-native LIO core behind the reference's slam_wrapper surface)";
    m.def("init_slam", &init_slam, "init slam", py::arg("mode"), py::arg("map_path"), py::arg("method"), py::arg("sensor_input"), py::arg("resolution"),
          py::arg("dist_threshold"), py::arg("degree_threshold"), py::arg("frame_range"));
    m.def("setup_slam", &setup_slam, py::call_guard<py::gil_scoped_release>());
    m.def("deinit_slam", &deinit_slam, "deinit slam");
    m.def("set_camera_param", &set_camera_param, "set camera parameters", py::arg("cameras"));
    m.def("set_ins_external_param", &set_ins_external_param, "set ins external param", py::arg("x"), py::arg("y"), py::arg("z"), py::arg("yaw"), py::arg("pitch"),
          py::arg("roll"));
    m.def("set_imu_external_param", &set_imu_external_param, "set imu external param", py::arg("x"), py::arg("y"), py::arg("z"), py::arg("yaw"), py::arg("pitch"),
          py::arg("roll"));
    m.def("set_ins_config", &set_ins_config, "set ins config", py::arg("dict"));
    m.def("set_init_pose", &set_init_pose, "set init pose", py::arg("x"), py::arg("y"), py::arg("z"), py::arg("yaw"), py::arg("pitch"), py::arg("roll"));
    m.def("get_estimate_pose", &get_estimate_pose, "get estimate pose", py::arg("x0"), py::arg("y0"), py::arg("x1"), py::arg("y1"));
    m.def("set_destination", &set_destination, "set destination", py::arg("enable"), py::arg("dest"), py::arg("port"));
    m.def("process", &process, "process", py::arg("points"), py::arg("points_attr"), py::arg("image_dict"), py::arg("image_stream_dict"), py::arg("image_param"),
          py::arg("rtk_dict"), py::arg("imu_list"), py::arg("timestamp"));
    m.def("update_odom", &update_odom, "update odom");
    m.def("get_graph_status", &get_graph_status, "get graph status");
    m.def("get_map_origin", &get_map_origin, "get map origin");
    m.def("set_map_origin", &set_map_origin, "set map origin", py::arg("lat"), py::arg("lon"), py::arg("alt"), py::arg("heading"), py::arg("pitch"), py::arg("roll"));
    m.def("get_color_map", &get_color_map, "get color map");
    m.def("merge_map", &merge_map, "merge map", py::arg("directory"));
    m.def("_read_g2o", &_read_g2o, py::arg("path"));
    m.def("_write_g2o", &_write_g2o, py::arg("path"), py::arg("record"));
    m.def("_last_merge", &_last_merge);
    m.def("get_graph_map", &get_graph_map, "get graph map");
    m.def("get_graph_edges", &get_graph_edges, "get graph edges");
    m.def("pointcloud_align", &pointcloud_align, "pointcloud align", py::arg("source_point"), py::arg("target_point"), py::arg("guess"));
    m.def("set_mapping_ground_constraint", &set_mapping_ground_constraint, "set mapping ground constraint", py::arg("enable"));
    m.def("get_mapping_ground_constraint", &get_mapping_ground_constraint, "get mapping ground constraint");
    m.def("set_mapping_constraint", &set_mapping_constraint, "set mapping constraint", py::arg("loop_closure"), py::arg("gravity_constraint"));
    m.def("set_map_colouration", &set_map_colouration, "set map colouration", py::arg("enable"));
    m.def("get_graph_meta", &get_graph_meta, "get graph meta");
    m.def("del_graph_vertex", &del_graph_vertex, "del graph vertex", py::arg("id"));
    m.def("add_graph_edge", &add_graph_edge, "add graph edge", py::arg("prev"), py::arg("prev_id"), py::arg("next"), py::arg("next_id"), py::arg("relative"));
    m.def("del_graph_edge", &del_graph_edge, "del graph edge", py::arg("id"));
    m.def("set_graph_vertex_fix", &set_graph_vertex_fix, "set graph vertex fix", py::arg("id"), py::arg("fix"));
    m.def("run_graph_optimization", &run_graph_optimization, "run graph optimization");
    m.def("run_robust_graph_optimization", &run_robust_graph_optimization, "run robust graph optimization", py::arg("mode"));
    m.def("add_graph_gnss", &add_graph_gnss, "one GNSS fix for a key frame of the pose graph; the ids of the edges added", py::arg("id"), py::arg("xyz"), py::arg("precision"),
          py::arg("dimension"), py::arg("orientation") = py::none());
    m.def("_graph_priors", &_graph_priors, "test visibility: the pose graph's live priors");
    m.def("dump_keyframe", &dump_keyframe, "dump keyframe", py::arg("directory"), py::arg("stamp"), py::arg("id"), py::arg("points_input"), py::arg("pose_input"));
    m.def("dump_odometry", &dump_odometry, "dump odometry", py::arg("directory"));
    m.def("set_export_map_config", &set_export_map_config, "set export map config", py::arg("z_min"), py::arg("z_max"), py::arg("color"));
    m.def("export_points", &export_points, "export points", py::arg("points_input"), py::arg("odom_input"));
    m.def("dump_map_points", &dump_map_points, "dump map points", py::arg("file"));
    m.def("dump_graph", &dump_graph, "dump graph", py::arg("directory"));
    m.def("align_pose", &align_pose, "align pose", py::arg("stamp1"), py::arg("stamp2"), py::arg("estimate1_py"), py::arg("estimate2_py"), py::arg("poses_stamp"),
          py::arg("poses_py"));
    m.def("save_undistortion_cloud", &save_undistortion_cloud, "save undistortion cloud", py::arg("file"), py::arg("points"), py::arg("points_attr"), py::arg("poses"));
    m.def("accumulate_cloud", &accumulate_cloud, "accumulate cloud", py::arg("points"), py::arg("points_attr"), py::arg("poses"), py::arg("odometry_type"),
          py::arg("extract_ground"));
    m.def("save_accumulate_cloud", &save_accumulate_cloud, "save accumulate cloud", py::arg("file"), py::arg("resolution"));
    m.def("texture_mesh", &texture_mesh, "texture mesh", py::arg("mesh_path"), py::arg("cloud_path"), py::arg("output_path"));
    m.def("set_colouration_config", &set_colouration_config, "set colouration config", py::arg("cameras"));
    m.def("set_map_odometrys", &set_map_odometrys, "set map odometrys", py::arg("poses"));
    m.def("colouration_frame", &colouration_frame, "colouration frame", py::arg("lidar_name"), py::arg("points"), py::arg("points_attr"), py::arg("image_dict"),
          py::arg("image_stream_dict"), py::arg("image_param"));
    m.def("save_render_cloud", &save_render_cloud, "save render cloud", py::arg("file"));
    m.def("set_colouration_seed", &set_colouration_seed, "seed of the ground test's draws in colouration_frame", py::arg("seed"));
    m.def("_colouration_last", &_colouration_last);
    m.def("_stamp_pose", &_stamp_pose, py::arg("stamp"), py::arg("start_idx"));
    m.def("set_keyframe_output", &set_keyframe_output, "key frames from process() through update_odom()", py::arg("enable"));
    m.def("set_loop_detection", &set_loop_detection, "loop detection over the key frames update_odom() hands out", py::arg("enable"));
    m.def("set_global_localization", &set_global_localization, "scan-context relocalisation in localisation mode", py::arg("enable"));
    m.def("_last_relocalization", &_last_relocalization);
    m.def("_last_estimate_pose", &_last_estimate_pose);
    m.def("set_pose_graph", &set_pose_graph, "the pose graph over the key frames and the loops", py::arg("enable"));
    m.def("_push_keyframe", &_push_keyframe, "test hook: a key frame for the next update_odom()", py::arg("points"), py::arg("pose"), py::arg("stamp"), py::arg("accum_distance"));
    m.def("set_gnss", &set_gnss, "the GNSS side (off by default).  FastLIO mapping: origin from the first valid fix, GNSS priors in the pose graph.  Localisation mode: an INS-aided "
          "initial pose (local Scan Context search), fixes fused by the pose filter, state Localizing(L+G) and a global-search threshold of 0.25, all "
          "four only with RTK among the sensors; merge_map takes a map recorded under another origin (re-anchored to the loaded map's) and carries "
          "both maps' GNSS priors",
          py::arg("enable"));
    m.def("_push_gnss", &_push_gnss, "test hook: what process() does with a fix", py::arg("rtk_dict"));
    m.def("set_gnss_moment", &set_gnss_moment, "the GNSS moment stage of run_robust_graph_optimization(\"mapping\") (off by default)", py::arg("enable"));
    m.def("_last_gnss_moment", &_last_gnss_moment, "test hook: the moment, the priors moved and the report of the last moment stage; {} when it did not run");
    m.def("_last_merged", &_last_merged, "test hook: points and stamps of the last RTKM frame");
    m.def("_gnss_state", &_gnss_state, "test hook: the state of the GNSS side");
    m.def("set_loop_config", &set_loop_config, "LoopDetector thresholds", py::arg("dict"));
    m.def("get_loop_edges", &get_loop_edges, "loop edges found so far");
    m.def("_last_odometry", &_last_odometry);
    m.def("_engine_handle", &_engine_handle);
    m.def("_transform_from_rpyt", &_transform_from_rpyt);
    m.def("_tum_relative_poses", &_tum_relative_poses, py::arg("poses"));
    m.def("_read_rgb_pcd", &_read_rgb_pcd, py::arg("path"));
    m.def("_read_obj", &_read_obj, py::arg("path"));
    m.def("set_ground_extraction", &set_ground_extraction,
          "accumulate_cloud(extract_ground=True) on the device (off by default); the RANSAC draws are this module's counter-based generator of (seed, draw), not PCL's",
          py::arg("enable"), py::arg("seed") = 0);
    m.def("_detect_ground", &_detect_ground, py::arg("points"), py::arg("preset") = 0, py::arg("seed") = 0);
    m.def("_write_mesh_ply", &_write_mesh_ply, py::arg("path"), py::arg("vertices"), py::arg("rgb"), py::arg("faces"));
    m.def("_set_capacity", &_set_capacity, py::arg("max_points"), py::arg("max_voxels"));
}
