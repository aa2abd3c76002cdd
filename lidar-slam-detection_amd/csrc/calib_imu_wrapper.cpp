// calib_imu_wrapper.cpp -- the reference's outer boundary of the lidar-IMU calibration: the pybind11 module `calib_imu_ext` with the seven
// calib_imu_* functions of sensor_driver/calibration/calib_wrapper.cpp:131-251 (names, argument names, return types), over the C ABI's
// lio_calib_imu_* (include/lio_hip.h).  They live in a module of their own because `calib_driver_ext` is pinned to hold the calib_ins_* half
// alone; lsd_amd/calib_driver.py joins the two under the reference's thirteen names.
//
//   calib_imu_reset            a fresh object (frames, IMU samples, map, last pose, the "no RTK" flag)
//   calib_imu_set_points       addLidarData(points, time / 1e6, pose = global_T, odom = delta_T); ignored from the 200th frame on
//   calib_imu_set_imu          rows of (stamp us, gyro deg/s x 3, acc g x 3)
//   calib_imu_calibrate        3 x 3 float32; zeros and a warning where the reference reads past the end (no IMU sample, no frame left)
//   calib_imu_get_lidar_poses / calib_imu_get_imu_poses   lists of 4 x 4 float32
//   calib_imu_get_lidar_T_R    4 x 4 float32: the pose of the frame against the local map, identity when the matcher did not converge
//
// A call before calib_imu_reset creates the object (the reference's static object exists from the import on; the effect is the same).  The
// device is opened by the first call that handles a cloud, not at import; without one that call raises RuntimeError.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/lio_hip.h"

namespace py = pybind11;

namespace {

lio_calib_imu* g_calib = nullptr;
constexpr uint32_t kMaxScanPoints = 1u << 19;  // one frame: 64 beams x 1875 azimuths is 120 000
constexpr uint32_t kMaxMapPoints = 1u << 23;   // 200 key frames filtered at 0.2 m

lio_calib_imu* handle() {
    if (!g_calib) {
        g_calib = lio_calib_imu_create(0, kMaxScanPoints, kMaxMapPoints);
        if (!g_calib) throw std::runtime_error(std::string("calib_imu_ext: ") + lio_last_error());
    }
    return g_calib;
}

void must(int64_t rc, const char* what) {
    if (rc < 0) throw std::runtime_error(std::string("calib_imu_ext: ") + what + ": " + lio_last_error());
}

void matrix_of(const py::array_t<float>& array, double M[16]) {
    auto ref = array.unchecked<2>();
    if (ref.shape(0) < 4 || ref.shape(1) < 4) throw std::invalid_argument("calib_imu_ext: a 4 x 4 array is expected");
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) M[4 * i + j] = ref(i, j);
}

// x y z intensity of every row, packed
std::vector<float> rows_of(const py::array_t<float>& array) {
    auto ref = array.unchecked<2>();
    if (ref.shape(0) > 0 && ref.shape(1) < 4) throw std::invalid_argument("calib_imu_ext: points must be N x (>= 4)");
    std::vector<float> rows((size_t)ref.shape(0) * 4);
    for (py::ssize_t i = 0; i < ref.shape(0); i++)
        for (int j = 0; j < 4; j++) rows[4 * (size_t)i + j] = ref(i, j);
    return rows;
}

py::array_t<float> matrix_out(const double* M, int n) {
    std::vector<float> data((size_t)n * n);
    for (int i = 0; i < n * n; i++) data[i] = (float)M[i];
    return py::array_t<float>(py::array::ShapeContainer({n, n}), data.data());
}

void calib_imu_reset() { must(lio_calib_imu_reset(handle()), "calib_imu_reset"); }

void calib_imu_set_points(py::array_t<float>& points, unsigned long long time, py::array_t<float>& odom, py::array_t<float>& pose) {
    double odomT[16], poseT[16];
    matrix_of(odom, odomT);
    matrix_of(pose, poseT);
    const std::vector<float> rows = rows_of(points);
    must(lio_calib_imu_add_frame(handle(), time, rows.data(), (uint32_t)(rows.size() / 4), 4, poseT, odomT), "calib_imu_set_points");
}

void calib_imu_set_imu(py::array_t<double>& array) {
    auto ref = array.unchecked<2>();
    if (ref.shape(0) > 0 && ref.shape(1) < 7) throw std::invalid_argument("calib_imu_ext: IMU rows must be N x (>= 7)");
    std::vector<double> rows((size_t)ref.shape(0) * 7);
    for (py::ssize_t i = 0; i < ref.shape(0); i++)
        for (int j = 0; j < 7; j++) rows[7 * (size_t)i + j] = ref(i, j);
    must(lio_calib_imu_add_imu(handle(), rows.data(), (uint32_t)ref.shape(0)), "calib_imu_set_imu");
}

py::array_t<float> calib_imu_calibrate() {
    double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int rc = lio_calib_imu_calibrate(handle(), R);
    if (rc == LIO_E_STATE) std::fprintf(stderr, "[calib_imu_ext] %s: zeros returned\n", lio_last_error());
    else must(rc, "calib_imu_calibrate");
    return matrix_out(R, 3);
}

template <typename F>
py::list poses_of(F fn, const char* what) {
    uint32_t aligned = 0;
    must(lio_calib_imu_counts(handle(), nullptr, nullptr, &aligned, nullptr, nullptr, nullptr), what);
    std::vector<double> P(16 * (size_t)(aligned ? aligned : 1));
    const int64_t n = fn(handle(), P.data(), aligned);
    must(n, what);
    py::list result;
    for (int64_t i = 0; i < n; i++) result.append(matrix_out(P.data() + 16 * i, 4));
    return result;
}

py::list calib_imu_get_lidar_poses() { return poses_of(lio_calib_imu_lidar_poses, "calib_imu_get_lidar_poses"); }
py::list calib_imu_get_imu_poses() { return poses_of(lio_calib_imu_imu_poses, "calib_imu_get_imu_poses"); }

py::array_t<float> calib_imu_get_lidar_T_R(py::array_t<float>& points) {
    const std::vector<float> rows = rows_of(points);
    double T[16];
    must(lio_calib_imu_lidar_pose(handle(), rows.data(), (uint32_t)(rows.size() / 4), 4, T), "calib_imu_get_lidar_T_R");
    return matrix_out(T, 4);
}

}  // namespace

PYBIND11_MODULE(calib_imu_ext, m) {
    m.doc() = "calibration interface: lidar-IMU";
    m.def("calib_imu_reset", &calib_imu_reset, "calib_imu_reset");
    m.def("calib_imu_set_points", &calib_imu_set_points, "calib_imu_set_points", py::arg("points"), py::arg("time"), py::arg("odom"), py::arg("pose"));
    m.def("calib_imu_set_imu", &calib_imu_set_imu, "calib_imu_set_imu", py::arg("array"));
    m.def("calib_imu_calibrate", &calib_imu_calibrate, "calib_imu_calibrate");
    m.def("calib_imu_get_lidar_poses", &calib_imu_get_lidar_poses, "calib_imu_get_lidar_poses");
    m.def("calib_imu_get_imu_poses", &calib_imu_get_imu_poses, "calib_imu_get_imu_poses");
    m.def("calib_imu_get_lidar_T_R", &calib_imu_get_lidar_T_R, "calib_imu_get_lidar_T_R");
    // test hooks of this project (leading underscore: not part of the reference's surface)
    m.def("_counts", []() {
        uint32_t f = 0, i = 0, a = 0, mp = 0, tp = 0;
        int flag = 0;
        must(lio_calib_imu_counts(handle(), &f, &i, &a, &mp, &tp, &flag), "_counts");
        return py::make_tuple(f, i, a, mp, tp, flag);
    });
    m.def("_set_max_iterations", [](int n) { must(lio_calib_imu_set_max_iterations(handle(), n), "_set_max_iterations"); });
}
