// calib_wrapper.cpp -- the reference's outer boundary of the lidar-INS calibration: the pybind11 module `calib_driver_ext` with the six
// calib_ins_* functions of sensor_driver/calibration/calib_wrapper.cpp:41-115 (names, argument names, behaviour), over the C ABI's
// lio_calib_ins_* (include/lio_hip.h).  The seven calib_imu_* names of the reference's module are NOT defined here: the lidar-IMU
// calibration has a module of its own, calib_imu_ext (calib_imu_wrapper.cpp).
//
//   calib_ins_reset                      joins a running optimisation, drops scans and odometry, current = best = Transform(initArray)
//   calib_ins_set_points                 ignored with a warning while an optimisation thread exists; ignored from the 21st scan on; N x >= 3
//   calib_ins_set_odom                   ignored with a warning while an optimisation thread exists
//   calib_ins_calibrate                  sets the scan poses at offset 0, then runs lio_calib_ins_calibrate on a std::thread (no GIL held)
//   calib_ins_get_calibration            {"finish", "percent"}: percent = evaluations / (2 max_evals) 100, 100 when finished
//   calib_ins_get_calibration_transform  4 x 4 float32 of the best transform
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <algorithm>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/lio_hip.h"

namespace py = pybind11;

namespace {

lio_calib_ins* g_calib = nullptr;
std::unique_ptr<std::thread> g_thread;
lio_calib_params g_params;

lio_calib_ins* handle() {
    if (!g_calib) {
        g_calib = lio_calib_ins_create(0);
        if (!g_calib) throw std::runtime_error(std::string("calib_driver_ext: the calibration needs a HIP device (there is no CPU fallback): ") + lio_last_error());
        lio_calib_default_params(&g_params);
    }
    return g_calib;
}

void must(int rc, const char* what) {
    if (rc < 0) throw std::runtime_error(std::string("calib_driver_ext: ") + what + ": " + lio_last_error());
}

void join() {
    if (g_thread) {
        py::gil_scoped_release release;
        g_thread->join();
    }
    g_thread.reset();
}

void matrix_of(const py::array_t<float>& array, float M[16]) {
    auto ref = array.unchecked<2>();
    if (ref.shape(0) < 4 || ref.shape(1) < 4) throw std::invalid_argument("calib_driver_ext: a 4 x 4 array is expected");
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) M[4 * i + j] = ref(i, j);
}

void calib_ins_reset(py::array_t<float>& initArray) {
    join();
    float M[16];
    matrix_of(initArray, M);
    must(lio_calib_ins_reset(handle(), M), "calib_ins_reset");
}

void calib_ins_set_points(py::array_t<float>& points, long long time) {
    if (g_thread) {
        std::fprintf(stderr, "[calib_driver_ext] INS calibration optimization is running, cannot set points\n");
        return;
    }
    uint32_t scans = 0;
    must(lio_calib_ins_counts(handle(), &scans, nullptr, nullptr), "calib_ins_set_points");
    if (scans >= 20) return;
    auto ref = points.unchecked<2>();
    if (ref.shape(0) > 0 && ref.shape(1) < 3) throw std::invalid_argument("calib_driver_ext: points must be N x (>= 3)");
    std::vector<float> xyz((size_t)ref.shape(0) * 3);
    for (py::ssize_t i = 0; i < ref.shape(0); i++)
        for (int j = 0; j < 3; j++) xyz[3 * (size_t)i + j] = ref(i, j);
    must(lio_calib_ins_add_scan(handle(), xyz.data(), (uint64_t)ref.shape(0), 3, time), "calib_ins_set_points");
}

void calib_ins_set_odom(py::array_t<float>& array, long long time) {
    if (g_thread) {
        std::fprintf(stderr, "[calib_driver_ext] INS calibration optimization is running, cannot set odometry\n");
        return;
    }
    float M[16];
    matrix_of(array, M);
    must(lio_calib_ins_add_odom(handle(), M, time), "calib_ins_set_odom");
}

void calib_ins_calibrate() {
    if (g_thread) {
        std::fprintf(stderr, "[calib_driver_ext] INS calibration optimization is running, waiting...\n");
        join();
    }
    lio_calib_ins* h = handle();
    uint32_t scans = 0;
    must(lio_calib_ins_counts(h, &scans, nullptr, nullptr), "calib_ins_calibrate");
    std::vector<float> mats(16 * std::max<uint32_t>(scans, 1));
    must(lio_calib_ins_scan_matrices(h, 0.0, mats.data()), "calib_ins_calibrate");  // lidar->setOdomOdomTransforms(*odom)
    const lio_calib_params p = g_params;
    g_thread.reset(new std::thread([h, p]() {
        // the thread selects the device itself (lio_calib_ins_calibrate does) and never touches Python
        if (lio_calib_ins_calibrate(h, &p) < 0) std::fprintf(stderr, "[calib_driver_ext] the calibration failed: %s\n", lio_last_error());
    }));
}

py::dict calib_ins_get_calibration() {
    int32_t evals = 0, finished = 0;
    must(lio_calib_ins_progress(handle(), &evals, nullptr, &finished), "calib_ins_get_calibration");
    py::dict result;
    // the reference's ratio runs a little past 100 (each stage adds one evaluation to its budget) before it is set to 100: held at 100 here
    const float percent = finished ? 100.0f : std::min(100.0f, float(evals) / (float(g_params.max_evals) * 2) * 100);
    result["finish"] = finished != 0;
    result["percent"] = percent;
    return result;
}

py::array_t<float> calib_ins_get_calibration_transform() {
    float M[16];
    must(lio_calib_ins_result(handle(), M), "calib_ins_get_calibration_transform");
    return py::array_t<float>(py::array::ShapeContainer({4, 4}), M);
}

}  // namespace

PYBIND11_MODULE(calib_driver_ext, m) {
    m.doc() = "calibration interface";
    m.def("calib_ins_reset", &calib_ins_reset, "calib_ins_reset", py::arg("initArray"));
    m.def("calib_ins_set_points", &calib_ins_set_points, "calib_ins_set_points", py::arg("points"), py::arg("time"));
    m.def("calib_ins_set_odom", &calib_ins_set_odom, "calib_ins_set_odom", py::arg("array"), py::arg("time"));
    m.def("calib_ins_calibrate", &calib_ins_calibrate, "calib_ins_calibrate");
    m.def("calib_ins_get_calibration", &calib_ins_get_calibration, "calib_ins_get_calibration");
    m.def("calib_ins_get_calibration_transform", &calib_ins_get_calibration_transform, "calib_ins_get_calibration_transform");
    // test hooks of this project (leading underscore: not part of the reference's surface)
    m.def("_counts", []() {
        uint32_t s = 0, o = 0;
        uint64_t n = 0;
        must(lio_calib_ins_counts(handle(), &s, &o, &n), "_counts");
        return py::make_tuple(s, o, n);
    });
    m.def("_set_max_evals", [](int n) {
        handle();
        if (n < 1) throw std::invalid_argument("calib_driver_ext: max_evals must be positive");
        g_params.max_evals = n;
    });
    m.add_object("_cleanup", py::capsule([]() {
        if (g_thread) g_thread->join();  // the handle is left to the process' end: the runtime may be gone already
        g_thread.reset();
    }));
}
