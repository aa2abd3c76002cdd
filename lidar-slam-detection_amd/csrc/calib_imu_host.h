// calib_imu_host.h -- the host half of the lidar-IMU calibration (calib_imu_host.cpp, f64, no device), shared with calib_imu.hip: the buffers
// and calib() / getLidarPose() / getImuPose() of the reference's CalibLidarImu (sensor_driver/calibration/lidar_imu/src/calib_lidar_imu.cpp).
// The stateless C entry points (lio_calib_imu_integrate / _interpolate / _time_align / _solve) are declared in include/lio_hip.h.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/lio_hip.h"

namespace lio {
namespace calib_imu {

constexpr uint32_t kMaxFrames = 200;  // calib_wrapper.cpp:142: frames are ignored from the 200th on

struct Frame {
    double stamp;   // s
    double T[16];   // delta_T: the motion since the key frame before, row-major
    double gT[16];  // global_T
};

struct Host {
    std::vector<double> imu_stamp;           // s
    std::vector<double> imu_gyr, imu_acc;    // 3 per sample: rad/s, m/s^2
    std::vector<double> imu_rot;             // 4 per sample (w, x, y, z); identity until calibrate integrates
    std::vector<Frame> frames;               // lidar_buffer_
    std::vector<Frame> aligned;              // aligned_lidar_imu_buffer_: the frame ...
    std::vector<double> aligned_q;           // ... and its interpolated attitude, 4 per entry
    double q_l_b[4] = {1.0, 0.0, 0.0, 0.0};  // the result as solve left it (sign free, unit)

    void reset();
    void add_imu(const double* rows, uint32_t n);  // (stamp us, gyro deg/s x3, acc g x3): /1e6, /180*pi, *9.81 (calib_wrapper.cpp:168-184)
    bool add_frame(uint64_t stamp_us, const double gT[16], const double dT[16]);  // false: the cap holds, nothing was added
    int calibrate(double R[9]);                    // calib(true); LIO_E_STATE where the reference reads past the end
    uint32_t n_poses() const { return aligned.empty() ? 0u : (uint32_t)aligned.size() - 1u; }
    void lidar_poses(double* out) const;           // n_poses() x 16
    void imu_poses(double* out) const;
};

}  // namespace calib_imu
}  // namespace lio
