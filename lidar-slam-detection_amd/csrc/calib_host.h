// calib_host.h -- the host half of the lidar-INS calibration (calib_host.cpp), shared with calib.hip: the reference's f32 Transform
// (sensor_driver/calibration/lidar_ins/include/transform.h) as a translation and a quaternion, its odometry interpolation, its scan
// subsampling, and the two derivative-free optimisers.  The C entry points are declared in include/lio_hip.h.
#pragma once
#include <stdint.h>

#include "../../include/lio_hip.h"

namespace lio {
namespace calib {

// the C ABI's 7 floats: tx, ty, tz, qw, qx, qy, qz
struct Se3f {
    float t[3];
    float q[4];  // w, x, y, z
};

Se3f se3_identity();
Se3f se3_exp(const float v[6]);                // transform.h:50-59
void se3_log(const Se3f& a, float v[6]);       // transform.h:61-65
Se3f se3_mul(const Se3f& a, const Se3f& b);    // transform.h:45-48
Se3f se3_inverse(const Se3f& a);               // transform.h:39-43
void se3_matrix(const Se3f& a, float M[16]);   // transform.h:31-37, row-major
Se3f se3_from_matrix(const float M[16]);       // transform.h:23-25

// Odom::getOdomTransform (sensor.cpp:14-44); m >= 2
Se3f interpolate(const int64_t* stamps, const Se3f* T, uint32_t m, int64_t stamp, uint32_t start_idx, uint32_t* match_idx);

}  // namespace calib
}  // namespace lio
