// geodesy.h -- the host-side f64 pose arithmetic geodesy.cpp shares with itself: Eigen's quaternion statements as the reference's
// interpolateTransform uses them.  The C entry points are declared in include/lio_hip.h.
#pragma once

namespace lio {
namespace geodesy {

// Eigen's Quaterniond(Matrix3d) (w, x, y, z) of the rotation block of a row-major 4 x 4, q * v, q1 * q2
void quat_of(const double T[16], double q[4]);
void quat_rotate(const double q[4], const double v[3], double o[3]);
void quat_mul(const double a[4], const double b[4], double o[4]);

}  // namespace geodesy
}  // namespace lio
