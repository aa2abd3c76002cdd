// calib_imu_host.cpp -- the host half of the lidar-IMU calibration, plain C++ in f64, no device: the reference's
// sensor_driver/calibration/lidar_imu/src/calib_lidar_imu.cpp restated statement by statement (calib():288-376, getInterpolatedAttitude,
// solve, getLidarPose, getImuPose) with the few Eigen rules it uses written out from Eigen 3.3's published source, since Eigen is not a
// dependency of the product:
//
//   quaternion product, inverse() = conjugate / squared norm (the integrated quaternions are NOT unit; a zero quaternion inverts to zero),
//   normalize() (left alone at norm 0), AngleAxisd(Quaterniond) (angle 2 atan2(|v|, |w|), the axis negated for w < 0, (1, 0, 0) at |v| = 0),
//   AngleAxis::toRotationMatrix, Quaterniond(Matrix3d) (the trace branch and the largest-diagonal branch), Quaternion::toRotationMatrix and
//   angularDistance (2 atan2(|v|, |w|) of a * conj(b)).
//
// solve's JacobiSVD is replaced by a one-sided Jacobi (Hestenes) iteration on the columns of the 4n x 4 matrix: plane rotations applied to A
// itself until its columns are orthogonal, V the accumulated rotations, the singular values the column norms.  It never forms A^T A, so the
// condition number is not squared; the answer is the column of V with the smallest norm, read as (w, x, y, z).  Its sign is free.
//
// Followed quirks: a second calibrate without reset appends the aligned pairs again; frames erased by the first call stay erased; scale == 0
// or > 1 gives the identity attitude; the walking IMU iterator steps back one and keeps its place across frames.  Stated deviations: no IMU
// sample or no frame left returns LIO_E_STATE where the reference reads imu_buffer_[0] of an empty vector or returns an uninitialised matrix.
#include "calib_imu_host.h"

#include <cmath>
#include <cstring>

namespace lio {
namespace calib_imu {
namespace {

struct Quat {
    double w, x, y, z;
};

inline Quat q_load(const double* p) { return Quat{p[0], p[1], p[2], p[3]}; }
inline void q_store(const Quat& q, double* p) { p[0] = q.w; p[1] = q.x; p[2] = q.y; p[3] = q.z; }

// Eigen/src/Geometry/Quaternion.h quat_product<Arch, Derived, Derived, double>
inline Quat q_mul(const Quat& a, const Quat& b) {
    return Quat{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
inline Quat q_conj(const Quat& q) { return Quat{q.w, -q.x, -q.y, -q.z}; }
inline double q_norm2(const Quat& q) { return q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w; }  // coefficient order x, y, z, w
inline Quat q_inverse(const Quat& q) {
    const double n2 = q_norm2(q);
    if (n2 > 0.0) return Quat{q.w / n2, -q.x / n2, -q.y / n2, -q.z / n2};
    return Quat{0.0, 0.0, 0.0, 0.0};
}
inline Quat q_normalized(const Quat& q) {
    const double n2 = q_norm2(q);
    if (!(n2 > 0.0)) return q;
    const double n = std::sqrt(n2);
    return Quat{q.w / n, q.x / n, q.y / n, q.z / n};
}

// Quaternion::toRotationMatrix (row-major)
void q_matrix(const Quat& q, double R[9]) {
    const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
    R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}

// quaternionbase_assign_impl<Other, 3, 3>: Quaterniond(Matrix3d), m row-major with the given row stride
Quat q_from_matrix(const double* m, int ld) {
    auto M = [&](int r, int c) { return m[r * ld + c]; };
    double q[3];
    Quat o;
    double t = M(0, 0) + M(1, 1) + M(2, 2);
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        o.w = 0.5 * t;
        t = 0.5 / t;
        o.x = (M(2, 1) - M(1, 2)) * t;
        o.y = (M(0, 2) - M(2, 0)) * t;
        o.z = (M(1, 0) - M(0, 1)) * t;
        return o;
    }
    int i = 0;
    if (M(1, 1) > M(0, 0)) i = 1;
    if (M(2, 2) > M(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(M(i, i) - M(j, j) - M(k, k) + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    o.w = (M(k, j) - M(j, k)) * t;
    q[j] = (M(j, i) + M(i, j)) * t;
    q[k] = (M(k, i) + M(i, k)) * t;
    o.x = q[0]; o.y = q[1]; o.z = q[2];
    return o;
}

// AngleAxis::operator=(QuaternionBase): the vector part's norm (stableNorm below epsilon: the same value up to rounding, taken by hypot)
void q_angle_axis(const Quat& q, double* angle, double axis[3]) {
    double n = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
    if (n < 2.220446049250313e-16) n = std::hypot(std::hypot(q.x, q.y), q.z);
    if (n != 0.0) {
        *angle = 2.0 * std::atan2(n, std::fabs(q.w));
        if (q.w < 0.0) n = -n;
        axis[0] = q.x / n; axis[1] = q.y / n; axis[2] = q.z / n;
    } else {
        *angle = 0.0;
        axis[0] = 1.0; axis[1] = 0.0; axis[2] = 0.0;
    }
}

// AngleAxis::toRotationMatrix (row-major)
void angle_axis_matrix(double angle, const double a[3], double R[9]) {
    const double s = std::sin(angle), c = std::cos(angle);
    const double sa[3] = {s * a[0], s * a[1], s * a[2]};
    const double ca[3] = {(1.0 - c) * a[0], (1.0 - c) * a[1], (1.0 - c) * a[2]};
    double tmp = ca[0] * a[1];
    R[1] = tmp - sa[2]; R[3] = tmp + sa[2];
    tmp = ca[0] * a[2];
    R[2] = tmp + sa[1]; R[6] = tmp - sa[1];
    tmp = ca[1] * a[2];
    R[5] = tmp - sa[0]; R[7] = tmp + sa[0];
    R[0] = ca[0] * a[0] + c; R[4] = ca[1] * a[1] + c; R[8] = ca[2] * a[2] + c;
}

double q_angular_distance(const Quat& a, const Quat& b) {
    const Quat d = q_mul(a, q_conj(b));
    return 2.0 * std::atan2(std::sqrt(d.x * d.x + d.y * d.y + d.z * d.z), std::fabs(d.w));
}

Quat interpolate(const Quat& qs, const Quat& qe, double scale) {
    if (0 == scale || scale > 1) return Quat{1.0, 0.0, 0.0, 0.0};
    const Quat d = q_normalized(q_mul(q_inverse(qs), qe));
    double angle, axis[3], R[9];
    q_angle_axis(d, &angle, axis);
    angle_axis_matrix(angle * scale, axis, R);
    return q_normalized(q_mul(qs, q_from_matrix(R, 3)));
}

void integrate(const double* t, const double* g, uint32_t n, double* rot) {
    if (n == 0) return;
    q_store(Quat{1.0, 0.0, 0.0, 0.0}, rot);
    for (uint32_t i = 1; i < n; i++) {
        const double dt = t[i] - t[i - 1];
        double a[3];
        for (int k = 0; k < 3; k++) a[k] = (0.5 * (g[3 * (i - 1) + k] + g[3 * i + k])) * dt;
        const Quat inc{1.0, 0.5 * a[0], 0.5 * a[1], 0.5 * a[2]};
        q_store(q_mul(q_load(rot + 4 * (i - 1)), inc), rot + 4 * i);
    }
}

// calib():303-346 over stamps alone: frames [0, *first) are erased, frames [*first, *first + *n_aligned) get an attitude
void time_align(const double* it, const double* irot, uint32_t ni, const double* ft, uint32_t nf, uint32_t* first, uint32_t* n_aligned, double* q_out) {
    uint32_t f0 = 0;
    for (; f0 < nf; f0++)
        if (ft[f0] >= it[0]) break;
    *first = f0;
    uint32_t last = 0, done = 0;
    for (uint32_t i = f0; i < nf; i++) {
        for (; last != ni; last++)
            if (it[last] >= ft[i]) break;
        if (last != 0) last--;
        const uint32_t i1 = last, i2 = last + 1;
        if (i2 == ni) break;
        const double scale = (ft[i] - it[i1]) / (it[i2] - it[i1]);
        q_store(interpolate(q_load(irot + 4 * i1), q_load(irot + 4 * i2), scale), q_out + 4 * done);
        done++;
    }
    *n_aligned = done;
}

// pairs: n x 8, (q_l w x y z, q_b w x y z)
Quat solve(const double* pairs, uint32_t n) {
    if (n == 0) return Quat{1.0, 0.0, 0.0, 0.0};
    const size_t rows = 4 * (size_t)n;
    std::vector<double> A(rows * 4);  // column-major: column c at A[c * rows]
    for (uint32_t i = 0; i < n; i++) {
        const Quat ql = q_load(pairs + 8 * i), qb = q_load(pairs + 8 * i + 4);
        // L(q_b): [w -v^T; v  w I + [v]x]     R(q_l): [w -v^T; v  w I - [v]x]
        const double Lm[16] = {qb.w, -qb.x, -qb.y, -qb.z,  qb.x, qb.w, -qb.z, qb.y,  qb.y, qb.z, qb.w, -qb.x,  qb.z, -qb.y, qb.x, qb.w};
        const double Rm[16] = {ql.w, -ql.x, -ql.y, -ql.z,  ql.x, ql.w, ql.z, -ql.y,  ql.y, -ql.z, ql.w, ql.x,  ql.z, ql.y, -ql.x, ql.w};
        const double deg = 180.0 / M_PI * q_angular_distance(qb, ql);
        const double huber = deg > 2.0 ? 2.0 / deg : 1.0;
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) A[(size_t)c * rows + 4 * i + r] = huber * (Lm[4 * r + c] - Rm[4 * r + c]);
    }
    double V[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // row-major
    for (int sweep = 0; sweep < 60; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                double* ap = &A[(size_t)p * rows];
                double* aq = &A[(size_t)q * rows];
                double app = 0.0, aqq = 0.0, apq = 0.0;
                for (size_t r = 0; r < rows; r++) { app += ap[r] * ap[r]; aqq += aq[r] * aq[r]; apq += ap[r] * aq[r]; }
                if (apq == 0.0 || std::fabs(apq) <= 2.220446049250313e-16 * std::sqrt(app * aqq)) continue;
                rotated = true;
                const double zeta = (aqq - app) / (2.0 * apq);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (size_t r = 0; r < rows; r++) {
                    const double x = ap[r], y = aq[r];
                    ap[r] = c * x - s * y;
                    aq[r] = s * x + c * y;
                }
                for (int r = 0; r < 4; r++) {
                    const double x = V[4 * r + p], y = V[4 * r + q];
                    V[4 * r + p] = c * x - s * y;
                    V[4 * r + q] = s * x + c * y;
                }
            }
        if (!rotated) break;
    }
    int best = 0;
    double best_n = 0.0;
    for (int c = 0; c < 4; c++) {
        double s = 0.0;
        for (size_t r = 0; r < rows; r++) s += A[(size_t)c * rows + r] * A[(size_t)c * rows + r];
        if (c == 0 || s < best_n) { best = c; best_n = s; }
    }
    return Quat{V[best], V[4 + best], V[8 + best], V[12 + best]};
}

void mat4_mul(const double* a, const double* b, double* o) {
    double r[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) r[4 * i + j] = ((a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j]) + a[4 * i + 3] * b[12 + j];
    std::memcpy(o, r, sizeof(r));
}

const double kEye4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

}  // namespace

void Host::reset() { *this = Host(); }

void Host::add_imu(const double* rows, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
        const double* r = rows + 7 * (size_t)i;
        imu_stamp.push_back(r[0] / 1000000.0);
        for (int k = 0; k < 3; k++) imu_gyr.push_back(r[1 + k] / 180.0 * M_PI);
        for (int k = 0; k < 3; k++) imu_acc.push_back(r[4 + k] * 9.81);
        imu_rot.push_back(1.0);
        for (int k = 0; k < 3; k++) imu_rot.push_back(0.0);
    }
}

bool Host::add_frame(uint64_t stamp_us, const double gT[16], const double dT[16]) {
    if (frames.size() >= kMaxFrames) return false;
    Frame f;
    f.stamp = (double)stamp_us / 1000000.0;
    std::memcpy(f.T, dT, sizeof(f.T));
    std::memcpy(f.gT, gT, sizeof(f.gT));
    frames.push_back(f);
    return true;
}

int Host::calibrate(double R[9]) {
    if (imu_stamp.empty()) return LIO_E_STATE;
    const uint32_t ni = (uint32_t)imu_stamp.size();
    integrate(imu_stamp.data(), imu_gyr.data(), ni, imu_rot.data());
    std::vector<double> ft(frames.size()), q(4 * frames.size() + 4);
    for (size_t i = 0; i < frames.size(); i++) ft[i] = frames[i].stamp;
    uint32_t first = 0, na = 0;
    time_align(imu_stamp.data(), imu_rot.data(), ni, ft.data(), (uint32_t)ft.size(), &first, &na, q.data());
    frames.erase(frames.begin(), frames.begin() + first);
    if (frames.empty()) return LIO_E_STATE;
    for (uint32_t i = 0; i < na; i++) {
        aligned.push_back(frames[i]);
        aligned_q.insert(aligned_q.end(), q.begin() + 4 * i, q.begin() + 4 * i + 4);
    }
    std::vector<double> pairs;
    for (size_t i = 1; i < aligned.size(); i++) {
        double p[8];
        q_store(q_from_matrix(aligned[i].T, 4), p);
        q_store(q_mul(q_inverse(q_load(&aligned_q[4 * (i - 1)])), q_load(&aligned_q[4 * i])), p + 4);
        pairs.insert(pairs.end(), p, p + 8);
    }
    const Quat r = solve(pairs.data(), (uint32_t)(pairs.size() / 8));
    q_store(r, q_l_b);
    q_matrix(q_normalized(r), R);
    return LIO_OK;
}

void Host::lidar_poses(double* out) const {
    double cur[16];
    std::memcpy(cur, kEye4, sizeof(cur));
    for (size_t i = 1; i < aligned.size(); i++) {
        mat4_mul(cur, aligned[i].T, cur);
        std::memcpy(out + 16 * (i - 1), cur, sizeof(cur));
    }
}

void Host::imu_poses(double* out) const {
    double cur[16];
    std::memcpy(cur, kEye4, sizeof(cur));
    const Quat qlb = q_load(q_l_b);
    for (size_t i = 1; i < aligned.size(); i++) {
        const Quat est = q_mul(q_inverse(q_load(&aligned_q[4 * (i - 1)])), q_load(&aligned_q[4 * i]));
        double R[9], T[16];
        q_matrix(q_mul(q_mul(q_inverse(qlb), est), qlb), R);
        std::memcpy(T, aligned[i].T, sizeof(T));
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) T[4 * r + c] = R[3 * r + c];
        mat4_mul(cur, T, cur);
        std::memcpy(out + 16 * (i - 1), cur, sizeof(cur));
    }
}

}  // namespace calib_imu
}  // namespace lio

using namespace lio::calib_imu;

extern "C" {

int lio_calib_imu_integrate(const double* stamps_s, const double* gyr_rad, uint32_t n, double* quat_wxyz_out) {
    if ((n && (!stamps_s || !gyr_rad)) || (n && !quat_wxyz_out)) return LIO_E_INVALID;
    integrate(stamps_s, gyr_rad, n, quat_wxyz_out);
    return LIO_OK;
}

int lio_calib_imu_interpolate(const double q_s[4], const double q_e[4], double scale, double out[4]) {
    if (!q_s || !q_e || !out) return LIO_E_INVALID;
    q_store(interpolate(q_load(q_s), q_load(q_e), scale), out);
    return LIO_OK;
}

int lio_calib_imu_time_align(const double* imu_stamps_s, const double* imu_quat_wxyz, uint32_t n_imu, const double* frame_stamps_s, uint32_t n_frames,
                             uint32_t* first_kept, uint32_t* n_aligned, double* quat_wxyz_out) {
    if (!imu_stamps_s || !imu_quat_wxyz || (n_frames && (!frame_stamps_s || !quat_wxyz_out)) || !first_kept || !n_aligned) return LIO_E_INVALID;
    if (n_imu == 0) return LIO_E_STATE;
    time_align(imu_stamps_s, imu_quat_wxyz, n_imu, frame_stamps_s, n_frames, first_kept, n_aligned, quat_wxyz_out);
    return LIO_OK;
}

int lio_calib_imu_solve(const double* pairs, uint32_t n, double quat_wxyz_out[4]) {
    if ((n && !pairs) || !quat_wxyz_out) return LIO_E_INVALID;
    q_store(solve(pairs, n), quat_wxyz_out);
    return LIO_OK;
}

}  // extern "C"
