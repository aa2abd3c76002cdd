// geodesy.cpp -- the GNSS side of mapping mode on the host, f64, no device (include/lio_hip.h, "Geodesy and the RTK track"):
//
//   lio_utm_*                UTMProjector (sensor_driver/common_lib/cpp_utils/UTMProjector.cpp:7-117), statement for statement, quirks kept
//   lio_grid_convergence     get_grid_convergence (UTMProjector.cpp:119-122)
//   lio_transform_from_rpyt  getTransformFromRPYT (slam/common/slam_utils.cpp:88-96)
//   lio_interpolate_transform  interpolateTransform (slam_utils.cpp:126-161) = the tail of RTKM::getInterpolatedTransform (rtkm.cpp:180-210)
//   lio_rtk_transform_*      computeRTKTransform, the zero_utm form (slam_utils.cpp:112-124) and RTKM's origin form (rtkm.cpp:125-139)
//   lio_rtk_track_*          RTKM's mTimedInsData: setOrigin / feedInsData / getInterpolatedTransform (rtkm.cpp:37-54, 91-95, 141-213)
//   lio_update_origin        graph_update_origin's coordinate change (hdl_graph_slam_nodelet.cpp:1396-1449): a map under another origin
//   lio_gnss_queue_*         the graph's gps_queue: set_origin / gps_callback / flush_gps_queue / interpolated_transform
//                            (hdl_graph_slam_nodelet.cpp:141-156, 349-460, 653-660) up to the point where an edge is added
//
// Built without contraction (-ffp-contract=off) like the rest of the library: the evaluation order below is the reference's.
#include "geodesy.h"

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../include/lio_hip.h"

namespace lio {
namespace geodesy {

void quat_of(const double T[16], double q[4]) {
    auto M = [&](int r, int c) { return T[r * 4 + c]; };
    const double t = M(0, 0) + M(1, 1) + M(2, 2);
    if (t > 0) {
        const double r = sqrt(t + 1.0), k = 0.5 / r;
        q[0] = 0.5 * r; q[1] = (M(2, 1) - M(1, 2)) * k; q[2] = (M(0, 2) - M(2, 0)) * k; q[3] = (M(1, 0) - M(0, 1)) * k;
        return;
    }
    int i = 0;
    if (M(1, 1) > M(0, 0)) i = 1;
    if (M(2, 2) > M(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    const double r = sqrt(M(i, i) - M(j, j) - M(k, k) + 1.0), kk = 0.5 / r;
    q[1 + i] = 0.5 * r;
    q[0] = (M(k, j) - M(j, k)) * kk; q[1 + j] = (M(j, i) + M(i, j)) * kk; q[1 + k] = (M(k, i) + M(i, k)) * kk;
}
void quat_rotate(const double q[4], const double v[3], double o[3]) {
    const double uv[3] = {2 * (q[2] * v[2] - q[3] * v[1]), 2 * (q[3] * v[0] - q[1] * v[2]), 2 * (q[1] * v[1] - q[2] * v[0])};
    o[0] = v[0] + q[0] * uv[0] + (q[2] * uv[2] - q[3] * uv[1]);
    o[1] = v[1] + q[0] * uv[1] + (q[3] * uv[0] - q[1] * uv[2]);
    o[2] = v[2] + q[0] * uv[2] + (q[1] * uv[1] - q[2] * uv[0]);
}
void quat_mul(const double a[4], const double b[4], double o[4]) {
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
    o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}

}  // namespace geodesy
}  // namespace lio

using namespace lio::geodesy;

namespace {

const double PI = 3.1415926535897932384626433832795;  // UTMProjector.cpp:5
constexpr double kAng2Rad = 0.01745329251994;         // the reference's truncated constant (slam_utils.cpp:88)

void mat_mul(const double a[16], const double b[16], double r[16]) {
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += a[i * 4 + k] * b[k * 4 + j];
            r[i * 4 + j] = s;
        }
}
void mat_identity(double m[16]) {
    for (int i = 0; i < 16; i++) m[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

}  // namespace

// mZoneWidth and mProjectNo are ints (UTMProjector.h:13-14): "unset" is any negative zone number, so a zone west of Greenwich never sticks
struct lio_utm {
    int zone_width;
    int project_no;
};

namespace {

// computeRTKTransform's tail, shared by both forms: heading less the grid convergence, yaw = -heading, getTransformFromRPYT
void rtk_pose(lio_utm* u, const lio_rtk_fix* f, double x, double y, double z, double T[16]) {
    const double heading = f->heading - lio_grid_convergence(lio_utm_longitude0(u), f->latitude, f->longitude);
    const double yaw = -heading;
    lio_transform_from_rpyt(x, y, z, yaw, f->pitch, f->roll, T);
}

}  // namespace

struct lio_rtk_track {
    lio_utm proj{6, -1};
    bool origin_set = false;
    lio_rtk_fix origin{};
    struct Entry { lio_rtk_fix fix; double T[16]; };
    std::map<uint64_t, Entry> data;  // mTimedInsData: a fix with a stamp already held replaces it
};

struct lio_gnss_queue {
    lio_utm proj{6, -1};
    bool have_zero = false;
    double zero_utm[3] = {0, 0, 0};
    std::vector<lio_rtk_fix> queue;
};

extern "C" {

lio_utm* lio_utm_create(int zone_width) {
    if (zone_width <= 0) return nullptr;
    return new lio_utm{zone_width, -1};
}
void lio_utm_destroy(lio_utm* u) { delete u; }
int lio_utm_zone(const lio_utm* u) { return u ? u->project_no : -1; }

// FromGlobalToLocal (UTMProjector.cpp:13-55)
int lio_utm_forward(lio_utm* u, double latitude, double longitude, double* x, double* y) {
    if (!u || !x || !y) return LIO_E_INVALID;
    const int mZoneWidth = u->zone_width;
    double iPI = PI / 180;
    double a = 6378137.0;
    double f = 1.0 / 298.257222101;
    if (u->project_no < 0) {
        u->project_no = floor(longitude / mZoneWidth);
    }
    double ProjNo = u->project_no;
    double longitude0 = ProjNo * mZoneWidth + mZoneWidth / 2;  // (mZoneWidth / 2 is an integer division)
    longitude0 = longitude0 * iPI;
    double longitude1 = longitude * iPI;
    double latitude1 = latitude * iPI;
    double e2 = 2 * f - f * f;
    double ee = e2 * (1.0 - e2);
    double NN = a / sqrt(1.0 - e2 * sin(latitude1) * sin(latitude1));
    double T = tan(latitude1) * tan(latitude1);
    double C = ee * cos(latitude1) * cos(latitude1);
    double A = (longitude1 - longitude0) * cos(latitude1);
    double M =
        a *
        ((1 - e2 / 4 - 3 * e2 * e2 / 64 - 5 * e2 * e2 * e2 / 256) * latitude1 -
         (3 * e2 / 8 + 3 * e2 * e2 / 32 + 45 * e2 * e2 * e2 / 1024) *
             sin(2 * latitude1) +
         (15 * e2 * e2 / 256 + 45 * e2 * e2 * e2 / 1024) * sin(4 * latitude1) -
         (35 * e2 * e2 * e2 / 3072) * sin(6 * latitude1));
    double xval =
        NN * (A + (1 - T + C) * A * A * A / 6 +
              (5 - 18 * T + T * T + 72 * C - 58 * ee) * A * A * A * A * A / 120);
    double yval =
        M + NN * tan(latitude1) *
                (A * A / 2 + (5 - T + 9 * C + 4 * C * C) * A * A * A * A / 24 +
                 (61 - 58 * T + T * T + 600 * C - 330 * ee) * A * A * A * A * A *
                     A / 720);
    double X0 = 1000000 * (ProjNo + 1) + 500000;
    double Y0 = 0;
    xval = xval + X0;
    yval = yval + Y0;
    *x = (xval - 500000) * 0.9996 + 500000;
    *y = yval * 0.9996;
    return LIO_OK;
}

// FromLocalToGlobal (UTMProjector.cpp:57-109): the zone from x when none is set, the zone width hard-coded to 6
int lio_utm_inverse(lio_utm* u, double x, double y, double* latitude, double* longitude) {
    if (!u || !latitude || !longitude) return LIO_E_INVALID;
    double iPI = PI / 180.0f;
    double mZoneWidth = 6;
    double a = 6378137.0;
    double f = 1.0 / 298.257222101;
    if (u->project_no < 0) {
        u->project_no = floor(x / 1000000) - 1;
    }
    double ProjNo = u->project_no + 1;
    double longitude0 = (ProjNo - 1) * mZoneWidth + mZoneWidth / 2;
    longitude0 = longitude0 * iPI;
    double X0 = ProjNo * 1000000 + 500000;
    double Y0 = 0;
    double xval = (x - 500000) / 0.9996 + 500000 - X0;
    double yval = y / 0.9996 - Y0;

    double e2 = 2 * f - f * f;
    double e1 = (1.0 - sqrt(1 - e2)) / (1.0 + sqrt(1 - e2));
    double ee = e2 * (1.0 - e2);

    double M = yval;
    double uu = M / (a * (1 - e2 / 4 - 3 * e2 * e2 / 64 - 5 * e2 * e2 * e2 / 256));
    double fai = uu + (3 * e1 / 2 - 27 * e1 * e1 * e1 / 32) * sin(2 * uu) +
                 (21 * e1 * e1 / 16 - 55 * e1 * e1 * e1 * e1 / 32) * sin(4 * uu) +
                 (151 * e1 * e1 * e1 / 96) * sin(6 * uu) +
                 (1097 * e1 * e1 * e1 * e1 / 512) * sin(8 * uu);
    double C = ee * cos(fai) * cos(fai);
    double T = tan(fai) * tan(fai);
    double NN = a / sqrt(1.0 - e2 * sin(fai) * sin(fai));
    double R =
        a * (1 - e2) /
        sqrt((1 - e2 * sin(fai) * sin(fai)) * (1 - e2 * sin(fai) * sin(fai)) *
             (1 - e2 * sin(fai) * sin(fai)));
    double D = xval / NN;

    double longitude1 =
        longitude0 + (D - (1 + 2 * T + C) * D * D * D / 6 +
                      (5 - 2 * C + 28 * T - 3 * C * C + 8 * ee + 24 * T * T) * D *
                          D * D * D * D / 120) /
                         cos(fai);
    double latitude1 =
        fai -
        (NN * tan(fai) / R) *
            (D * D / 2 -
             (5 + 3 * T + 10 * C - 4 * C * C - 9 * ee) * D * D * D * D / 24 +
             (61 + 90 * T + 298 * C + 45 * T * T - 256 * ee - 3 * C * C) * D * D *
                 D * D * D * D / 720);

    *longitude = longitude1 / iPI;
    *latitude = latitude1 / iPI;
    return LIO_OK;
}

// GetLongitude0 (UTMProjector.cpp:111-117): int arithmetic; with no zone set the reference warns and answers from -1
double lio_utm_longitude0(const lio_utm* u) {
    if (!u) return 0.0;
    return u->project_no * u->zone_width + u->zone_width / 2;
}

double lio_grid_convergence(double longitude0, double lat, double lon) {
    return atan(tan((lon - longitude0) / 180.0 * M_PI) * sin(lat / 180.0 * M_PI)) * 180.0 / M_PI;
}

// getTransformFromRPYT (slam_utils.cpp:89-96): translation * Rz(yaw) * Rx(pitch) * Ry(roll), angles in degrees
void lio_transform_from_rpyt(double x, double y, double z, double yaw, double pitch, double roll, double T16[16]) {
    const double cy = cos(yaw * kAng2Rad), sy = sin(yaw * kAng2Rad);
    const double cp = cos(pitch * kAng2Rad), sp = sin(pitch * kAng2Rad);
    const double cr = cos(roll * kAng2Rad), sr = sin(roll * kAng2Rad);
    double Rz[16], Rx[16], Ry[16], T[16], a[16], b[16];
    mat_identity(Rz); mat_identity(Rx); mat_identity(Ry); mat_identity(T);
    Rz[0] = cy; Rz[1] = -sy; Rz[4] = sy; Rz[5] = cy;
    Rx[5] = cp; Rx[6] = -sp; Rx[9] = sp; Rx[10] = cp;
    Ry[0] = cr; Ry[2] = sr; Ry[8] = -sr; Ry[10] = cr;
    T[3] = x; T[7] = y; T[11] = z;
    mat_mul(T, Rz, a);
    mat_mul(a, Rx, b);
    mat_mul(b, Ry, T16);
}

void lio_quat_of_transform(const double T[16], double wxyz[4]) { quat_of(T, wxyz); }

// interpolateTransform (slam_utils.cpp:126-161): the pose a fraction `ratio` of the way from pre to next, along the translation and the
// angle-axis of pre^-1 next
void lio_interpolate_transform(const double pre[16], const double next[16], double ratio, double out[16]) {
    double q[4], qi[4], qn[4], dq[4];
    quat_of(pre, q);
    qi[0] = q[0]; qi[1] = -q[1]; qi[2] = -q[2]; qi[3] = -q[3];
    quat_of(next, qn);
    const double t[3] = {pre[3], pre[7], pre[11]}, tn[3] = {next[3], next[7], next[11]};
    double a[3], b[3];
    quat_rotate(qi, t, a);
    quat_rotate(qi, tn, b);
    const double dt[3] = {-a[0] + b[0], -a[1] + b[1], -a[2] + b[2]};
    quat_mul(qi, qn, dq);
    // Eigen::AngleAxisd(q): angle = 2 atan2(|vec|, |w|), the axis vec / |vec| with the sign of w; no rotation: angle 0 about x
    double n = sqrt(dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]), angle = 0, axis[3] = {1, 0, 0};
    if (n != 0.0) {
        angle = 2.0 * atan2(n, fabs(dq[0]));
        if (dq[0] < 0) n = -n;
        for (int i = 0; i < 3; i++) axis[i] = dq[1 + i] / n;
    }
    const double lt[3] = {ratio * dt[0], ratio * dt[1], ratio * dt[2]};
    const double lr[3] = {ratio * (angle * axis[0]), ratio * (angle * axis[1]), ratio * (angle * axis[2])};
    const double norm = sqrt(lr[0] * lr[0] + lr[1] * lr[1] + lr[2] * lr[2]);
    double tq[4] = {1, 0, 0, 0};
    if (!(norm < 1e-8)) {
        const double sh = sin(0.5 * norm), ch = cos(0.5 * norm);
        tq[0] = ch; tq[1] = sh * (lr[0] / norm); tq[2] = sh * (lr[1] / norm); tq[3] = sh * (lr[2] / norm);
    }
    double rt[3], nq[4];
    quat_rotate(q, lt, rt);
    quat_mul(q, tq, nq);
    mat_identity(out);
    const double w = nq[0], x = nq[1], y = nq[2], z = nq[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    out[0] = 1 - (tyy + tzz); out[1] = txy - twz; out[2] = txz + twy;
    out[4] = txy + twz; out[5] = 1 - (txx + tzz); out[6] = tyz - twx;
    out[8] = txz - twy; out[9] = tyz + twx; out[10] = 1 - (txx + tyy);
    for (int i = 0; i < 3; i++) out[4 * i + 3] = t[i] + rt[i];
}

// computeRTKTransform(projector, data, zero_utm) (slam_utils.cpp:112-124)
int lio_rtk_transform_utm(lio_utm* u, const lio_rtk_fix* fix, const double zero_utm[3], double T[16]) {
    if (!u || !fix || !zero_utm || !T) return LIO_E_INVALID;
    double dataX, dataY, dataZ;
    lio_utm_forward(u, fix->latitude, fix->longitude, &dataX, &dataY);
    dataX -= zero_utm[0];
    dataY -= zero_utm[1];
    dataZ = fix->altitude - zero_utm[2];
    rtk_pose(u, fix, dataX, dataY, dataZ, T);
    return LIO_OK;
}

// RTKM::computeRTKTransform(origin, data) (rtkm.cpp:125-139): the origin is projected again on every call
int lio_rtk_transform_origin(lio_utm* u, const lio_rtk_fix* origin, const lio_rtk_fix* fix, double T[16]) {
    if (!u || !origin || !fix || !T) return LIO_E_INVALID;
    double originX, originY;
    double dataX, dataY, dataZ;
    lio_utm_forward(u, origin->latitude, origin->longitude, &originX, &originY);
    lio_utm_forward(u, fix->latitude, fix->longitude, &dataX, &dataY);
    dataX -= originX;
    dataY -= originY;
    dataZ = fix->altitude - origin->altitude;
    rtk_pose(u, fix, dataX, dataY, dataZ, T);
    return LIO_OK;
}

// graph_update_origin (hdl_graph_slam_nodelet.cpp:1396-1449) without its graph: two projectors made fresh, each fixed to its zone by its own
// origin; a translation goes back to latitude / longitude by the `from` projector and forward again by the `to` projector
int lio_update_origin(const lio_rtk_fix* from, const lio_rtk_fix* to, double* poses16, uint32_t n_poses, double* xyz, uint32_t n_xyz) {
    if (!from || !to || (n_poses && !poses16) || (n_xyz && !xyz)) return LIO_E_INVALID;
    lio_utm projector_from{6, -1}, projector_to{6, -1};
    double zero_utm_from[2], zero_utm_to[2];
    lio_utm_forward(&projector_from, from->latitude, from->longitude, &zero_utm_from[0], &zero_utm_from[1]);
    lio_utm_forward(&projector_to, to->latitude, to->longitude, &zero_utm_to[0], &zero_utm_to[1]);
    auto move = [&](double* x, double* y, double* z) {
        double lat, lon;
        lio_utm_inverse(&projector_from, *x + zero_utm_from[0], *y + zero_utm_from[1], &lat, &lon);
        double new_local_x, new_local_y;
        lio_utm_forward(&projector_to, lat, lon, &new_local_x, &new_local_y);
        *x = new_local_x - zero_utm_to[0];
        *y = new_local_y - zero_utm_to[1];
        *z = *z + from->altitude - to->altitude;
    };
    for (uint32_t k = 0; k < n_xyz; k++) move(xyz + 3 * (size_t)k, xyz + 3 * (size_t)k + 1, xyz + 3 * (size_t)k + 2);
    for (uint32_t k = 0; k < n_poses; k++) move(poses16 + 16 * (size_t)k + 3, poses16 + 16 * (size_t)k + 7, poses16 + 16 * (size_t)k + 11);
    return LIO_OK;
}

// ---- the RTK track --------------------------------------------------------------------------------------------------------------------------
lio_rtk_track* lio_rtk_track_create(void) { return new lio_rtk_track(); }
void lio_rtk_track_destroy(lio_rtk_track* t) { delete t; }

// RTKM::setOrigin (rtkm.cpp:37-54): the first one wins; T = the origin's own pose (what mLastOdom becomes)
int lio_rtk_track_set_origin(lio_rtk_track* t, const lio_rtk_fix* rtk, double T[16]) {
    if (!t || !rtk) return LIO_E_INVALID;
    if (t->origin_set) return 0;
    t->origin_set = true;
    t->origin = *rtk;
    double easting, northing;
    lio_utm_forward(&t->proj, rtk->latitude, rtk->longitude, &easting, &northing);
    double M[16];
    lio_rtk_transform_origin(&t->proj, &t->origin, rtk, M);
    if (T) memcpy(T, M, sizeof(M));
    return 1;
}
int lio_rtk_track_origin(const lio_rtk_track* t, lio_rtk_fix* out) {
    if (!t) return LIO_E_INVALID;
    if (t->origin_set && out) *out = t->origin;
    return t->origin_set ? 1 : 0;
}
// RTKM::feedInsData (rtkm.cpp:91-95)
int lio_rtk_track_feed(lio_rtk_track* t, int rtk_valid, const lio_rtk_fix* fix) {
    if (!t || !fix) return LIO_E_INVALID;
    if (!(rtk_valid && t->origin_set)) return 0;
    lio_rtk_track::Entry e;
    e.fix = *fix;
    lio_rtk_transform_origin(&t->proj, &t->origin, fix, e.T);
    t->data[fix->stamp_us] = e;
    return 1;
}
int lio_rtk_track_size(const lio_rtk_track* t) { return t ? (int)t->data.size() : LIO_E_INVALID; }

// RTKM::getInterpolatedTransform (rtkm.cpp:141-213); T is written only when the track answers
int lio_rtk_track_interpolate(const lio_rtk_track* t, uint64_t timestamp, double T[16]) {
    if (!t || !T) return LIO_E_INVALID;
    if (!t->origin_set) return LIO_RTK_NO_ORIGIN;
    auto hit = t->data.find(timestamp);
    if (hit != t->data.end()) {
        memcpy(T, hit->second.T, sizeof(double) * 16);
        return LIO_RTK_EXACT;
    }
    if (t->data.size() <= 1) return LIO_RTK_TOO_FEW;
    if (timestamp < t->data.begin()->second.fix.stamp_us) return LIO_RTK_EARLY;
    if (timestamp > t->data.rbegin()->second.fix.stamp_us) return LIO_RTK_LATE;
    // reverse search for the closest fix
    auto it = t->data.rbegin();
    while (it != t->data.rend()) {
        if (it->first <= timestamp) break;
        it++;
    }
    const lio_rtk_track::Entry& pre = it->second;
    it--;
    const lio_rtk_track::Entry& next = it->second;
    const double t_diff_ratio = static_cast<double>(timestamp - pre.fix.stamp_us) / static_cast<double>(next.fix.stamp_us - pre.fix.stamp_us);
    lio_interpolate_transform(pre.T, next.T, t_diff_ratio, T);
    return LIO_RTK_INTERPOLATED;
}

// ---- the graph's GNSS queue ---------------------------------------------------------------------------------------------------------------
lio_gnss_queue* lio_gnss_queue_create(void) { return new lio_gnss_queue(); }
void lio_gnss_queue_destroy(lio_gnss_queue* q) { delete q; }

// set_origin (hdl_graph_slam_nodelet.cpp:141-156)
int lio_gnss_queue_set_origin(lio_gnss_queue* q, const lio_rtk_fix* rtk, int have_keyframe, double last_keyframe_z, double zero_utm[3]) {
    if (!q || !rtk) return LIO_E_INVALID;
    double altitude = rtk->altitude;
    if (have_keyframe) altitude -= last_keyframe_z;
    double easting, northing;
    lio_utm_forward(&q->proj, rtk->latitude, rtk->longitude, &easting, &northing);
    q->zero_utm[0] = easting; q->zero_utm[1] = northing; q->zero_utm[2] = altitude;
    q->have_zero = true;
    if (zero_utm) memcpy(zero_utm, q->zero_utm, sizeof(q->zero_utm));
    return LIO_OK;
}
int lio_gnss_queue_push(lio_gnss_queue* q, const lio_rtk_fix* fix) {  // gps_callback
    if (!q || !fix) return LIO_E_INVALID;
    q->queue.push_back(*fix);
    return LIO_OK;
}
int lio_gnss_queue_size(const lio_gnss_queue* q) { return q ? (int)q->queue.size() : LIO_E_INVALID; }
int lio_gnss_queue_stamps(const lio_gnss_queue* q, uint64_t* stamps, uint32_t cap) {
    if (!q) return LIO_E_INVALID;
    const size_t n = q->queue.size();
    if (n > cap) return -(int)n;
    for (size_t i = 0; i < n; i++) stamps[i] = q->queue[i].stamp_us;
    return (int)n;
}

// flush_gps_queue (hdl_graph_slam_nodelet.cpp:358-460) up to the edge: which key frame takes which pair of fixes, and what the edge is built from
int lio_gnss_queue_flush(lio_gnss_queue* q, const uint64_t* kf_stamps, uint8_t* kf_has_fix, uint32_t n_kf, double last_xyz[3], lio_gnss_match* out,
                         uint32_t cap) {
    if (!q || (n_kf && (!kf_stamps || !kf_has_fix)) || !last_xyz || (cap && !out)) return LIO_E_INVALID;
    if (n_kf == 0 || q->queue.empty()) return 0;
    if (!q->have_zero) return LIO_E_STATE;  // (the reference dereferences an unset zero_utm here)
    std::vector<lio_rtk_fix>& gq = q->queue;
    uint32_t n_out = 0;
    size_t gps_cursor = 0;
    for (uint32_t k = 0; k < n_kf; k++) {
        const uint64_t stamp = kf_stamps[k];
        if (stamp > gq.back().stamp_us) break;
        if (stamp < gq[gps_cursor].stamp_us || kf_has_fix[k]) continue;
        // find the gps data which is closest to the keyframe
        size_t first_gps = gps_cursor, second_gps = gps_cursor;
        for (; second_gps != gq.size(); second_gps++) {
            const double dt = (gq[first_gps].stamp_us - double(stamp)) / 1000000.0;
            const double dt2 = (gq[second_gps].stamp_us - double(stamp)) / 1000000.0;
            if (dt <= 0 && dt2 >= 0 && (dt2 - dt) < 2.0) break;
            first_gps = second_gps;
        }
        if (second_gps == gq.size()) break;
        gps_cursor = first_gps;
        const lio_rtk_fix& pre = gq[first_gps];
        const lio_rtk_fix& next = gq[second_gps];
        if (pre.precision != next.precision) continue;
        const int gps_dim = pre.dimension;
        // interpolated_transform (:653-660): the ratio's denominator carries a + 1
        const double t_diff_ratio = static_cast<double>(stamp - pre.stamp_us) / static_cast<double>(next.stamp_us - pre.stamp_us + 1);
        double preT[16], nextT[16], utm[16];
        lio_rtk_transform_utm(&q->proj, &pre, q->zero_utm, preT);
        lio_rtk_transform_utm(&q->proj, &next, q->zero_utm, nextT);
        lio_interpolate_transform(preT, nextT, t_diff_ratio, utm);
        double xyz[3] = {utm[3], utm[7], utm[11]};
        xyz[2] = (gps_dim == 2) ? 0 : xyz[2];
        double update_threshold;
        if (pre.precision < 100.0) update_threshold = 10.0;
        else if (pre.precision < 1000.0) update_threshold = 20.0;
        else update_threshold = 50.0;
        const double d[3] = {last_xyz[0] - xyz[0], last_xyz[1] - xyz[1], last_xyz[2] - xyz[2]};
        if (sqrt(last_xyz[0] * last_xyz[0] + last_xyz[1] * last_xyz[1] + last_xyz[2] * last_xyz[2]) > 0 &&
            sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < update_threshold)
            continue;
        kf_has_fix[k] = 1;
        for (int i = 0; i < 3; i++) last_xyz[i] = xyz[i];
        if (n_out < cap) {
            lio_gnss_match& m = out[n_out];
            m.keyframe = (int32_t)k;
            m.dimension = gps_dim;
            m.first_stamp_us = pre.stamp_us;
            m.second_stamp_us = next.stamp_us;
            for (int i = 0; i < 3; i++) m.xyz[i] = xyz[i];
            double w[4];  // Quaterniond(utm_transform.block<3, 3>(0, 0)).normalize(), handed out as (x, y, z, w)
            quat_of(utm, w);
            const double nn = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2] + w[3] * w[3]);
            m.quat[0] = w[1] / nn; m.quat[1] = w[2] / nn; m.quat[2] = w[3] / nn; m.quat[3] = w[0] / nn;
            m.precision = pre.precision;
        }
        n_out++;
    }
    const uint64_t last_stamp = kf_stamps[n_kf - 1];
    auto remove_loc = std::upper_bound(gq.begin(), gq.end(), last_stamp, [](const uint64_t& s, const lio_rtk_fix& f) { return s < f.stamp_us; });
    gq.erase(gq.begin(), remove_loc);
    return n_out > cap ? -(int)n_out : (int)n_out;
}

}  // extern "C"
