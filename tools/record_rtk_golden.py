#!/usr/bin/env python3
"""Records tests/golden/rtk.npz from the reference's own UTMProjector (sensor_driver/common_lib/cpp_utils/UTMProjector.cpp) and mergePoints
(slam/common/slam_utils.cpp:249-273).

The reference's translation units are compiled, together with the small harness below (the project's own: plain C entry points), into a
TEMPORARY directory outside the tree; nothing compiled is kept, the file holds only arrays.  slam_utils.cpp is compiled over oracle/ref_shims
(read, not changed) the way oracle/ref_slam_utils.cpp does it.

Projection: tests/rtk_cases.py's projection_cases() -- each (lat, lon) through a FRESH projector and through one PINNED by a first call
PIN_OFFSET degrees of longitude away; the inverse of both forward results through both kinds of projector (a fresh one derives its zone from x);
the zone numbers, GetLongitude0 and get_grid_convergence of both.  mergePoints: the five cases of the kernel test at small n (the merged
points and stamps before the static transform: the shims carry no pcl::transformPointCloud).

    python tools/record_rtk_golden.py [--reference /path/to/reference]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]

HARNESS = r"""
#define __MAPPING_TYPES_H  // slam_utils.h sits beside the real mapping_types.h: keep it out, use the shim
#include "ref_shims/mapping_types.h"
#include <common/slam_utils.cpp>
#include <cstdlib>
uint64_t gps2Utc(int, double) { abort(); }
int getGPSweek(const uint64_t&) { abort(); }
double getGPSsecond(const uint64_t&) { abort(); }
struct Peek : UTMProjector { int zone() const { return mProjectNo; } };
extern "C" {
// fresh: one projector per call.  out = x, y, zone, longitude0, convergence, then the inverse of (x, y) by a fresh projector: lat, lon
void h_fresh(double lat, double lon, double* out) {
    Peek p;
    p.FromGlobalToLocal(lat, lon, out[0], out[1]);
    out[2] = p.zone();
    out[3] = p.GetLongitude0();
    out[4] = get_grid_convergence(out[3], lat, lon);
}
// pinned: the first call at (lat, pin_lon) fixes the zone
void h_pinned(double lat, double lon, double pin_lon, double* out) {
    Peek p;
    double px, py;
    p.FromGlobalToLocal(lat, pin_lon, px, py);
    p.FromGlobalToLocal(lat, lon, out[0], out[1]);
    out[2] = p.zone();
    out[3] = p.GetLongitude0();
    out[4] = get_grid_convergence(out[3], lat, lon);
}
void h_inverse_fresh(double x, double y, double* out) {
    Peek p;
    p.FromLocalToGlobal(x, y, out[0], out[1]);
    out[2] = p.zone();
}
void h_inverse_pinned(double lat, double pin_lon, double x, double y, double* out) {
    Peek p;
    double px, py;
    p.FromGlobalToLocal(lat, pin_lon, px, py);
    p.FromLocalToGlobal(x, y, out[0], out[1]);
    out[2] = p.zone();
}
// mergePoints over n_clouds clouds laid end to end; cloud 0 is the base ("0-base"; the others follow in std::map order of the names given)
int h_merge(int n_clouds, const float* xyzi, const uint32_t* stamps, const int* n_points, const uint64_t* headers, uint64_t scan_period,
            float* out_xyzi, uint32_t* out_stamps) {
    std::map<std::string, PointCloudAttrPtr> points;
    size_t at = 0;
    for (int l = 0; l < n_clouds; l++) {
        PointCloudAttrPtr f(new PointCloudAttr());
        f->cloud->points.resize(n_points[l]);
        f->attr.resize(n_points[l]);
        for (int i = 0; i < n_points[l]; i++, at++) {
            Point& p = f->cloud->points[i];
            p.x = xyzi[4 * at]; p.y = xyzi[4 * at + 1]; p.z = xyzi[4 * at + 2]; p.intensity = xyzi[4 * at + 3];
            f->attr[i].id = 0;
            f->attr[i].stamp = stamps[at];
        }
        f->cloud->header.stamp = headers[l];
        char name[16];
        snprintf(name, sizeof(name), "%c-lidar", 'a' + l);
        points[name] = f;
    }
    PointCloudAttrPtr m = mergePoints("a-lidar", points, scan_period);
    for (size_t i = 0; i < m->cloud->points.size(); i++) {
        const Point& p = m->cloud->points[i];
        out_xyzi[4 * i] = p.x; out_xyzi[4 * i + 1] = p.y; out_xyzi[4 * i + 2] = p.z; out_xyzi[4 * i + 3] = p.intensity;
        out_stamps[i] = m->attr[i].stamp;
    }
    return (int)m->cloud->points.size();
}
}
"""


def build(ref, tmp):
    src = os.path.join(tmp, "rtk_harness.cpp")
    open(src, "w").write(HARNESS)
    lib = os.path.join(tmp, "librtk_ref.so")
    utils = os.path.join(ref, "sensor_driver", "common_lib", "cpp_utils")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-ffp-contract=off", "-fopenmp", "-DEIGEN_DONT_VECTORIZE",
                           "-I" + os.path.join(ROOT, "oracle", "ref_shims"), "-I" + os.path.join(ROOT, "oracle"),
                           "-I" + os.path.join(ref, "slam", "thirdparty", "fast_gicp", "thirdparty", "Eigen"), "-I" + os.path.join(ref, "slam"), "-I" + utils,
                           src, os.path.join(utils, "UTMProjector.cpp"), "-o", lib])
    return C.CDLL(lib)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("LSD_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rtk.npz"))
    a = ap.parse_args()
    import rtk_cases as R

    dbl = C.c_double
    P = lambda x, t: x.ctypes.data_as(C.POINTER(t))
    lat, lon = R.projection_cases()
    n = len(lat)
    fresh, pinned = np.zeros((n, 5)), np.zeros((n, 5))
    inv = np.zeros((n, 4, 3))  # fresh of fresh, pinned of pinned, fresh of pinned, pinned of fresh: lat, lon, zone
    out = {}
    with tempfile.TemporaryDirectory(prefix="rtk_golden_") as tmp:
        L = build(a.reference, tmp)
        for k in range(n):
            la, lo, pin = float(lat[k]), float(lon[k]), float(lon[k]) + R.PIN_OFFSET
            L.h_fresh(dbl(la), dbl(lo), P(fresh[k], dbl))
            L.h_pinned(dbl(la), dbl(lo), dbl(pin), P(pinned[k], dbl))
            L.h_inverse_fresh(dbl(fresh[k, 0]), dbl(fresh[k, 1]), P(inv[k, 0], dbl))
            L.h_inverse_pinned(dbl(la), dbl(pin), dbl(pinned[k, 0]), dbl(pinned[k, 1]), P(inv[k, 1], dbl))
            L.h_inverse_fresh(dbl(pinned[k, 0]), dbl(pinned[k, 1]), P(inv[k, 2], dbl))
            L.h_inverse_pinned(dbl(la), dbl(pin), dbl(fresh[k, 0]), dbl(fresh[k, 1]), P(inv[k, 3], dbl))
        for name in R.MERGE_CASES:
            c = R.merge_case(name, small=True)
            pts = np.ascontiguousarray(np.concatenate(c["clouds"]), np.float32)
            st = np.ascontiguousarray(np.concatenate(c["stamps"]), np.uint32)
            n_l = np.array([len(p) for p in c["clouds"]], np.int32)
            hd = np.array(c["headers"], np.uint64)
            op, os_ = np.zeros((len(pts) + 1, 4), np.float32), np.zeros(len(pts) + 1, np.uint32)
            m = L.h_merge(len(n_l), P(pts, C.c_float), P(st, C.c_uint32), P(n_l, C.c_int), P(hd, C.c_uint64), C.c_uint64(c["period"]), P(op, C.c_float),
                          P(os_, C.c_uint32))
            out["merge_%s_points" % name], out["merge_%s_stamps" % name] = op[:m].copy(), os_[:m].copy()
            out["merge_%s_input_hash" % name] = np.array([hash_of(pts), hash_of(st), hash_of(hd)])
            print(f"mergePoints {name}: {len(pts)} points in {len(n_l)} clouds -> {m}")
    np.savez_compressed(a.out, lat=lat, lon=lon, pin_offset=np.float64(R.PIN_OFFSET), fresh=fresh, pinned=pinned, inverse=inv, **out)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, {n} projection cases")


def hash_of(a):
    import zlib

    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


if __name__ == "__main__":
    main()
