"""The reference's `calibration.lidar_calibration` package over the device: same names, same argument orders.

    from lsd_amd.calib_lidar import align_points_to_xyplane, align_pq_to_known, align_points
    from lsd_amd.calib_lidar import xyzrpy_to_transform, xyzrpy_to_rt, rt_to_xyzrpy

The crop and the RANSAC of the ground calibration run on the device (`lio.GroundCalib`, csrc/calib_ground.hip; include/lio_hip.h states the
rules); the rest are a few f64 operations on the host.  Deviations from the reference:
  1. the draws of `fit_plane` are `lio_ground_draw(seed, attempt, n)` or the caller's `draws`, not numpy's global generator;
  2. `calc_rot_from` of two parallel vectors is the identity (the reference divides 0 by 0);
  3. `fit_plane` gives up after 11 * num_iteration attempts (the reference loops forever over a cloud whose triples are all colinear);
  4. ValueError names the cases the reference fails in by accident or answers with non-finite numbers;
  5. a polygon has at most `lio.GroundCalib.MAX_VERTICES` vertices.
There is no CPU fallback: without a device the first call that needs one raises.
"""
import numpy as np

from . import lio

_handles = {}


def _handle(device=0):
    if device not in _handles:
        _handles[device] = lio.GroundCalib(device)
    return _handles[device]


def _polygon(polygon):
    poly = np.asarray(polygon, np.float64)
    if poly.ndim != 2 or poly.shape[1] < 2:
        raise ValueError("polygon: m x 2 vertices are required")
    poly = np.ascontiguousarray(poly[:, :2])
    if len(poly) < 3:
        raise ValueError(f"polygon: fewer than 3 vertices ({len(poly)})")
    if len(poly) > lio.GroundCalib.MAX_VERTICES:
        raise ValueError(f"polygon: more than {lio.GroundCalib.MAX_VERTICES} vertices ({len(poly)})")
    return poly


def _cloud(points):
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] < 3:
        raise ValueError("points: n x (3 or more) is required")
    return np.ascontiguousarray(pts, np.float32)


def crop_points(points, polygon, device=0):
    """the rows of `points` (n x 3 or wider, taken as f32) whose (x, y) lies inside the polygon, in input order"""
    pts, poly = _cloud(points), _polygon(polygon)
    g = _handle(device)
    g.crop(pts, poly)
    return pts[g.indices()]


def _fit(g, n, sigma, num_iteration, thresh, seed, draws):
    if n < 3:
        raise ValueError(f"fit_plane: fewer than 3 points ({n})")
    if num_iteration < 1:
        raise ValueError(f"fit_plane: num_iteration = {num_iteration}")
    p = g.params(sigma=float(sigma), num_iteration=int(num_iteration), thresh=float(thresh), seed=int(seed) & 0xFFFFFFFF)
    if draws is not None:
        d = np.asarray(draws).reshape(-1, 3)
        if d.size and (d.min() < 0 or d.max() >= n or (d[:, 0] == d[:, 1]).any() or (d[:, 0] == d[:, 2]).any() or (d[:, 1] == d[:, 2]).any()):
            raise ValueError("fit_plane: a draw is not three distinct indices into the points")
    found, coef = g.fit(p, draws)
    return found, coef.astype(np.float64)


def fit_plane(points, sigma=1e-2, num_iteration=1000, thresh=0.9, seed=0, draws=None, device=0):
    """(a, b, c, d) f64 of the plane fit_plane's loop ends with, zeros when it found none; the arithmetic is f32 (points are taken as f32)"""
    pts = _cloud(points)
    if len(pts) < 3:
        raise ValueError(f"fit_plane: fewer than 3 points ({len(pts)})")
    g = _handle(device)
    g.set_points(pts)
    return _fit(g, len(pts), sigma, num_iteration, thresh, seed, draws)[1]


def calc_rot_from(vec1, vec2):
    """the rotation (Rodrigues) that turns the direction of vec1 into that of vec2; parallel vectors: the identity"""
    a = np.asarray(vec1, np.float64).reshape(3)
    b = np.asarray(vec2, np.float64).reshape(3)
    with np.errstate(invalid="ignore", divide="ignore"):
        a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    axis = np.cross(a, b)
    cos = np.dot(a, b)
    sin = np.sqrt(np.dot(axis, axis))
    if not sin > 0.0:
        if not np.isfinite(cos):
            raise ValueError("calc_rot_from: a vector is zero or not finite")
        if cos < 0.0:
            raise ValueError("calc_rot_from: opposite vectors leave the axis undefined")
        return np.eye(3)
    n = axis / np.linalg.norm(axis)
    skew = np.array([[0.0, -n[2], n[1]], [n[2], 0.0, -n[0]], [-n[1], n[0], 0.0]])
    return cos * np.eye(3) + (1 - cos) * np.outer(n, n) + sin * skew


def plane_to_transform(coef):
    """the 4 x 4 f64 transform of a fitted plane (a, b, c, d): the rotation of its normal onto +z, the translation (0, 0, d / c) with the
    quotient taken in f64 of the f32 coefficients, as the reference does on fit_plane's f64 array"""
    a, b, c, d = (float(v) for v in coef)
    if c == 0.0 or not np.isfinite(d / c):
        raise ValueError("align_points_to_xyplane: the plane is vertical (c = 0), d / c is not finite")
    T = np.eye(4)
    T[:3, :3] = calc_rot_from(np.array([a, b, c]), np.array([0.0, 0.0, 1.0]))
    T[2, 3] = d / c
    return T


def align_points_to_xyplane(points, roi_xy, seed=0, draws=None, device=0):
    """the 4 x 4 f64 transform that levels the lidar and puts the floor inside roi_xy at z = 0; points flat or n x 4 f32"""
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 4))
    poly = _polygon(roi_xy)
    g = _handle(device)
    n = g.crop(pts, poly)
    if n < 3:
        raise ValueError(f"align_points_to_xyplane: fewer than 3 points inside the polygon ({n})")
    found, coef = _fit(g, n, 0.05, 100, 0.9, seed, draws)
    if not found:
        raise ValueError("align_points_to_xyplane: no plane found")
    return plane_to_transform(coef)


def _similarity_rows(p0, p1, A, b):
    x0, y0 = float(p0[0]), float(p0[1])
    A += [[x0, -y0, 1.0, 0.0], [y0, x0, 0.0, 1.0]]
    b += [float(p1[0]), float(p1[1])]


def align_pq_to_known(p, q, pp, qq):
    """(R 3 x 3, t 3): the planar rotation (with scale) and shift that take p to pp and q to qq, from the 4 x 4 system in (cos, sin, dx, dy)"""
    A, b = [], []
    _similarity_rows(p, pp, A, b)
    _similarity_rows(q, qq, A, b)
    cos, sin, dx, dy = np.linalg.inv(np.array(A)) @ np.array(b)
    return np.array([[cos, -sin, 0.0], [sin, cos, 0.0], [0.0, 0.0, 1.0]]), np.array([dx, dy, 0.0])


def align_points(p0s, p1s):
    """the 4 x 4 transform of the least-squares planar (cos, sin, dx, dy) that takes the points p0s to p1s"""
    A, b = [], []
    for p0, p1 in zip(p0s, p1s):
        _similarity_rows(p0, p1, A, b)
    cos, sin, dx, dy = np.linalg.pinv(np.array(A)) @ np.array(b)
    T = np.eye(4)
    T[:2, :2] = [[cos, -sin], [sin, cos]]
    T[:2, 3] = [dx, dy]
    return T


# ---- transform.py: intrinsic Z-X-Y Euler angles (yaw about z, then pitch about the new x, then roll about the new y), degrees ----
def _rot_zxy(roll, pitch, yaw):
    r, p, y = np.deg2rad([roll, pitch, yaw])
    cz, sz, cx, sx, cy, sy = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    return np.array([[cz * cy - sz * sx * sy, -sz * cx, cz * sy + sz * sx * cy],
                     [sz * cy + cz * sx * sy, cz * cx, sz * sy - cz * sx * cy],
                     [-cx * sy, sx, cx * cy]])


def xyzrpy_to_rt(xyzrpy):
    roll, pitch, yaw = xyzrpy[3:]
    return _rot_zxy(roll, pitch, yaw), np.array(xyzrpy[:3])


def xyzrpy_to_transform(xyzrpy):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = xyzrpy_to_rt(xyzrpy)
    return T


def rt_to_xyzrpy(rot, t):
    R = np.asarray(rot, np.float64)
    pitch = np.arcsin(min(1.0, max(-1.0, R[2, 1])))
    yaw = np.arctan2(-R[0, 1], R[1, 1])
    roll = np.arctan2(-R[2, 0], R[2, 2])
    return list(t) + [float(v) for v in np.rad2deg([roll, pitch, yaw])]
