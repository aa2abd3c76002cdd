"""The numpy restatement behind tests/test_keyframe_*.py: the mapping mode's key-frame producer (hdl_graph_slam_nodelet.cpp:163-246,
keyframe_updater.hpp:42-75, information_matrix_calculator.cpp:110-138, slam.cpp:400-411, slam_utils.cpp:236-241) by the rules include/lio_hip.h
states.  Distances are brute force in f32 with the index's operation order, ((dx*dx) + dy*dy) + dz*dz with d = p - q, every operation rounded on
its own (numpy's f32 arithmetic); the voxel grid and the undistortion are the existing oracle's.  Nothing here calls the library under test."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

DBL_MAX = np.finfo(np.float64).max
F32 = np.float32


# ---- keyframe_updater.hpp:60-75 -------------------------------------------------------------------------------------------------------------
def rigid_inverse(T):
    R, t = T[:3, :3], T[:3, 3]
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R.T, -R.T @ t
    return out


def decide(prev, pose, D, A):
    """(need, must, dx, da, dx64): dx, da are the f32 values is_update stores (as Python floats), dx64 what update() accumulates"""
    prev, pose = np.asarray(prev, np.float64).reshape(4, 4), np.asarray(pose, np.float64).reshape(4, 4)
    R = prev[:3, :3].T @ pose[:3, :3]
    t = prev[:3, :3].T @ (pose[:3, 3] - prev[:3, 3])
    dx64 = float(np.sqrt(t @ t))
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    c = (np.trace(R) - 1.0) / 2.0
    ang = np.arctan2(np.sqrt(v @ v) / 2.0, c)  # (sin, cos) of the angle from the antisymmetric part and the trace
    dx, da = float(F32(dx64)), float(F32(ang / np.pi * 180.0))
    need = not (dx < D / 2.0 and da < A / 2.0)
    must = need and (dx >= D * 3.0 / 2.0 or da >= A * 3.0 / 2.0)
    return need, must, dx, da, dx64


# ---- the two filters ------------------------------------------------------------------------------------------------------------------------
def d2_f32(q, pts):
    """f32 squared distances from one query to every row of pts, the index's order"""
    dx, dy, dz = pts[:, 0] - q[0], pts[:, 1] - q[1], pts[:, 2] - q[2]
    return ((dx * dx) + dy * dy) + dz * dz


def radius_keep(xyzi, radius=1.0, min_neighbours=3):
    """(kept input indices ascending, rows dropped as not finite): a finite point stays iff more than min_neighbours finite points, itself included,
    have d2 <= f32(radius * radius)"""
    p = np.ascontiguousarray(xyzi, F32).reshape(-1, 4)
    fin = np.isfinite(p[:, :3]).all(1)
    idx = np.flatnonzero(fin)
    q = p[idx, :3]
    r2 = F32(radius * radius)
    keep = np.zeros(len(q), bool)
    for a in range(0, len(q), 512):
        b = q[a:a + 512]
        dx, dy, dz = q[None, :, 0] - b[:, None, 0], q[None, :, 1] - b[:, None, 1], q[None, :, 2] - b[:, None, 2]
        d2 = ((dx * dx) + dy * dy) + dz * dz
        keep[a:a + 512] = (d2 <= r2).sum(1) > min_neighbours
    return idx[keep].astype(np.uint32), int(len(p) - len(idx))


def range_keep(xyzi, rng):
    """pointsDistanceFilter(0, rng): the f32 |x|, |y| against the doubles, strictly"""
    p = np.ascontiguousarray(xyzi, F32).reshape(-1, 4)
    ax, ay = np.abs(p[:, 0]).astype(np.float64), np.abs(p[:, 1]).astype(np.float64)
    return (ax > 0.0) & (ax < rng) & (ay > 0.0) & (ay < rng)


def filters(xyzi, radius, min_neighbours, rng):
    """indices kept by the radius filter and then, rng > 0, the range filter; and the count after the radius filter alone"""
    p = np.ascontiguousarray(xyzi, F32).reshape(-1, 4)
    idx, dropped = radius_keep(p, radius, min_neighbours)
    n_rad = len(idx)
    if rng > 0:
        idx = idx[range_keep(p[idx], rng)]
    return idx, n_rad, dropped


# ---- transforms -----------------------------------------------------------------------------------------------------------------------------
def transform_f32(xyzi, T):
    """pcl::transformPointCloud with T.cast<float>(): f32, terms left to right"""
    p = np.ascontiguousarray(xyzi, F32).reshape(-1, 4)
    M = np.asarray(T, np.float64).reshape(4, 4).astype(F32)
    out = p.copy()
    for r in range(3):
        out[:, r] = ((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3]
    return out


def transform_f64(xyzi, T):
    """pcl::transformPointCloud with a Matrix4d: f64, terms left to right, cast to f32"""
    p = np.ascontiguousarray(xyzi, F32).reshape(-1, 4)
    M = np.asarray(T, np.float64).reshape(4, 4)
    x, y, z = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64), p[:, 2].astype(np.float64)
    out = p.copy()
    for r in range(3):
        out[:, r] = (((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]).astype(F32)
    return out


# ---- calc_fitness_score ---------------------------------------------------------------------------------------------------------------------
def nearest_d2_brute(src, target):
    """the f32 squared distance from every row of src to its nearest row of target, brute force"""
    s, t = np.ascontiguousarray(src, F32)[:, :3], np.ascontiguousarray(target, F32)[:, :3]
    out = np.full(len(s), np.inf, F32)
    for a in range(0, len(s), 256):
        b = s[a:a + 256]
        dx, dy, dz = t[None, :, 0] - b[:, None, 0], t[None, :, 1] - b[:, None, 1], t[None, :, 2] - b[:, None, 2]
        out[a:a + 256] = (((dx * dx) + dy * dy) + dz * dz).min(1)
    return out


def nearest_d2_gated(src, target, max_range):
    """nearest_d2_brute where it matters: the brute-force f32 minimum over the target points within sqrt(max_range) + 1 % of the query (a k-d
    tree in f64 only SELECTS them: a point outside that ball has an f32 d2 above max_range, so neither the gate nor a gated minimum can see
    it), +inf where there is none.  tests/test_keyframe_cpu.py checks it against nearest_d2_brute."""
    from scipy.spatial import cKDTree

    s, t = np.ascontiguousarray(src, F32)[:, :3], np.ascontiguousarray(target, F32)[:, :3]
    out = np.full(len(s), np.inf, F32)
    if len(t) == 0:
        return out
    near = cKDTree(t.astype(np.float64)).query_ball_point(s.astype(np.float64), np.sqrt(max_range) * 1.01)
    for i, c in enumerate(near):
        if c:
            out[i] = d2_f32(s[i], t[np.asarray(c)]).min()
    return out


def fitness(local_map, cloud, T, max_range=1.0, gated=True):
    """(score, nr): calc_fitness_score(local_map, cloud, T, nr, max_range)"""
    if len(cloud) == 0 or len(local_map) == 0:
        return DBL_MAX, 0
    moved = transform_f32(cloud, T)
    d2 = nearest_d2_gated(moved, local_map, max_range) if gated else nearest_d2_brute(moved, local_map)
    inl = d2 <= F32(max_range)
    nr = int(inl.sum())
    return (float(d2[inl].astype(np.float64).sum() / nr), nr) if nr else (DBL_MAX, 0)


# ---- the local map's ring -------------------------------------------------------------------------------------------------------------------
def ring_append(local_map, cloud, T, cap):
    out = np.concatenate([local_map.reshape(-1, 4), transform_f64(cloud, T)]) if len(cloud) else local_map.reshape(-1, 4)
    return np.ascontiguousarray(out[max(0, len(out) - cap):], F32)


# ---- cloud_callback -------------------------------------------------------------------------------------------------------------------------
class RefKeyFramer:
    def __init__(self, D=1.0, A=10.0, resolution=0.2, key_frame_range=50.0, scan_period=0.1, radius=1.0, min_neighbours=3, cap=100000, local_map_distance=2.0,
                 fitness_range=1.0):
        self.D, self.A, self.res, self.rng, self.period = D, A, resolution, key_frame_range, scan_period
        self.radius, self.min_nb, self.cap, self.fit_range = radius, min_neighbours, cap, fitness_range
        self.step = max(1, int(np.round(local_map_distance / D)))
        self.reset()

    def reset(self):
        self.first, self.prev, self.accum = True, np.eye(4), 0.0
        self.best_score, self.best_inlier, self.average, self.count = DBL_MAX, 0.0, 0.0, 0
        self.best = None
        self.local_map = np.zeros((0, 4), F32)
        self.out = []
        self.contests = []  # (lhs, rhs) of every election comparison

    def push(self, xyzi, stamp_us, header_us, odom, delta=None, pose_stamps=None, poses=None):
        import oracle

        odom = np.asarray(odom, np.float64).reshape(4, 4)
        rep = dict(first=0, need=0, must=0, elected=0, emitted=0, nr=0, n_downsampled=0, score=DBL_MAX, dx=0.0, da=0.0)
        pts = np.ascontiguousarray(xyzi, F32).reshape(-1, 4)
        if len(pts) == 0:
            return self._close(rep)
        if self.first:
            self.first, self.prev = False, odom.copy()
            ds = oracle.voxel_downsample(pts, self.res)
            self.local_map = ring_append(np.zeros((0, 4), F32), ds, odom, self.cap)
            rep.update(first=1, n_downsampled=len(ds))
            return self._close(rep)
        need, must, dx, da, dx64 = decide(self.prev, odom, self.D, self.A)
        rep.update(need=int(need), must=int(must), dx=dx, da=da)
        if not need:
            return self._close(rep)
        if poses is not None and len(poses):
            und = oracle.undistort_poses(pts, stamp_us, header_us, pose_stamps, poses) if len(poses) >= 2 else pts
        else:
            und = oracle.undistort_delta(pts, stamp_us, np.asarray(delta, np.float64).astype(F32), self.period)
        ds = oracle.voxel_downsample(und, self.res)
        score, nr = fitness(self.local_map, ds, odom, self.fit_range)
        inlier = float(F32(nr) / F32(len(ds))) if len(ds) else float("nan")
        lhs, rhs = score * 0.8 + (1.0 - inlier) * 0.2, self.best_score * 0.8 + (1.0 - self.best_inlier) * 0.2
        self.contests.append((lhs, rhs))
        if lhs <= rhs:
            self.best_score, self.best_inlier = score, inlier
            self.best = (ds, odom.copy(), int(header_us))
            rep["elected"] = 1
        rep.update(nr=nr, n_downsampled=len(ds), score=score)
        if must:
            self.accum += dx64
            self.prev = odom.copy()
            if self.best is not None:
                cloud, pose, stamp = self.best
                idx, n_rad, _ = filters(cloud, self.radius, self.min_nb, self.rng)
                self.out.append(dict(points=cloud[idx], pose=pose, stamp=stamp, accum_distance=self.accum, n_before_filters=len(cloud), n_after_radius=n_rad))
                self.count += 1
                self.average = (self.average * (self.count - 1) + self.best_score) / self.count
                self.best_score = DBL_MAX
                if self.count % self.step == 0:
                    self.local_map = ring_append(self.local_map, cloud, pose, self.cap)
                rep["emitted"] = 1
        return self._close(rep)

    def _close(self, rep):
        rep.update(accum_distance=self.accum, average_score=self.average, local_map_size=len(self.local_map))
        return rep


# ---- the drive of tests/test_keyframe_gpu.py ------------------------------------------------------------------------------------------------
def drive_frames(n=40, seed=7):
    """n frames along a synth trajectory: (points, stamps, header stamp us, odometry pose, delta pose, pose stamps, pose list)"""
    from lsd_amd import synth

    scene = synth.Scene(half=60.0, n_boxes=25, seed=seed)
    tr = synth.Trajectory(t_static=0.0, speed=6.0, tau=0.5, sway=1.0, yaw_amp=0.3)

    def pose(t):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = tr.R(t), tr.pos(t)
        return T

    frames = []
    for k in range(n):
        tb = 1.0 + 0.1 * k
        pts, st = synth.make_sweep(scene, tr, tb, seed=100 + k, n_beams=16, n_az=250, fov_deg=(-20.0, 10.0))
        T0 = pose(tb)
        inv0 = rigid_inverse(T0)
        stamps = np.array([0, 50_000, 100_000], np.uint64) + np.uint64(round(tb * 1e6))
        plist = np.stack([inv0 @ pose(tb + 0.05 * j) for j in range(3)])
        frames.append((pts, st, int(round(tb * 1e6)), T0, inv0 @ pose(tb + 0.1), stamps, plist))
    return frames
