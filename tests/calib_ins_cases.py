"""The lidar-INS calibration restated in numpy (sensor_driver/calibration/lidar_ins of the reference): the subsampling draws, the f32
Transform rules and an f64 form of them, the odometry interpolation with its quirks, the capped k-NN cost (brute force in f32 in the stated
operation order for small clouds, scipy's cKDTree in f64 for large ones), and the scene and drive of the end-to-end case."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calib_ins_e2e.npz")
METRICS = {0: (4, 10.0), 1: (2, 1.0)}  # metric -> (K = k + 1, cap on the squared distance): global, local


# ---- Scan::Scan's draws: std::default_random_engine + std::uniform_real_distribution<float>(0, 1) --------------------------------------------
def draws(stamp, n):
    x = (int(stamp) % (1 << 64)) % 2147483647 or 1
    out = np.empty(n, np.float32)
    for i in range(n):
        x = 16807 * x % 2147483647
        v = np.float32(x - 1) / np.float32(2147483646)
        out[i] = v if v < 1 else np.nextafter(np.float32(1), np.float32(0))
    return out


def keep_mask(n, stamp):
    ratio = min(np.float32(1.0), np.float32(6000.0) / np.float32(n + 1))
    return draws(stamp, n) < ratio


# ---- Transform: (t, q = w x y z); every operation in dtype dt ---------------------------------------------------------------------------------
def _a(v, dt):
    return np.asarray(v, dt)


def rotate(q, v, dt):
    q, v = _a(q, dt), _a(v, dt)
    uv = np.cross(q[1:], v).astype(dt)
    uv = uv + uv
    return (v + q[0] * uv + np.cross(q[1:], uv).astype(dt)).astype(dt)


def qmul(a, b, dt):
    a, b = _a(a, dt), _a(b, dt)
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]], dt)


def se3_exp(v, dt=np.float64):
    v = _a(v, dt)
    n = np.sqrt((v[3] * v[3] + v[4] * v[4]) + v[5] * v[5])
    if n < dt(1e-8):
        return np.concatenate([v[:3], _a([1, 0, 0, 0], dt)])
    ha = dt(0.5) * n
    return np.concatenate([v[:3], [np.cos(ha)], np.sin(ha) * (v[3:] / n)]).astype(dt)


def se3_log(T, dt=np.float64):
    T = _a(T, dt)
    q = T[3:]
    n = np.sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3])
    if n < np.finfo(dt).eps:
        m = np.abs(q[1:]).max()
        n = m * np.sqrt(((q[1:] / m) ** 2).sum()) if m > 0 else dt(0)
    if n == 0:
        return np.concatenate([T[:3], _a([0, 0, 0], dt)])
    angle = dt(2) * np.arctan2(n, abs(q[0]))
    if q[0] < 0:
        n = -n
    return np.concatenate([T[:3], angle * (q[1:] / n)]).astype(dt)


def se3_mul(a, b, dt=np.float64):
    a, b = _a(a, dt), _a(b, dt)
    return np.concatenate([a[:3] + rotate(a[3:], b[:3], dt), qmul(a[3:], b[3:], dt)]).astype(dt)


def se3_inverse(a, dt=np.float64):
    a = _a(a, dt)
    qi = np.array([a[3], -a[4], -a[5], -a[6]], dt)
    return np.concatenate([-rotate(qi, a[:3], dt), qi]).astype(dt)


def se3_matrix(a, dt=np.float64):
    a = _a(a, dt)
    w, x, y, z = a[3:]
    two = dt(2)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    one = dt(1)
    M = np.eye(4, dtype=dt)
    M[:3, :3] = [[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]]
    M[:3, 3] = a[:3]
    return M


def se3_from_matrix(M, dt=np.float64):
    """an f64 quaternion of the rotation block (any branch: only used on the f64 side of a comparison)"""
    from scipy.spatial.transform import Rotation

    M = np.asarray(M, np.float64)
    x, y, z, w = Rotation.from_matrix(M[:3, :3]).as_quat()
    return np.concatenate([M[:3, 3], [w, x, y, z]]).astype(dt)


def interpolate(stamps, Ts, stamp, start_idx=0, dt=np.float64):
    """Odom::getOdomTransform: (transform, match index); Ts m x 7"""
    m = len(stamps)
    idx = start_idx
    while idx < m - 1 and stamp > stamps[idx]:
        idx += 1
    if idx > 0:
        idx -= 1
    ratio = float(int(stamp) - int(stamps[idx])) / float(int(stamps[idx + 1]) - int(stamps[idx]))
    d = se3_log(se3_mul(se3_inverse(Ts[idx], dt), Ts[idx + 1], dt), dt)
    return se3_mul(Ts[idx], se3_exp(dt(ratio) * d, dt), dt), idx


def scan_poses(stamps, Ts, scan_stamps, time_offset, dt=np.float64):
    """Lidar::setOdomOdomTransforms: the match index is carried from scan to scan"""
    out, idx = [], 0
    for s in scan_stamps:
        T, idx = interpolate(stamps, Ts, int(s) + int(1000000.0 * time_offset), idx, dt)
        out.append(T)
    return out


# ---- the cost ----------------------------------------------------------------------------------------------------------------------------------
def combined_f32(mats, scans):
    """x' = ((m00 x + m01 y) + m02 z) + m03 in separately rounded f32; mats S x 16 f32, scans a list of n_s x 3 f32"""
    out = []
    for M, p in zip(np.asarray(mats, np.float32).reshape(-1, 4, 4), scans):
        p = np.asarray(p, np.float32).reshape(-1, 3)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        out.append(np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], 1))
    return np.concatenate(out).astype(np.float32) if out else np.zeros((0, 3), np.float32)


def terms_brute_f32(cloud, metric):
    """n x K: the K smallest of d2 = ((dx dx) + dy dy) + dz dz (f32) to the whole cloud, the point itself included, capped"""
    K, cap = METRICS[metric]
    c = np.asarray(cloud, np.float32)
    with np.errstate(over="ignore"):
        d = c[None, :, :] - c[:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.minimum(np.sort(d2, axis=1)[:, :K], np.float32(cap)).astype(np.float32)


def cost_kdtree(cloud, metric):
    """the cost in f64 through scipy's cKDTree"""
    from scipy.spatial import cKDTree

    K, cap = METRICS[metric]
    c = np.asarray(cloud, np.float64)
    d, _ = cKDTree(c).query(c, k=K)
    return float(np.minimum(d * d, cap).sum())


class Restated:
    """the calibration's state on the host in f64: kept scans, odometry, and the cost of a candidate x (6 or 7 parameters)"""

    def __init__(self, scans, scan_stamps, odom_T7, odom_stamps):
        self.scans = [np.asarray(s, np.float64).reshape(-1, 3) for s in scans]
        self.scan_stamps, self.odom_T7, self.odom_stamps = list(scan_stamps), [np.asarray(t, np.float64) for t in odom_T7], list(odom_stamps)
        self.poses = scan_poses(self.odom_stamps, self.odom_T7, self.scan_stamps, 0.0)

    def cloud(self, x):
        if len(x) > 6:
            self.poses = scan_poses(self.odom_stamps, self.odom_T7, self.scan_stamps, float(x[6]))
        T = se3_exp(np.asarray(x[:6], np.float64))
        out = []
        for P, s in zip(self.poses, self.scans):
            M = se3_matrix(se3_mul(P, T))
            out.append(s @ M[:3, :3].T + M[:3, 3])
        return np.concatenate(out)

    def cost(self, x, metric):
        return cost_kdtree(self.cloud(x), metric)


# ---- the end-to-end case -----------------------------------------------------------------------------------------------------------------------
# a small yard (surfaces 3 to 12 m away: the points of one scan lie closer together than the initial error moves them) and a slow drive that
# turns through almost a full circle: the mismatch between scans that a wrong extrinsic causes grows with the rotation between them
E2E = dict(scene=dict(half=9.0, n_boxes=14, seed=3, box_size=(1.0, 3.0), box_h=(1.0, 4.0), keep_clear=5.0),
           traj=dict(p0=(-2.0, -2.0, 1.8), t_static=0.0, speed=0.6, yaw_amp=2.5, sway=1.0), scan_seed=100, n_scans=6, n_beams=32, n_az=400, t0=2.0, dt_scan=1.5, odom_rate=100.0, stamp0=1_700_000_000_000_000,
           truth=(0.08, -0.06, 0.25, 0.04, -0.05, 0.02), init=(0.48, -0.40, 0.20, 0.075, -0.085, 0.045))


def e2e_inputs():
    """(scans: list of raw n x 3 f32 in the lidar frame, scan stamps (us), odometry 4 x 4 f32 list, odometry stamps (us))"""
    from lsd_amd import synth
    from scipy.spatial.transform import Rotation

    c = E2E
    scene = synth.Scene(**c["scene"])
    traj = synth.Trajectory(**c["traj"])
    Tl = se3_matrix(se3_exp(np.array(c["truth"], np.float64)))
    scans, stamps = [], []
    for i in range(c["n_scans"]):
        t = c["t0"] + i * c["dt_scan"]
        Rb, pb = traj.R(t), traj.pos(t)
        Rl, pl = Rb @ Tl[:3, :3], pb + Rb @ Tl[:3, 3]
        raw, _ = synth.make_scan(scene, pl, Rotation.from_matrix(Rl).as_quat(), seed=c["scan_seed"] + i, n_beams=c["n_beams"], n_az=c["n_az"])
        scans.append(np.ascontiguousarray(raw[:, :3], np.float32))
        stamps.append(c["stamp0"] + int(round(t * 1e6)))
    odom, ostamps = [], []
    n_od = int((c["t0"] + c["n_scans"] * c["dt_scan"] + 1.0) * c["odom_rate"])
    for j in range(n_od):
        t = j / c["odom_rate"]
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = traj.R(t), traj.pos(t)
        odom.append(M.astype(np.float32))
        ostamps.append(c["stamp0"] + int(round(t * 1e6)))
    return scans, stamps, odom, ostamps


def checksum(scans):
    import hashlib

    h = hashlib.sha256()
    for s in scans:
        h.update(np.ascontiguousarray(s, np.float32).tobytes())
    return h.hexdigest()


def e2e_restated(scans, stamps, odom, ostamps):
    """the restated state over the points the product keeps (the draws are the restatement's own)"""
    kept = [s[keep_mask(len(s), st)] for s, st in zip(scans, stamps)]
    return Restated(kept, stamps, [se3_from_matrix(M) for M in odom], ostamps)


def pose_errors(x, truth):
    """|dx|, |dy|, |dz| (m) and |droll|, |dpitch|, |dyaw| (rad, of the relative rotation's vector) between exp(x) and exp(truth)"""
    a, b = se3_exp(np.asarray(x[:6], np.float64)), se3_exp(np.asarray(truth, np.float64))
    d = se3_log(se3_mul(se3_inverse(b), a))
    return np.abs(a[:3] - b[:3]), np.abs(d[3:])
