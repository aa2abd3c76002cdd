"""The lidar-IMU calibration's yardstick: the host half of calib_lidar_imu.cpp restated in numpy f64 (quaternions are (w, x, y, z); Eigen's
rules for the product, inverse, normalize, AngleAxisd(Quaterniond), toRotationMatrix, Quaterniond(Matrix3d), angularDistance), the solve over
numpy.linalg.svd, the object's bookkeeping, the local map as a list of clouds over the oracle's pcl::VoxelGrid, and the seeded cases: a drive
that rotates about all three axes (a yaw-only drive leaves the solve rank-deficient), a gyro stream from synth.imu_stream, and lidar deltas
from a known extrinsic rotation."""
import numpy as np

from lsd_amd import synth

EYE_Q = np.array([1.0, 0.0, 0.0, 0.0])
MAX_FRAMES = 200
LEAF = 0.2


def q_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def q_conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def q_norm2(q):
    return q[1] * q[1] + q[2] * q[2] + q[3] * q[3] + q[0] * q[0]


def q_inv(q):
    n2 = q_norm2(q)
    return q_conj(q) / n2 if n2 > 0 else np.zeros(4)


def q_normalized(q):
    n2 = q_norm2(q)
    return q / np.sqrt(n2) if n2 > 0 else q.copy()


def q_to_R(q):
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def q_from_R(M):
    t = M[0, 0] + M[1, 1] + M[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return np.array([w, (M[2, 1] - M[1, 2]) * t, (M[0, 2] - M[2, 0]) * t, (M[1, 0] - M[0, 1]) * t])
    i = 0
    if M[1, 1] > M[0, 0]:
        i = 1
    if M[2, 2] > M[i, i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = np.sqrt(M[i, i] - M[j, j] - M[k, k] + 1.0)
    q = np.zeros(4)
    q[1 + i] = 0.5 * t
    t = 0.5 / t
    q[0] = (M[k, j] - M[j, k]) * t
    q[1 + j] = (M[j, i] + M[i, j]) * t
    q[1 + k] = (M[k, i] + M[i, k]) * t
    return q


def angle_axis(q):
    n = np.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    if n < np.finfo(np.float64).eps:
        n = np.hypot(np.hypot(q[1], q[2]), q[3])
    if n != 0:
        angle = 2 * np.arctan2(n, abs(q[0]))
        if q[0] < 0:
            n = -n
        return angle, q[1:] / n
    return 0.0, np.array([1.0, 0.0, 0.0])


def aa_to_R(angle, a):
    s, c = np.sin(angle), np.cos(angle)
    sa, ca = s * a, (1 - c) * a
    R = np.zeros((3, 3))
    t = ca[0] * a[1]
    R[0, 1], R[1, 0] = t - sa[2], t + sa[2]
    t = ca[0] * a[2]
    R[0, 2], R[2, 0] = t + sa[1], t - sa[1]
    t = ca[1] * a[2]
    R[1, 2], R[2, 1] = t - sa[0], t + sa[0]
    R[0, 0], R[1, 1], R[2, 2] = ca[0] * a[0] + c, ca[1] * a[1] + c, ca[2] * a[2] + c
    return R


def angular_distance(a, b):
    d = q_mul(a, q_conj(b))
    return 2 * np.arctan2(np.sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3]), abs(d[0]))


def rot_angle(Ra, Rb):
    """angle of Ra^T Rb, from the skew part (exact near zero, where arccos of the trace loses half the digits)"""
    D = Ra.T @ Rb
    s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(s, 0.5 * (np.trace(D) - 1.0)))


def integrate(t, g):
    t, g = np.asarray(t, np.float64), np.asarray(g, np.float64).reshape(-1, 3)
    rot = np.zeros((len(t), 4))
    if len(t):
        rot[0] = EYE_Q
    for i in range(1, len(t)):
        a = (0.5 * (g[i - 1] + g[i])) * (t[i] - t[i - 1])
        rot[i] = q_mul(rot[i - 1], np.array([1.0, 0.5 * a[0], 0.5 * a[1], 0.5 * a[2]]))
    return rot


def interpolate(qs, qe, scale):
    if scale == 0 or scale > 1:
        return EYE_Q.copy()
    d = q_normalized(q_mul(q_inv(qs), qe))
    angle, axis = angle_axis(d)
    return q_normalized(q_mul(qs, q_from_R(aa_to_R(angle * scale, axis))))


def time_align(it, irot, ft):
    """(frames erased at the front, attitudes of the aligned frames that follow them)"""
    first = 0
    while first < len(ft) and not ft[first] >= it[0]:
        first += 1
    last, out = 0, []
    for i in range(first, len(ft)):
        while last != len(it) and not it[last] >= ft[i]:
            last += 1
        if last != 0:
            last -= 1
        if last + 1 == len(it):
            break
        scale = (ft[i] - it[last]) / (it[last + 1] - it[last])
        out.append(interpolate(irot[last], irot[last + 1], scale))
    return first, np.array(out).reshape(-1, 4)


def _L(q):
    w, x, y, z = q
    return np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])


def _R(q):
    w, x, y, z = q
    return np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]])


def solve(pairs, weighted=True):
    """pairs: n x 8 (q_lidar, q_imu); the right singular vector of the smallest singular value"""
    pairs = np.asarray(pairs, np.float64).reshape(-1, 8)
    if len(pairs) == 0:
        return EYE_Q.copy()
    A = np.zeros((4 * len(pairs), 4))
    for i, p in enumerate(pairs):
        ql, qb = p[:4], p[4:]
        deg = 180.0 / np.pi * angular_distance(qb, ql)
        huber = 2.0 / deg if (weighted and deg > 2.0) else 1.0
        A[4 * i:4 * i + 4] = huber * (_L(qb) - _R(ql))
    return np.linalg.svd(A)[2][3].copy()


class Restated:
    """CalibLidarImu's host side as calib_wrapper.cpp drives it"""

    def __init__(self):
        self.it, self.gyr, self.frames, self.aligned, self.q_l_b = [], [], [], [], EYE_Q.copy()

    def add_imu(self, rows):
        for r in np.asarray(rows, np.float64).reshape(-1, 7):
            self.it.append(r[0] / 1000000.0)
            self.gyr.append(r[1:4] / 180.0 * np.pi)

    def add_frame(self, stamp_us, gT, dT):
        if len(self.frames) >= MAX_FRAMES:
            return
        self.frames.append((int(stamp_us) / 1000000.0, np.array(dT, np.float64), np.array(gT, np.float64)))

    def pairs(self):
        out = []
        for i in range(1, len(self.aligned)):
            out.append(np.concatenate([q_from_R(self.aligned[i][0][1][:3, :3]), q_mul(q_inv(self.aligned[i - 1][1]), self.aligned[i][1])]))
        return np.array(out).reshape(-1, 8)

    def calibrate(self):
        """the 3 x 3, or None where the reference reads past the end"""
        if not self.it:
            return None
        rot = integrate(self.it, self.gyr)
        first, q = time_align(self.it, rot, [f[0] for f in self.frames])
        del self.frames[:first]
        if not self.frames:
            return None
        for i in range(len(q)):
            self.aligned.append((self.frames[i], q[i]))
        self.q_l_b = solve(self.pairs())
        return q_to_R(q_normalized(self.q_l_b))

    def lidar_poses(self):
        cur, out = np.eye(4), []
        for i in range(1, len(self.aligned)):
            cur = cur @ self.aligned[i][0][1]
            out.append(cur.copy())
        return np.array(out).reshape(-1, 4, 4)

    def imu_poses(self):
        cur, out = np.eye(4), []
        for i in range(1, len(self.aligned)):
            est = q_mul(q_inv(self.aligned[i - 1][1]), self.aligned[i][1])
            T = self.aligned[i][0][1].copy()
            T[:3, :3] = q_to_R(q_mul(q_mul(q_inv(self.q_l_b), est), self.q_l_b))
            cur = cur @ T
            out.append(cur.copy())
        return np.array(out).reshape(-1, 4, 4)


# ---- seeded cases --------------------------------------------------------------------------------------------------------------------------
def euler_R(roll_deg, pitch_deg, yaw_deg):
    r, p, y = np.radians([roll_deg, pitch_deg, yaw_deg])
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


GENERAL = (20.0, -10.0, 35.0)


def drive(**over):
    """a drive that turns about all three axes within a second"""
    kw = dict(t_static=0.0, speed=3.0, tau=1.0, sway=0.5, yaw_amp=0.6, pitch_amp=0.25, roll_amp=0.3, heading=0.2)
    kw.update(over)
    return synth.Trajectory(**kw)


def imu_rows(traj, t0, t1, rate=200.0):
    """rows as calib_imu_set_imu takes them: stamp us, gyro deg/s, acc g"""
    rows = [np.concatenate([[round(t * 1e6)], g * 180.0 / np.pi, a / 9.81]) for t, g, a in synth.imu_stream(traj, t0, t1, rate=rate)]
    return np.array(rows).reshape(-1, 7)


def body_pose(traj, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = traj.R(float(t)), traj.pos(float(t))
    return T


def frame_list(traj, stamps_us, ext_R):
    """(stamp us, global_T, delta_T) per frame for a lidar mounted with ext_R (lidar -> body): the lidar's motion since the frame before"""
    X = np.eye(4)
    X[:3, :3] = ext_R
    out, prev, T0 = [], None, None
    for s in stamps_us:
        Tl = body_pose(traj, s / 1e6) @ X
        if T0 is None:
            T0 = Tl
        g = np.linalg.inv(T0) @ Tl
        d = np.eye(4) if prev is None else np.linalg.inv(prev) @ g
        out.append((int(s), g, d))
        prev = g
    return out


def host_case(ext=GENERAL, n_frames=12, t0=0.5, dt_us=100000, offset_us=2300, imu_t0=0.4, imu_t1=2.0, rate=200.0, traj=None):
    """the general case: 12 frames 0.1 s apart, stamped between IMU samples, a 200 Hz gyro stream that covers them"""
    traj = traj or drive()
    stamps = [round(t0 * 1e6) + offset_us + dt_us * i for i in range(n_frames)]
    R = euler_R(*ext)
    return dict(traj=traj, R=R, imu=imu_rows(traj, imu_t0, imu_t1, rate), frames=frame_list(traj, stamps, R))


def run(obj, case, n_calibrate=1):
    """feed a case to an object with add_imu / add_frame / calibrate (the restatement, or an adapter around the product)"""
    obj.add_imu(case["imu"])
    for s, g, d in case["frames"]:
        obj.add_frame(s, g, d)
    R = None
    for _ in range(n_calibrate):
        R = obj.calibrate()
    return R


# ---- the odometry's side: scans of a scene, the map as a list of clouds, the twin over the public entries ---------------------------------
def quat_xyzw_of_R(R):
    q = q_from_R(np.asarray(R, np.float64))
    return np.array([q[1], q[2], q[3], q[0]])


class LidarDrive(synth.Trajectory):
    """a lidar that moves by `step` metres and turns by `step_deg` (roll, pitch, yaw) per frame period, on a body whose IMU is mounted with
    ext_R (lidar -> body): lidar_T(t) is the lidar's world pose, R(t) / pos(t) the body's (what synth.imu_stream differentiates)"""

    def __init__(self, step=(0.4, 0.15, 0.0), step_deg=(-0.8, 1.0, 2.5), ext_R=np.eye(3), period=0.1):
        super().__init__(t_static=0.0)
        self.step, self.step_deg, self.ext_R, self.period = np.asarray(step, np.float64), step_deg, np.asarray(ext_R, np.float64), period

    def lidar_T(self, t):
        k = float(t) / self.period
        T = np.eye(4)
        T[:3, :3] = euler_R(self.step_deg[0] * k, self.step_deg[1] * k, self.step_deg[2] * k)
        T[:3, 3] = np.array([0.0, 0.0, 1.8]) + self.step * k
        return T

    def R(self, t):
        return self.lidar_T(t)[:3, :3] @ self.ext_R.T

    def pos(self, t):
        return self.lidar_T(t)[:3, 3]


def scan_drive(n_frames=8, n_az=360, n_beams=16, seed=3, drive=None):
    """scans along a LidarDrive, one per period from t = 0: [(points n x 4 f32, world pose 4 x 4)]"""
    drive = drive or LidarDrive()
    scene = synth.Scene(half=30.0, n_boxes=14, seed=seed, box_size=(2.0, 8.0), keep_clear=4.0)
    out = []
    for i in range(n_frames):
        T = drive.lidar_T(i * drive.period)
        pts, _ = synth.make_scan(scene, T[:3, 3], quat_xyzw_of_R(T[:3, :3]), seed=100 + i, n_beams=n_beams, n_az=n_az, max_range=60.0)
        out.append((pts, T))
    return out


def transform_f64(T, pts):
    """pcl::transformPointCloud(in, out, Matrix4d): f64, terms left to right, cast to f32; the intensity kept"""
    T = np.asarray(T, np.float64)
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    out = pts.copy()
    for r in range(3):
        out[:, r] = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32)
    return out


def voxel_filter(pts, leaf=LEAF):
    import oracle

    return oracle.voxel_downsample(np.ascontiguousarray(pts, np.float32), leaf)


class MapBook:
    """local_map_ as the list [raw scan 0, filter(T_k scan_k), ...]"""

    def __init__(self):
        self.clouds = []

    def first(self, pts):
        self.clouds = [np.ascontiguousarray(pts, np.float32).copy()]

    def key_frame(self, pts, gT):
        self.clouds.append(voxel_filter(transform_f64(gT, np.ascontiguousarray(pts, np.float32))))

    def map(self):
        return np.concatenate(self.clouds, 0)

    def target(self):
        return self.map() if len(self.clouds) == 1 else voxel_filter(self.map())


def sorted_rows(p):
    p = np.ascontiguousarray(p, np.float32)
    return p[np.lexsort(p.view(np.uint32).T[::-1])]


def f32_round(T):
    return np.asarray(T, np.float64).astype(np.float32).astype(np.float64)


class Twin:
    """get_lidar_T_R / addLidarData built from the public entries with a host round trip per stage: lio_scan_voxel_downsample for the frame,
    lio_cloud_append_host + the cloud filter for the key frame, a host concatenation and a lio_cloud filter of the whole map,
    lio_gicp_set_target / _set_source / _align with lio_estimate_matcher_params, the f32 rounding"""

    def __init__(self, max_points=1 << 16, max_scan=None):
        import ctypes as C

        from lsd_amd import capi, lio

        lp = capi.LoopParams()
        capi.lib().lio_loop_default_params(C.byref(lp))
        self.prm = capi.NdtParams()
        capi.lib().lio_estimate_matcher_params(C.byref(self.prm))
        self.lio = lio
        self.scan = lio.Scan(max_raw=max_scan or max_points, max_ds=max_scan or max_points)
        self.g = lio.Gicp(grid_resolution=lp.grid_resolution, max_points=max_points, k=lp.k_correspondences)
        self.g.set_voxel_mode(lp.voxel_resolution, 1)
        self.book, self.last, self.max_iterations = MapBook(), np.eye(4), self.prm.max_iterations
        self.target = None

    def filter_frame(self, pts):
        self.scan.upload(pts)
        n = self.scan.voxel_downsample(LEAF)
        return self.scan.get_ds()[:n].copy()

    def lidar_pose(self, pts):
        ds = self.filter_frame(pts)
        if not self.book.clouds:
            self.book.first(pts)
            self.target = self.book.map()
            self.g.set_target(self.target)
            self.last = np.eye(4)
            return np.eye(4)
        self.g.set_source(ds)
        T, conv, it = self.g.align(f32_round(self.last), max_corr_dist=1.0, rotation_epsilon_deg=self.prm.rotation_epsilon_deg,
                                   transformation_epsilon=self.prm.transformation_epsilon, max_iterations=self.max_iterations, max_process_time_ms=-1.0)
        if not conv:
            return np.eye(4)
        self.last = f32_round(T)
        return self.last.copy()

    def add_frame(self, pts, gT):
        c = self.lio.Cloud()
        c.append_host(pts, T=gT)
        c.voxel_downsample(LEAF)
        self.book.clouds.append(c.download().copy())
        c.close()
        whole = self.lio.Cloud()
        whole.append_host(self.book.map())
        whole.voxel_downsample(LEAF)
        self.target = whole.download().copy()
        whole.close()
        self.g.set_target(self.target)


def cfg_of(T):
    """(x, y, z, yaw, pitch, roll) with the angles in degrees (the key-frame rule of ImuCalib.is_keyframe compares these)"""
    R = np.asarray(T, np.float64)[:3, :3]
    yaw, pitch, roll = np.arctan2(R[1, 0], R[0, 0]), np.arcsin(-np.clip(R[2, 0], -1, 1)), np.arctan2(R[2, 1], R[2, 2])
    return np.concatenate([np.asarray(T, np.float64)[:3, 3], np.degrees([yaw, pitch, roll])])


class KeyFrameRule:
    """ImuCalib.is_keyframe: the first frame is remembered and is no key frame; then 2.0 m or 5.0 in the norm of the angle differences"""

    def __init__(self):
        self.last = None

    def __call__(self, T):
        c = cfg_of(T)
        if self.last is None:
            self.last = c
            return False
        if np.linalg.norm(c[:3] - self.last[:3]) > 2.0 or np.linalg.norm(c[3:] - self.last[3:]) > 5.0:
            self.last = c
            return True
        return False
