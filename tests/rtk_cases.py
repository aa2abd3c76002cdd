"""The numpy / plain-Python restatement of the GNSS side of mapping mode (include/lio_hip.h, "Geodesy and the RTK track" and "Several lidars
into one frame"), and the seeded cases the tests share.  Written from the reference's statements, independent of the library:

  UtmRef                UTMProjector (UTMProjector.cpp:7-117)          grid_convergence      get_grid_convergence (:119-122)
  transform_from_rpyt   getTransformFromRPYT (slam_utils.cpp:88-96)    interpolate_transform interpolateTransform (slam_utils.cpp:126-161)
  rtk_transform_utm / rtk_transform_origin   the two computeRTKTransform forms (slam_utils.cpp:112-124, rtkm.cpp:125-139)
  TrackRef              RTKM's mTimedInsData (rtkm.cpp:37-54, 91-95, 141-213)
  GnssQueueRef          the graph's gps_queue (hdl_graph_slam_nodelet.cpp:141-156, 349-460, 653-660)
  merge_points          mergePoints + preprocessPoints (slam_utils.cpp:249-273, slam_base.h:83-85)

Scalars are Python floats (IEEE f64, one rounding per operation, evaluated left to right like the C++)."""
import bisect
import math

import numpy as np

PI = 3.1415926535897932384626433832795
ANG2RAD = 0.01745329251994
NO_ORIGIN, TOO_FEW, EARLY, LATE, EXACT, INTERPOLATED = "no_origin", "too_few", "early", "late", "exact", "interpolated"


class UtmRef:
    def __init__(self, zone_width=6):
        self.zone_width = int(zone_width)
        self.project_no = -1

    def forward(self, latitude, longitude):
        zw = self.zone_width
        iPI = PI / 180
        a = 6378137.0
        f = 1.0 / 298.257222101
        if self.project_no < 0:
            self.project_no = int(math.floor(longitude / zw))
        ProjNo = float(self.project_no)
        longitude0 = ProjNo * zw + zw // 2
        longitude0 = longitude0 * iPI
        longitude1 = longitude * iPI
        latitude1 = latitude * iPI
        e2 = 2 * f - f * f
        ee = e2 * (1.0 - e2)
        sin, cos, tan, sqrt = math.sin, math.cos, math.tan, math.sqrt
        NN = a / sqrt(1.0 - e2 * sin(latitude1) * sin(latitude1))
        T = tan(latitude1) * tan(latitude1)
        C = ee * cos(latitude1) * cos(latitude1)
        A = (longitude1 - longitude0) * cos(latitude1)
        M = a * ((1 - e2 / 4 - 3 * e2 * e2 / 64 - 5 * e2 * e2 * e2 / 256) * latitude1 -
                 (3 * e2 / 8 + 3 * e2 * e2 / 32 + 45 * e2 * e2 * e2 / 1024) * sin(2 * latitude1) +
                 (15 * e2 * e2 / 256 + 45 * e2 * e2 * e2 / 1024) * sin(4 * latitude1) -
                 (35 * e2 * e2 * e2 / 3072) * sin(6 * latitude1))
        xval = NN * (A + (1 - T + C) * A * A * A / 6 + (5 - 18 * T + T * T + 72 * C - 58 * ee) * A * A * A * A * A / 120)
        yval = M + NN * tan(latitude1) * (A * A / 2 + (5 - T + 9 * C + 4 * C * C) * A * A * A * A / 24 +
                                          (61 - 58 * T + T * T + 600 * C - 330 * ee) * A * A * A * A * A * A / 720)
        X0 = 1000000 * (ProjNo + 1) + 500000
        xval = xval + X0
        yval = yval + 0.0
        return (xval - 500000) * 0.9996 + 500000, yval * 0.9996

    def inverse(self, x, y):
        iPI = PI / 180.0
        zw = 6.0
        a = 6378137.0
        f = 1.0 / 298.257222101
        if self.project_no < 0:
            self.project_no = int(math.floor(x / 1000000) - 1)
        ProjNo = float(self.project_no + 1)
        longitude0 = (ProjNo - 1) * zw + zw / 2
        longitude0 = longitude0 * iPI
        X0 = ProjNo * 1000000 + 500000
        xval = (x - 500000) / 0.9996 + 500000 - X0
        yval = y / 0.9996 - 0.0
        sin, cos, tan, sqrt = math.sin, math.cos, math.tan, math.sqrt
        e2 = 2 * f - f * f
        e1 = (1.0 - sqrt(1 - e2)) / (1.0 + sqrt(1 - e2))
        ee = e2 * (1.0 - e2)
        M = yval
        u = M / (a * (1 - e2 / 4 - 3 * e2 * e2 / 64 - 5 * e2 * e2 * e2 / 256))
        fai = (u + (3 * e1 / 2 - 27 * e1 * e1 * e1 / 32) * sin(2 * u) + (21 * e1 * e1 / 16 - 55 * e1 * e1 * e1 * e1 / 32) * sin(4 * u) +
               (151 * e1 * e1 * e1 / 96) * sin(6 * u) + (1097 * e1 * e1 * e1 * e1 / 512) * sin(8 * u))
        C = ee * cos(fai) * cos(fai)
        T = tan(fai) * tan(fai)
        NN = a / sqrt(1.0 - e2 * sin(fai) * sin(fai))
        R = a * (1 - e2) / sqrt((1 - e2 * sin(fai) * sin(fai)) * (1 - e2 * sin(fai) * sin(fai)) * (1 - e2 * sin(fai) * sin(fai)))
        D = xval / NN
        longitude1 = longitude0 + (D - (1 + 2 * T + C) * D * D * D / 6 +
                                   (5 - 2 * C + 28 * T - 3 * C * C + 8 * ee + 24 * T * T) * D * D * D * D * D / 120) / cos(fai)
        latitude1 = fai - (NN * tan(fai) / R) * (D * D / 2 - (5 + 3 * T + 10 * C - 4 * C * C - 9 * ee) * D * D * D * D / 24 +
                                                 (61 + 90 * T + 298 * C + 45 * T * T - 256 * ee - 3 * C * C) * D * D * D * D * D * D / 720)
        return latitude1 / iPI, longitude1 / iPI

    def longitude0(self):
        return float(self.project_no * self.zone_width + self.zone_width // 2)


def grid_convergence(longitude0, lat, lon):
    return math.atan(math.tan((lon - longitude0) / 180.0 * math.pi) * math.sin(lat / 180.0 * math.pi)) * 180.0 / math.pi


def transform_from_rpyt(x, y, z, yaw, pitch, roll):
    cy, sy = math.cos(yaw * ANG2RAD), math.sin(yaw * ANG2RAD)
    cp, sp = math.cos(pitch * ANG2RAD), math.sin(pitch * ANG2RAD)
    cr, sr = math.cos(roll * ANG2RAD), math.sin(roll * ANG2RAD)
    Rz = np.array([[cy, -sy, 0, 0], [sy, cy, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    Rx = np.array([[1, 0, 0, 0], [0, cp, -sp, 0], [0, sp, cp, 0], [0, 0, 0, 1.0]])
    Ry = np.array([[cr, 0, sr, 0], [0, 1, 0, 0], [-sr, 0, cr, 0], [0, 0, 0, 1.0]])
    T = np.eye(4)
    T[:3, 3] = [x, y, z]
    return T @ Rz @ Rx @ Ry


def _quat_of(R):  # Eigen's Quaterniond(Matrix3d): (w, x, y, z)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        r = math.sqrt(t + 1.0)
        k = 0.5 / r
        q[:] = [0.5 * r, (R[2, 1] - R[1, 2]) * k, (R[0, 2] - R[2, 0]) * k, (R[1, 0] - R[0, 1]) * k]
        return q
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    r = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    kk = 0.5 / r
    q[1 + i] = 0.5 * r
    q[0] = (R[k, j] - R[j, k]) * kk
    q[1 + j] = (R[j, i] + R[i, j]) * kk
    q[1 + k] = (R[k, i] + R[i, k]) * kk
    return q


def _qrot(q, v):
    u = q[1:]
    uv = 2.0 * np.cross(u, v)
    return v + q[0] * uv + np.cross(u, uv)


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def _qmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def interpolate_transform(pre, nxt, ratio):
    q = _quat_of(pre[:3, :3])
    qi = q * np.array([1, -1, -1, -1.0])
    t, tn = pre[:3, 3], nxt[:3, 3]
    dt = -_qrot(qi, t) + _qrot(qi, tn)
    dq = _qmul(qi, _quat_of(nxt[:3, :3]))
    n = math.sqrt(dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3])
    angle, axis = 0.0, np.array([1.0, 0, 0])
    if n != 0.0:  # Eigen::AngleAxisd(q)
        angle = 2.0 * math.atan2(n, abs(dq[0]))
        axis = dq[1:] / (-n if dq[0] < 0 else n)
    lt, lr = ratio * dt, ratio * (angle * axis)
    norm = math.sqrt(lr[0] * lr[0] + lr[1] * lr[1] + lr[2] * lr[2])
    tq = np.array([1.0, 0, 0, 0])
    if not norm < 1e-8:
        tq = np.concatenate([[math.cos(0.5 * norm)], math.sin(0.5 * norm) * (lr / norm)])
    out = np.eye(4)
    out[:3, :3] = _qmat(_qmul(q, tq))
    out[:3, 3] = t + _qrot(q, lt)
    return out


def fix(stamp_us=0, latitude=0.0, longitude=0.0, altitude=0.0, heading=0.0, pitch=0.0, roll=0.0, precision=100.0, dimension=2):
    return dict(stamp_us=int(stamp_us), latitude=float(latitude), longitude=float(longitude), altitude=float(altitude), heading=float(heading),
                pitch=float(pitch), roll=float(roll), precision=float(precision), dimension=int(dimension))


def _rtk_pose(proj, f, x, y, z):
    heading = f["heading"] - grid_convergence(proj.longitude0(), f["latitude"], f["longitude"])
    return transform_from_rpyt(x, y, z, -heading, f["pitch"], f["roll"])


def rtk_transform_utm(proj, f, zero_utm):
    x, y = proj.forward(f["latitude"], f["longitude"])
    return _rtk_pose(proj, f, x - zero_utm[0], y - zero_utm[1], f["altitude"] - zero_utm[2])


def rtk_transform_origin(proj, origin, f):
    ox, oy = proj.forward(origin["latitude"], origin["longitude"])
    x, y = proj.forward(f["latitude"], f["longitude"])
    return _rtk_pose(proj, f, x - ox, y - oy, f["altitude"] - origin["altitude"])


class TrackRef:
    def __init__(self):
        self.proj = UtmRef()
        self.origin = None
        self.data = {}

    def set_origin(self, f):
        if self.origin is not None:
            return False, None
        self.origin = dict(f)
        self.proj.forward(f["latitude"], f["longitude"])
        return True, rtk_transform_origin(self.proj, self.origin, f)

    def feed(self, f, valid=True):
        if not (valid and self.origin is not None):
            return False
        self.data[f["stamp_us"]] = (dict(f), rtk_transform_origin(self.proj, self.origin, f))
        return True

    def interpolate(self, stamp):
        if self.origin is None:
            return NO_ORIGIN, None
        if stamp in self.data:
            return EXACT, self.data[stamp][1]
        keys = sorted(self.data)
        if len(keys) <= 1:
            return TOO_FEW, None
        if stamp < keys[0]:
            return EARLY, None
        if stamp > keys[-1]:
            return LATE, None
        i = bisect.bisect_right(keys, stamp) - 1  # the last fix at or before the stamp; the next one follows it
        pre, nxt = keys[i], keys[i + 1]
        ratio = float(stamp - pre) / float(nxt - pre)
        return INTERPOLATED, interpolate_transform(self.data[pre][1], self.data[nxt][1], ratio)


class GnssQueueRef:
    def __init__(self):
        self.proj = UtmRef()
        self.zero_utm = None
        self.queue = []
        self.last_xyz = np.zeros(3)

    def set_origin(self, f, last_keyframe_z=None):
        alt = f["altitude"] - last_keyframe_z if last_keyframe_z is not None else f["altitude"]
        e, n = self.proj.forward(f["latitude"], f["longitude"])
        self.zero_utm = np.array([e, n, alt])
        return self.zero_utm.copy()

    def push(self, f):
        self.queue.append(dict(f))

    def stamps(self):
        return np.array([f["stamp_us"] for f in self.queue], np.uint64)

    def flush(self, kf_stamps, kf_has_fix):
        """the reference's flush_gps_queue; kf_has_fix (list / array of 0 / 1) is updated in place"""
        out = []
        gq = self.queue
        if len(kf_stamps) == 0 or not gq:
            return out
        cursor = 0
        for k, stamp in enumerate(int(s) for s in kf_stamps):
            if stamp > gq[-1]["stamp_us"]:
                break
            if stamp < gq[cursor]["stamp_us"] or kf_has_fix[k]:
                continue
            first = second = cursor
            while second != len(gq):
                dt = (float(gq[first]["stamp_us"]) - float(stamp)) / 1000000.0
                dt2 = (float(gq[second]["stamp_us"]) - float(stamp)) / 1000000.0
                if dt <= 0 and dt2 >= 0 and (dt2 - dt) < 2.0:
                    break
                first = second
                second += 1
            if second == len(gq):
                break
            cursor = first
            pre, nxt = gq[first], gq[second]
            if pre["precision"] != nxt["precision"]:
                continue
            ratio = float(stamp - pre["stamp_us"]) / float(nxt["stamp_us"] - pre["stamp_us"] + 1)
            T = interpolate_transform(rtk_transform_utm(self.proj, pre, self.zero_utm), rtk_transform_utm(self.proj, nxt, self.zero_utm), ratio)
            xyz = T[:3, 3].copy()
            if pre["dimension"] == 2:
                xyz[2] = 0.0
            p = pre["precision"]
            threshold = 10.0 if p < 100.0 else (20.0 if p < 1000.0 else 50.0)
            if np.linalg.norm(self.last_xyz) > 0 and np.linalg.norm(self.last_xyz - xyz) < threshold:
                continue
            kf_has_fix[k] = 1
            self.last_xyz = xyz.copy()
            q = _quat_of(T[:3, :3])
            q = q / np.linalg.norm(q)
            out.append(dict(keyframe=k, dimension=pre["dimension"], first=pre["stamp_us"], second=nxt["stamp_us"], xyz=xyz,
                            quat=np.array([q[1], q[2], q[3], q[0]]), precision=p))
        last = int(kf_stamps[-1])
        keep_from = bisect.bisect_right([f["stamp_us"] for f in gq], last)
        del gq[:keep_from]
        return out


def gnss_information(m):
    """the information matrices flush_gps_queue hands to the graph for a match (hdl_graph_slam_nodelet.cpp:421-441): (xyz 3 x 3, rotation 3 x 3 or None)"""
    info = np.eye(3) / m["precision"]
    if m["dimension"] == 2:
        info[2, 2] = 1.0 / (np.linalg.norm(m["xyz"]) * np.linalg.norm(m["xyz"]))
    rot = np.eye(3) / (m["precision"] * 10.0) if m["dimension"] == 6 else None
    return info, rot


# ---- several lidars into one frame -------------------------------------------------------------------------------------------------------------
def transform_f64(points, T):
    """pcl::transformPointCloud with a Matrix4d: f64, terms left to right, one cast to f32"""
    p = np.asarray(points, np.float32)
    x, y, z = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64), p[:, 2].astype(np.float64)
    out = p.copy()
    for r in range(3):
        out[:, r] = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32)
    return out


def merge_points(clouds, stamps, headers, scan_period_us, T=None, transform=True):
    """mergePoints (slam_utils.cpp:249-273) then preprocessPoints: (points, stamps, kept, early, late); cloud 0 is the base"""
    pts, sts = [np.asarray(clouds[0], np.float32).reshape(-1, 4)], [np.asarray(stamps[0], np.uint32)]
    L = len(clouds)
    kept, early, late = np.zeros(L, np.uint32), np.zeros(L, np.uint32), np.zeros(L, np.uint32)
    kept[0] = len(pts[0])
    for l in range(1, L):
        shift = float(int(headers[l])) - float(int(headers[0]))
        s = np.asarray(stamps[l], np.uint32).astype(np.float64) + shift
        with np.errstate(invalid="ignore"):
            k = (s >= 0) & (s <= float(int(scan_period_us)))
        pts.append(np.asarray(clouds[l], np.float32).reshape(-1, 4)[k])
        sts.append(s[k].astype(np.uint32))
        kept[l], early[l], late[l] = k.sum(), (s < 0).sum(), (s > float(int(scan_period_us))).sum()
    p, s = np.concatenate(pts), np.concatenate(sts)
    if transform:
        with np.errstate(invalid="ignore", over="ignore"):
            p = transform_f64(p, np.eye(4) if T is None else np.asarray(T, np.float64).reshape(4, 4))
    return p, s, kept, early, late


PERIOD_US = 100000
BIG_T = transform_from_rpyt(1e5, -2e5, 33.25, 37.0, 1.5, -2.0)  # a translation of 1e5 m: a contracted multiply-add would show in the last bit


def _cloud(rng, n, lo, hi):
    p = np.empty((n, 4), np.float32)
    p[:, :3] = rng.uniform(-80, 80, (n, 3))
    p[:, 3] = rng.uniform(0, 255, n)
    return p, rng.integers(lo, hi + 1, n).astype(np.uint32) if n else np.zeros(0, np.uint32)


def merge_case(name, small=False):
    """the five cases of the kernel test (tiles / edges / L = 1 / L = 16 / non-finite): dict(clouds, stamps, headers, period, T).  `small`: the same
    structure at the sizes the golden was recorded with"""
    rng = np.random.default_rng({"tiles": 11, "edges": 12, "single": 13, "sixteen": 14, "nonfinite": 15}[name])
    H = (1 << 40) + 123456  # header stamps above 2^32
    sz = (lambda n: max(n // 64, 3)) if small else (lambda n: n)
    if name == "tiles":  # sizes around the tile of 2048, an empty cloud in the middle, one wholly rejected, one wholly kept, both signs of shift
        spec = [(300, 0, None), (2047, +30000, None), (2048, -30000, None), (0, +5, None), (2049, +200000, "rejected"), (4097, 0, "kept"), (1500, -99999, None)]
        clouds, stamps, headers = [], [], []
        for n, shift, kind in spec:
            n = sz(n) if n else 0
            p, s = _cloud(rng, n, 0, PERIOD_US)
            clouds.append(p), stamps.append(s), headers.append(H + shift)
        return dict(clouds=clouds, stamps=stamps, headers=headers, period=PERIOD_US, T=BIG_T)
    if name == "edges":  # stamps landing exactly on 0 and on the period (kept), on -1 and period + 1 (dropped)
        base = _cloud(rng, sz(300), 0, PERIOD_US)
        n = sz(2100)
        p, s = _cloud(rng, n, 5000, PERIOD_US - 5000)
        s[0::7] = 5000            # + shift -5000 -> 0: kept
        s[1::7] = 4999            # -> -1: dropped
        q, t = _cloud(rng, n, 0, PERIOD_US - 7000)
        t[0::5] = PERIOD_US - 7000  # + shift 7000 -> period: kept
        t[1::5] = PERIOD_US - 6999  # -> period + 1: dropped
        return dict(clouds=[base[0], p, q], stamps=[base[1], s, t], headers=[H, H - 5000, H + 7000], period=PERIOD_US, T=BIG_T)
    if name == "single":  # L = 1: the transform alone, stamps past the period stay (the base is ungated)
        p, s = _cloud(rng, sz(2500), 0, 3 * PERIOD_US)
        return dict(clouds=[p], stamps=[s], headers=[H], period=PERIOD_US, T=BIG_T)
    if name == "sixteen":
        clouds, stamps, headers = [], [], []
        for l in range(16):
            p, s = _cloud(rng, sz(137 + 97 * l), 0, PERIOD_US)
            clouds.append(p), stamps.append(s), headers.append(H + (l - 8) * 9000)
        return dict(clouds=clouds, stamps=stamps, headers=headers, period=PERIOD_US, T=BIG_T)
    if name == "nonfinite":  # NaN and inf points pass through like any other
        base = _cloud(rng, sz(300), 0, PERIOD_US)
        p, s = _cloud(rng, sz(2200), 0, PERIOD_US)
        p[3::11, 0] = np.nan
        p[5::13, 1] = np.inf
        p[7::17, 2] = -np.inf
        p[2::19, 3] = np.nan
        base[0][1::23, 2] = np.nan
        return dict(clouds=[base[0], p], stamps=[base[1], s], headers=[H, H + 20000], period=PERIOD_US, T=transform_from_rpyt(1.0, 2.0, 0.5, 10.0, 1.0, 2.0))
    raise KeyError(name)


MERGE_CASES = ("tiles", "edges", "single", "sixteen", "nonfinite")


# ---- seeded tracks and queues ------------------------------------------------------------------------------------------------------------------
def seeded_fixes(seed, n=None, lat0=None, lon0=None, t0=1_700_000_000_000_000, step_us=50000, jitter=True):
    """a drive of n fixes: about 1 m per fix along a slowly turning heading, stamps step_us apart (jittered)"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(3, 40)) if n is None else n
    lat = float(rng.uniform(-60, 60)) if lat0 is None else lat0
    lon = float(rng.uniform(0.5, 170)) if lon0 is None else lon0
    heading = float(rng.uniform(0, 360))
    out, t = [], t0
    for _ in range(n):
        out.append(fix(t, lat, lon, float(rng.uniform(-5, 60)), heading % 360.0, float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3))))
        heading += float(rng.uniform(-4, 4))
        lat += 1.0 * math.cos(math.radians(heading)) / 111320.0
        lon += 1.0 * math.sin(math.radians(heading)) / (111320.0 * max(math.cos(math.radians(lat)), 0.2))
        t += step_us + (int(rng.integers(-2000, 2001)) if jitter else 0)
    return out


def seeded_queue(seed):
    """fixes and key-frame stamps for one flush scenario: (origin, fixes, kf_stamps, kf_has_fix, last_keyframe_z)"""
    rng = np.random.default_rng(1000 + seed)
    step = int(rng.choice([50000, 500000, 1000000, 2100000]))
    fixes = seeded_fixes(seed, n=int(rng.integers(2, 30)), step_us=step)
    precisions = [0.05, 0.05, 0.05, 150.0, 2000.0]
    cur = float(rng.choice(precisions))
    dim = int(rng.choice([2, 3, 6]))
    for f in fixes:
        if rng.random() < 0.15:
            cur = float(rng.choice(precisions))
        f["precision"], f["dimension"] = cur, dim
        if rng.random() < 0.1:  # (a drive that jumps: the gate has something to refuse and something to pass)
            f["latitude"] += float(rng.uniform(-3e-4, 3e-4))
    t_lo, t_hi = fixes[0]["stamp_us"] - 2 * step, fixes[-1]["stamp_us"] + 2 * step
    n_kf = int(rng.integers(1, 12))
    kf = np.sort(rng.integers(t_lo, t_hi, n_kf)).astype(np.uint64)
    if rng.random() < 0.3 and n_kf > 1:
        kf[int(rng.integers(0, n_kf))] = fixes[int(rng.integers(0, len(fixes)))]["stamp_us"]  # a key frame exactly on a fix
        kf = np.sort(kf)
    has = (rng.random(n_kf) < 0.15).astype(np.uint8)
    z = float(rng.uniform(-2, 2)) if rng.random() < 0.5 else None
    return fixes[0], fixes, kf, has, z


# ---- the projection set of tests/golden/rtk.npz -------------------------------------------------------------------------------------------------
def projection_cases():
    """(lat, lon) of the golden: latitudes -60 .. 60 with 0, longitudes in three zones (one west of Greenwich), on a central meridian and
    within 1e-9 degrees of both sides of a zone edge.  The pinned projector's first call is at (lat, lon + PIN_OFFSET)."""
    lats = np.array([-60.0, -45.5, -31.25, -12.0, -1e-7, 0.0, 0.3, 17.75, 31.0, 44.44, 60.0])
    lons = []
    for lo in (120.0, 6.0, -78.0):  # zones 20, 1 and -13
        lons += [lo + 1e-9, lo + 0.37, lo + 1.9, lo + 3.0, lo + 3.0 + 1e-6, lo + 4.6, lo + 5.93, lo + 6.0 - 1e-9]
    lons += [120.0 - 1e-9, 126.0 + 1e-9, 6.0 - 1e-9, -72.0 + 1e-9, 0.25, 179.5, -179.5, 121.473]
    la, lo = np.meshgrid(lats, np.array(lons), indexing="ij")
    rng = np.random.default_rng(2024)
    extra = np.stack([rng.uniform(-60, 60, 48), np.concatenate([rng.uniform(120, 126, 16), rng.uniform(6, 12, 16), rng.uniform(-78, -72, 16)])], axis=1)
    return np.concatenate([la.reshape(-1), extra[:, 0]]), np.concatenate([lo.reshape(-1), extra[:, 1]])


PIN_OFFSET = 2.5
