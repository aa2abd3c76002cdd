"""References and seeded cases for the motion-compensation kernels (csrc/undistort.hip).  Nothing here calls the library under test.

The IMU backward propagation (ImuProcess::UndistortPcl, IMU_Processing.hpp:371-404) has three references here:

  flow(case, oracle)   the walk of oracle/lio_oracle.cpp::undistort_pcl restated on explicit poses: the filters (point_filter_num, the f32
                       blind radius), t = f64(f32(stamp) / 1000f) / 1000.0, the last head with off < t, the earliest kept point (lowest
                       index among equal t_ms) compensated again by every earlier head with off < t, each pass on the f32 result of the one
                       before.  Every point goes through the oracle's own undistort_point (orc_undistort_point, the function
                       oracle.undistort_point wraps; called with cached argument pointers because there are tens of thousands of points).
                       Bit-level reference wherever no sine or cosine is taken.
  restate64(...)       undistort_point in numpy float64, operation for operation in Eigen's order, BEFORE the cast to f32 (sin / cos are
                       math.sin / math.cos, the host libm the oracle calls).  Checked against the oracle after the cast, bit for bit
                       (tests/test_undistort_cpu.py).
  exact(...)           the same per-point formula in numpy.longdouble (64-bit mantissa), closed-form Rodrigues matrix and quaternion
                       rotations, no attempt at evaluation order: the unrounded value of every coordinate.

Error budget E of a case = max |restate64 - exact| over the case's single-pass points: what a dozen f64 roundings and the host libm
cost the ORACLE.  The device is held to |device - exact| <= ulp_f32(exact) / 2 + 8 E (tests/test_undistort_gpu.py).  E as measured
here (metres; x86-64 glibc; a case's E depends on its seed alone):

    still                      3.84e-14
    still-above                3.71e-14
    rotating                   3.88e-14
    repeat-head0               3.85e-14
    repeat-middle              3.62e-14
    repeat-last                4.11e-14
    repeat-zero                3.41e-14
    repeat-tie3                4.06e-14
    repeat-blind               3.19e-14
    repeat-decimated           4.24e-14
    repeat-tail_wg             4.08e-14
    repeat-index0              3.81e-14
    sizes-n1-p5                0.00e+00
    sizes-n255-p5              2.48e-14
    sizes-n256-p5              1.90e-14
    sizes-n257-p5              2.46e-14
    sizes-n700-p2              3.21e-14
    sizes-n700-p3              2.63e-14
    sizes-n700-p127            3.51e-14
    sizes-n700-p128            2.56e-14
    sizes-n900-p6-onoffset     2.68e-14
    sizes-n900-p6-beyond       2.96e-14
    sizes-n300-p2-onoffset     2.20e-14

(sizes-n1-p5: its one point is the repeated one, no single-pass point.  test_undistort_cpu.py prints every case's E and checks it against
this table to one unit of the figure's leading digit.)

Labels of a point: FILTERED (written as NaN), UNTOUCHED (t <= poses[0].off), STILL (|gyr| <= 1e-7: identity rotation), TAYLOR
(| |gyr| dt | < 0.5), LIBRARY (>= 0.5), REPEATED (the earliest kept point when more than one segment lies before it).
"""
import ctypes as C
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "undistort_cases needs an x87-style long double (64-bit mantissa) for its high-precision reference"

F32, F64, U32 = np.float32, np.float64, np.uint32
FILTERED, UNTOUCHED, STILL, TAYLOR, LIBRARY, REPEATED = range(6)
LABELS = ("filtered", "untouched", "still", "taylor", "library", "repeated")
POSE_WORDS = 22  # off, acc[3], gyr[3], vel[3], pos[3], R[9]: ImuPoseDev
NAN_BITS = 0x7FC00000


# ---------------------------------------------------------------------------------------------------------------- small helpers
def rand_quat(rng, max_angle=None):
    if max_angle is None:
        q = rng.normal(size=4)
    else:
        ax = rng.normal(size=3)
        a = rng.uniform(0.2, 1.0) * max_angle
        q = np.r_[np.sin(a / 2) * ax / np.linalg.norm(ax), np.cos(a / 2)]
    return q / np.linalg.norm(q)


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rand_dir(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def cloud(rng, n, r_min=5.0, r_max=80.0):
    """n points r_min..r_max metres from the sensor, random intensities"""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = np.empty((n, 4), F32)
    p[:, :3] = (d * rng.uniform(r_min, r_max, (n, 1))).astype(F32)
    p[:, 3] = rng.uniform(0, 255, n).astype(F32)
    return p


def point_time(stamp_us):
    """(t_ms f32, t f64) of a stamp: added_pt.curvature = stamp / 1000.0f, then curvature / double(1000)"""
    t_ms = np.asarray(stamp_us, U32).astype(F32) / F32(1000.0)
    return t_ms, t_ms.astype(F64) / 1000.0


def ulp_f32(x):
    """spacing of f32 at |x| (x: any float array), the subnormal spacing below the smallest normal"""
    a = np.abs(np.asarray(x, F64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    e = np.where(2.0 ** e > a, e - 1, e)  # log2 rounding just below a power of two
    e = np.where(2.0 ** (e + 1) <= a, e + 1, e)
    return 2.0 ** (np.maximum(e, -126) - 23)


def make_poses(rng, offs, gyrs, accs=None):
    """pose rows for the offsets `offs` (poses[0] first); gyrs[k] / accs[k] are the TAIL values of segment k = rows k+1"""
    m = len(offs)
    P = np.zeros((m, POSE_WORDS))
    P[:, 0] = offs
    for k in range(m):
        P[k, 1:4] = rng.uniform(-12, 12, 3) if accs is None or k == 0 else accs[k - 1]
        P[k, 4:7] = rng.uniform(-1, 1, 3) if k == 0 else gyrs[k - 1]  # row 0's acc / gyr are never read
        P[k, 7:10] = rng.uniform(-8, 8, 3)
        P[k, 10:13] = rng.uniform(-6, 6, 3)
        P[k, 13:22] = quat_to_R(rand_quat(rng, 0.6)).reshape(9)
    return P


def new_case(rng, name, pts, stamp, poses, blind=0.1, filter_num=1, undistort=1):
    return dict(name=name, pts=np.ascontiguousarray(pts, F32), stamp=np.ascontiguousarray(stamp, U32), poses=np.ascontiguousarray(poses, F64),
                end_pos=rng.uniform(-6, 6, 3), end_rot=rand_quat(rng, 0.7), ril=rand_quat(rng, 0.3), til=rng.uniform(-0.3, 0.3, 3),
                blind=float(blind), filter_num=int(filter_num), undistort=int(undistort))


# ---------------------------------------------------------------------------------------------------------------- the walk
def walk(case):
    """who is kept, which segment compensates it, who is the earliest: dict(keep, t_ms, t, h, first, passes)"""
    p, n = case["pts"], len(case["pts"])
    idx = np.arange(n)
    keep = np.ones(n, bool) if case["filter_num"] <= 1 else (idx % case["filter_num"] == 0)
    r2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]  # f32, left to right
    keep &= r2.astype(F64) > case["blind"] * case["blind"]
    t_ms, t = point_time(case["stamp"])
    h = np.full(n, -1)
    first, passes = -1, 0
    if case["undistort"]:
        off = case["poses"][:-1, 0]  # heads
        for k in range(len(off)):  # the last head with off < t
            h[t > off[k]] = k
        h[~keep] = -1
        if keep.any():
            kept = idx[keep]
            first = int(kept[np.argmin(t_ms[kept])])  # argmin returns the lowest index among equals
            passes = int(1 + sum(t[first] > off[k] for k in range(h[first]))) if h[first] >= 0 else 0
    return dict(keep=keep, t_ms=t_ms, t=t, h=h, first=first, passes=passes)


def labels(case, w=None):
    w = w or walk(case)
    n = len(case["pts"])
    lab = np.full(n, FILTERED)
    lab[w["keep"]] = UNTOUCHED
    if not case["undistort"]:
        return lab
    sel = w["h"] >= 0
    g = case["poses"][w["h"][sel] + 1, 4:7]
    nrm = np.sqrt(g[:, 0] * g[:, 0] + (g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]))
    th = nrm * (w["t"][sel] - case["poses"][w["h"][sel], 0])
    lab[sel] = np.where(nrm > 0.0000001, np.where(np.abs(th) < 0.5, TAYLOR, LIBRARY), STILL)
    if w["passes"] > 1:
        lab[w["first"]] = REPEATED
    return lab


def gyr_dt(case, w=None):
    """|gyr| dt of every point as the kernel forms it (NaN where no segment applies)"""
    w = w or walk(case)
    out = np.full(len(case["pts"]), np.nan)
    sel = w["h"] >= 0
    g = case["poses"][w["h"][sel] + 1, 4:7]
    out[sel] = np.sqrt(g[:, 0] * g[:, 0] + (g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])) * (w["t"][sel] - case["poses"][w["h"][sel], 0])
    return out


# ---------------------------------------------------------------------------------------------------------------- flow reference
class _OraclePoint:
    """orc_undistort_point with the argument pointers of one case prepared once"""

    def __init__(self, oracle, case):
        self.fn = oracle.lib().orc_undistort_point
        f64p, f32p = C.POINTER(C.c_double), C.POINTER(C.c_float)
        self.keep = [np.ascontiguousarray(case[k], F64) for k in ("end_pos", "end_rot", "ril", "til")]
        self.tail = [a.ctypes.data_as(f64p) for a in self.keep]
        self.P = case["poses"]
        base = self.P.ctypes.data
        ptr = lambda row, word: C.cast(C.c_void_p(base + 8 * (row * POSE_WORDS + word)), f64p)  # noqa: E731
        # head R, head vel, head pos, tail acc, tail gyr
        self.seg = [(ptr(k, 13), ptr(k, 7), ptr(k, 10), ptr(k + 1, 1), ptr(k + 1, 4)) for k in range(len(self.P) - 1)]
        self.pin, self.pout = np.zeros(3, F32), np.zeros(3, F32)
        self.a_in, self.a_out = self.pin.ctypes.data_as(f32p), self.pout.ctypes.data_as(f32p)

    def __call__(self, k, dt, p3):
        self.pin[:] = p3
        self.fn(*self.seg[k], float(dt), self.a_in, *self.tail, self.a_out)
        return self.pout.copy()


def flow(case, oracle, w=None, rows=None):
    """the cloud as oracle/lio_oracle.cpp::undistort_pcl leaves it (dropped points NaN, as the device writes them); rows: compensate
    these points only (the other compensated points are left as uploaded)"""
    w = w or walk(case)
    out = case["pts"].copy()
    out[~w["keep"], :3] = np.array([NAN_BITS] * 3, U32).view(F32)
    if not case["undistort"]:
        return out
    call = _OraclePoint(oracle, case)
    off, t, h = case["poses"][:, 0], w["t"], w["h"]
    for i in (np.nonzero(h >= 0)[0] if rows is None else [r for r in rows if h[r] >= 0]):
        out[i, :3] = call(h[i], t[i] - off[h[i]], out[i, :3])
        if i == w["first"]:
            for k in range(h[i] - 1, -1, -1):
                if t[i] > off[k]:
                    out[i, :3] = call(k, t[i] - off[k], out[i, :3])
    return out


# ---------------------------------------------------------------------------------------------------------------- f64 restatement
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _qrot(q, v):  # Eigen QuaternionBase::_transformVector
    uv = _cross(q, v)
    uv = [u + u for u in uv]
    c2 = _cross(q, uv)
    return [(v[a] + q[3] * uv[a]) + c2[a] for a in range(3)]


def _gather(case, sel, w):
    """per-point operands of the points `sel` (index array): head / tail rows, dt, the f32 point"""
    h = w["h"][sel]
    head, tail = case["poses"][h], case["poses"][h + 1]
    return head, tail, w["t"][sel] - head[:, 0], case["pts"][sel, :3]


def restate64(case, sel, w=None, p3=None):
    """undistort_point of oracle/lio_oracle.cpp in float64, one IEEE operation per numpy operation, before the cast to f32: (len(sel), 3)"""
    w = w or walk(case)
    head, tail, dt, p = _gather(case, sel, w)
    if p3 is not None:
        p = p3
    k = len(dt)
    w0, w1, w2 = tail[:, 4], tail[:, 5], tail[:, 6]
    n = np.sqrt(w0 * w0 + (w1 * w1 + w2 * w2))
    rot = n > 0.0000001
    ns = np.where(rot, n, 1.0)
    ax, ay, az = w0 / ns, w1 / ns, w2 / ns
    z = np.zeros(k)
    K = [[z, -az, ay], [az, z, -ax], [-ay, ax, z]]
    th = n * dt
    sn = np.array([math.sin(v) for v in th])  # the host libm, as std::sin in the oracle (numpy's own sin may be a SIMD variant)
    cs = 1.0 - np.array([math.cos(v) for v in th])
    eye = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    Rd = [[None] * 3 for _ in range(3)]
    for i in range(3):
        sK = [cs * K[i][c] for c in range(3)]
        for j in range(3):
            kk = sK[0] * K[0][j] + (sK[1] * K[1][j] + sK[2] * K[2][j])
            Rd[i][j] = np.where(rot, (eye[i][j] + sn * K[i][j]) + kk, eye[i][j])
    R = head[:, 13:22].reshape(k, 3, 3)
    Ri = [[R[:, i, 0] * Rd[0][j] + (R[:, i, 1] * Rd[1][j] + R[:, i, 2] * Rd[2][j]) for j in range(3)] for i in range(3)]
    Pi = [p[:, a].astype(F64) for a in range(3)]
    epos, til = case["end_pos"], case["til"]
    T = [head[:, 10 + a] + head[:, 7 + a] * dt + 0.5 * tail[:, 1 + a] * dt * dt - epos[a] for a in range(3)]
    ril, er = case["ril"], case["end_rot"]
    pl = _qrot(ril, Pi)
    pl = [pl[a] + til[a] for a in range(3)]
    pw = [(Ri[a][0] * pl[0] + (Ri[a][1] * pl[1] + Ri[a][2] * pl[2])) + T[a] for a in range(3)]
    pe = _qrot([-er[0], -er[1], -er[2], er[3]], pw)
    pe = [pe[a] - til[a] for a in range(3)]
    pc = _qrot([-ril[0], -ril[1], -ril[2], ril[3]], pe)
    return np.stack(pc, axis=1)


# ---------------------------------------------------------------------------------------------------------------- long double
def exact(case, sel, w=None):
    """the unrounded value of the same formula, numpy.longdouble: (len(sel), 3).  The identity-rotation rule (|gyr| <= 1e-7 as the f64
    norm says) is part of the formula and is kept."""
    w = w or walk(case)
    head, tail, dt, p = _gather(case, sel, w)
    k = len(dt)
    head, tail, dt, p = head.astype(LD), tail.astype(LD), dt.astype(LD), p.astype(LD)
    g64 = case["poses"][w["h"][sel] + 1, 4:7]
    rot = np.sqrt(g64[:, 0] * g64[:, 0] + (g64[:, 1] * g64[:, 1] + g64[:, 2] * g64[:, 2])) > 0.0000001
    g = tail[:, 4:7]
    n = np.sqrt((g * g).sum(1))
    a = g / np.where(rot, n, LD(1))[:, None]
    K = np.zeros((k, 3, 3), LD)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
    th = n * dt
    sh = np.sin(th / 2)
    Rd = np.eye(3, dtype=LD)[None] + np.sin(th)[:, None, None] * K + (2 * sh * sh)[:, None, None] * np.einsum("kij,kjl->kil", K, K)
    Rd[~rot] = np.eye(3, dtype=LD)
    Ri = np.einsum("kij,kjl->kil", head[:, 13:22].reshape(k, 3, 3), Rd)

    def qrot(q, v):
        qv = np.broadcast_to(np.asarray(q[:3], LD), v.shape)
        uv = 2 * np.cross(qv, v)
        return v + LD(q[3]) * uv + np.cross(qv, uv)

    ril, er = np.asarray(case["ril"], LD), np.asarray(case["end_rot"], LD)
    conj = np.array([-1, -1, -1, 1], LD)
    T = head[:, 10:13] + head[:, 7:10] * dt[:, None] + LD(0.5) * tail[:, 1:4] * (dt * dt)[:, None] - np.asarray(case["end_pos"], LD)
    pl = qrot(ril, p) + np.asarray(case["til"], LD)
    pw = np.einsum("kij,kj->ki", Ri, pl) + T
    pe = qrot(er * conj, pw) - np.asarray(case["til"], LD)
    return qrot(ril * conj, pe)


def single_pass(case, w=None):
    """indices of the points that are compensated exactly once"""
    w = w or walk(case)
    sel = w["h"] >= 0
    if w["passes"] > 1:
        sel = sel.copy()
        sel[w["first"]] = False
    return np.nonzero(sel)[0]


def error_budget(case, w=None):
    """E: the oracle's own f64 distance from the unrounded value, over the single-pass points"""
    w = w or walk(case)
    sel = single_pass(case, w)
    if len(sel) == 0:
        return 0.0
    return float(np.abs(restate64(case, sel, w).astype(LD) - exact(case, sel, w)).max())


# ---------------------------------------------------------------------------------------------------------------- IMU cases
def _uniform_offsets(m, seg=0.01):
    return np.arange(m) * seg


def case_still(rng_seed=101, n=20000, above=False):
    """no sine taken: every tail's |gyr| is 0, exactly 1e-7, or a normal value below it (above=True: nextafter(1e-7, 1), which does rotate)"""
    rng = np.random.default_rng(rng_seed)
    m = 13
    offs = _uniform_offsets(m, 0.05)  # long segments: a rotation taken or left out by mistake moves a point by up to 8e-7 m
    gyrs = []
    for k in range(m - 1):
        mag = (0.0, 1e-7, 10.0 ** -int(rng.integers(8, 150)))[k % 3]
        if above:  # (after the draw: both variants get the same cloud, stamps and poses otherwise)
            mag = np.nextafter(1e-7, 1.0)
        g = np.zeros(3)
        g[k % 3] = mag if k % 2 else -mag  # one axis: the norm is |mag| exactly
        gyrs.append(g)
    stamp = rng.integers(0, int(offs[-1] * 1e6) + 3000, n).astype(U32)
    stamp[7] = 0
    pts = cloud(rng, n)
    pts[11, :3] = [0.01, 0.02, -0.03]  # inside the blind radius
    return new_case(rng, "still-above" if above else "still", pts, stamp, make_poses(rng, offs, gyrs))


def case_rotating(rng_seed=202, n=20000):
    """|gyr| of 0.3, 2 and 4-8 rad/s over segments whose lengths let |gyr| dt cover [0, 0.7]; |gyr| dt = 0.5 exactly and within 1e-6 on
    either side of it.  Returns the case; case["boundary"] = the indices of the three boundary groups (below, exact, above)."""
    rng = np.random.default_rng(rng_seed)
    mags = [2.0, 0.3, 2.0, 4.0, 5.0, 6.0, 7.0, 8.0, 6.5, 7.5, 8.0, None, None, 0.3]
    lens = [0.30, 0.10, 0.30] + [0.7 / g for g in mags[3:11]] + [0.1, 0.1, 0.1]
    offs = np.concatenate([[0.0], np.cumsum(lens)])
    gyrs = [np.array([0.0, 2.0, 0.0])] + [None if g is None else g * rand_dir(rng) for g in mags[1:]]
    # the stamps are spread so that every segment gets the same share whatever its length
    seg_of = rng.integers(0, len(lens), n)
    frac = rng.uniform(0, 1, n)
    stamp = np.clip(((offs[seg_of] + frac * np.asarray(lens)[seg_of]) * 1e6).astype(np.int64), 1, None).astype(U32)
    bnd = {}
    for name, k, side in (("below", 11, -5e-7), ("above", 12, +5e-7)):
        s_us = int((offs[k] + 0.08) * 1e6)
        dt = float(point_time([s_us])[1][0]) - offs[k]
        gyrs[k] = ((0.5 + side) / dt) * rand_dir(rng)
        bnd[name] = np.arange(40) + (100 if name == "below" else 200)
        stamp[bnd[name]] = s_us
    bnd["exact"] = np.arange(40) + 300
    stamp[bnd["exact"]] = 250000  # t = 0.25 exactly, |gyr| = 2 exactly: |gyr| dt == 0.5, the library side
    stamp[5] = 0  # the earliest point is untouched: nothing is repeated in this case
    pts = cloud(rng, n)
    c = new_case(rng, "rotating", pts, stamp, make_poses(rng, offs, gyrs))
    c["boundary"] = bnd
    return c


def case_repeat(variant, rng_seed=303):
    """the earliest kept point and who it is.  Variants: head0 (earliest stamp > 0 in segment 0: nothing repeated), middle, last (every
    earlier segment repeats), zero (earliest stamp 0: untouched), tie3 (three points share the earliest stamp), blind / decimated (the
    earliest raw point is dropped, the next kept one is repeated), tail_wg (index n - 1 of n = 16385 + 200: the last, partial workgroup
    of 65), index0"""
    names = ["head0", "middle", "last", "zero", "tie3", "blind", "decimated", "tail_wg", "index0"]
    rng = np.random.default_rng(rng_seed + names.index(variant))
    m = 9
    offs = _uniform_offsets(m, 0.0125)  # 8 segments, 100 ms
    gyrs = [rng.uniform(0.2, 1.5) * rand_dir(rng) for _ in range(m - 1)]
    n = 16385 + 200 if variant == "tail_wg" else 3001
    seg_us = 12500
    lo = {"head0": 3000, "middle": 4 * seg_us + 700, "last": 7 * seg_us + 900, "zero": 0, "tie3": 5 * seg_us + 11, "blind": 3 * seg_us + 40,
          "decimated": 2 * seg_us + 77, "tail_wg": 6 * seg_us + 5, "index0": 3 * seg_us + 123}[variant]
    stamp = rng.integers(lo + 50, 8 * seg_us + 2000, n).astype(U32)
    pts = cloud(rng, n)
    filter_num = 1
    at = {"tail_wg": n - 1, "index0": 0}.get(variant, 1234)
    stamp[at] = lo
    if variant == "tie3":
        stamp[[2000, 700]] = lo  # 700 is the lowest index of the three
    elif variant == "blind":
        pts[at, :3] = [0.03, -0.02, 0.01]
        stamp[2222] = lo + 9  # the next kept point
    elif variant == "decimated":
        filter_num = 3
        assert at % 3 != 0
        stamp[2222 // 3 * 3] = lo + 9
    return new_case(rng, "repeat-" + variant, pts, stamp, make_poses(rng, offs, gyrs), filter_num=filter_num)


REPEAT_VARIANTS = ("head0", "middle", "last", "zero", "tie3", "blind", "decimated", "tail_wg", "index0")
# (index of the repeated point or None, passes it takes) each variant promises
REPEAT_EXPECT = {"head0": (None, 1), "middle": (1234, 5), "last": (1234, 8), "zero": (None, 0), "tie3": (700, 6), "blind": (2222, 4),
                 "decimated": (2220, 3), "tail_wg": (16584, 7), "index0": (0, 4)}


def case_sizes(n, n_poses, rng_seed=404, beyond=False, on_offset=False):
    """n points against n_poses poses; beyond: a third of the stamps lie after the last pose; on_offset: the points 0 .. 9 (as far as there
    are any) carry a stamp whose t IS a pose offset (the offset is built from the stamp by the kernel's formula): the earlier segment's"""
    rng = np.random.default_rng(rng_seed + 1000 * n_poses + n)
    seg_us = 800
    stamps_at = (np.arange(n_poses) * seg_us).astype(U32)
    offs = point_time(stamps_at)[1].copy()  # every offset is the t of a stamp
    gyrs = [rng.uniform(0.2, 3.0) * rand_dir(rng) for _ in range(n_poses - 1)]
    hi = int(stamps_at[-1])
    stamp = rng.integers(1, hi + (hi // 2 if beyond else 0) + 2, n).astype(U32)
    if on_offset:
        k = min(n, 10)
        stamp[:k] = stamps_at[rng.integers(1, n_poses, k)] if n_poses > 2 else stamps_at[1]
    name = "sizes-n%d-p%d%s%s" % (n, n_poses, "-beyond" if beyond else "", "-onoffset" if on_offset else "")
    return new_case(rng, name, cloud(rng, n), stamp, make_poses(rng, offs, gyrs))


def case_filters(filter_num, rng_seed=505, n=1500):
    """undistort = 0: decimation and the blind radius alone.  Points 0 / 3 / 6 ... of the first 60 sit ON the radius (r2 == blind^2 in
    f32: dropped), their successors one f32 step outside (kept)."""
    rng = np.random.default_rng(rng_seed + filter_num)
    pts = cloud(rng, n, 0.05, 30.0)
    blind = 2.0  # blind^2 = 4 = f32(2 * 2 + 0 + 0)
    for j in range(20):
        a = rng.permutation(3)
        on = np.zeros(3, F32)
        on[a[0]] = F32(2.0) * (1 if j % 2 else -1)
        out = on.copy()
        out[a[0]] = np.nextafter(on[a[0]], F32(np.sign(on[a[0]]) * 4))
        inn = on.copy()
        inn[a[0]] = np.nextafter(on[a[0]], F32(0))
        pts[3 * j, :3], pts[3 * j + 1, :3], pts[3 * j + 2, :3] = on, out, inn
    c = new_case(rng, "filters-%d" % filter_num, pts, rng.integers(0, 100000, n).astype(U32), make_poses(rng, _uniform_offsets(3), [np.zeros(3)] * 2),
                 blind=blind, filter_num=filter_num, undistort=0)
    c["edge"] = dict(on=np.arange(20) * 3, outside=np.arange(20) * 3 + 1, inside=np.arange(20) * 3 + 2)
    return c


def all_imu_cases():
    """every compensating case the GPU tests use (the CPU tests walk them all)"""
    out = [case_still(), case_still(above=True), case_rotating()]
    out += [case_repeat(v) for v in REPEAT_VARIANTS]
    out += [case_sizes(n, 5) for n in (1, 255, 256, 257)]
    out += [case_sizes(700, p) for p in (2, 3, 127, 128)]
    out += [case_sizes(900, 6, on_offset=True), case_sizes(900, 6, beyond=True), case_sizes(300, 2, on_offset=True)]
    return out


# ---------------------------------------------------------------------------------------------------------------- pose-list cases
POSE_TILE = 2048
POSE_SIZES = (2047, 2048, 2049, 4097, 3 * 2048 + 5)
POSE_SIZE_STRIDED = 257 * 2048 + 3  # more than 256 tiles: the strided part of the fold over the tiles before
POSE_LAYOUTS = ("sorted", "shuffled", "late_at_0", "late_at_wave_end", "late_at_tile_end", "late_at_tile1", "past_last_early")
POSE_LAYOUTS_STRIDED = ("late_at_tile1", "late_at_tile256")  # the carried maximum is read in the first / in the second trip of the fold


def pose_list_translations(n_poses, step_us=1000, header=1_000_000):
    """identity rotations; pose i is moved by (+-2^a, +-2^b, +-2^c) with exponents in -6 .. 1, the triple distinct for every pose (and
    large enough to show in the f32 coordinates of a cloud within 60 m)"""
    ps = np.uint64(header) + np.arange(n_poses, dtype=np.uint64) * np.uint64(step_us)
    T = np.tile(np.eye(4), (n_poses, 1, 1))
    for i in range(1, n_poses):
        e = (i % 8, (i // 8) % 8, (3 * i + 1) % 8)
        T[i, :3, 3] = [(-1) ** (i + a) * 2.0 ** (e[a] - 6) for a in range(3)]
    return ps, T.reshape(n_poses, 16)


def pose_list_case(n, layout, n_poses=12, rng_seed=606, T=None):
    """stamps of n points in one of POSE_LAYOUTS over n_poses poses; header stamp and pose stamps; pose matrices (pure translations unless
    T is given).  Pure translation is 'exact on both sides' in the sense that oracle and device perform the same four f32 operations per
    coordinate (ratio, ratio * t, 0 * z + t', x + that) with no sine or cosine: any difference is a wrong segment, not rounding."""
    rng = np.random.default_rng(rng_seed + n % 9973 + 31 * (POSE_LAYOUTS + POSE_LAYOUTS_STRIDED[1:]).index(layout) + 7 * n_poses)
    step = 1000
    header = 1_000_000
    ps, Tt = pose_list_translations(n_poses, step, header)
    T = Tt if T is None else T
    last = (n_poses - 1) * step
    # the layouts with one late stamp keep the others in the first 60 % of the pose list, so that the carried interval shows everywhere
    stamp = np.sort(rng.integers(0, (last if layout in ("sorted", "shuffled") else last * 6 // 10) + 1, n)).astype(U32)
    late = U32(last - 3)  # in the last interval
    if layout == "shuffled":
        stamp = rng.permutation(stamp)
    elif layout == "late_at_0":
        stamp[0] = late
    elif layout == "late_at_wave_end":
        stamp[min(n - 1, 64 * 8 - 1)] = late  # the last point of the last lane of wave 0 (8 consecutive points per thread)
    elif layout == "late_at_tile_end":
        stamp[min(n - 1, POSE_TILE - 1)] = late
    elif layout == "late_at_tile1":
        stamp[min(n - 1, POSE_TILE)] = late
    elif layout == "late_at_tile256":
        stamp[256 * POSE_TILE + 5] = late
    elif layout == "past_last_early":
        stamp[min(n - 1, 300)] = U32(last + 17)
    pts = cloud(rng, n, 2.0, 60.0)
    return dict(name="poses-%d-%s-p%d" % (n, layout, n_poses), pts=pts, stamp=stamp, header=header, pose_stamps=ps, pose_T=T)


def pose_list_segments(case):
    """plain restatement of the walk's segment choice: seg[i] = interval used by point i, n_poses where none (the prefix maximum of need)"""
    lim = (case["pose_stamps"][1:] - np.uint64(case["header"])).astype(np.uint64)
    need = 1 + np.searchsorted(lim, case["stamp"].astype(np.uint64), side="left")  # first i with stamp <= limit[i]
    return np.maximum.accumulate(need)
