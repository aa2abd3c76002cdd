"""The lidar ground calibration restated on the CPU (a test helper, not a test; it calls nothing under test): the rules of include/lio_hip.h's
lio_calib_ground_* in numpy -- the crossing-number crop in f64, the draws in Python integer arithmetic, the colinearity test, the plane and the
point-plane test in numpy float32 (every operation its own rounding), fit_plane's sequential loop -- and, for the bench tool, the same rules
once more as scalar Python loops over every point (`crop_loop`, `fit_loop`: the shape of the reference's own code)."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calib_ground.npz")
FIT_CASES = ("base", "early", "skipped", "ties")
SIGMA, NUM_ITERATION, THRESH = 0.05, 100, 0.9  # what align_points_to_xyplane passes
ATTEMPTS_PER_ITERATION = 11                   # the attempt cap: 11 * num_iteration
F32 = np.float32


def golden():
    return np.load(GOLDEN)


# ---- crop ----
def crop_mask(points, polygon):
    """bool per point: an odd number of edges with down.y < y < up.y and xi > x, everything f64"""
    P = np.asarray(points, np.float32)
    poly = np.asarray(polygon, np.float64)
    x, y = P[:, 0].astype(np.float64), P[:, 1].astype(np.float64)
    cn = np.zeros(len(P), np.int64)
    m = len(poly)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for e in range(m):
            p, q = poly[e], poly[(e + 1) % m]
            up, down = (p, q) if p[1] > q[1] else (q, p)
            hit = (down[1] < y) & (y < up[1])
            xi = down[0] + ((up[0] - down[0]) * (y - down[1])) / (up[1] - down[1])
            cn += hit & (xi > x)
    return (cn & 1).astype(bool)


# ---- draws ----
def _mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def draw(seed, j, n):
    """lio_ground_draw's rule (include/lio_hip.h): three distinct indices below n >= 3"""
    s = _mix32(seed ^ 0x9E3779B9)
    r0, r1, r2 = _mix32(s + 3 * j), _mix32(s + 3 * j + 1), _mix32(s + 3 * j + 2)
    i0 = (r0 * n) >> 32
    i1 = (r1 * (n - 1)) >> 32
    if i1 >= i0:
        i1 += 1
    i2 = (r2 * (n - 2)) >> 32
    lo, hi = min(i0, i1), max(i0, i1)
    if i2 >= lo:
        i2 += 1
    if i2 >= hi:
        i2 += 1
    return i0, i1, i2


# ---- planes and counts ----
def planes(P, triples):
    """(planes m x 4 f32, NaN where colinear; colinear m bool) of the triples into the n x 3 f32 points"""
    P = np.asarray(P, np.float32)[:, :3]
    t = np.asarray(triples, np.int64).reshape(-1, 3)
    p1, p2, p3 = P[t[:, 0]], P[t[:, 1]], P[t[:, 2]]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u, v = p2 - p1, p3 - p1
        a = u[:, 1] * v[:, 2] - v[:, 1] * u[:, 2]
        b = u[:, 2] * v[:, 0] - v[:, 2] * u[:, 0]
        c = u[:, 0] * v[:, 1] - v[:, 0] * u[:, 1]
        col = (np.abs(a) + np.abs(b)) + np.abs(c) < F32(1e-5)
        norm = np.sqrt((a * a + b * b) + c * c)
        d = -((a * p1[:, 0] + b * p1[:, 1]) + c * p1[:, 2])
        pl = np.stack([a / norm, b / norm, c / norm, d / norm], 1)
        neg = ~(c > 0)
        pl[neg] = -pl[neg]
    assert pl.dtype == np.float32
    pl[col] = np.nan
    return pl, col


def counts(P, pl, sigma):
    """per plane: the points with |((a x + b y) + c z) + d| < (float)sigma in f32; NaN does not count"""
    P = np.asarray(P, np.float32)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    out = np.zeros(len(pl), np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for h, (a, b, c, d) in enumerate(np.asarray(pl, np.float32)):
            v = ((a * x + b * y) + c * z) + d
            out[h] = np.count_nonzero(np.abs(v) < F32(sigma))
    return out


# ---- the loop ----
class Replay:
    """fit_plane's loop fed one attempt at a time"""

    def __init__(self, n, num_iteration, thresh):
        self.n, self.num_iteration, self.thresh = n, num_iteration, thresh
        self.iterations = self.attempts = self.skipped = self.best = 0
        self.winner, self.early_exit, self.done = -1, False, False

    def feed(self, colinear, count):
        assert not self.done
        j = self.attempts
        self.attempts += 1
        if colinear:
            self.skipped += 1
        else:
            self.iterations += 1
            if float(int(count)) > self.thresh * float(self.n):
                self.winner, self.early_exit, self.done = j, True, True
                return
            if int(count) > self.best:
                self.best, self.winner = int(count), j
            if self.iterations >= self.num_iteration:
                self.done = True
        if self.attempts >= ATTEMPTS_PER_ITERATION * self.num_iteration:
            self.done = True

    def result(self):
        return dict(iterations=self.iterations, attempts=self.attempts, skipped=self.skipped, winner=self.winner, early_exit=self.early_exit)


def replay(colinear, cnts, n, num_iteration, thresh):
    """the loop over a list of attempts (flags and counts); a list that runs out ends it"""
    r = Replay(n, num_iteration, thresh)
    for col, c in zip(colinear, cnts):
        if r.done:
            break
        r.feed(bool(col), c)
    return r.result()


def fit(P, sigma=SIGMA, num_iteration=NUM_ITERATION, thresh=THRESH, seed=0, draws=None, chunk=64):
    """dict(found, coef f32[4], triples, colinear, counts, planes of the attempts consumed, + replay's fields)"""
    P = np.ascontiguousarray(np.asarray(P, np.float32)[:, :3])
    n = len(P)
    assert n >= 3 and num_iteration >= 1
    total = ATTEMPTS_PER_ITERATION * num_iteration
    if draws is not None:
        draws = np.asarray(draws, np.int64).reshape(-1, 3)
        total = min(total, len(draws))
    r = Replay(n, num_iteration, thresh)
    T, C, N, PL = [], [], [], []
    pos = 0
    while not r.done and pos < total:
        m = min(chunk, total - pos)
        tr = draws[pos:pos + m] if draws is not None else np.array([draw(seed, pos + t, n) for t in range(m)], np.int64)
        pl, col = planes(P, tr)
        cnt = counts(P, pl, sigma)
        for t in range(m):
            if r.done:
                break
            r.feed(col[t], cnt[t])
            T.append(tr[t]); C.append(col[t]); N.append(cnt[t]); PL.append(pl[t])
        pos += m
    out = r.result()
    out.update(found=out["winner"] >= 0, coef=PL[out["winner"]].copy() if out["winner"] >= 0 else np.zeros(4, np.float32),
               triples=np.array(T, np.uint32).reshape(-1, 3), colinear=np.array(C, bool), counts=np.array(N, np.uint32),
               planes=np.array(PL, np.float32).reshape(-1, 4))
    return out


# ---- host side ----
def rot_to_z(coef):
    """Rodrigues' rotation of the unit direction of (a, b, c) onto (0, 0, 1), f64; the identity when they are parallel"""
    a = np.asarray(coef[:3], np.float64)
    a = a / np.sqrt(a @ a)
    ax = np.array([a[1], -a[0], 0.0])  # a x (0, 0, 1)
    s, c = np.sqrt(ax @ ax), a[2]
    if s == 0.0:
        return np.eye(3)
    k = ax / s
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return c * np.eye(3) + (1 - c) * np.outer(k, k) + s * K


def euler_zxy_matrix(roll, pitch, yaw):
    """Rz(yaw) Rx(pitch) Ry(roll), degrees: the intrinsic Z-X-Y convention"""
    r, p, y = np.deg2rad([roll, pitch, yaw])
    Rz = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, math.cos(p), -math.sin(p)], [0, math.sin(p), math.cos(p)]])
    Ry = np.array([[math.cos(r), 0, math.sin(r)], [0, 1, 0], [-math.sin(r), 0, math.cos(r)]])
    return Rz @ Rx @ Ry


# ---- the same rules as scalar loops over every point (the bench tool's stand-in for the reference's loop; not used by the tests' checks) ----
def crop_loop(points, polygon):
    poly = [(float(v[0]), float(v[1])) for v in np.asarray(polygon, np.float64)]
    kept = []
    for i in range(len(points)):
        x, y = float(points[i][0]), float(points[i][1])
        cn = 0
        for e in range(len(poly)):
            p, q = poly[e], poly[e + 1 if e + 1 < len(poly) else 0]
            up, down = (p, q) if p[1] > q[1] else (q, p)
            if down[1] < y < up[1]:
                if down[0] + ((up[0] - down[0]) * (y - down[1])) / (up[1] - down[1]) > x:
                    cn += 1
        if cn & 1:
            kept.append(i)
    return kept


def fit_loop(P, sigma, num_iteration, thresh, seed):
    """fit_plane with the seeded draws, one numpy-f32 scalar operation at a time: (coef, winner)"""
    P = np.asarray(P, np.float32)
    n, sig = len(P), F32(sigma)
    best, coef, winner, it, j = 0, np.zeros(4, np.float32), -1, 0, 0
    while it < num_iteration and j < ATTEMPTS_PER_ITERATION * num_iteration:
        tr = draw(seed, j, n)
        j += 1
        pl, col = planes(P, [tr])
        if col[0]:
            continue
        it += 1
        a, b, c, d = pl[0]
        cnt = 0
        for p in P:
            x, y, z = p
            if abs(((a * x + b * y) + c * z) + d) < sig:
                cnt += 1
        if cnt > thresh * n:
            return pl[0], j - 1
        if cnt > best:
            best, coef, winner = cnt, pl[0], j - 1
    return coef, winner
