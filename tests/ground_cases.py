"""The ground detector restated on the CPU (a test helper, not a test): the stages of include/lio_hip.h's lio_ground_* in numpy -- the clip in f64
on z, the 10 nearest neighbours from scipy's cKDTree re-ranked by the f32 distance and then by index, centroid / scatter / numpy.linalg.eigh
in f64, the draws in Python integer arithmetic, the plane and the point-plane test in numpy float32 (every operation its own rounding),
and ransac.hpp's sequential loop."""
import math

import numpy as np

K = 10
BAD = 0xFFFFFFFF
DEFAULTS = dict(sensor_height=0.0, clip_low=1.5, clip_high=1.5, normal_thresh_deg=20.0, distance_threshold=0.1, min_points=1024,
                floor_normal_thresh_deg=10.0, max_iterations=1000, probability=0.99)


def scene(seed=42):
    """about 94 000 points in random order: a gently tilted plane (z = -1 + 0.02 x - 0.01 y, sigma 2 cm) in an 80 m x 80 m patch, a wall,
    a 25 degree ramp and uniform clutter; not ring-structured"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-40, 40, (60_000, 2))
    plane = np.column_stack([xy, -1 + 0.02 * xy[:, 0] - 0.01 * xy[:, 1] + rng.normal(0, 0.02, 60_000)])
    wall = np.column_stack([np.full(20_000, 12.0) + rng.normal(0, 0.02, 20_000), rng.uniform(-30, 30, 20_000), rng.uniform(-1.4, 6.0, 20_000)])
    rx, ry = rng.uniform(-30, -20, 8_000), rng.uniform(-10, 10, 8_000)
    ramp = np.column_stack([rx, ry, -1.2 + math.tan(math.radians(25.0)) * (rx + 30) + rng.normal(0, 0.02, 8_000)])
    clutter = np.column_stack([rng.uniform(-40, 40, 6_000), rng.uniform(-40, 40, 6_000), rng.uniform(-3, 8, 6_000)])
    p = np.concatenate([plane, wall, ramp, clutter])
    p = np.column_stack([p, rng.uniform(0, 255, len(p))]).astype(np.float32)
    return p[rng.permutation(len(p))]


def clip(pts, sensor_height=0.0, clip_low=1.5, clip_high=1.5):
    """indices kept: finite, and sensor_height - clip_low <= z < sensor_height + clip_high with z in f64"""
    p = np.asarray(pts, np.float32)
    z = p[:, 2].astype(np.float64)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(p[:, :3]).all(1) & (z >= sensor_height - clip_low) & (z < sensor_height + clip_high)
    return np.nonzero(keep)[0]


def _d2(a, b):
    d = (a - b).astype(np.float32)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float32) + d[..., 2] * d[..., 2]).astype(np.float32)


def self_knn(xyz, k=K, extra=6):
    """(idx n x k, tie n bool): the k nearest of every point among the points, ascending (f32 d2, index); tie: the k-th and the (k+1)-th are
    equally far in f32 (none expected on the test scenes), or the candidates cannot prove the k-th place"""
    from scipy.spatial import cKDTree

    P = np.ascontiguousarray(xyz, np.float32)
    kk = min(k + extra, len(P))
    dist, cand = cKDTree(P.astype(np.float64)).query(P.astype(np.float64), k=kk, workers=16)
    dc = _d2(P[cand], P[:, None, :])
    order = np.lexsort((cand, dc), axis=-1)
    ci, cd = np.take_along_axis(cand, order, 1), np.take_along_axis(dc, order, 1)
    tie = (cd[:, k - 1] == cd[:, k]) | ~(cd[:, k].astype(np.float64) < dist[:, -1] ** 2 * (1 - 1e-5)) if kk > k else np.zeros(len(P), bool)
    return ci[:, :k], tie


def normals(xyz, idx):
    """per point: the unit eigenvector of the smallest eigenvalue of the scatter of its neighbours about their centroid (f64, eigh), the
    eigen-gap (l1 - l0) / l2, and the angle of the normal to the z axis in degrees (folded to [0, 90])"""
    nb = np.asarray(xyz, np.float32)[idx].astype(np.float64)
    d = nb - nb.mean(1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", d, d)
    w, v = np.linalg.eigh(cov)
    n = v[:, :, 0]
    gap = (w[:, 1] - w[:, 0]) / np.maximum(w[:, 2], 1e-300)
    ang = np.degrees(np.arccos(np.clip(np.abs(n[:, 2]), 0, 1)))
    return n, gap, ang


def _mix(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def draw(seed, j, n):
    """draw j of a run with `seed` over n >= 3 points, in Python integers"""
    s = _mix((seed & 0xFFFFFFFF) ^ 0x9E3779B9)
    r = [_mix((s + 3 * j + t) & 0xFFFFFFFF) for t in range(3)]
    i0 = (r[0] * n) >> 32
    i1 = (r[1] * (n - 1)) >> 32
    i1 += i1 >= i0
    i2 = (r[2] * (n - 2)) >> 32
    lo, hi = min(i0, i1), max(i0, i1)
    i2 += i2 >= lo
    i2 += i2 >= hi
    return i0, i1, i2


def plane(p0, p1, p2):
    """(nx, ny, nz, d) in f32, every operation rounded on its own, or None for a bad draw (zero or non-finite squared cross product)"""
    f = np.float32
    p0, p1, p2 = (np.asarray(p, f) for p in (p0, p1, p2))
    with np.errstate(all="ignore"):
        a, b = p1 - p0, p2 - p0
        c = np.array([f(a[1] * b[2]) - f(a[2] * b[1]), f(a[2] * b[0]) - f(a[0] * b[2]), f(a[0] * b[1]) - f(a[1] * b[0])], f)
        l2 = f(f(c[0] * c[0]) + f(c[1] * c[1])) + f(c[2] * c[2])
        if not (l2 > 0 and np.isfinite(l2)):
            return None
        n = c / np.sqrt(l2)
        d = -(f(f(n[0] * p0[0]) + f(n[1] * p0[1])) + f(n[2] * p0[2]))
    return np.array([n[0], n[1], n[2], d], f)


def residual_ok(xyz, pl, thr=0.1):
    """the f32 test |((nx x + ny y) + nz z) + d| < thr per point"""
    f = np.float32
    P = np.asarray(xyz, f)
    pl = np.asarray(pl, f)
    v = ((pl[0] * P[:, 0] + pl[1] * P[:, 1]).astype(f) + pl[2] * P[:, 2]).astype(f) + pl[3]
    with np.errstate(invalid="ignore"):
        return np.abs(v.astype(f)) < f(thr)


def ransac(xyz, seed, n_scored, thr=0.1, max_iterations=1000, probability=0.99):
    """the run over the filtered points: for the first n_scored draws (a multiple of 64, what the device scored) the triples, counts (BAD for
    a bad draw) and planes; and ransac.hpp's loop over them: dict(iterations, skipped, draws_used, winner).  Raises when the loop needs
    more draws than were scored."""
    P = np.asarray(xyz, np.float32)
    N = len(P)
    tri = np.array([draw(seed, j, N) for j in range(n_scored)], np.int64).reshape(n_scored, 3)
    counts = np.zeros(n_scored, np.uint32)
    planes = np.full((n_scored, 4), np.nan, np.float32)
    for j in range(n_scored):
        pl = plane(P[tri[j, 0]], P[tri[j, 1]], P[tri[j, 2]])
        if pl is None:
            counts[j] = BAD
        else:
            planes[j] = pl
            counts[j] = int(residual_ok(P, pl, thr).sum())
    it = sk = j = 0
    k, best, winner = 1.0, -1, -1
    logp = math.log(1.0 - probability)
    eps = np.finfo(np.float64).eps
    while it < k and sk < 10 * max_iterations:
        if j >= n_scored:
            raise AssertionError("the loop needs more draws than were scored")
        c = int(counts[j])
        j += 1
        if c == BAD:
            sk += 1
            continue
        if c > best:
            best, winner = c, j - 1
            w = best * (1.0 / N)
            pno = min(1.0 - eps, max(eps, 1.0 - math.pow(w, 3.0)))
            k = logp / math.log(pno)
        it += 1
        if it > max_iterations:
            break
    return tri, counts, planes, dict(iterations=it, skipped=sk, draws_used=j, winner=winner)
