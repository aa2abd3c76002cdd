"""The detection front end's rules restated in numpy f32, and the cases of its tests.

The rules are those of include/lio_hip.h ("Detection front end"): the reference's preprocess_kernel.cu and voxelization_kernel.cu run one thread
after another in index order.  Every product, sum and quotient is its own f32 numpy operation, so nothing is contracted; numpy's f32 -> f16
conversion rounds to nearest even, keeps subnormals and overflows to inf.  tools/record_voxelize_golden.py runs the reference's own two files
over CASES and DEVIATIONS and stores what they give in tests/golden/voxelize.npz and voxelize_deviations.npz.

A case is (params, calls): params a dict (min, max, size, max_voxels, P, max_points, frames, order), calls a list of (rows (n, 5) f32,
motion (4, 4) f32, realtime).
"""
import math
import os

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "voxelize.npz")
GOLDEN_DEV = os.path.join(HERE, "golden", "voxelize_deviations.npz")
XYZ, ZYX = 1, 2
EYE = np.eye(4, dtype=F)


# ---- the rules -------------------------------------------------------------------------------------------------------------------------------
def grid_size(mn, mx, size):
    """compute_grid_size: (int)std::round((max - min) / size) per axis in f32 (std::round: halves away from zero)"""
    q = (np.asarray(mx, F) - np.asarray(mn, F)) / np.asarray(size, F)
    return [int(math.floor(float(v) + 0.5)) for v in q]


def transform_rows(rows, motion):
    """transform_kernel: x y z by rows 0..2 of the 4 x 4 in f32, left to right; channel 3 copied; channel 4 + 0.1 in f64"""
    r = np.asarray(rows, F)
    m = np.asarray(motion, F).reshape(4, 4)
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    out = r.copy()
    with np.errstate(all="ignore"):
        for k in range(3):
            out[:, k] = ((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3]
        out[:, 4] = (r[:, 4].astype(np.float64) + 0.1).astype(F)
    return out


class Window:
    """PreprocessImplement::forward's window with the counts zeroed by a non-realtime call (the rule here)"""

    def __init__(self, max_points, frames):
        self.max_points, self.frames = int(max_points), int(frames)
        self.reset()

    def reset(self):
        self.counts = [0] * self.frames
        self.rows = np.zeros((0, 5), F)

    def forward(self, rows, motion, realtime):
        rows = np.ascontiguousarray(rows, F).reshape(-1, 5)
        n = min(len(rows), self.max_points)
        assert n > 0
        if realtime:
            total = len(self.rows) - self.counts[-1]
            n = max(min(n, self.max_points - total), 1)
            self.counts = [n] + self.counts[:-1]
            self.rows = np.concatenate([rows[:n], transform_rows(self.rows[:total], motion)])
        else:
            self.counts = [n] + [0] * (self.frames - 1)
            self.rows = rows[:n].copy()
        return self.rows


def voxelize(rows, p):
    """dict(features uint16 (V, 5), indices int32 (V, 4), counts uint32 (V,), real, in_range, kept, slots (V, P) point indices or -1)"""
    rows = np.ascontiguousarray(rows, F).reshape(-1, 5)
    mn, mx, sz = (np.asarray(p[k], F) for k in ("min", "max", "size"))
    g = grid_size(mn, mx, sz)
    P, cap = int(p["P"]), int(p["max_voxels"])
    xyz = rows[:, :3]
    with np.errstate(all="ignore"):
        f = np.floor((xyz - mn) / sz)
        ok = np.isfinite(xyz).all(1) & (xyz >= mn).all(1) & (xyz < mx).all(1) & (f >= 0).all(1) & (f < F(2147483648.0)).all(1)
    idx = np.where(ok[:, None], f, 0).astype(np.int64)
    ok &= (idx < np.asarray(g, np.int64)).all(1)
    sel = np.flatnonzero(ok)
    key = (idx[sel, 2] * g[1] + idx[sel, 1]) * g[0] + idx[sel, 0]
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(len(uniq), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(uniq))
    vid = rank[inv.reshape(-1)]  # voxel id of every counted point: the rank of its voxel's first point
    real = len(uniq)
    V = min(real, cap)
    live = vid < cap
    pts, vid = sel[live], vid[live]
    order = np.argsort(vid, kind="stable")  # points of a voxel together, in window order
    pts, vid = pts[order], vid[order]
    raw = np.bincount(vid, minlength=V).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(raw)[:-1]]) if V else np.zeros(0, np.int64)
    pos = np.arange(len(pts)) - start[vid]
    slots = np.full((V, P), -1, np.int64)
    keep = pos < P
    slots[vid[keep], pos[keep]] = pts[keep]
    counts = np.minimum(raw, P)
    acc = rows[slots[:, 0]].copy() if V else np.zeros((0, 5), F)
    with np.errstate(all="ignore"):
        for s in range(1, P):
            m = counts > s
            acc[m] = acc[m] + rows[slots[m, s]]
        mean = acc / counts.astype(F)[:, None]
        feat = mean.astype(np.float16).view(np.uint16)
    head = slots[:, 0]
    ix, iy, iz = (idx[head, k].astype(np.int32) for k in range(3))
    zero = np.zeros(V, np.int32)
    indices = np.stack([zero, iz, iy, ix] if int(p["order"]) == ZYX else [zero, ix, iy, iz], axis=1).astype(np.int32).reshape(V, 4)
    return dict(features=feat.reshape(V, 5), indices=indices, counts=counts.astype(np.uint32), real=real, in_range=len(sel), kept=int(counts.sum()),
                slots=slots)


def run_case(case):
    """the restatement over a case: per call dict(window, window_counts, features, indices, counts, num, real, in_range, kept)"""
    p, calls = case
    w = Window(p["max_points"], p["frames"])
    out = []
    for rows, motion, realtime in calls:
        win = w.forward(rows, motion, realtime)
        r = voxelize(win, p)
        r.update(window=win.copy(), window_counts=np.asarray(w.counts, np.int32), num=len(r["counts"]))
        out.append(r)
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
def params(mn=(0, 0, 0), mx=(8, 8, 4), size=(1, 1, 1), max_voxels=300, P=5, max_points=8192, frames=1, order=ZYX):
    return dict(min=np.asarray(mn, F), max=np.asarray(mx, F), size=np.asarray(size, F), max_voxels=max_voxels, P=P, max_points=max_points, frames=frames,
                order=order)


def rows_of(xyz, seed=0):
    """(n, 5) rows over the given coordinates: intensity an integer below 256, time a multiple of 1 / 64"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    rng = np.random.default_rng(1000 + seed)
    r = np.zeros((len(xyz), 5), F)
    r[:, :3] = xyz
    r[:, 3] = rng.integers(0, 256, len(xyz))
    r[:, 4] = rng.integers(0, 64, len(xyz)) / 64.0
    return r


def random_rows(n, seed, lo=(-1, -1, -1), hi=(9, 9, 5), step=16):
    """n rows with coordinates on a 1 / step lattice over a box a little larger than the small grid (some points fall outside)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo), np.asarray(hi)
    xyz = rng.integers(lo * step, hi * step, (n, 3)) / float(step)
    return rows_of(xyz, seed)


def single(p, rows):
    return (p, [(rows, EYE, False)])


def one_voxel_rows(n, cell=(3, 2, 1), seed=0):
    """n distinct-looking rows inside one cell of the small grid"""
    rng = np.random.default_rng(50 + seed)
    xyz = np.asarray(cell) + rng.integers(1, 63, (n, 3)) / 64.0
    return rows_of(xyz, seed)


def crowded(k, seed):
    """k points in cell (3, 2, 1) among 40 points elsewhere, interleaved"""
    a, b = one_voxel_rows(k, seed=seed), random_rows(40, 70 + seed)
    b = b[~((np.floor(b[:, 0]) == 3) & (np.floor(b[:, 1]) == 2) & (np.floor(b[:, 2]) == 1))]
    rows = np.concatenate([a, b])
    return rows[np.random.default_rng(seed).permutation(len(rows))]


def every_cell():
    """256 points, every one its own voxel of the 8 x 8 x 4 grid"""
    c = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    return rows_of(c + 0.5, 3)[np.random.default_rng(4).permutation(256)]


def cap_rows():
    """90 points over exactly 12 voxels, the last voxel entered by the last three points only"""
    rng = np.random.default_rng(8)
    cells = np.array([[i % 8, (3 * i) % 8, (i // 4) % 4] for i in range(11)])
    pick = np.concatenate([np.arange(11), rng.integers(0, 11, 76)])[rng.permutation(87)]
    xyz = cells[pick] + rng.integers(1, 63, (87, 3)) / 64.0
    last = np.array([7, 7, 3]) + rng.integers(1, 63, (3, 3)) / 64.0
    return rows_of(np.concatenate([xyz, last]), 8)


def below(v):
    return np.nextafter(F(v), F(-np.inf))


def above(v):
    return np.nextafter(F(v), F(np.inf))


def face_rows():
    """finite points on and about the faces of the small grid"""
    pts = [(0, 0, 0), (8, 1, 1), (1, 8, 1), (1, 1, 4), (below(8), below(8), below(4)), (below(3), 1, 1), (3, 1, 1), (above(3), 1, 1),
           (1, below(5), 1), (1, 5, 1), (1, above(5), 1), (1, 1, below(2)), (1, 1, 2), (1, 1, above(2)),
           (-0.5, 1, 1), (8.5, 1, 1), (1, -0.5, 1), (1, 8.5, 1), (1, 1, -0.5), (1, 1, 4.5), (below(0), 1, 1), (-0.0, 2, 2), (1e30, 1, 1), (-1e30, 1, 1),
           (1, 1, 3e38), (4, 4, 2)]
    return rows_of(np.asarray(pts, F), 5)


def nonfinite_rows():
    """NaN and +-inf in each coordinate among good points"""
    pts = [(1.5, 1.5, 1.5)]
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            q = [2.5, 3.5, 1.5]
            q[k] = bad
            pts.append(tuple(q))
        pts.append((4.5, 1.5, 0.5))
    r = rows_of(np.asarray(pts, F), 6)
    r[0, 3] = np.nan  # a non-finite channel of a good point is data: it goes into the mean
    return r


YAML = dict(mn=(-64.0, -64.0, -2), mx=(64.0, 64.0, 4), size=(0.1, 0.1, 0.15))  # sensor_inference/cfgs/detection_object.yaml


def yaml_rows():
    """2000 full-precision points in the configuration's range, its corners and the largest floats below them included"""
    rng = np.random.default_rng(12)
    xyz = (rng.random((1960, 3)) * np.array([132.0, 132.0, 6.4]) - np.array([66.0, 66.0, 2.2])).astype(F)
    xyz[:200] = (xyz[:200] * F(0.1)).astype(F)  # a dense middle: voxels with several points
    edge = []
    for sx in (F(-64), below(64), F(64)):
        for sy in (F(-64), below(64), F(64)):
            for sz in (F(-2), below(4), F(4)):
                edge.append((sx, sy, sz))
    edge += [(below(-64), 0, 0), (0, 0, below(-2)), (63.95, 63.95, 3.9), (63.9, -63.9, 3.85), (-0.05, -0.05, -0.05), (0.05, 0.05, 0.05),
             (0.1, 0.2, 0.15), (0.3, 0.6, 0.45), (12.7, -12.7, 1.0)]
    edge = np.asarray(edge, F)
    edge = np.concatenate([edge, edge[:40 - len(edge)]]) if len(edge) < 40 else edge[:40]
    r = rows_of(np.concatenate([xyz, edge]), 12)
    r[:, 3] = rng.random(len(r)).astype(F) * F(255)
    r[:, 4] = rng.random(len(r)).astype(F)
    return r


def f16_rows():
    """means in f16's subnormal range, a mean halfway between two f16 values (to even), an intensity beyond f16 (inf), a negative zero"""
    r = np.zeros((9, 5), F)
    r[0:2, :3] = (0.5, 0.5, 0.5)      # voxel 0: intensities 2e-6 and 4e-6, mean 3e-6: subnormal in f16
    r[0, 3], r[1, 3] = 2e-6, 4e-6
    r[2:4, :3] = (1.5, 0.5, 0.5)      # voxel 1: intensities 2048 and 2050, mean 2049: halfway between 2048 and 2050 in f16, to even 2048
    r[2, 3], r[3, 3] = 2048, 2050
    r[4:6, :3] = (2.5, 0.5, 0.5)      # voxel 2: 2050 and 2052, mean 2051: halfway between 2050 and 2052, to even 2052
    r[4, 3], r[5, 3] = 2050, 2052
    r[6, :3] = (3.5, 0.5, 0.5)        # voxel 3: 70000 -> inf, time 65520 -> inf (the first value that rounds up to it), 65519 stays finite
    r[6, 3], r[6, 4] = 70000, 65520
    r[7, :3] = (4.5, 0.5, 0.5)
    r[7, 3], r[7, 4] = 65519, -0.0    # voxel 4: a negative zero survives a sum that starts from slot 0's value
    r[8, :3] = (5.5, 0.5, 0.5)
    r[8, 3], r[8, 4] = 6e-8, 2.9e-8   # voxel 5: the smallest f16 subnormal and a value below half of it (to zero)
    return r


def rigid(yaw=0.03, pitch=-0.01, roll=0.02, t=(0.8, -0.05, 0.02)):
    """a general rigid motion as f32 4 x 4"""
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    R = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return m.astype(F)


def sweep(n, seed):
    """n full-precision rows about the middle of the small grid"""
    rng = np.random.default_rng(200 + seed)
    r = np.zeros((n, 5), F)
    r[:, :3] = (rng.random((n, 3)) * np.array([9.0, 9.0, 4.5]) - np.array([0.5, 0.5, 0.25])).astype(F)
    r[:, 3] = rng.random(n).astype(F) * F(255)
    return r


WIN = dict(max_points=1000, frames=3, max_voxels=300)


def window_case(n, calls=5):
    """`calls` realtime calls of n points under a general rigid motion"""
    return (params(**WIN), [(sweep(n, k), rigid(0.03 + 0.01 * k), True) for k in range(calls)])


def window_full_case():
    """two sweeps fill the window exactly; the third call stores one point, the fourth is clamped, the fifth pops"""
    return (params(**WIN), [(sweep(500, 10), EYE, True), (sweep(500, 11), rigid(), True), (sweep(300, 12), rigid(), True), (sweep(300, 13), rigid(), True),
                            (sweep(300, 14), rigid(), True)])


def window_identity_case():
    """identity motion: x y z pass through bit for bit, channel 4 takes the double rule once per sweep"""
    return (params(**WIN), [(sweep(100, 20 + k), EYE, True) for k in range(4)])


def window_mixed_case():
    """realtime, a non-realtime call in between, realtime again until the window pops.  (After ONE realtime call the older counts are still zero,
    so the reference's stale counts do not show; the case with two realtime calls first is DEVIATIONS["stale_counts"])"""
    return (params(**WIN), [(sweep(200, 30), EYE, True), (sweep(150, 32), rigid(), False), (sweep(120, 33), rigid(), True), (sweep(120, 34), rigid(), True),
                            (sweep(400, 35), rigid(), True)])


def _cases():
    c = {}
    for n in (1, 63, 64, 65, 2047, 2048, 2049, 4097):
        c[f"tile_{n}"] = single(params(), random_rows(n, n))
    for name, k in (("slots_p", 5), ("slots_p1", 6)):
        rows = crowded(k, k)
        c[name] = single(params(), rows)
        c[name + "_rev"] = single(params(), rows[::-1].copy())
    rows = one_voxel_rows(4096, seed=9)
    c["slots_4096"] = single(params(), rows)
    c["slots_4096_rev"] = single(params(), rows[::-1].copy())
    cells = every_cell()
    c["ids_a"] = single(params(), cells)
    c["ids_b"] = single(params(), cells[np.random.default_rng(17).permutation(256)])
    for name, mv in (("cap_eq", 12), ("cap_less", 11), ("cap_one", 1)):
        c[name] = single(params(max_voxels=mv), cap_rows())
    c["faces"] = single(params(), face_rows())
    c["yaml"] = single(params(max_voxels=4000, **YAML), yaml_rows())
    c["f16"] = single(params(), f16_rows())
    c["order_xyz"] = single(params(order=XYZ), random_rows(65, 65))
    c["p1"] = single(params(P=1), random_rows(300, 41))
    c["p32"] = single(params(P=32, max_voxels=40), random_rows(3000, 42))
    c["window_300"] = window_case(300)
    c["window_400"] = window_case(400)  # the third call is clamped to 200, the fourth pops 400
    c["window_full"] = window_full_case()
    c["window_identity"] = window_identity_case()
    c["window_mixed"] = window_mixed_case()
    return c


def _deviations():
    d = {}
    # grid 10 over a range of 0.96: x = 0.97 fails the range test and passes the grid test (index 9)
    p = params(mn=(0, 0, 0), mx=(0.96, 1, 1), size=(0.1, 0.5, 0.5))
    d["grid_only"] = single(p, rows_of(np.asarray([(0.05, 0.25, 0.25), (0.97, 0.25, 0.25), (0.55, 0.75, 0.25)], F), 1))
    d["nonfinite"] = single(params(), nonfinite_rows())
    d["stale_counts"] = (params(**WIN), [(sweep(10, 40), EYE, True), (sweep(10, 41), rigid(), True), (sweep(5, 42), rigid(), False), (sweep(4, 43), rigid(), True)])
    return d


CASES = _cases()
DEVIATIONS = _deviations()
WHAT = ("features", "indices", "counts", "num", "real", "window_counts")


def load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def check_call(got, want, what=WHAT + ("window",)):
    """every named array of two per-call records is equal; returns the names that differ"""
    return [k for k in what if not np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=(k == "window"))]
