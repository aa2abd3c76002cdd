"""Scenes of the bird's-eye image tests and the numpy restatement of the rules of include/lio_hip.h (lio_bev_*), in this project's own
words.  The restatement is what the device is held to bit for bit; tests/test_bev_cpu.py holds the restatement to results recorded from
the reference's convert_cloud_image.py (tests/golden/bev.npz)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bev.npz")
BASE_PPM, BASE_WINDOW = 5, 8.0
F32 = np.float32


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
def base_scene(n=60_000, seed=7):
    """60 m x 40 m of dark ground with a brightness ramp along x, two bright stripes and an 18 m square hole; n x 4 f32"""
    rng = np.random.default_rng(seed)
    pts = np.zeros((0, 4), F32)
    while len(pts) < n:
        m = 2 * n
        x, y = rng.uniform(0.0, 60.0, m), rng.uniform(0.0, 40.0, m)
        keep = ~((x > 30.0) & (x < 48.0) & (y > 11.0) & (y < 29.0))
        x, y = x[keep], y[keep]
        inten = 0.04 + 0.10 * x / 60.0 + rng.normal(0.0, 0.012, len(x))
        stripe = (np.abs(y - 8.0) < 0.15) | (np.abs(x - 15.0) < 0.15)
        inten = np.where(stripe, 0.55 + rng.normal(0.0, 0.05, len(x)), inten)
        inten = np.clip(inten, 0.001, 1.0)
        z = 0.02 * np.sin(x / 7.0) + rng.normal(0.0, 0.01, len(x))
        # a coarse lattice keeps the recorded fixture small and puts points exactly on half-pixel offsets (x = j + 0.5 at 5 px/m)
        x, y, z, inten = np.round(x * 256.0) / 256.0, np.round(y * 256.0) / 256.0, np.round(z * 1024.0) / 1024.0 + 0.0, np.round(inten * 2.0**20) / 2.0**20
        pts = np.concatenate([pts, np.stack([x, y, z, inten], 1).astype(F32)])
    pts = pts[:n].copy()
    # the corners pin the bounds: 301 x 201 pixels at 5 px/m
    pts[0, :2], pts[1, :2] = (0.0, 0.0), (60.0, 40.0)
    return pts


def golden_points(g):
    """the input cloud of the golden file (stored as its lattice numbers, column by column)"""
    return np.stack([g["x256"] / 256.0, g["y256"] / 256.0, g["z1024"] / 1024.0, g["i2p20"] / 2.0**20], 1).astype(F32)


def cut_ranks(n):
    return int(n * 0.01), int(n * 0.999)


def cut_intensities_unique(pts):
    """True when the intensities at the two cut ranks occur once among the finite points (numpy's unstable argsort then cannot matter)"""
    inten = np.sort(pts[:, 3])
    lo, hi = cut_ranks(len(inten))
    return all(np.count_nonzero(inten == inten[r]) == 1 for r in (lo - 1, lo, hi - 1, hi) if 0 <= r < len(inten))


# ---- the rules ------------------------------------------------------------------------------------------------------------------------------
def grey_table():
    t = np.arange(65536, dtype=np.float64) * (1.0 / 65535.0)
    t[-1] = 1.0
    return np.trunc(t * 65535.0).astype(np.uint16)


def pixels_of(pts, ppm):
    """finite mask, (xs, ys) per point (-1 for a dropped one), image_w, image_h, bounds"""
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 4)
    fin = np.isfinite(pts[:, 0]) & np.isfinite(pts[:, 1]) & np.isfinite(pts[:, 3])
    if not fin.any():
        raise ValueError("no finite point")
    x, y = pts[fin, 0], pts[fin, 1]
    x_min, x_max, y_min, y_max = x.min(), x.max(), y.min(), y.max()
    w = int(np.ceil((float(x_max) - float(x_min)) * ppm)) + 1
    h = int(np.ceil((float(y_max) - float(y_min)) * ppm)) + 1
    xy = np.full((len(pts), 2), -1, np.int32)
    xy[fin, 0] = np.rint((x - x_min) * F32(ppm)).astype(np.int32)
    xy[fin, 1] = np.rint((-(y - y_max)) * F32(ppm)).astype(np.int32)
    return fin, xy, w, h, (float(x_min), float(x_max), float(y_min), float(y_max))


def kept_of(pts, fin):
    """input indices of the kept points, ascending in (intensity, index) with -0.0 equal to +0.0"""
    idx = np.flatnonzero(fin)
    inten = np.ascontiguousarray(pts, F32).reshape(-1, 4)[idx, 3] + F32(0.0)  # (-0.0 + 0.0 = +0.0)
    order = idx[np.argsort(inten, kind="stable")]
    lo, hi = cut_ranks(len(idx))
    return order[lo:hi]


def segment_means(keys_sorted, vals):
    """sequential f32 sum of vals over each run of equal keys (in the given order) divided by the f32 count"""
    n = len(keys_sorted)
    head = np.flatnonzero(np.r_[True, keys_sorted[1:] != keys_sorted[:-1]]) if n else np.zeros(0, np.int64)
    cnt = np.diff(np.r_[head, n])
    s = np.zeros(len(head), F32)
    live = np.arange(len(head))
    r = 0
    while len(live):
        s[live] = s[live] + vals[head[live] + r]
        r += 1
        live = live[cnt[live] > r]
    return keys_sorted[head], s / cnt.astype(F32), cnt


def scatter_of(pts, xy, kept, w):
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 4)
    key = xy[kept, 1].astype(np.int64) * w + xy[kept, 0].astype(np.int64)
    o = np.argsort(key, kind="stable")
    ks, src = key[o], kept[o]
    pk, pI, cnt = segment_means(ks, pts[src, 3])
    _, pz, _ = segment_means(ks, pts[src, 2])
    return pk.astype(np.uint32), pI, pz, cnt


EDGES = (np.arange(1025, dtype=np.float64) * 65535.0 / 1024.0).astype(F32)
TERM_MAX = 8388608.0


def bins_of(v):
    """numpy's uniform-bin search of values in [0, 65535]"""
    i = ((v / F32(65535.0)) * F32(1024.0)).astype(np.int64)
    i[i == 1024] = 1023
    i[v < EDGES[i]] -= 1
    up = (v >= EDGES[i + 1]) & (i != 1023)
    i[up] += 1
    return i


def fixed_sum(x):
    """the project's mean rule: the exact integer sum of rint(clamp(x) * 2^16) (NaN: 0)"""
    x = np.asarray(x, np.float64)
    t = np.rint(np.clip(np.where(np.isnan(x), 0.0, x), -TERM_MAX, TERM_MAX) * 65536.0).astype(np.int64)
    return int(t.sum(dtype=np.int64))


def clip_steps(mean32):
    """the table of clip limits (f64 values) from the f32 mean of v"""
    with np.errstate(divide="ignore", invalid="ignore"):
        c0 = F32(20480.0) / F32(mean32)
    tab = []
    if c0 > F32(1.0):
        c = F32(c0)
        tab.append(float(c))
        while c < F32(120.0) and len(tab) < 1280:
            c = F32(c + F32(0.1))
            tab.append(float(c))
    else:
        c = 1.0
        tab.append(c)
        while c < 120.0 and len(tab) < 1280:
            c = c + 0.1
            tab.append(c)
    return tab


def node_equalise(inten):
    """one node over the mean intensities of its window: (step, clip, value function) or None when no value lies in [0, 65535]"""
    v = inten.astype(F32) * F32(65535.0)
    inr = (v >= 0) & (v <= F32(65535.0))
    if not inr.any():
        return None
    hist = np.bincount(bins_of(v[inr]), minlength=1024).astype(np.float64)
    dens = hist / np.diff(EDGES).astype(np.float64) / float(int(hist.sum()))
    cdf = np.cumsum(dens)
    cdf = 65535.0 * cdf / cdf[-1]
    slope = (cdf[1:] - cdf[:-1]) / (EDGES[1:1024].astype(np.float64) - EDGES[:1023].astype(np.float64))

    def interp(u):
        x = u.astype(np.float64)
        out = np.empty(len(u), np.float64)
        low, high = u < 0, u >= EDGES[1023]
        out[low], out[high] = cdf[0], cdf[1023]
        mid = ~(low | high)
        j = bins_of(u[mid])
        xj = EDGES[j].astype(np.float64)
        out[mid] = np.where(x[mid] == xj, cdf[j], slope[j] * (x[mid] - xj) + cdf[j])
        return out

    def value(u, c):
        with np.errstate(invalid="ignore"):
            return u.astype(np.float64) * np.minimum(interp(u) / np.maximum(u, F32(0.001)).astype(np.float64), c)

    count = len(v)
    mean32 = F32((fixed_sum(v) / 65536.0) / float(count))
    tab = clip_steps(mean32)
    target = count * 20480 * 65536
    reached = lambda k: fixed_sum(value(v, tab[k])) >= target  # noqa: E731
    kmax = len(tab) - 1
    if (v < 0).any():
        k = 0
        while k < kmax and not reached(k):
            k += 1
    else:
        lo, hi = 0, kmax
        while lo < hi:
            mid = (lo + hi) // 2
            if reached(mid):
                hi = mid
            else:
                lo = mid + 1
        k = lo

    def result(u):
        t = value(u.astype(F32) * F32(65535.0), tab[k])
        return np.clip(np.where(np.isnan(t), 0.0, t), 0.0, 65535.0).astype(F32)

    return k, tab[k], result


def geometry(w, h, window, ppm):
    P = int(window * ppm)
    hp = int(P / 2)
    q = int(hp / 2)
    W, H = int((w + hp) / hp) * hp, int((h + hp) / hp) * hp
    return P, hp, q, W, H, W // hp + 1, H // hp + 1


def convert_of(pkey, pI, w, h, window, ppm):
    """dict(count, step, clip per node; eq per pixel; image)"""
    P, hp, q, W, H, nx, ny = geometry(w, h, window, ppm)
    xs, ys = (pkey.astype(np.int64) % w), (pkey.astype(np.int64) // w)
    count, step, clip = np.zeros(nx * ny, np.uint32), np.full(nx * ny, -1, np.int32), np.zeros(nx * ny)
    eq = pI.astype(F32).copy()
    for ix in range(nx):
        for iy in range(ny):
            xi, yi, node = ix * hp, iy * hp, ix * ny + iy
            big = (xs >= xi - P) & (xs <= xi + P) & (ys >= yi - P) & (ys <= yi + P)
            count[node] = np.count_nonzero(big)
            if count[node] <= 100:
                continue
            res = node_equalise(pI[big])
            if res is None:
                continue
            step[node], clip[node], fn = res
            small = (xs >= xi - q) & (xs <= xi + q) & (ys >= yi - q) & (ys <= yi + q)
            eq[small] = fn(pI[small])  # (nodes in xi-major order: a later node overwrites a shared border)
    g = np.rint(eq)
    g = np.where(g >= 0, np.minimum(g, F32(65535.0)), F32(0.0)).astype(np.int64)
    image = np.zeros((H, W), np.uint16)
    image[ys, xs] = grey_table()[g]
    return dict(count=count, step=step, clip=clip, eq=eq, image=image, geometry=(P, hp, q, W, H, nx, ny))


def restate(pts, window, ppm):
    """every stage of the device for n x 4 points"""
    fin, xy, w, h, bounds = pixels_of(pts, ppm)
    kept = kept_of(pts, fin)
    pkey, pI, pz, cnt = scatter_of(pts, xy, kept, w)
    out = convert_of(pkey, pI, w, h, window, ppm)
    out.update(fin=fin, xy=xy, w=w, h=h, bounds=bounds, kept=kept.astype(np.uint32), pkey=pkey, pI=pI, pz=pz, pcount=cnt)
    return out


_cache = {}


def base_restated():
    """the base scene and its restatement, computed once per process and shared (read-only)"""
    if "base" not in _cache:
        pts = base_scene()
        res = restate(pts, BASE_WINDOW, BASE_PPM)
        for a in [pts] + [v for v in res.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _cache["base"] = (pts, res)
    return _cache["base"]


def write_pcd(path, pts, order=("x", "y", "z", "intensity"), data="binary", extra=None):
    """a PCD file of n x 4 points with the fields in `order` (an optional extra f32 field `extra` of ones comes first)"""
    cols = {"x": 0, "y": 1, "z": 2, "intensity": 3}
    names = ([extra] if extra else []) + list(order)
    tab = np.ones((len(pts), len(names)), F32)
    for j, nme in enumerate(names):
        if nme in cols:
            tab[:, j] = pts[:, cols[nme]]
    head = "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS {}\nSIZE {}\nTYPE {}\nCOUNT {}\nWIDTH {}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {}\nDATA {}\n".format(
        " ".join(names), " ".join(["4"] * len(names)), " ".join(["F"] * len(names)), " ".join(["1"] * len(names)), len(pts), len(pts), data)
    with open(path, "wb") as f:
        f.write(head.encode())
        if data == "ascii":
            f.write("\n".join(" ".join(repr(float(v)) for v in row) for row in tab).encode() + b"\n")
        else:
            f.write(tab.tobytes())
