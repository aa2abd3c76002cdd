"""Cases and references for the GICP kernels of csrc/gicp.hip alone (tests/test_gicp_edges_cpu.py, tests/test_gicp_edges_gpu.py).
Nothing here imports the library: numpy, mpmath and oracle/gicp.py only.

Everything is judged in DEVICE order: the array a test hands to these functions is the cloud as lio_gicp_download returns it (on the CPU: the
cloud as built), and a neighbour or a pair is the smallest key (d2 in f32, index in that array).  Ties of distance and duplicate points are
therefore decided, and no point is masked out.

  expected_lists      the k smallest keys of every point within its own cloud, ascending
  cov_exact           mean and centred sum / k of a list in long double
  lam_min             smallest eigenvalue of a symmetric 3 x 3, closed form evaluated by mpmath at 60 digits
  plane_quality       of a regularised matrix o = I - (1 - 1e-3) v0 v0^T: v0, |trace(v0 v0^T) - 1|, eigen-residual |C v0 - (v0^T C v0) v0|,
                      Rayleigh excess v0^T C v0 - lam_min
  oracle_E            the largest residual / excess the f64 route of oracle/gicp.py::covariances (f64 centring, numpy eigh and svd) attains
                      against the same long-double C: the device is given 8 E (two backward-stable solvers, a few ulp apart, behind the same
                      f64 centring; the factor was fixed before the device was run)
  expected_pairs      nearest target key of transform_f(T, source), taken iff d2 < f32(max_corr_dist^2) strictly
  maha_exact          long-double (C_B + R C_A R^T)^-1
  cost_exact          long-double H, b, err over given pairs and Mahalanobis matrices, and the sum of |addend| over the points per component
  standin_*           the kernels' SEARCH RULE restated in numpy (cells, rings in the kernel's enumeration, batches of sixteen against a stale
                      k-th key, the two-register list, the ring caps and the pool sweep), with one seeded mistake at a time: the CPU test shows
                      that every mistake changes what some case expects
"""
import os
import sys

import mpmath
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import gicp as OG  # noqa: E402

LD = np.longdouble
F32 = np.float32
G = LD(1) - LD("1e-3")
EPS = 2.0 ** -53
COV_RINGS, CORR_RINGS = 65, 16  # csrc/gicp.hip: kGicpCovRings, kGicpCorrRings (rings 0 .. cap, then the pool sweep)
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------
def d2_f32(q, pts):
    """[m, n] squared distances, oracle/gicp.py::_d2_f32 (the kernel's own expression)"""
    with np.errstate(over="ignore", invalid="ignore"):  # a coordinate of 3e38 is a case: its distances are +inf
        return OG._d2_f32(np.asarray(q, F32), np.asarray(pts, F32))


def sorted_keys(q, pts):
    """indices [m, n] by ascending (d2, index), and the d2 in that order"""
    d2 = d2_f32(q, pts)
    order = np.argsort(d2, axis=1, kind="stable")  # stable: equal d2 stay by rising index
    return order, np.take_along_axis(d2, order, axis=1)


def expected_lists(P, k):
    order, d2 = sorted_keys(P, P)
    return order[:, :k].astype(np.int32), d2[:, :k]


def check_lists(P, k, nbr):
    """the device's [n, 32] lists against the expectation: the first k exactly, the rest -1 or keys not smaller than the k-th; returns the
    number of points that differ (0 = pass)"""
    want, d2k = expected_lists(P, k)
    bad = np.any(nbr[:, :k] != want, axis=1)
    n = len(P)
    tail = nbr[:, k:]
    if tail.size:
        ok = (tail >= -1) & (tail < n)
        t = np.clip(tail, 0, n - 1)
        e = P[t, :3].astype(F32) - P[:, None, :3].astype(F32)
        td2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        kth_d2, kth_i = d2k[:, -1][:, None], want[:, -1][:, None]
        later = (td2 > kth_d2) | ((td2 == kth_d2) & (t > kth_i))
        bad |= np.any(~ok | ((tail >= 0) & ~later), axis=1)
    return int(bad.sum()), want


def cov_exact(P, idx):
    """[n, 3, 3] long double: neighbours - mean, centred sum / k"""
    nb = P[idx][..., :3].astype(LD)
    nb = nb - nb.sum(axis=1, keepdims=True) / LD(idx.shape[1])
    return np.einsum("nka,nkb->nab", nb, nb) / LD(idx.shape[1])


def _mp(x):
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


_LAM = {}  # by the matrix's bytes: the same lists come again with every grid resolution and every second run


def lam_min(C):
    """[n] long double: the smallest eigenvalue of each symmetric 3 x 3 (trigonometric closed form, 60 digits)"""
    out = np.zeros(len(C), LD)
    with mpmath.workdps(60):
        for i, c in enumerate(C):
            key = c.tobytes()
            if key in _LAM:
                out[i] = _LAM[key]
                continue
            a = [[_mp(c[r, s]) for s in range(3)] for r in range(3)]
            p1 = a[0][1] ** 2 + a[0][2] ** 2 + a[1][2] ** 2
            q = (a[0][0] + a[1][1] + a[2][2]) / 3
            p2 = (a[0][0] - q) ** 2 + (a[1][1] - q) ** 2 + (a[2][2] - q) ** 2 + 2 * p1
            if p2 == 0:
                lam = q
            else:
                p = mpmath.sqrt(p2 / 6)
                b = [[(a[r][s] - (q if r == s else 0)) / p for s in range(3)] for r in range(3)]
                det = (b[0][0] * (b[1][1] * b[2][2] - b[1][2] * b[2][1]) - b[0][1] * (b[1][0] * b[2][2] - b[1][2] * b[2][0]) +
                       b[0][2] * (b[1][0] * b[2][1] - b[1][1] * b[2][0]))
                r_ = max(mpmath.mpf(-1), min(mpmath.mpf(1), det / 2))
                lam = q + 2 * p * mpmath.cos(mpmath.acos(r_) / 3 + 2 * mpmath.pi / 3)
            hi = float(lam)
            out[i] = _LAM[key] = LD(hi) + LD(float(lam - mpmath.mpf(hi)))
    return out


def eig_exact(C, lam0):
    """unit eigenvector of lam0 [n, 3] (the largest cross product of two rows of C - lam0 I) and the gap lam1 - lam0, long double"""
    A = C - lam0[:, None, None] * np.eye(3, dtype=LD)
    cr = np.stack([np.cross(A[:, 0], A[:, 1]), np.cross(A[:, 0], A[:, 2]), np.cross(A[:, 1], A[:, 2])], 1)
    nn = np.sqrt((cr * cr).sum(-1))
    j = np.argmax(nn, axis=1)
    v = cr[np.arange(len(C)), j]
    nv = nn[np.arange(len(C)), j]
    v = v / np.where(nv > 0, nv, LD(1))[:, None]
    # lam1 from the trace and the sum of the principal 2 x 2 minors: lam1 + lam2 = tr - lam0, lam1 lam2 = minors - lam0 (tr - lam0)
    tr = C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2]
    mn = (C[:, 0, 0] * C[:, 1, 1] - C[:, 0, 1] ** 2) + (C[:, 0, 0] * C[:, 2, 2] - C[:, 0, 2] ** 2) + (C[:, 1, 1] * C[:, 2, 2] - C[:, 1, 2] ** 2)
    s, pr = tr - lam0, mn - lam0 * (tr - lam0)
    disc = np.sqrt(np.maximum(s * s - 4 * pr, LD(0)))
    lam1 = (s - disc) / 2
    return v, np.maximum(lam1 - lam0, LD(0))


def v0_of(o):
    """v0 v0^T and v0 recovered from a regularised matrix o = I - (1 - 1e-3) v0 v0^T (long double)"""
    vv = (np.eye(3, dtype=LD) - o.astype(LD)) / G
    j = np.argmax(np.abs(vv[:, [0, 1, 2], [0, 1, 2]]), axis=1)
    col = vv[np.arange(len(o)), :, j]
    d = np.sqrt(np.abs(vv[np.arange(len(o)), j, j]))
    return vv, col / np.where(d > 0, d, LD(1))[:, None]


def plane_quality(o, C, lam0):
    """per point: |trace(v0 v0^T) - 1|, the eigen-residual and the Rayleigh excess of the v0 inside o, against C"""
    vv, v = v0_of(o)
    tr = np.abs(vv[:, 0, 0] + vv[:, 1, 1] + vv[:, 2, 2] - 1)
    v = v / np.sqrt((v * v).sum(-1))[:, None]
    Cv = np.einsum("nab,nb->na", C, v)
    rho = (v * Cv).sum(-1)
    res = np.sqrt(((Cv - rho[:, None] * v) ** 2).sum(-1))
    return tr, res, rho - lam0


def oracle_planes(P, idx):
    """the f64 route of oracle/gicp.py::covariances on the given lists: regularised matrices from numpy's eigh and from its svd"""
    k = idx.shape[1]
    nb = P[idx][..., :3].astype(np.float64)
    nb = nb - nb.mean(axis=1, keepdims=True)
    cov = np.einsum("nka,nkb->nab", nb, nb) / k
    _, V = np.linalg.eigh(cov)
    o1 = np.eye(3) - (1 - 1e-3) * np.einsum("na,nb->nab", V[:, :, 0], V[:, :, 0])
    U, _, _ = np.linalg.svd(cov)
    o2 = np.eye(3) - (1 - 1e-3) * np.einsum("na,nb->nab", U[:, :, 2], U[:, :, 2])
    return o1, o2


def oracle_E(P, idx, C=None, lam0=None, skip=()):
    """E of a cloud: the largest eigen-residual or Rayleigh excess of the oracle's f64 route (eigh and svd) against the long-double C"""
    C = cov_exact(P, idx) if C is None else C
    lam0 = lam_min(C) if lam0 is None else lam0
    E = LD(0)
    for o in oracle_planes(P, idx):
        _, res, exc = plane_quality(o, C, lam0)
        keep = np.ones(len(P), bool)
        keep[list(skip)] = False
        E = max(E, res[keep].max(), np.abs(exc[keep]).max())
    return float(E)


def check_planes(P, k, cov, E, factor=8.0, skip=()):
    """assertions (a)-(c) and the Davis-Kahan comparison on a device's covariances [n, 3, 3] given in the order of P; returns a dict of the
    worst figures (ratios to each bound); raises AssertionError with the point's index"""
    idx, _ = expected_lists(P, k)
    C = cov_exact(P, idx)
    lam0 = lam_min(C)
    assert np.all(np.isfinite(cov)), "a covariance is not finite"
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    tr, res, exc = plane_quality(cov, C, lam0)
    assert tr.max() <= 1e-12, ("trace", int(np.argmax(tr)), float(tr.max()))
    bound = LD(factor * E)
    keep = np.ones(len(P), bool)
    keep[list(skip)] = False  # rows held to (a) and (b) only (the one point at 3e38 of the overflow case, whose covariance is of size 1e76)
    both = np.where(keep, np.maximum(res, np.abs(exc)), LD(0))
    worst_c = both.max()
    assert worst_c <= bound, ("eigen-residual / Rayleigh excess", int(np.argmax(both)), float(worst_c), float(bound))
    # Davis-Kahan where the plane is determined: v v^T - u u^T has the eigenvalues +-sin(theta), so every entry is at most sin(theta) <=
    # residual bound / gap.  v v^T is taken from the device's matrix as (I - o) / g divided by its trace (the length of v0 is (b)'s business);
    # the 4 * 2^-53 are the three roundings of forming 1 - g n n in f64, over g
    v, gap = eig_exact(C, lam0)
    normC = np.sqrt((C * C).sum((1, 2)))
    det = (gap > LD("1e-6") * normC) & keep
    ratio_dk = 0.0
    if det.any():
        vv, _ = v0_of(cov[det])
        vv = vv / (vv[:, 0, 0] + vv[:, 1, 1] + vv[:, 2, 2])[:, None, None]
        diff = np.abs(vv - np.einsum("na,nb->nab", v[det], v[det])).max((1, 2))
        lim = bound / gap[det] + LD(4 * 2.0 ** -53)
        ratio_dk = float((diff / lim).max())
        assert ratio_dk <= 1.0, ("Davis-Kahan", int(np.nonzero(det)[0][np.argmax(diff / lim)]), ratio_dk)
    return dict(trace=float(tr.max()), c_ratio=float(worst_c / bound) if bound > 0 else 0.0, dk_ratio=ratio_dk, determined=int(det.sum()), n=len(P))


def expected_pairs(S, Tg, T, max_corr_dist):
    """[n_src] int32 (-1 = none) and the f32 squared distances; a transformed point that is not finite has no pair"""
    with np.errstate(invalid="ignore", over="ignore"):
        q = OG.transform_f(T, S)
    d2 = d2_f32(q, Tg)
    d2n = np.where(np.isnan(d2), np.inf, d2)
    j = np.argmin(d2n, axis=1)  # the first of equal minima: the lower index
    sq = d2[np.arange(len(S)), j]
    m2 = np.float64(max_corr_dist) * np.float64(max_corr_dist)
    thr = F32(3.0e38) if m2 > 3.0e38 else F32(m2)
    ok = np.isfinite(q).all(axis=1) & (sq < thr)
    return np.where(ok, j, -1).astype(np.int32), sq


def maha_exact(cov_t, cov_s, corr, T):
    """long-double (C_B + R C_A R^T)^-1 for the rows with a pair (adjugate / determinant), and its 2-norm in f64"""
    R = np.asarray(T, np.float64)[:3, :3].astype(LD)
    has = np.nonzero(corr >= 0)[0]
    M = cov_t[corr[has]].astype(LD) + np.einsum("ab,nbc,dc->nad", R, cov_s[has].astype(LD), R)
    inv = np.zeros_like(M)
    for r in range(3):
        for c in range(3):
            r1, r2, c1, c2 = (r + 1) % 3, (r + 2) % 3, (c + 1) % 3, (c + 2) % 3
            inv[:, c, r] = M[:, r1, c1] * M[:, r2, c2] - M[:, r1, c2] * M[:, r2, c1]
    det = (M[:, 0, :] * inv[:, :, 0]).sum(-1)
    inv = inv / det[:, None, None]
    return has, inv, np.linalg.norm(inv.astype(np.float64), 2, axis=(1, 2))


def cost_exact(S, Tg, corr, maha, T, derivatives=True):
    """long-double sums over the given pairs and matrices: (H, b, err) and, for the bound, the sum over the points of the absolute value of
    each point's addend (the 29 numbers a lane of the cost kernel contributes), formed in long double with the actual e = b - T a"""
    T = np.asarray(T, np.float64).astype(LD)
    R, t = T[:3, :3], T[:3, 3]
    has = np.nonzero(corr >= 0)[0]
    a, b = S[has, :3].astype(LD), Tg[corr[has], :3].astype(LD)
    M = maha[has].astype(LD)
    ta = a @ R.T + t
    e = b - ta
    err_i = np.einsum("na,nab,nb->n", e, M, e)
    H = b6 = H_abs = b_abs = None
    if derivatives:
        J = np.zeros((len(has), 3, 6), LD)
        J[:, 0, 1], J[:, 0, 2], J[:, 1, 0], J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = -ta[:, 2], ta[:, 1], ta[:, 2], -ta[:, 0], -ta[:, 1], ta[:, 0]
        J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = -1
        H_i = np.einsum("nar,nab,nbc->nrc", J, M, J)
        b_i = np.einsum("nar,nab,nb->nr", J, M, e)
        H, b6, H_abs, b_abs = H_i.sum(0), b_i.sum(0), np.abs(H_i).sum(0), np.abs(b_i).sum(0)
    return dict(H=H, b=b6, err=err_i.sum(), H_abs=H_abs, b_abs=b_abs, err_abs=np.abs(err_i).sum(), n=len(has))


COST_ULPS = 64 + 12  # per component: (64 + 12) 2^-53 sum |addend|; the 12 = shuffle (6), LDS (2) and report-kernel (5) tree depth, rounded up


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' search rule in numpy, with seeded mistakes
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("tie_high", "corr_le", "ring_early", "gap_unshrunk", "tie_stop", "no_carry", "kth_at_k", "mean_by_found", "cov_by_found", "no_sweep")


def cell_of(P, res):
    """pos2grid_ndt: floor(x / res - 0.5) in f32"""
    P = np.asarray(P, F32)
    return np.floor(P[..., :3] / F32(res) - F32(0.5)).astype(np.int64)


def gap_cells(p, res, cell, shrink=True):
    """gicp.hip::cell_gap_cells over the three axes: distance to the nearest face of the own cell in cells, shrunk, not clamped (f32)"""
    x = np.asarray(p, F32)[:3]
    res = F32(res)
    f = x / res - F32(0.5) - cell.astype(F32)
    g = np.minimum(f, F32(1.0) - f)
    if shrink:
        g = g - F32(1e-6) * (F32(1.0) + np.abs(x / res))
    return F32(g.min())


def ring_floor2(r, g, res, mut=None):
    """gicp.hip::ring_floor2: the squared distance below which nothing lies outside ring r; a search stops at a key STRICTLY below it"""
    if mut == "ring_early":
        r = r + 1
    if mut == "tie_stop":  # the rule before: r res + the clamped gap, squared, and stop at <=
        reach = F32(F32(r) * F32(res) + (g * F32(res) if g > 0 else F32(0)))
        return np.nextafter(reach * reach, F32(np.inf))
    reach = F32((F32(r) + g) * F32(res))
    return F32((reach * reach) * (F32(1.0) - F32(4e-6))) if reach > 0 else F32(0)


_SHELLS = {}


def shell(r):
    """the cells of ring r in the order of hashgrid.h::shell_cell: the two z faces, then the perimeter of every layer between them"""
    if r not in _SHELLS:
        if r == 0:
            _SHELLS[r] = np.zeros((1, 3), np.int64)
        else:
            s = 2 * r + 1
            yy, xx = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
            face = np.stack([xx.ravel(), yy.ravel()], 1)
            lo = np.column_stack([face, np.full(len(face), -r)])
            hi = np.column_stack([face, np.full(len(face), r)])
            q = np.arange(8 * r)
            dx = np.where(q < s, q - r, np.where(q < 2 * s, q - s - r, np.where(q - 2 * s >= s - 2, r, -r)))
            w = q - 2 * s
            dy = np.where(q < s, -r, np.where(q < 2 * s, r, w - (w >= s - 2) * (s - 2) - r + 1))
            layers = [np.column_stack([dx, dy, np.full(8 * r, z)]) for z in range(-r + 1, r)]
            _SHELLS[r] = np.concatenate([lo, hi] + layers).astype(np.int64)
            assert len(_SHELLS[r]) == 2 * s * s + (2 * r - 1) * 8 * r
    return _SHELLS[r]


class Grid:
    """cells of a cloud: the points of a cell are contiguous in the given order (as the first batch into an empty device grid is laid out)"""

    def __init__(self, P, res):
        self.P, self.res = np.asarray(P, F32), res
        self.cells = {}
        for i, c in enumerate(map(tuple, cell_of(self.P, res))):
            self.cells.setdefault(c, []).append(i)
        self.cells = {c: np.array(v, np.int64) for c, v in self.cells.items()}
        ks = np.array(list(self.cells), np.int64)
        self.lo, self.hi = ks.min(0), ks.max(0)

    def ring(self, cell, r):
        """index arrays of the occupied cells of ring r around `cell`, in the kernel's order"""
        lo, hi = self.lo - cell, self.hi - cell
        if r > 0 and (np.any(lo > r) or np.any(hi < -r) or r > max(np.abs(lo).max(), np.abs(hi).max())):
            return []  # the ring lies outside the cloud's bounding box, or around it
        sh = shell(r)
        ok = np.all((sh >= lo) & (sh <= hi), axis=1)
        return [self.cells[c] for c in map(tuple, sh[ok] + cell) if c in self.cells]


def _key(d2, idx, tie_high):
    lowbits = (np.uint64(0xFFFFFFFF) - idx.astype(np.uint64)) if tie_high else idx.astype(np.uint64)
    return (np.asarray(d2, F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | lowbits


def _kth(lst, k, mut):
    pos = k - 1
    if mut == "kth_at_k":  # __shfl(e0, k, 16) / __shfl(e1, k - 16, 16): the lane index wraps inside the register
        pos = (k % 16) if k <= 16 else 16 + ((k - 16) % 16)
    return lst[pos]


def _offer(lst, keys, k, mut):
    """one batch of up to sixteen candidates against the stale k-th key"""
    take = keys[keys < _kth(lst, k, mut)]
    if len(take):
        places = 16 if mut == "no_carry" else 32  # without the carry position 16 never receives anything
        lst = np.concatenate([np.sort(np.concatenate([lst[:places], take]))[:places], np.full(32 - places, NONE)])
    return lst


def standin_knn(P, k, res, mut=None, queries=None):
    """[n, 32] int32 lists by the cov kernel's rule, and the [n, 3, 3] long-double C the kernel's division rule gives"""
    P = np.asarray(P, F32)
    grid = Grid(P, res)
    n = len(P)
    out = np.full((n, 32), -1, np.int32)
    tie_high = mut == "tie_high"
    for i in (range(n) if queries is None else queries):
        p = P[i]
        cell = cell_of(p, res)
        gap = gap_cells(p, res, cell, shrink=mut != "gap_unshrunk")
        lst = np.full(32, NONE)

        def offer_all(idx):
            nonlocal lst
            for j0 in range(0, len(idx), 16):
                j = idx[j0:j0 + 16]
                d2 = d2_f32(p[None, :3], P[j])[0]
                lst = _offer(lst, _key(d2, j, tie_high), k, mut)

        within = False
        for r in range(COV_RINGS + 1):
            for idx in grid.ring(cell, r):
                offer_all(idx)
            kth = _kth(lst, k, mut)
            within = kth != NONE and np.uint32(kth >> np.uint64(32)).view(F32) < ring_floor2(r, gap, res, mut)
            if within:
                break
        if not within and mut != "no_sweep":
            lst = np.full(32, NONE)
            offer_all(np.arange(n))
        low = (lst & np.uint64(0xFFFFFFFF)).astype(np.int64)
        if tie_high:
            low = 0xFFFFFFFF - low
        out[i] = np.where(lst != NONE, low, -1)
    return out


def standin_cov(P, k, lists, mut=None, queries=None):
    """the kernel's mean / covariance rule on given [n, 32] lists, long double: sums over the places < k that are filled, divided by k"""
    n = len(P)
    C = np.zeros((n, 3, 3), LD)
    for i in (range(n) if queries is None else queries):
        first = lists[i, :k]
        first = first[first >= 0]
        found = int((lists[i] >= 0).sum())
        nb = P[first, :3].astype(LD)
        m = nb.sum(0) / LD(found if mut == "mean_by_found" else k)
        d = nb - m
        C[i] = d.T @ d / LD(found if mut == "cov_by_found" else k)
    return C


def standin_corr(S, Tg, T, max_corr_dist, res, mut=None):
    """[n_src] int32 by the corr kernel's rule"""
    Tg = np.asarray(Tg, F32)
    grid = Grid(Tg, res)
    with np.errstate(invalid="ignore", over="ignore"):
        q = OG.transform_f(T, S)
    m2 = np.float64(max_corr_dist) * np.float64(max_corr_dist)
    max_d2 = F32(3.0e38) if m2 > 3.0e38 else F32(m2)
    tie_high = mut == "tie_high"
    out = np.full(len(S), -1, np.int32)
    for i, p in enumerate(q):
        if not np.all(np.abs(p) <= np.finfo(F32).max):
            continue
        cell = cell_of(p, res)
        gap = gap_cells(p, res, cell, shrink=mut != "gap_unshrunk")
        bk = NONE

        def best_of(idx, bk):
            d2 = d2_f32(p[None], Tg[idx])[0]
            keys = _key(d2, idx, tie_high)[~np.isnan(d2)]
            return min(bk, keys.min()) if len(keys) else bk

        settled = False
        for r in range(CORR_RINGS + 1):
            for idx in grid.ring(cell, r):
                bk = best_of(idx, bk)
            floor2 = ring_floor2(r, gap, res, mut)
            settled = (bk != NONE and np.uint32(bk >> np.uint64(32)).view(F32) < floor2) or floor2 > max_d2
            if settled:
                break
        if not settled and mut != "no_sweep":
            bk = best_of(np.arange(len(Tg)), bk)
        if bk == NONE:
            continue
        best = np.uint32(bk >> np.uint64(32)).view(F32)
        low = int(bk & np.uint64(0xFFFFFFFF))
        if tie_high:
            low = 0xFFFFFFFF - low
        if (best <= max_d2) if mut == "corr_le" else (best < max_d2):
            out[i] = low
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _cloud(xyz):
    xyz = np.asarray(xyz, np.float64)
    return np.column_stack([xyz, np.zeros(len(xyz))]).astype(F32)


def pose(rotvec, t):
    T = OG.se3_exp(np.concatenate([np.asarray(rotvec, np.float64), np.zeros(3)]))
    T[:3, 3] = t
    return T


POSE_A = pose([0.02, -0.03, 0.05], [0.05, -0.04, 0.02])
POSE_B = pose([0.021, -0.028, 0.052], [0.06, -0.06, 0.025])


def _case(name, target, source, k, res, T=None, maxd=2.0, **more):
    return dict(name=name, target=_cloud(target), source=_cloud(source), k=k, res=res, T=np.eye(4) if T is None else T, maxd=maxd, **more)


K_EDGE_KS, K_EDGE_GRIDS = (3, 15, 16, 17, 31, 32), (0.25, 1.0, 4.0)


def k_edges(k, res):
    """1: one uniform cloud of 600 points in a 6 m box; at 4.0 the cells hold more than 32 points, at 0.25 a query needs many rings"""
    rng = np.random.default_rng(101)
    tgt = rng.uniform(0, 6, (600, 3))
    src = rng.uniform(0, 6, (150, 3))
    return _case(f"k_edges/k{k}/g{res}", tgt, src, k, res, POSE_A)


def n_edges(k, extra):
    """2: n = k and n = k + 1 points over several cells"""
    rng = np.random.default_rng(200 + k + extra)
    return _case(f"n_edges/k{k}/n{k + extra}", rng.uniform(-2, 2, (k + extra, 3)), rng.uniform(-2, 2, (k + extra, 3)), k, 1.0, POSE_A)


def lattice(res, k):
    """3: every coordinate on a cell face (m + 0.5) res, spacing res, with the two f32 neighbours of every face value; mixed signs; at
    res = 0.3 two more blocks out at x / res = +-333.  Exact ties everywhere.  Source: the cell centres, equidistant from eight corners."""
    r32 = F32(res)
    blocks = [(-2, -2, -2)] if res == 1.0 else [(-2, -2, -2), (331, -2, -1), (-335, -1, -2), (331, 331, -335)]
    pts, cen = [], []
    for bx, by, bz in blocks:
        m = np.stack(np.meshgrid(np.arange(4) + bx, np.arange(4) + by, np.arange(4) + bz, indexing="ij"), -1).reshape(-1, 3)
        face = ((m.astype(F32) + F32(0.5)) * r32).astype(F32)
        pts += [face, np.nextafter(face, F32(np.inf)), np.nextafter(face, F32(-np.inf))]
        cen.append(((m[::3].astype(F32) + F32(1.0)) * r32).astype(F32))
    tgt = np.concatenate(pts)
    rng = np.random.default_rng(300)
    tgt = tgt[rng.permutation(len(tgt))]
    return _case(f"lattice/g{res}/k{k}", tgt, np.concatenate(cen), k, res, None, 2.0 * res)


def duplicates(k=10):
    """4: some points occur 2, k and k + 3 times (k + 3 copies: an all-duplicate list, C = 0)"""
    rng = np.random.default_rng(400)
    base = rng.uniform(-3, 3, (60, 3))
    reps = np.ones(60, int)
    reps[[3, 17, 40]] = 2
    reps[[5, 29]] = k
    reps[[11, 50]] = k + 3
    tgt = np.repeat(base, reps, axis=0)
    tgt = tgt[rng.permutation(len(tgt))]
    src = np.concatenate([np.repeat(base[[5, 11, 20]], 4, axis=0) + 0.01, rng.uniform(-3, 3, (20, 3))])
    return _case(f"duplicates/k{k}", tgt, src, k, 1.0, None, 2.0)


NEAR_DIRS = [(-1, 0, 0), (0, 1, 0), (0, 0, -1), (-1, -1, 0), (1, 0, 1), (0, -1, 1), (-1, -1, -1), (1, 1, 1), (1, -1, 1)]


def near_beats_home():
    """5: queries whose own cell holds far points while a face, edge or corner neighbour cell holds a nearer one (res 1, cell m = [m + 0.5, m + 1.5)).
    Groups 10 cells apart.  k-NN groups (k = 3): the query, two far points in its cell, the near one next door.  1-NN groups: the query is a
    source point; its cell holds one far target point, the cell next door the near one."""
    tgt, src = [], []
    for g, d in enumerate(NEAR_DIRS):
        d = np.array(d, float)
        for kind in (0, 1):
            base = np.array([10.0 * g, 20.0 * kind, 0.0]) + 0.5  # the low corner of a cell
            q = base + 0.5 + 0.4 * d           # 0.1 from the face(s) towards d
            near = q + 0.15 * d                # across them
            far1, far2 = base + 0.5 - 0.1 * d + 0.2 * (d == 0), base + 0.5 - 0.2 * d - 0.25 * (d == 0)
            if kind == 0:
                tgt += [q, far1, far2, near]
            else:
                tgt += [far1, near]
                src.append(q)
    # the far points must be farther than the near one and nearer than one cell + the gap: checked by the CPU test
    rng = np.random.default_rng(500)
    src += list(rng.uniform(-3, -1, (4, 3)) + [0, 0, 50])
    return _case("near_beats_home", np.array(tgt), np.array(src), 3, 1.0, None, 2.0)


def sparse(beyond):
    """6: a cluster of 200 points and one point 40 cells away (k = 20, res 0.5); beyond: also five points 70 cells away, whose lists need
    fifteen points of the cluster, past the last ring of the search"""
    rng = np.random.default_rng(600)
    cl = rng.uniform(0, 2, (200, 3))
    pts = [cl, [[23.0, 1.0, 1.0]]]
    if beyond:
        pts.append(np.array([1.0, 36.2, 1.0]) + rng.uniform(0, 0.4, (5, 3)))
    src = np.concatenate([rng.uniform(0, 2, (20, 3)), [[22.5, 1.0, 1.2]]])
    return _case("sparse/" + ("beyond" if beyond else "lone"), np.concatenate(pts), src, 20, 0.5, None, 2.0)


def threshold(which):
    """7: identity pose, max_corr_dist 2.0, a source point at the origin; exact: a target point at exactly (2, 0, 0), d2 == 4.0f, no pair;
    below: at nextafter(2, 0), a pair; tie: two target points at equal d2, the lower index wins.  Pads far outside the threshold."""
    rng = np.random.default_rng(700)  # generic pads: collinear ones on whole numbers would give the oracle an exact eigenvector and E = 0
    pad_t = (rng.uniform(-3, 3, (4, 3)) + [60.0, 50.0, 0.0]).tolist()
    pad_s = (rng.uniform(-3, 3, (3, 3)) + [-60.0, -50.0, 0.0]).tolist()
    two = F32(2.0)
    hit = {"exact": [[two, 0, 0]], "below": [[np.nextafter(two, F32(0)), 0, 0]], "tie": [[0, 1.5, 0], [-1.5, 0, 0], [0, 0, 1.5], [0, -1.5, 0]]}[which]
    tgt = np.array(pad_t[:2] + hit + pad_t[2:], np.float32)
    return _case("threshold/" + which, tgt, np.array([[0, 0, 0]] + pad_s, np.float32), 3, 1.0, None, 2.0)


def no_pairs():
    """8: max_corr_dist = 0"""
    c = n_edges(20, 1)
    c.update(name="no_pairs", maxd=0.0)
    return c


COST_SIZES = (127, 128, 129, 4097)


def cost_sizes(n_src):
    """9: the cost kernel's block edges (128 lanes a block; 4097 rows = 33 partial rows, past the report kernel's 32-lane stride)"""
    rng = np.random.default_rng(900)
    tgt = rng.uniform(0, 6, (500, 3))
    src = np.random.default_rng(900 + n_src).uniform(0, 6, (n_src, 3))
    return _case(f"cost_sizes/{n_src}", tgt, src, 10, 1.0, pose([0.3, -0.2, 0.5], [0.4, -0.3, 0.2]), 2.0, T2=pose([0.31, -0.19, 0.52], [0.38, -0.33, 0.22]))


def far_source():
    """10: no correspondence distance (inf); some source points 20 cells from the nearest target point (res 0.5): past the corr kernel's last ring"""
    rng = np.random.default_rng(1000)
    tgt = rng.uniform(0, 3, (300, 3))
    src = np.concatenate([rng.uniform(0, 3, (30, 3)), [[13.0, 1.0, 1.0], [1.0, -10.0, 2.0], [9.0, 9.5, 10.0], [1.5, 1.5, 13.2]]])
    return _case("far_source", tgt, src, 20, 0.5, POSE_A, np.inf)


def overflow_source():
    """a finite source point whose transformed position overflows f32 under a finite pose (45 degrees about z: s x + c y > FLT_MAX): no pair for
    that row, exact pairs for the rest, max_corr_dist = inf.  Never run against a corr kernel without the entry check."""
    c = far_source()
    src = c["source"].copy()
    src[7, :3] = [3.0e38, 3.0e38, 0.0]
    c.update(name="overflow_source", source=src, T=pose([0, 0, np.pi / 4], [0.1, 0.0, 0.0]), row=7)
    return c


def all_cases():
    """every case the GPU file runs, by name"""
    out = [k_edges(k, g) for k in K_EDGE_KS for g in K_EDGE_GRIDS]
    out += [n_edges(k, e) for k in (20, 32) for e in (0, 1)]
    out += [lattice(1.0, 7), lattice(1.0, 20), lattice(0.3, 7), lattice(0.3, 20)]
    out += [duplicates(), near_beats_home(), sparse(False), sparse(True)]
    out += [threshold(w) for w in ("exact", "below", "tie")]
    out += [no_pairs()] + [cost_sizes(n) for n in COST_SIZES] + [far_source()]
    return out
