"""Cases and references for the point-to-plane kernels of csrc/p2plane.hip alone (tests/test_p2plane_edges_cpu.py,
tests/test_p2plane_edges_gpu.py).  Nothing here imports the library or the oracle: numpy only.  Where a case needs the reference's plane fit
(the bisection of case 2) the caller hands it in as a function.

A case is a map cloud, a list of downsampled body points, a state and, per body point, tags saying what the point is there for:
  kind    "gate" (a +-32 ulp sweep of the residual gate), "gate0" (the same over a plane through the world origin), "origin" (the body origin),
          "thresh" (a cluster whose fifth point sits near esti_plane's 0.1 m threshold), "rank:<name>", "count:<k>", "tilt"
  group   the sweep / cluster the point belongs to
  step    the position inside a sweep (ulps from its centre), else 0
  want5   the point is meant to find exactly five neighbours
  height  the designed signed distance from the cluster's plane (0 where that has no meaning)

Geometry (unless a case says otherwise): map resolution 0.5 (the map keys a point by round(x / res): the cell of an integer coordinate c is
[c - 0.25, c + 0.25)), stencil 19, clusters of five points centred on lattice nodes with odd integer coordinates (2 m apart: no stencil
sees two clusters; the few nodes off that lattice are checked for the same), in-plane offsets (+-0.1, +-0.1) and (0.02, 0.03).

  world()            cases 1, 3, 4, 5 and the step-0 clusters of case 2 in ONE map, identity pose -- or, with a pose, cases 1 and 5 seen
                     through it (case 6: the body points are the inverse transform of the world points in f64)
  thresh_steps()     case 2: 41 small cases, step k = the fifth neighbour k f32 ulps past the last value the reference accepts
  tail_cloud()       case 7: the distinct points repeated cyclically to length n, rotated so that a given point comes last
  classify_case()    case 8: a small map of units, one per branch of map_incremental's rule, and n distinct points on fine lattices
  gate / classify_rule / degeneracy_sums / rows_*   plain restatements
"""
import math

import numpy as np

F32 = np.float32
LD = np.longdouble
U = 2.0 ** -53
RES = 0.5
STENCIL = 19
OFFS = np.array([[0.1, 0.1], [0.1, -0.1], [-0.1, 0.1], [-0.1, -0.1], [0.02, 0.03]])
Q_UV = (0.013, -0.007)  # in-plane offset of a query from its cluster's centre: no two neighbours at one distance
TAIL_SIZES = (1, 2, 63, 64, 65, 2047, 2048, 2049, 14336, 14337, 16384, 16385, 30784, 30785)
CLASSIFY_SIZES = (1, 255, 256, 257, 65536, 65537, 65793)
T_CONTRI, T_STRONG = F32(0.1736), F32(0.7070)

POSE6 = dict(pos=(0.37, -0.52, 0.81), q_wi=(0.12, -0.07, 0.31), ril=(-0.05, 0.09, 0.04), til=(0.11, -0.06, 0.23))  # rotation vectors


# ---------------------------------------------------------------------------------------------------------------------------------
# small tools
# ---------------------------------------------------------------------------------------------------------------------------------
def f32_step(x, k):
    """the f32 value(s) k representable steps away from x (k may be an array)"""
    b = np.asarray(x, F32).view(np.int32).astype(np.int64)
    o = np.where(b >= 0, b, -(b & 0x7FFFFFFF)) + np.asarray(k, np.int64)
    return np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32).view(F32)


def quat_from_rotvec(r):
    r = np.asarray(r, np.float64)
    a = np.linalg.norm(r)
    if a == 0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([r / a * math.sin(a / 2), [math.cos(a / 2)]])


def quat_rot(q, v, conj=False):
    """q (xyzw) applied to rows of v, in v's dtype (f64 or long double)"""
    v = np.asarray(v)
    x, y, z, w = [v.dtype.type(c) for c in q]
    if conj:
        x, y, z = -x, -y, -z
    u = np.stack([y * v[..., 2] - z * v[..., 1], z * v[..., 0] - x * v[..., 2], x * v[..., 1] - y * v[..., 0]], -1)
    u = u + u
    c = np.stack([y * u[..., 2] - z * u[..., 1], z * u[..., 0] - x * u[..., 2], x * u[..., 1] - y * u[..., 0]], -1)
    return v + w * u + c


def make_state(pos=(0, 0, 0), q_wi=(0, 0, 0, 1), q_il=(0, 0, 0, 1), t_il=(0, 0, 0)):
    """26 doubles: pos3 rot4(xyzw) R_il4 t_il3 vel3 bg3 ba3 grav3"""
    s = np.zeros(26)
    s[0:3], s[3:7], s[7:11], s[11:14] = pos, q_wi, q_il, t_il
    s[23:26] = (0.0, 0.0, -9.809)
    return s


def pose6_state():
    return make_state(POSE6["pos"], quat_from_rotvec(POSE6["q_wi"]), quat_from_rotvec(POSE6["ril"]), POSE6["til"])


def is_identity(state):
    return np.array_equal(state[:14], make_state()[:14])


def world_to_body(state, pw):
    """inverse of p_w = R_wi (R_il p_b + t_il) + pos, f64"""
    pi = quat_rot(state[3:7], np.asarray(pw, np.float64) - state[0:3], conj=True)
    return quat_rot(state[7:11], pi - state[11:14], conj=True)


def basis(normal):
    """(u, v, n): n the unit normal, u and v span the plane; the axes themselves for an axis-aligned normal"""
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    e = np.zeros(3)
    e[(int(np.argmax(np.abs(n))) + 1) % 3] = 1.0
    u = e - n * np.dot(e, n)
    u /= np.linalg.norm(u)
    return u, np.cross(n, u), n


class Case:
    def __init__(self, name, map_pts, ds, state, tags):
        self.name, self.map, self.ds, self.state = name, map_pts, ds, state
        self.kind, self.group, self.step, self.want5, self.height = tags

    def __len__(self):
        return len(self.ds)

    def idx(self, prefix):
        return np.flatnonzero(np.char.startswith(self.kind, prefix))

    def sweeps(self, prefix):
        """index arrays, one per sweep of exactly that kind, in step order"""
        out = []
        ii = np.flatnonzero(self.kind == prefix)
        for g in np.unique(self.group[ii]):
            j = ii[self.group[ii] == g]
            out.append(j[np.argsort(self.step[j], kind="stable")])
        return out


class _Builder:
    def __init__(self, state):
        self.state = state
        self.map, self.world, self.tags = [], [], []
        self.n_groups = 0

    def cluster(self, pts3):
        """map points; their intensities number them"""
        for p in np.asarray(pts3, np.float64).reshape(-1, 3):
            self.map.append([p[0], p[1], p[2], float(len(self.map) + 1)])

    def group(self):
        self.n_groups += 1
        return self.n_groups - 1

    def query(self, pw3, kind, group, step=0, want5=True, height=0.0):
        self.world.append(np.asarray(pw3, np.float64))
        self.tags.append((kind, group, step, want5, height))

    def body_norm(self, pw3):
        """|p_body| of the f32 body point the world point becomes"""
        pb = world_to_body(self.state, np.asarray(pw3, np.float64)).astype(F32).astype(np.float64)
        return float(np.linalg.norm(pb))

    def finish(self, name):
        w = np.array(self.world, np.float64).reshape(-1, 3)
        pb = w.astype(F32) if is_identity(self.state) else world_to_body(self.state, w).astype(F32)
        ds = np.concatenate([pb, np.arange(len(pb), dtype=F32)[:, None] + F32(1)], 1).astype(F32)
        mp = np.array(self.map, np.float64).reshape(-1, 4).astype(F32)
        t = self.tags
        tags = (np.array([a[0] for a in t], dtype=str), np.array([a[1] for a in t], np.int64), np.array([a[2] for a in t], np.int64),
                np.array([a[3] for a in t], bool), np.array([a[4] for a in t], np.float64))
        return Case(name, mp, ds, self.state, tags)


def cluster_points(node, normal, offs=OFFS, scale=1.0):
    u, v, _ = basis(normal)
    c = np.asarray(node, np.float64)
    return c + scale * (np.asarray(offs)[:, :1] * u + np.asarray(offs)[:, 1:] * v)


def at(node, normal, uv, h):
    u, v, n = basis(normal)
    return np.asarray(node, np.float64) + uv[0] * u + uv[1] * v + h * n


# ---------------------------------------------------------------------------------------------------------------------------------
# the nodes
# ---------------------------------------------------------------------------------------------------------------------------------
Z, X, TILT = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.36, 0.48, 0.8)
# case 1: (node, side of the plane); |p| from 1.1 m to 14 m; the last three lie on z = 0, a plane through the world origin (A n = -1 has no solution)
GATE_NODES = [((0, 0, 1), +1), ((1, 1, 1), -1), ((1, -1, 3), +1), ((-3, 1, -1), +1), ((3, 3, -3), -1), ((-5, -3, 3), -1), ((5, -5, 1), +1),
              ((-7, 5, -1), -1), ((7, 7, 3), +1), ((9, -7, 5), -1), ((-7, -9, -5), +1), ((-9, 9, 1), +1), ((9, 9, 5), -1)]
GATE0_NODES = [((2, 2, 0), +1), ((-4, 0, 0), -1), ((6, -2, 0), +1)]
# case 2: three nodes for each of three orientations
THRESH_NODES = [((3, 1, -3), Z), ((-5, 3, 5), Z), ((7, -7, 1), Z), ((-3, 5, 1), X), ((5, -1, -5), X), ((-7, -3, 3), X),
                ((1, -3, 5), TILT), ((-1, 7, -1), TILT), ((9, 1, 3), TILT)]
FAR_NODES = [(64, -72, 3), (88, 61, -2), (-75, -80, 5)]
_RESERVED = {n for n, _ in GATE_NODES} | {n for n, _ in THRESH_NODES}


def free_nodes(seed=7):
    """the odd-integer lattice inside +-9 m without the nodes named above, in a fixed shuffled order"""
    ax = np.arange(-9, 10, 2)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    g = g[np.random.default_rng(seed).permutation(len(g))]
    return [tuple(int(c) for c in n) for n in g if tuple(int(c) for c in n) not in _RESERVED]


def _gate_sweep(b, kind, node, side, normal=Z):
    """65 queries whose height over the cluster's plane steps by f32 ulps of the stepped coordinate around the solution of h = sqrt(|p_body|) / 9"""
    b.cluster(cluster_points(node, normal))
    g = b.group()
    h = 0.2
    for _ in range(60):  # fixed point; |p| hardly depends on h
        h = math.sqrt(b.body_norm(at(node, normal, Q_UV, side * h))) / 9.0
    p0 = at(node, normal, Q_UV, side * h)
    ax = int(np.argmax(np.abs(basis(normal)[2])))
    for k in range(-32, 33):
        p = p0.copy()
        p[ax] = float(f32_step(F32(p0[ax]), k))
        b.query(p, kind, g, step=k, height=side * h)


def thresh_cluster(node, normal, t=None):
    """the five points (f32) of a case-2 cluster; t = the fifth point's coordinate along the normal's dominant axis (None: on the plane)"""
    p = cluster_points(node, normal).astype(F32)
    if t is not None:
        p[4, int(np.argmax(np.abs(basis(normal)[2])))] = F32(t)
    return p


def _oi(x):
    """f32 -> an integer that orders like the value"""
    b = int(F32(x).view(np.int32))
    return b if b >= 0 else -(b & 0x7FFFFFFF)


def thresh_ordered(node, normal, t, q):
    """the cluster as xyzi rows in the order the search hands the neighbours of query q over, nearest first: the fit's rounding depends on the
    order of its rows"""
    p = thresh_cluster(node, normal, t)
    e = p - np.asarray(q, F32)
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    return np.c_[p[np.argsort(d2, kind="stable")], np.zeros(5, F32)].astype(F32)


def thresh_flip(node, normal, esti_plane, q=None):
    """the last f32 value of the fifth point's stepped coordinate that `esti_plane` (five xyzi rows -> (ok, plane)) accepts next to one it
    rejects, by bisection over the f32 values between a lift of 0.03 m (accepted) and one of 0.45 m (rejected).  (A n = -1 is no orthogonal
    regression: where the fit flips depends on where the cluster lies, 0.06 m to 0.3 m at these nodes.)"""
    _, _, n = basis(normal)
    ax = int(np.argmax(np.abs(n)))
    base = thresh_cluster(node, normal)[4, ax]
    if q is None:
        q = at(node, normal, Q_UV, 0.05)

    def ok(t):
        return esti_plane(thresh_ordered(node, normal, t, q))[0]

    lo, hi = F32(base + 0.03 / n[ax]), F32(base + 0.45 / n[ax])
    assert ok(lo) and not ok(hi), (node, normal)
    sgn = 1 if hi > lo else -1
    while abs(_oi(hi) - _oi(lo)) > 1:
        mid = f32_step(lo, sgn * (abs(_oi(hi) - _oi(lo)) // 2)).reshape(())[()]
        if ok(mid):
            lo = mid
        else:
            hi = mid
    return lo


# a tenth sweep for the comparison itself: a plane 3 cm from the world origin, its fifth neighbour lifted TOWARDS the origin.  Every term of
# v = ((a x + b y) + c z) + d is then smaller than 0.125, so v moves over the same f32 grid 0.1f lies on, in steps of less than one grid point per
# ulp of the lift: some step has |v| == 0.1f exactly, which `fabsf(v) > threshold` accepts.  (At the other nodes |d| >= 1 and v moves in steps of
# 2^-23 or more: it never equals 0.1f.)  Its query sits on the fitted plane, 0.4 m from the origin, where the residual gate is far away.
THRESH_TIE = ((0.0, 0.0, 0.03125), (0.0, 0.0, -1.0))
_TIE_XY = (0.35, 0.2)


def thresh_tie(esti_plane):
    """(the flip of the tie sweep, its query)"""
    node, normal = THRESH_TIE
    q0 = np.array([_TIE_XY[0], _TIE_XY[1], node[2]])
    t = thresh_flip(node, normal, esti_plane, q0)
    pl = esti_plane(thresh_ordered(node, normal, t, q0))[1].astype(np.float64)
    return t, np.array([q0[0], q0[1], -(pl[0] * q0[0] + pl[1] * q0[1] + pl[3]) / pl[2]])


def plane_residuals(plane, five):
    """esti_plane's v of the five neighbours, f32, its order of operations"""
    pl, p = np.asarray(plane, F32), np.asarray(five, F32)
    return ((pl[0] * p[:, 0] + pl[1] * p[:, 1]) + pl[2] * p[:, 2]) + pl[3]


def _thresh_query(b, node, normal, g, k, q=None):
    b.query(at(node, normal, Q_UV, 0.05) if q is None else q, "thresh", g, step=k, height=0.05 if q is None else 0.0)


RANK_SETS = ("collinear", "coincident2", "coincident3", "coincident5", "tie_x", "tie_y", "tie_z", "far0", "far1", "far2", "origin")
Q4 = [((0.013, -0.007), 0.03), ((-0.021, 0.017), -0.04), ((0.034, 0.009), 0.06), ((-0.008, -0.026), -0.02)]


def _rank_cluster(name, node):
    """(points, normal the queries are laid out by)"""
    c = np.asarray(node, np.float64)
    if name == "collinear":
        d = np.array([1.0, 0.5, 0.25])
        return c + np.array([-0.1, -0.05, 0.01, 0.05, 0.1])[:, None] * d, Z
    if name.startswith("coincident"):
        m = int(name[-1])
        p = cluster_points(node, Z)
        p[:m] = p[0]
        return p, Z
    if name.startswith("tie_"):
        # dyadic offsets: every square and every partial sum of a column's norm is exact in f32, and the two in-plane columns hold the same
        # values in another order -> two columns of exactly equal norm, whatever order the neighbours arrive in (the strict `>` keeps the first)
        nrm = {"x": X, "y": (0.0, 1.0, 0.0), "z": Z}[name[-1]]
        offs = np.array([[0.125, 0.125], [0.125, -0.125], [-0.125, 0.125], [-0.125, -0.125], [0.0625, 0.0625]])
        return cluster_points(node, nrm, offs), nrm
    if name.startswith("far"):
        return cluster_points(node, TILT, scale=0.1), TILT  # 1 cm spread at 60 - 90 m: the norm downdate branch t2 <= sqrt(eps)
    if name == "origin":
        # holds the world origin and is symmetric about it: sum p = 0, so the least-squares normal is 0 and the "plane" 0 / 0
        return np.array([[0.125, 0.125, 0], [0.125, -0.125, 0], [-0.125, 0.125, 0], [-0.125, -0.125, 0], [0, 0, 0]], np.float64), Z
    raise KeyError(name)


COUNTS = (0, 1, 2, 3, 4, 5, 8)
OFFS8 = np.concatenate([OFFS, [[0.05, -0.08], [-0.06, 0.04], [0.0, -0.12]]])
N_TILT = 200


def world(state=None, esti_plane=None):
    """cases 1, 3, 4, 5 and (given `esti_plane`) the step-0 clusters of case 2, identity pose; with a state: cases 1 and 5 through that pose"""
    ident = state is None
    b = _Builder(make_state() if ident else state)
    for node, side in GATE_NODES:
        _gate_sweep(b, "gate", node, side)
    for node, side in GATE0_NODES:
        _gate_sweep(b, "gate0", node, side)
    free = free_nodes()
    if ident:
        if esti_plane is not None:
            for node, normal in THRESH_NODES:
                b.cluster(thresh_cluster(node, normal, thresh_flip(node, normal, esti_plane)))
                _thresh_query(b, node, normal, b.group(), 0)
        for name in RANK_SETS:
            node = (0, 0, 0) if name == "origin" else FAR_NODES[int(name[-1])] if name.startswith("far") else free.pop()
            pts, nrm = _rank_cluster(name, node)
            b.cluster(pts)
            g = b.group()
            for uv, h in Q4:
                b.query(at(node, nrm, uv, h), "rank:" + name, g, height=h)
            if name == "origin":
                b.query((0.0, 0.0, 0.0), "origin", g)  # sqrt(|p_body|) = 0: a division by zero in the gate
        for k in COUNTS:
            node = free.pop()
            b.cluster(cluster_points(node, Z, OFFS8[:k]))
            g = b.group()
            for uv, h in Q4:
                b.query(at(node, Z, uv, h), "count:%d" % k, g, want5=k >= 5, height=h)
    rng = np.random.default_rng(11)
    for j in range(N_TILT):
        node = free.pop()
        nrm = rng.normal(size=3)
        b.cluster(cluster_points(node, nrm))
        h = 0.07 if j == 0 else float(rng.uniform(-0.08, 0.08))  # (the first one is the designated last point of the tails: |residual| > 0.05)
        b.query(at(node, nrm, Q_UV, h), "tilt", b.group(), height=h)
    if not ident:
        b.world.append(np.asarray(quat_rot(b.state[3:7], b.state[11:14]) + b.state[0:3]))  # the body origin, wherever the pose puts it
        b.tags.append(("origin", b.group(), 0, False, 0.0))
    case = b.finish("world" if ident else "world_pose")
    case.ds[case.idx("origin"), :3] = 0.0  # exactly
    return case


def thresh_steps(esti_plane, steps=range(-20, 21)):
    """case 2: one small case per step k; in it every (node, orientation), and the tie sweep last, has its fifth neighbour k f32 ulps beyond the
    last accepted value (the way a lift grows), so step 0 is accepted and step 1 rejected"""
    flips = [(node, normal, thresh_flip(node, normal, esti_plane), None) for node, normal in THRESH_NODES]
    flips.append(THRESH_TIE + thresh_tie(esti_plane))
    out = []
    for k in steps:
        b = _Builder(make_state())
        for node, normal, t, q in flips:
            n = basis(normal)[2]
            sgn = 1 if n[int(np.argmax(np.abs(n)))] > 0 else -1
            b.cluster(thresh_cluster(node, normal, f32_step(t, sgn * k).reshape(())[()]))
            _thresh_query(b, node, normal, b.group(), k, q)
        out.append(b.finish("thresh[%+d]" % k))
    return out


def tail_cloud(ds, n, last):
    """the points repeated cyclically to length n, rotated so that point `last` of ds is point n - 1"""
    return np.ascontiguousarray(ds[(np.arange(n) - (n - 1) + last) % len(ds)])


# ---------------------------------------------------------------------------------------------------------------------------------
# case 8: map_incremental
# ---------------------------------------------------------------------------------------------------------------------------------
BRANCHES = ("no_neighbour", "far_all_axes", "exact_half", "lt5_kept", "five_dropped", "five_tie_kept")
_UNIT_TYPES = ("none", "far", "exact", "lt5_1", "lt5_2", "lt5_3", "lt5_4", "five")
_UNIT_BASES = [(0, 0, 0), (4, 0, 0), (0, 4, 0), (4, 4, 0), (0, 0, 4), (4, 0, 4), (0, 4, 4), (4, 4, 4),
               (-4, -4, -4), (-8, -4, -4), (-4, -8, -4), (-8, -8, -4), (-4, -4, -8), (-8, -4, -8), (-4, -8, -8), (-8, -8, -8)]
_N_TIE = 16
_LAT, _LAT_STEP = 17, 2.0 ** -11  # 17^3 = 4913 distinct points per unit, in a cube of 8 mm


def _unit_map(kind, base):
    """map points of one unit, relative to the leaf cell [base, base + 0.5)^3 whose centre is base + 0.25; the unit's points sit in the cell's
    far corner (0.48 .. 0.49 on every axis), 0.4 m from the centre"""
    far = [(0.51, 0.512, 0.511), (0.55, 0.56, 0.57), (0.56, 0.52, 0.53), (0.53, 0.57, 0.52), (0.58, 0.54, 0.59)]
    near = [(0.35, 0.36, 0.34), (0.40, 0.45, 0.43), (0.44, 0.41, 0.46), (0.46, 0.44, 0.42), (0.42, 0.46, 0.45)]
    if kind == "none":
        p = []
    elif kind == "far":  # all five beyond the corner: the nearest is more than half a leaf from the centre on all three axes
        p = far
    elif kind == "exact":  # the nearest sits at EXACTLY half a leaf on x (strict comparison: not "far"), and a neighbour nearer to the centre drops the point
        p = [(0.5, 0.512, 0.511), near[0]] + far[2:]
    elif kind.startswith("lt5"):  # 1 .. 4 neighbours, the first nearer to the centre than the point: kept all the same
        p = near[:int(kind[-1])]
    else:  # five neighbours inside the cell, one nearer to the centre: dropped
        p = near
    return np.asarray(base, np.float64) + np.array(p, np.float64).reshape(-1, 3)


def classify_case(n):
    """n distinct points: first the `five_tie_kept` cells (one point each: its mirror image through the cell's centre is a map point, so
    dq == dist exactly), then the units' lattices in turn"""
    mp, pts = [], []
    for t in range(_N_TIE):
        base = np.array([12.0 + 2 * (t % 4), 2.0 * (t // 4) - 3.0, -6.0])
        mid = base + 0.25
        # dyadic: +-d about the centre is exact in f32.  The centre of a leaf cell is a CORNER of the map's cells (keys round, leaves floor), and the
        # stencil of 19 has no corner cells: d and the other neighbours stay in the plane z = centre so that everything is a face or edge cell away
        d = np.array([0.0625 + 2.0 ** -7 * t, 0.03125 + 2.0 ** -8 * t, 0.0])
        mp += [mid - d, mid + (0.2, 0.19, 0.0), mid + (0.21, -0.2, 0.0), mid + (-0.2, 0.21, 0.0), mid + (0.19, 0.22, 0.0)]
        pts.append(mid + d)
    for u, base in enumerate(_UNIT_BASES):
        mp += list(_unit_map(_UNIT_TYPES[u % len(_UNIT_TYPES)], base))
    nu = len(_UNIT_BASES)
    i = np.arange(max(n - _N_TIE, 0))
    u, l = i % nu, i // nu
    assert l.size == 0 or l.max() < _LAT ** 3
    lat = np.stack([l % _LAT, (l // _LAT) % _LAT, l // (_LAT * _LAT)], 1) * _LAT_STEP + 0.48
    fill = np.asarray(_UNIT_BASES, np.float64)[u] + lat
    w = np.concatenate([np.array(pts).reshape(-1, 3), fill])[:n]
    ds = np.concatenate([w, np.arange(n)[:, None] + 1000.0], 1).astype(F32)
    mpa = np.array(mp, np.float64).reshape(-1, 3)
    mpa = np.concatenate([mpa, np.arange(len(mpa))[:, None] + 1.0], 1).astype(F32)
    assert len(np.unique(ds[:, :3], axis=0)) == n
    return mpa, ds


def classify_rule(pw, nn, cnt, leaf=0.5, ekf_inited=True):
    """map_incremental's decision per point (laserMapping.cpp:523-563) from the world point (f32), its neighbours [n, 5, >=3] and their count:
    (class 0 dropped / 1 PointToAdd / 2 PointNoNeedDownsample, branch name)"""
    pw, nn = np.asarray(pw, F32)[:, :3], np.asarray(nn, F32)[:, :, :3]
    n = len(pw)
    fs = np.float64(F32(leaf))
    mid = (np.floor(pw.astype(np.float64) / fs) * fs + 0.5 * fs).astype(F32)

    def d2(a):
        e = a - mid
        return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]  # f32, calc_dist's order

    dist = d2(pw)
    half = 0.5 * fs
    a0 = np.abs((nn[:, 0] - mid).astype(np.float64))
    far = np.all(a0 > half, axis=1)
    exact = ~far & np.all(a0 >= half, axis=1)
    dq = np.stack([d2(nn[:, k]) for k in range(5)], 1)
    have = np.arange(5)[None, :] < np.asarray(cnt)[:, None]
    nearer = np.any((dq < dist[:, None]) & have, axis=1)
    tie = ~nearer & np.any((dq == dist[:, None]) & have, axis=1)
    cls = np.ones(n, np.int64)
    branch = np.full(n, "kept", dtype="U16")
    judged = (cnt > 0) & bool(ekf_inited)
    branch[~judged] = "no_neighbour" if ekf_inited else "not_inited"
    cls[judged & far] = 2
    branch[judged & far] = "far_all_axes"
    rest = judged & ~far
    cls[rest & (cnt >= 5) & nearer] = 0
    branch[rest & (cnt < 5) & nearer] = "lt5_kept"
    branch[rest & (cnt >= 5) & nearer] = "five_dropped"
    branch[rest & (cnt >= 5) & tie] = "five_tie_kept"
    branch[rest & exact & (cnt >= 5) & nearer] = "exact_half"
    return cls, branch


# ---------------------------------------------------------------------------------------------------------------------------------
# restatements of the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def gate(plane, pw, pb):
    """the residual gate of laserMapping.cpp:860-871 given the fitted plane(s) [n, 4] f32, world and body points (f32):
    pd2 = ((a x + b y) + c z) + d in f32; s = float(1 - 0.9 |pd2| / sqrt(|p_body|)) with the right side in f64; selected iff s > 0.9"""
    plane, pw, pb = np.asarray(plane, F32).reshape(-1, 4), np.asarray(pw, F32).reshape(-1, 4)[:, :3], np.asarray(pb, F32).reshape(-1, 4)[:, :3]
    with np.errstate(all="ignore"):
        pd2 = ((plane[:, 0] * pw[:, 0] + plane[:, 1] * pw[:, 1]) + plane[:, 2] * pw[:, 2]) + plane[:, 3]
        b = pb.astype(np.float64)
        pbn = np.sqrt(b[:, 0] * b[:, 0] + (b[:, 1] * b[:, 1] + b[:, 2] * b[:, 2]))
        sc = (1 - 0.9 * np.abs(pd2.astype(np.float64)) / np.sqrt(pbn)).astype(F32)
        return sc.astype(np.float64) > 0.9, pd2


def degeneracy_sums(normvec, V):
    """the six sums of laserMapping.cpp:946-964 over the rows of normvec (the selected points' planes, f32) against the columns of V: normalise in
    f64, dot, cast to f32, compare with 0.1736f / 0.7070f, add the f32 values widened to f64 (exact: the order of addition cannot matter).
    Returns (contri[3], strong[3], dotp[n, 3] f32)"""
    f = np.asarray(normvec, F32)[:, :3].astype(np.float64)
    V = np.asarray(V, np.float64).reshape(3, 3)
    nn = np.sqrt(f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2])
    with np.errstate(all="ignore"):
        f = np.where((nn > 0)[:, None], f / nn[:, None], f)
    dot = np.stack([np.abs(f[:, 0] * V[0, e] + f[:, 1] * V[1, e] + f[:, 2] * V[2, e]) for e in range(3)], 1).astype(F32)
    contri = np.array([math.fsum(dot[dot[:, e] > T_CONTRI, e].astype(np.float64)) for e in range(3)])
    strong = np.array([math.fsum(dot[dot[:, e] > T_STRONG, e].astype(np.float64)) for e in range(3)])
    return contri, strong, dot


def rows_identity(normvec, ds):
    """Jacobian rows (n, p x n) and h = -pd2 under the identity pose, f64.  Every entry is ONE correctly rounded f64 operation on exact products
    of f32 values (p_imu = p_body and C = n exactly), so these have the device's bits"""
    n = np.asarray(normvec, F32).astype(np.float64)
    p = np.asarray(ds, F32)[:, :3].astype(np.float64)
    row = np.stack([n[:, 0], n[:, 1], n[:, 2], p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                    p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0]], 1)
    return row, -n[:, 3]


def rows_longdouble(normvec, ds, state):
    """rows, h and the magnitudes M of the allowance under any pose, long double: (n, p_imu x (R_wi^T n)), p_imu = R_il p + t_il;
    M = 1 for the normal columns, 2 |p_imu| for the cross-product columns, |pd2| for the residual"""
    n = np.asarray(normvec, F32).astype(LD)
    p = np.asarray(ds, F32)[:, :3].astype(LD)
    pi = quat_rot(state[7:11], p) + state[11:14].astype(LD)
    c = quat_rot(state[3:7], n[:, :3], conj=True)
    row = np.concatenate([n[:, :3], np.cross(pi, c)], 1)
    pn = np.sqrt((pi * pi).sum(1))
    M = np.stack([np.ones_like(pn)] * 3 + [2 * pn] * 3, 1)
    return row, -n[:, 3], M, np.abs(n[:, 3])


def sums_exact(row, h, sel):
    """exactly rounded sums (math.fsum) of the addends row[a] row[c], row[a] h, |h| over the selected points, and the sums of |addend|:
    (JtJ[6, 6], Jtr[6], sum_abs_res), (the same of |addend|)"""
    r, hh = np.asarray(row, np.float64)[sel], np.asarray(h, np.float64)[sel]
    J, Ja, g, ga = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros(6), np.zeros(6)
    for a in range(6):
        for c in range(6):
            t = r[:, a] * r[:, c]
            J[a, c], Ja[a, c] = math.fsum(t), math.fsum(np.abs(t))
        t = r[:, a] * hh
        g[a], ga[a] = math.fsum(t), math.fsum(np.abs(t))
    s = math.fsum(np.abs(hh))
    return (J, g, s), (Ja, ga, s)


def gamma(n):
    """Higham's gamma_{n-1}: the bound on |computed - exact| / sum |addend| of ANY order of adding n numbers in f64"""
    return (n - 1) * U / (1 - (n - 1) * U) if n > 1 else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# driving the CPU oracle (handed in by the caller: this module imports nothing of the project)
# ---------------------------------------------------------------------------------------------------------------------------------
def oracle_engine(oracle_mod, map_pts, state, ekf_inited=True):
    o = oracle_mod.Lio(res=RES, stencil=STENCIL, capacity=1 << 40, threads=4)
    o.map_add(map_pts)
    o.set_state(state)
    o.set_flags(ekf_inited=ekf_inited, first_scan=False)
    return o


def oracle_pass(o, converge=True):
    """one h_share_model_geometric of the oracle + the world points it left"""
    r = o.linearize(converge=converge)
    r["world"] = o.get_ds_world()
    return r


def oracle_search(oracle_mod, case):
    o = oracle_engine(oracle_mod, case.map, case.state)
    o.set_ds(case.ds)
    return o, oracle_pass(o, True)


def rows_u32(a):
    """rows of an [n, 4] f32 array as sortable records of their bits"""
    return np.sort(np.ascontiguousarray(a, F32).view(np.uint32).view([("a", np.uint32, 4)]).ravel(), order="a")


def classify_oracle(oracle_mod, n, ekf_inited=True):
    """case 8 through the oracle: search at the identity state, then map_incremental; (map, ds, results)"""
    mp, ds = classify_case(n)
    o = oracle_engine(oracle_mod, mp, make_state(), ekf_inited=ekf_inited)
    o.set_ds(ds)
    r = oracle_pass(o, True)
    r["n_add"] = o.map_incremental()
    r["dump"] = o.map_dump().copy()
    r["stats"] = (o.map_num_points, o.map_num_voxels)
    return mp, ds, r
