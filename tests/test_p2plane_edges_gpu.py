"""The kernels of csrc/p2plane.hip alone, at their gates, ties and tails, on a real MI355X: linearize_kernel (the 5 x 3 QR, the plane threshold,
the residual gate), the pass that does not search, the quad / LDS reduction and finalize_kernel's fold, degeneracy_kernel, classify_kernel and
classify_scatter_kernel -- on the constructed cases of tests/p2plane_edge_cases.py, against the CPU oracle and plain numpy restatements.

Per-point results (neighbours, plane, gate, world point) are compared bit for bit.  Sums are compared with an allowance DERIVED from the
arithmetic, never with a relative tolerance: under the identity pose every addend has the device's bits and only the order of addition differs
(gamma_{n-1} sum |addend|); under a general pose (n + 64) u sum M M with the magnitudes M of p2plane_edge_cases.rows_longdouble.
Worst err / allowance measured on the MI355X: see docs/kernels.md, "what the point-to-plane tests pin"."""
import ctypes as C

import numpy as np
import pytest

import p2plane_edge_cases as E

pytestmark = pytest.mark.gpu


def _dev():
    from lsd_amd import capi

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _map(pts, max_points=8192, max_voxels=8192):
    from lsd_amd import lio

    m = lio.Map(resolution=E.RES, stencil=E.STENCIL, max_points=max_points, max_voxels=max_voxels)
    if len(pts):
        m.add(pts)
    return m


@pytest.fixture(scope="module")
def W(oracle_mod):
    return E.world(esti_plane=oracle_mod.esti_plane)


@pytest.fixture(scope="module")
def Wref(oracle_mod, W):
    return E.oracle_search(oracle_mod, W)[1]


@pytest.fixture(scope="module")
def P(oracle_mod):
    return E.world(state=E.pose6_state())


def _check_points(case, ref, got, mt, world, ds=None):
    """device against oracle, per point, bit for bit"""
    name = case if isinstance(case, str) else case.name
    assert got["n_ds"] == len(ref["selected"]), name
    assert np.array_equal(ref["nn_cnt"], mt["nn_cnt"]), name
    have = np.arange(5)[None, :] < ref["nn_cnt"][:, None]
    assert np.array_equal(_u32(ref["nn"][..., :3])[have], _u32(mt["nn"][..., :3])[have]), name
    assert np.array_equal(ref["selected"], mt["selected"]), (name, np.flatnonzero(ref["selected"] != mt["selected"])[:8])
    sel = ref["selected"].astype(bool)
    assert np.array_equal(_u32(ref["normvec"][sel]), _u32(mt["normvec"][sel])), name  # plane and .w = pd2
    assert got["n_eff"] == ref["n_eff"] == int(sel.sum()), name
    assert np.array_equal(_u32(ref["world"]), _u32(world)), name


def _run(lio, m, s, state, redo_knn=True):
    got = lio.linearize(m, s, state, redo_knn=redo_knn)
    return got, s.get_match(), s.get_world()


def _ratio(err, allow):
    """worst err / allowance; a component whose allowance is 0 (all addends 0) must be exact"""
    err, allow = np.abs(np.asarray(err, np.float64)).ravel(), np.asarray(allow, np.float64).ravel()
    assert np.all(err[allow == 0] == 0)
    return float(np.max(err[allow > 0] / allow[allow > 0])) if np.any(allow > 0) else 0.0


def _check_sums_identity(got, mt, ds):
    """JtJ (all 36), Jtr, nnT and sum_abs_res against math.fsum over addends that have the device's bits; returns the worst err / allowance"""
    sel = mt["selected"].astype(bool)
    n = len(ds)
    assert got["n_ds"] == n and got["n_eff"] == int(sel.sum())
    row, h = E.rows_identity(mt["normvec"], ds)
    (J, g, sres), (Ja, ga, sa) = E.sums_exact(row, h, sel)
    gam = E.gamma(n)
    assert np.array_equal(got["JtJ"], got["JtJ"].T)
    return max(_ratio(got["JtJ"] - J, gam * Ja), _ratio(got["Jtr"] - g, gam * ga), _ratio(got["nnT"] - J[:3, :3], gam * Ja[:3, :3]),
               _ratio(got["sum_abs_res"] - sres, gam * sa))


def test_points_match_the_oracle_cases_1_to_5(oracle_mod, W, Wref):
    """cases 1, 3, 4, 5 (and step 0 of case 2) in one map, identity pose: neighbour counts, neighbour bits, the gate, plane and residual bits,
    N_eff and the world points.  Pinned on the way, because the REFERENCE does it (tests/test_p2plane_edges_cpu.py): collinear and coincident
    neighbours are accepted; a not-finite plane passes the 0.1 m test and fails the gate; the body origin divides by zero and is not selected."""
    _dev()
    from lsd_amd import lio

    m, s = _map(W.map), lio.Scan(max_raw=1 << 14, max_ds=1 << 14)
    s.set_ds(W.ds)
    got, mt, world = _run(lio, m, s, W.state)
    _check_points(W, Wref, got, mt, world)
    for k in (0, 1, 2, 3, 4):
        assert not mt["selected"][W.idx("count:%d" % k)].any()
    assert not mt["selected"][W.idx("origin")].any() and not mt["selected"][W.idx("rank:origin")].any()
    import ref as refmod

    if refmod.available():  # where device and oracle agree they also agree with the reference's own esti_plane
        for i in np.concatenate([W.idx("rank:"), W.idx("thresh")]):
            ok, plane = refmod.esti_plane(mt["nn"][i])
            if mt["selected"][i]:
                assert ok and np.array_equal(_u32(plane[:3]), _u32(mt["normvec"][i, :3])), (W.kind[i], plane, mt["normvec"][i])


def test_plane_threshold_sweep(oracle_mod):
    """case 2: the fifth neighbour +-20 f32 ulps around the lift at which the reference's esti_plane flips (bisected on the oracle), three nodes
    for each of a z-normal, an x-normal and a tilted plane, and the sweep next to the origin in which some step has |v| == 0.1f exactly (accepted:
    the comparison is `>`): the device flips where the oracle does, step by step"""
    _dev()
    from lsd_amd import lio

    import ref as refmod

    steps = E.thresh_steps(oracle_mod.esti_plane)
    m, s = _map([]), lio.Scan(max_raw=1 << 12, max_ds=1 << 12)
    sel = []
    for case in steps:
        ref = E.oracle_search(oracle_mod, case)[1]
        m.clear()
        m.add(case.map)
        s.set_ds(case.ds)
        got, mt, world = _run(lio, m, s, case.state)
        _check_points(case, ref, got, mt, world)
        assert _check_sums_identity(got, mt, case.ds) < 1.0
        sel.append(mt["selected"])
        if refmod.available():
            for i in range(len(case)):
                ok, plane = refmod.esti_plane(mt["nn"][i])
                assert ok == bool(mt["selected"][i])  # (the queries sit 5 cm off the plane: the residual gate is far away)
    sel = np.array(sel)
    assert np.all(sel.sum(0) > 0) and np.all(sel.sum(0) < len(steps))  # both outcomes at every (node, orientation)


def test_points_and_sums_through_a_pose(oracle_mod, P):
    """case 6: cases 1 and 5 through a generic pose and extrinsics.  Per point as above; the sums against long-double rows built from the
    downloaded planes with the allowance (n + 64) u sum_j M_ja M_jc, M = 1 for the normal columns, 2 |p_imu| for the cross-product columns and
    |pd2| for the residual (64: more than the f64 operations behind one row entry); lio_p2plane_rows against the same rows within 64 u M"""
    _dev()
    from lsd_amd import capi, lio

    ref = E.oracle_search(oracle_mod, P)[1]
    m, s = _map(P.map), lio.Scan(max_raw=1 << 14, max_ds=1 << 14)
    s.set_ds(P.ds)
    got, mt, world = _run(lio, m, s, P.state)
    _check_points(P, ref, got, mt, world)
    sel = mt["selected"].astype(bool)
    n = len(P)
    row, h, M, Mh = E.rows_longdouble(mt["normvec"], P.ds, P.state)
    r, hh, Ms, Mhs = row[sel], h[sel], M[sel], Mh[sel]
    k = (n + 64) * E.U
    J = np.array([[(r[:, a] * r[:, c]).sum() for c in range(6)] for a in range(6)])
    Ja = np.array([[(Ms[:, a] * Ms[:, c]).sum() for c in range(6)] for a in range(6)], np.float64)
    g = np.array([(r[:, a] * hh).sum() for a in range(6)])
    ga = np.array([(Ms[:, a] * Mhs).sum() for a in range(6)], np.float64)
    worst = max(_ratio((got["JtJ"].astype(E.LD) - J).astype(np.float64), k * Ja), _ratio((got["Jtr"].astype(E.LD) - g).astype(np.float64), k * ga),
                _ratio((got["nnT"].astype(E.LD) - J[:3, :3]).astype(np.float64), k * Ja[:3, :3]),
                _ratio(float(E.LD(got["sum_abs_res"]) - np.abs(hh).sum()), k * float(Mhs.sum())))
    print(f"\n[p2plane edges] pose: n={n} n_eff={got['n_eff']} worst err/allowance = {worst:.4f}")
    assert worst < 1.0
    # the rows the host forms for the N_eff < 23 path
    pose, ext = lio._pose_ext(P.state)
    rows, hv = np.zeros((n, 6)), np.zeros(n)
    cnt = capi.check(capi.lib().lio_p2plane_rows(s.h, capi.ptr(pose, C.c_double), capi.ptr(ext, C.c_double), capi.ptr(rows, C.c_double),
                                                  capi.ptr(hv, C.c_double), n), "rows")
    assert cnt == int(sel.sum())
    wr = _ratio((rows[:cnt].astype(E.LD) - r).astype(np.float64), 64 * E.U * Ms.astype(np.float64))
    print(f"[p2plane edges] pose: lio_p2plane_rows worst err / (64 u M) = {wr:.4f}")
    assert wr < 1.0 and np.array_equal(hv[:cnt], hh.astype(np.float64))


def test_sums_at_the_tails(oracle_mod, W, Wref):
    """cases 1-5 and every size of case 7 (the distinct points repeated to length n; nb = ceil(n / 64) = 1, 2, 32, 33, 224, 225, 256, 257, 481,
    482: the edges of fold_partials' eight-deep loop and of its guarded tail).  Point n - 1 is selected with |residual| > 0.05, so a lane beyond n
    -- its loads are clamped to point n - 1 -- that contributed would change N_eff.  The sizes run from the largest down on ONE scan: the
    partial sums of the blocks beyond nb are then those of a larger cloud, not zeros, and a fold that read one of them shows.
    Identity pose: every Jacobian entry is one correctly rounded f64 operation on exact products of f32 values, so rows, addends and |r| built in
    numpy from the (bit-equal) planes have the device's bits; only the order of addition differs.  Reference: math.fsum; allowance: gamma_{n-1}
    sum |addend| per component, u = 2^-53.  No rtol."""
    _dev()
    from lsd_amd import lio

    m, s = _map(W.map), lio.Scan(max_raw=1 << 15, max_ds=1 << 15)
    o = E.oracle_engine(oracle_mod, W.map, W.state)
    last = W.idx("tilt")[0]
    worst = {}
    for n in sorted(E.TAIL_SIZES, reverse=True) + [len(W)]:
        ds = W.ds if n == len(W) else E.tail_cloud(W.ds, n, last)
        o.set_ds(ds)
        ref = E.oracle_pass(o, True)
        s.set_ds(ds)
        got, mt, world = _run(lio, m, s, W.state)
        _check_points("tail[%d]" % n, ref, got, mt, world)
        if n != len(W):
            assert mt["selected"][n - 1] == 1 and abs(mt["normvec"][n - 1, 3]) > 0.05
        worst[n] = _check_sums_identity(got, mt, ds)
    print("\n[p2plane edges] tails: worst err/allowance per n: " + ", ".join(f"{n}: {worst[n]:.4f}" for n in sorted(worst)))
    assert max(worst.values()) < 1.0


def test_pass_that_does_not_search(oracle_mod, W):
    """the cached-plane pass (redo_knn = 0): after the searching pass at s1, a pass at s2 = s1 + 3 cm along z, then one back at s1 -- against the
    oracle driven through the same sequence.  `selected` is equal at every step and a point that dropped out stays out although its gate would
    pass again; the plane of a point still selected keeps the bits of the searching pass, .w is the new residual; the sums as at the tails (a
    translation leaves the rows' arithmetic exact).  Then a fresh, shorter, DIFFERENT cloud on the same scan and a pass that does not search:
    the selection flags and planes of the earlier cloud are what the reference would use too, and nothing else is selected."""
    _dev()
    from lsd_amd import lio

    s1 = W.state
    s2 = s1.copy()
    s2[2] += 0.03
    m, s = _map(W.map), lio.Scan(max_raw=1 << 14, max_ds=1 << 14)
    o = E.oracle_engine(oracle_mod, W.map, s1)
    o.set_ds(W.ds)
    s.set_ds(W.ds)
    ref1 = E.oracle_pass(o, True)
    got1, mt1, w1 = _run(lio, m, s, s1, True)
    _check_points("pass1", ref1, got1, mt1, w1)
    prev, worst = mt1, []
    outs = []
    for name, st in (("pass2", s2), ("pass3", s1)):
        o.set_state(st)
        ref = E.oracle_pass(o, False)
        got, mt, w = _run(lio, m, s, st, False)
        assert np.array_equal(ref["selected"], mt["selected"]), name
        sel = mt["selected"].astype(bool)
        assert not np.any(sel & ~prev["selected"].astype(bool)), name  # nobody comes back
        assert np.array_equal(_u32(mt["normvec"][sel, :3]), _u32(mt1["normvec"][sel, :3])), name  # the cached plane
        assert np.array_equal(_u32(mt["normvec"][sel, 3]), _u32(ref["normvec"][sel, 3])), name
        assert got["n_eff"] == ref["n_eff"] == int(sel.sum()) and np.array_equal(_u32(w), _u32(ref["world"])), name
        worst.append(_check_sums_identity(got, mt, W.ds))
        outs.append(sel)
        prev = mt
    first = mt1["selected"].astype(bool)
    dropped = first & ~outs[0]
    assert dropped.sum() >= 50 and outs[0].sum() >= 50  # the 3 cm pushed sweep points over the gate, and left others inside
    assert not outs[1][dropped].any()  # back at s1 their gate passes (pass 1 selected them there), and they stay out
    print(f"\n[p2plane edges] no-search passes: worst err/allowance = {max(worst):.4f}")
    assert max(worst) < 1.0
    # a shorter, different cloud, not searched
    short = np.ascontiguousarray(W.ds[::-1][:500])
    o.set_ds(short)
    s.set_ds(short)
    o.set_state(s1)
    ref = E.oracle_pass(o, False)
    got, mt, w = _run(lio, m, s, s1, False)
    assert got["n_ds"] == 500 and np.array_equal(ref["selected"], mt["selected"])
    sel = mt["selected"].astype(bool)
    assert np.array_equal(_u32(ref["normvec"][sel]), _u32(mt["normvec"][sel])) and got["n_eff"] == ref["n_eff"] == int(sel.sum())
    assert not np.any(sel & ~outs[1][:500])
    assert _check_sums_identity(got, mt, short) < 1.0


def _orthonormal_with_first(v):
    v = v / np.linalg.norm(v)
    e = np.zeros(3)
    e[int(np.argmin(np.abs(v)))] = 1.0
    a = np.cross(v, e)
    a /= np.linalg.norm(a)
    return np.stack([v, a, np.cross(v, a)], 1)  # columns


def test_degeneracy_kernel(oracle_mod, W, Wref):
    """degeneracy_kernel through lio_p2plane_degeneracy, after the searching pass on cases 1-5: all six sums EQUAL (==) to the numpy restatement
    over the selected points.  Every addend is an f32 value widened to f64 and a few thousand of them add exactly in f64, so no order of
    addition can change a bit: equality is the right comparison.  The eigenvector matrices put chosen points ON the two thresholds:
    n_j . v = t (1 + k 2^-23), k = -2 .. 2, t = 0.1736f and 0.7070f, for 32 points of distinct normals."""
    _dev()
    from lsd_amd import lio

    m, s = _map(W.map), lio.Scan(max_raw=1 << 14, max_ds=1 << 14)
    s.set_ds(W.ds)
    got, mt, world = _run(lio, m, s, W.state)
    assert np.array_equal(mt["selected"], Wref["selected"])
    sel = np.flatnonzero(mt["selected"])
    nv = mt["normvec"][sel]

    def check(V, tag):
        c, st = s.degeneracy(V)
        wc, ws, dot = E.degeneracy_sums(nv, V)
        assert np.array_equal(c, wc) and np.array_equal(st, ws), (tag, c, wc, st, ws)
        return dot

    check(np.eye(3), "identity")
    Rg = E.quat_rot(E.quat_from_rotvec([0.3, -0.5, 0.7]), np.eye(3))
    check(Rg, "generic")
    tilt = [i for i in W.idx("tilt") if mt["selected"][i]][:32]
    assert len(tilt) == 32 and len(np.unique(_u32(mt["normvec"][tilt, :3]), axis=0)) == 32
    for t in (E.T_CONTRI, E.T_STRONG):
        both = 0
        for j in tilt:
            nh = mt["normvec"][j, :3].astype(np.float64)
            nh /= np.linalg.norm(nh)
            w = _orthonormal_with_first(nh)[:, 1]
            sides = set()
            for k in (-2, -1, 0, 1, 2):
                c = float(t) * (1.0 + k * 2.0 ** -23)
                V = _orthonormal_with_first(c * nh + np.sqrt(1.0 - c * c) * w)
                dot = check(V, (float(t), int(j), k))
                sides.add(bool(dot[np.searchsorted(sel, j), 0] > t))
            both += sides == {False, True}
        assert both >= 1, float(t)  # the point sat on each side of its threshold
    # block edges of the kernel's 256-point workgroups, and a workgroup without a selected point
    last = W.idx("tilt")[0]
    empty = np.repeat(W.ds[W.idx("count:0")[:1]], 256, 0)
    clouds = [E.tail_cloud(W.ds, n, last) for n in (255, 256, 257)] + [np.concatenate([W.ds[:256], empty, W.ds[256:400]])]
    for ds in clouds:
        s.set_ds(ds)
        got, mt, world = _run(lio, m, s, W.state)
        sel = np.flatnonzero(mt["selected"])
        nv = mt["normvec"][sel]
        assert len(sel) > 20
        if len(ds) > 512:
            assert not mt["selected"][256:512].any() and mt["selected"][512:].any()
        check(Rg, len(ds))
        check(np.eye(3), len(ds))


@pytest.mark.parametrize("n", E.CLASSIFY_SIZES)
def test_classify(oracle_mod, n):
    """case 8, classify_kernel + classify_scatter_kernel through lio_map_incremental after a search at the same state: one group of points per
    branch of the rule (no neighbour; nearest neighbour beyond half a leaf on all axes; the same with one axis at EXACTLY half a leaf -- the
    comparison is strict; 1-4 neighbours, one nearer the centre: kept; five, one nearer: dropped; five, one mirrored through the centre so that
    dq == dist: kept, strict <).  All points are distinct, so membership in the map afterwards tells each point's class.  The three sizes above
    65 536 need more than 256 workgroups: the second trip of the scatter's prefix loop."""
    _dev()
    from lsd_amd import lio

    mp, ds, ref = E.classify_oracle(oracle_mod, n)
    cls, branch = E.classify_rule(ref["world"], ref["nn"], ref["nn_cnt"])
    m, s = _map(mp, max_points=200_000, max_voxels=100_000), lio.Scan(max_raw=1 << 17, max_ds=100_000)
    s.set_ds(ds)
    state = E.make_state()
    got, mt, world = _run(lio, m, s, state)
    assert np.array_equal(ref["nn_cnt"], mt["nn_cnt"])
    n_add = lio.map_incremental(m, s, state, map_leaf=0.5, ekf_inited=True)
    assert n_add == ref["n_add"] == int((cls > 0).sum())
    assert m.stats() == ref["stats"]
    dump = m.dump()
    assert np.array_equal(E.rows_u32(dump), E.rows_u32(ref["dump"]))
    ids = set(dump[dump[:, 3] >= 1000.0][:, 3].astype(np.int64).tolist())
    member = np.array([int(w) in ids for w in ds[:, 3]])
    assert np.array_equal(member, cls > 0), np.flatnonzero(member != (cls > 0))[:8]


@pytest.mark.parametrize("n", (257, 65537))
def test_classify_before_the_filter_is_initialised(oracle_mod, n):
    """ekf_inited = 0: every point is added, whatever its neighbours"""
    _dev()
    from lsd_amd import lio

    mp, ds, ref = E.classify_oracle(oracle_mod, n, ekf_inited=False)
    m, s = _map(mp, max_points=200_000, max_voxels=100_000), lio.Scan(max_raw=1 << 17, max_ds=100_000)
    s.set_ds(ds)
    state = E.make_state()
    _run(lio, m, s, state)
    assert lio.map_incremental(m, s, state, map_leaf=0.5, ekf_inited=False) == ref["n_add"] == n
    assert m.stats() == ref["stats"] and np.array_equal(E.rows_u32(m.dump()), E.rows_u32(ref["dump"]))
