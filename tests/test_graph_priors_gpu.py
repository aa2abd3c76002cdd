"""The pose graph's priors on the device (lio_graph_add_prior, DCS2, lio_graph_remove_gnss_outliers) against tests/graph_prior_cases.py's f64
restatement of the rules in include/lio_hip.h.  Graphs use min_edges = 1 unless a test is about the minimum."""
import functools

import numpy as np
import pytest

import graph_cases as GC
import graph_prior_cases as PC
from lsd_amd import capi, lio

pytestmark = pytest.mark.gpu

POS_TOL, ROT_TOL = 1e-4, 1e-5  # the project's parity tolerance (metres, radians)


def _both(spec, remove=(), **params):
    params.setdefault("min_edges", 1)
    return PC.build(spec, lio.PoseGraph(**params), remove), PC.build(spec, PC.Graph(), remove)


def _spec_special():
    """12 chained nodes (node 0 fixed) and a thirteenth without a binary edge; the ids of the priors of interest by name"""
    rng = np.random.default_rng(61)
    s = GC.spec_chain(12, 60, loops=((11, 2), (9, 1)), noise=(0.05, 0.02))
    X = [T for T, _ in s["nodes"]]
    # node 7 is turned 2.8 rad about z, its measured orientation -2.8 rad: both quaternions have w >= 0 and m . q < 0
    X[7] = GC.tq_to_T([7.0, 1.0, 0.2], GC.rotvec_q([0, 0, 2.8]))
    s["nodes"][7] = (X[7], False)
    s["nodes"].append((GC.random_pose(rng, 3.0), False))
    ids, E = {}, s["edges"]

    def add(name, e):
        ids[name] = len(E)
        E.append(e)

    for k, kind in enumerate((PC.XYZ, PC.QUAT, PC.PLANE, PC.XYZ, PC.PLANE)):  # five priors of all three types on node 3, Huber on two
        add("five_%d" % k, PC.random_prior(rng, 3, X[3], kind, kernel=PC.HUBER if k in (1, 2) else PC.NONE, delta=0.3))
    add("fixed", PC.random_prior(rng, 0, X[0], PC.XYZ, err=0.2))
    add("lonely", PC.random_prior(rng, 12, s["nodes"][12][0], PC.QUAT, err=0.2))
    add("removed", PC.random_prior(rng, 5, X[5], PC.PLANE))
    add("quat_flip", PC.prior(7, PC.QUAT, GC.rotvec_q([0, 0, -2.8]), PC.random_info3(rng)))
    world = np.array([0.0, 0.0, 1.0, -1.8])  # the measured normal is the node's own view of it turned by 0.2 rad about an axis perpendicular to it
    nl = X[8][:3, :3].T @ world[:3]
    axis = np.cross(nl, [1.0, 0.0, 0.0]) / np.linalg.norm(np.cross(nl, [1.0, 0.0, 0.0]))
    add("tilt", PC.prior(8, PC.PLANE, np.concatenate([GC.q_to_R(GC.rotvec_q(0.2 * axis)) @ nl, [world[3] + X[8][:3, 3] @ world[:3]]]), PC.random_info3(rng), plane=world))
    add("dcs_in", PC.prior(4, PC.XYZ, X[4][:3, 3] + 0.01, np.eye(3), PC.DCS2, 5.0))               # chi2 << phi: s >= 1
    add("dcs_out", PC.prior(6, PC.XYZ, X[6][:3, 3] + [3.0, -2.0, 1.0], np.eye(3), PC.DCS2, 2.0))  # chi2 = 14 > phi: s < 1, rho' < 0
    T = s["truth"]
    add("edge_dcs_in", (10, 4, GC.inv_T(T[10]) @ T[4], GC.random_info(rng), PC.DCS2, 1.0e4))
    add("edge_dcs_out", (8, 2, GC.inv_T(T[8]) @ T[2] @ GC.tq_to_T([2.0, 1.0, 0.0], GC.rotvec_q([0, 0, 0.3])), GC.random_info(rng), PC.DCS2, 1.0))
    return s, ids


def _spec_one():
    rng = np.random.default_rng(62)
    X = GC.random_pose(rng, 2.0)
    return dict(nodes=[(X, False)], edges=[PC.random_prior(rng, 0, X, PC.PLANE, err=0.2)], truth=[X])


SPECIAL, SPECIAL_IDS = _spec_special()
LIN_CASES = {
    "one_prior": (_spec_one(), ()),
    "255_interleaved": (PC.spec_interleaved(255, 63), ()),
    "257_interleaved": (PC.spec_interleaved(257, 64), (101, 300)),  # a removed prior and a removed binary edge among them
    "special": (SPECIAL, (SPECIAL_IDS["removed"],)),
}


@pytest.mark.parametrize("name", list(LIN_CASES))
def test_linearize_against_the_restatement(name):
    spec, remove = LIN_CASES[name]
    g, r = _both(spec, remove)
    try:
        E = len(spec["edges"])
        got = g.linearize(E)
        want = r.linearize()[:5]
        for what, a, b in zip(("errors", "chi2", "rho1", "b", "Hdiag"), got, want):
            scale = np.abs(b).max()
            print(name, what, "largest entry", scale, "max difference / largest", np.abs(a - b).max() / scale)
            assert np.abs(a - b).max() <= 1e-11 * scale, what
        assert abs(g.chi2() - r.chi2()) <= 1e-11 * r.chi2()
        fr, to, ids = g.edges()
        assert list(ids) == [k for k, e in enumerate(r.edges) if e["live"]]
        assert all((t == -1) == (r.edges[k]["j"] is None) and f == r.edges[k]["i"] for f, t, k in zip(fr, to, ids))
        P, Q = g.priors(), r.priors()
        assert [p["id"] for p in P] == [p["id"] for p in Q] and all(not got[0][p["id"], 3:].any() for p in P)
        for p, q in zip(P, Q):
            assert (p["node"], p["type"], p["kernel"], p["delta"]) == (q["node"], q["type"], q["kernel"], q["delta"])
            # (the normalisation is one square root and one division over sums taken in another order than numpy's: a few ulp of the entry)
            ulp4 = 4 * np.finfo(np.float64).eps
            assert (np.abs(p["measurement"] - q["measurement"]) <= ulp4 * np.maximum(1.0, np.abs(q["measurement"]))).all()
            assert (np.abs(p["plane"] - q["plane"]) <= ulp4 * np.maximum(1.0, np.abs(q["plane"]))).all()
            assert np.array_equal(p["information"], q["information"])
        rho1 = want[2]
        if name.endswith("interleaved"):
            assert E == 2 * int(name.split("_")[0]) and E > 256  # the ids span more than one chi2 partial
            kinds = [r.edges[k]["kernel"] for k in range(E)]
            for kern in (PC.HUBER, PC.DCS2):  # both branches of both kernels, on priors
                on = np.array([r.edges[k]["live"] and r.edges[k]["j"] is None and kinds[k] == kern for k in range(E)])
                assert (rho1[on] == 1.0).any() and (rho1[on] != 1.0).any(), kern
        if name == "257_interleaved":
            assert r.edges[101]["j"] is None and r.edges[300]["j"] is not None and not got[0][101].any() and not got[0][300].any() and got[0][103].any()
            assert 101 not in ids and 300 not in ids and len(ids) == E - 2
        if name == "one_prior":
            assert got[4][0].any() and got[3][0].any()
        if name == "special":
            I = SPECIAL_IDS
            node3 = [I["five_%d" % k] for k in range(5)]
            assert [r.edges[k]["type"] for k in node3] == [PC.XYZ, PC.QUAT, PC.PLANE, PC.XYZ, PC.PLANE] and all(r.edges[k]["i"] == 3 for k in node3)
            assert not got[3][0].any() and not got[4][0].any() and got[1][I["fixed"]] > 0           # a prior on the fixed node: chi2 only
            assert got[4][12].any() and np.abs(got[4][12][:3, :3]).max() == 0.0                     # the lonely node is active through its QUAT prior
            assert not got[0][I["removed"]].any() and got[1][I["removed"]] == 0.0 and I["removed"] not in ids
            e = r.edges[I["quat_flip"]]
            assert e["m"][3] >= 0 and r.q[7][3] >= 0 and e["m"] @ r.q[7] < 0
            e = r.edges[I["tilt"]]
            tilt = np.arccos(np.clip(e["m"][:3] @ (GC.q_to_R(r.q[8]).T @ e["plane"][:3]), -1, 1))
            assert abs(tilt - 0.2) < 1e-9 and np.abs(want[0][I["tilt"], :2]).max() > 0.05
            assert rho1[I["dcs_in"]] == 1.0 and rho1[I["edge_dcs_in"]] == 1.0
            assert rho1[I["dcs_out"]] < 0.0 and rho1[I["edge_dcs_out"]] < 0.0  # (DCS2 has no branch between: rho' is 1 up to chi2 = phi and negative beyond)
            assert got[2][I["dcs_out"]] < 0.0 and got[2][I["edge_dcs_out"]] < 0.0 and got[2][I["dcs_in"]] == 1.0 and got[2][I["edge_dcs_in"]] == 1.0
    finally:
        g.close()


@functools.lru_cache(maxsize=None)
def _gnss_reference():
    r = PC.build(PC.spec_gnss(), PC.Graph())
    removed, rep, scales = r.remove_gnss_outliers(1.0, 100, min_edges=1)
    return removed, rep, r.estimates()


def test_gnss_scene_outliers_and_estimates():
    """Device against the restatement (exact solve) on 60 free nodes, XYZ priors on every third (Omega = I / 0.05), two of them 15 m off; the
    outlier stage at 1.0 m, 100 iterations per optimisation.  Measured on the CPU with the restatement alone: it flags exactly the planted two
    (scale 0.0087 and 0.0088; every other prior's scale >= 1.99); numpy.linalg.solve against the restatement's own conjugate gradients at
    cg_epsilon = 1e-10 agree to 4.47e-15 relative in the final chi2 (0.8197766000936146 against 0.8197766000936183), 6.1e-9 m and 1.5e-8 rad
    in pose, and end on different stop reasons (rho_zero against trials): the chi2 margin is 10 x 4.47e-15, stop reasons are not compared."""
    MARGIN = 10 * 4.47e-15
    spec = PC.spec_gnss()
    want_removed, rrep, Y = _gnss_reference()
    g = PC.build(spec, lio.PoseGraph(min_edges=1))
    try:
        assert not g.fixed().any()
        removed, rep = g.remove_gnss_outliers(1.0, 100)
        X = g.estimates()
        dp = max(GC.pose_diff(a, b)[0] for a, b in zip(X, Y))
        da = max(GC.pose_diff(a, b)[1] for a, b in zip(X, Y))
        rel = abs(rep["chi2_final"] - rrep["chi2_final"]) / rrep["chi2_final"]
        print("device", removed, rep, "restatement", want_removed, rrep, "pose", dp, da, "chi2 relative difference", rel, "times", g.last_times())
        assert removed == spec["planted"] == want_removed and len(removed) == 2
        left = g.priors()
        assert len(left) == 18 and all(p["kernel"] == PC.DCS2 and p["delta"] == 20.0 for p in left) and not set(removed) & {p["id"] for p in left}
        assert dp <= POS_TOL and da <= ROT_TOL
        assert rel <= MARGIN
    finally:
        g.close()


@functools.lru_cache(maxsize=None)
def _floor_reference():
    r = PC.build(PC.spec_floor(), PC.Graph())
    it, rep = r.optimize(100, min_edges=1)
    return rep, r.estimates()


def test_floor_scene_holds_the_height():
    """Device against the restatement (exact solve) on the 60-node chain whose every odometry edge is pitched by 0.004 rad, PLANE priors of the
    floor on every fifth node, nothing fixed, 100 iterations.  Plane priors leave x, y and the heading of the whole graph free, so the poses are
    compared as X_0^-1 X_k (as test_graph_gpu.test_no_fixed_node does) and the heights as they are, all at the parity tolerance.  Measured on the
    CPU with the restatement alone, numpy.linalg.solve against its own conjugate gradients: 1.8e-9 m and 9.4e-11 rad in X_0^-1 X_k, 9.2e-12 m in
    height, but 2.0e-3 m in the free directions; 5.68e-16 relative in the final chi2 (0.0011442925483169674 against 0.001144292548316968), so
    the chi2 margin is 5.68e-15.  The largest height error against the truth falls from 1.286 m (no priors) to 0.058 m."""
    MARGIN = 10 * 5.68e-16
    spec = PC.spec_floor()
    rrep, Y = _floor_reference()
    g = PC.build(spec, lio.PoseGraph(min_edges=1))
    bare = PC.build(PC.spec_floor(with_priors=False), lio.PoseGraph(min_edges=1))
    try:
        n, rep = g.optimize(100)
        X = g.estimates()
        dp = max(GC.pose_diff(GC.inv_T(X[0]) @ a, GC.inv_T(Y[0]) @ b)[0] for a, b in zip(X, Y))
        da = max(GC.pose_diff(GC.inv_T(X[0]) @ a, GC.inv_T(Y[0]) @ b)[1] for a, b in zip(X, Y))
        dz = max(abs(a[2, 3] - b[2, 3]) for a, b in zip(X, Y))
        rel = abs(rep["chi2_final"] - rrep["chi2_final"]) / rrep["chi2_final"]
        nb, brep = bare.optimize(100)
        height = lambda Z: max(abs(a[2, 3] - t[2, 3]) for a, t in zip(Z, spec["truth"]))
        h_with, h_bare = height(X), height(bare.estimates())
        print("device", n, rep, "restatement", rrep, "relative pose", dp, da, "height", dz, "chi2 relative difference", rel, "height error with priors", h_with,
              "without", h_bare, "bare", nb, brep)
        assert len(g.priors()) == 12 and rep["n_active"] == 60
        assert dp <= POS_TOL and da <= ROT_TOL and dz <= POS_TOL
        assert rel <= MARGIN
        assert h_with < h_bare
    finally:
        g.close()
        bare.close()


def test_run_to_run_determinism_with_priors():
    g = lio.PoseGraph(min_edges=1)
    try:
        runs = []
        for _ in range(2):
            g.reset()
            PC.build(PC.spec_gnss(), g)
            removed, rep = g.remove_gnss_outliers(1.0, 30)
            lin = g.linearize(len(PC.spec_gnss()["edges"]))
            runs.append((removed, rep["chi2_final"], rep["trials"], rep["cg_iterations_total"], np.concatenate([g.estimates().ravel()] + [a.ravel() for a in lin])))
        assert runs[0][:4] == runs[1][:4] and np.array_equal(runs[0][4].view(np.uint64), runs[1][4].view(np.uint64))
    finally:
        g.close()


def test_add_prior_and_set_kernel_refusals():
    g = lio.PoseGraph(min_edges=1)
    try:
        a, b = g.add_node(np.eye(4)), g.add_node(np.eye(4))
        L, p64 = capi.lib(), lambda x: None if x is None else capi.ptr(x, capi.C.c_double)
        W, m, up = np.eye(3), np.array([1.0, 2.0, 3.0, 1.0]), np.array([0.0, 0.0, 1.0, 0.0])
        asym = W.copy()
        asym[0, 1] = 1e-6
        nan3, nanm = W.copy(), m.copy()
        nan3[1, 1], nanm[1] = np.nan, np.inf
        f = lambda node, kind, mm, pl, w, kern=0, d=1.0: L.lio_graph_add_prior(g.h, node, kind, p64(mm), p64(pl), p64(w), kern, d)
        INV = capi.LIO_E_INVALID
        assert f(5, PC.XYZ, m, None, W) == INV and f(-1, PC.XYZ, m, None, W) == INV and f(a, 3, m, None, W) == INV          # node, type
        assert f(a, PC.XYZ, m, None, W, 7) == INV and f(a, PC.XYZ, m, None, W, PC.HUBER, 0.0) == INV and f(a, PC.XYZ, m, None, W, PC.DCS2, -1.0) == INV
        assert f(a, PC.XYZ, nanm, None, W) == INV and f(a, PC.XYZ, m, None, nan3) == INV and f(a, PC.XYZ, m, None, W, PC.HUBER, np.nan) == INV
        assert f(a, PC.QUAT, np.zeros(4), None, W) == INV and f(a, PC.PLANE, np.array([0.0, 0, 0, 1]), up, W) == INV
        assert f(a, PC.PLANE, up, np.array([0.0, 0, 0, 1]), W) == INV and f(a, PC.PLANE, up, None, W) == INV
        assert f(a, PC.XYZ, m, None, asym) == INV
        assert g.priors() == [] and len(g.edges()[0]) == 0
        assert g.add_edge(a, b, np.eye(4), np.eye(6)) == 0 and f(a, PC.XYZ, m, None, W) == 1 and f(b, PC.PLANE, 2.0 * up, 3.0 * up, W, PC.DCS2, 2.0) == 2
        P = g.priors()
        assert [p["id"] for p in P] == [1, 2] and np.array_equal(P[1]["measurement"], up) and np.array_equal(P[1]["plane"], up) and P[1]["kernel"] == PC.DCS2
        k = lambda e, kern, d: L.lio_graph_set_kernel(g.h, e, kern, d)
        assert k(3, 0, 1.0) == INV and k(0, 7, 1.0) == INV and k(1, PC.HUBER, 0.0) == INV and k(0, PC.DCS2, np.nan) == INV
        assert k(0, PC.DCS2, 3.0) == 0 and k(1, PC.HUBER, 0.5) == 0
        assert (g.priors()[0]["kernel"], g.priors()[0]["delta"]) == (PC.HUBER, 0.5)
        g.remove_edge(1)
        assert k(1, 0, 1.0) == INV and L.lio_graph_remove_edge(g.h, 1) == INV and [p["id"] for p in g.priors()] == [2]
        assert f(a, PC.XYZ, m, None, W) == 3 and g.add_edge(b, a, np.eye(4), np.eye(6), PC.DCS2, 1.0) == 4  # ids are shared and not reused
        assert list(g.edges()[1]) == [1, -1, -1, 0]
    finally:
        g.close()


def test_set_kernel_on_resident_edges_changes_the_cost():
    spec, _ = LIN_CASES["special"]
    g, r = _both(spec)
    try:
        g.chi2()  # everything is on the device now
        for e, kern, d in ((SPECIAL_IDS["dcs_out"], PC.HUBER, 1.0), (SPECIAL_IDS["edge_dcs_out"], PC.NONE, 1.0), (3, PC.DCS2, 1e-3)):
            g.set_kernel(e, kern, d)
            r.set_kernel(e, kern, d)
        got, want = g.linearize(len(spec["edges"])), r.linearize()[:5]
        for a, b in zip(got, want):
            assert np.abs(a - b).max() <= 1e-11 * np.abs(b).max()
        assert abs(g.chi2() - r.chi2()) <= 1e-11 * r.chi2()
    finally:
        g.close()


def test_minimum_edge_count_counts_priors():
    spec = GC.spec_chain(10, 12, noise=(0.05, 0.02))  # 9 binary edges
    g = GC.build(spec, lio.PoseGraph())
    try:
        before = g.estimates().copy()
        assert g.optimize(20)[0] == -1 and g.remove_gnss_outliers(1.0, 20)[0] is None
        assert np.array_equal(before.view(np.uint64), g.estimates().view(np.uint64))
        g.add_prior(9, PC.XYZ, spec["truth"][9][:3, 3], np.eye(3))
        n, rep = g.optimize(20)
        assert n >= 1 and rep["n_live_edges"] == 10 and rep["chi2_final"] < rep["chi2_initial"]
    finally:
        g.close()


def test_a_graph_without_priors_is_untouched_by_them():
    """the same graph, once never having seen a prior and once with a prior added and removed again (so that the prior kernels and the chi2 variant
    that follows placeholders run): the same bits; and the prior-free graph still agrees with graph_cases' restatement"""
    spec = GC.spec_huber()
    a, b = GC.build(spec, lio.PoseGraph(min_edges=1)), GC.build(spec, lio.PoseGraph(min_edges=1))
    try:
        b.remove_edge(b.add_prior(5, PC.XYZ, [100.0, 0.0, 0.0], np.eye(3)))
        E = len(spec["edges"])
        la, lb = a.linearize(E), b.linearize(E + 1)
        for x, y in zip(la, lb):
            assert np.array_equal(x.view(np.uint64), y[:len(x)].view(np.uint64))
        want = GC.build(spec, GC.Graph()).linearize()[:5]
        for x, y in zip(la, want):
            assert np.abs(x - y).max() <= 1e-11 * np.abs(y).max()
        (na, ra), (nb, rb) = a.optimize(30), b.optimize(30)
        assert na == nb and all(ra[k] == rb[k] for k in ("chi2_final", "trials", "accepted", "cg_iterations_total", "lambda", "stop"))
        assert np.array_equal(a.estimates().view(np.uint64), b.estimates().view(np.uint64)) and a.chi2() == b.chi2()
    finally:
        a.close()
        b.close()


# ---- the slam_wrapper: floor edges from the key frames' clouds, GNSS fixes, the robust optimisation ------------------------------------------

N_FRAMES, FRAME_STEP = 12, 60.0


@functools.lru_cache(maxsize=None)
def _frames(bias):
    """12 key frames 60 m of accumulated distance apart: (cloud, odometry pose, accumulated distance).  Every cloud is the sensor's own view of a
    floor 1.8 m below it (2500 points, sigma 1 cm) and two walls (1500 points); the odometry pitches by `bias` rad per step"""
    rng = np.random.default_rng(71)
    step = GC.tq_to_T([FRAME_STEP, 0.0, 0.0], GC.rotvec_q([0.0, bias, 0.0]))
    pose, out = GC.tq_to_T([0.0, 0.0, 1.8], [0.0, 0.0, 0.0, 1.0]), []
    for k in range(N_FRAMES):
        floor = np.column_stack([rng.uniform(-15, 15, (2500, 2)), -1.8 + rng.normal(0, 0.01, 2500)])
        wall = np.column_stack([rng.uniform(-15, 15, 1500), np.where(rng.random(1500) < 0.5, -9.0, 9.0) + rng.normal(0, 0.01, 1500), rng.uniform(-1.8, 4.0, 1500)])
        cloud = np.column_stack([np.concatenate([floor, wall]), rng.uniform(0, 255, 4000)]).astype(np.float32)
        out.append((cloud[rng.permutation(4000)], pose.copy(), FRAME_STEP * k))
        pose = pose @ step
    return out


def _wrapper_run(frames, graph_on, ground, after=None):
    """the key frames through update_odom() -> (odoms of the last call that had any, priors, edges, meta, loops, what `after` returned)"""
    import slam_wrapper as sw

    assert sw.init_slam("mapping", "", "FastLIO", ["0-lidar", "IMU"], 0.5, 0.2, 10.0, 60.0) == ["IMU", "0-lidar"]
    try:
        sw.set_pose_graph(graph_on)
        sw.set_mapping_ground_constraint(ground)
        assert sw.get_mapping_ground_constraint() == ground
        odoms = {}
        for k, (cloud, pose, accum) in enumerate(frames):
            sw._push_keyframe(cloud, pose, 1000 * k, accum)
            d = sw.update_odom()
            assert len(d["keyframes"]) == 1
            if d["odoms"]:
                odoms = {int(i): np.array(T) for i, T in d["odoms"].items()}
        extra = after(sw) if after else None
        return odoms, sw._graph_priors(), sw.get_graph_edges(), sw.get_graph_meta(), sw.get_loop_edges(), extra
    finally:
        sw.deinit_slam()


def _pair_informations(frames):
    """the information matrices the wrapper gives its odometry edges: the loop bank's pair information of frame k against k - 1"""
    d = lio.LoopDetector()
    try:
        infos = [None]
        for k, (cloud, pose, accum) in enumerate(frames):
            assert d.add_keyframe(cloud, pose, accum) == k
            if k:
                infos.append(d.pair_information(k, k - 1, GC.inv_T(pose) @ frames[k - 1][1])[2])
        return infos
    finally:
        d.close()


def test_wrapper_floor_constraint():
    """Pitch-biased odometry (0.004 rad per 60 m step) with the ground constraint on: a PLANE prior on every second key frame, node 0 released,
    and the odoms of update_odom() against the restatement replayed call by call from _graph_priors() and the graph's edges.  As in
    test_floor_scene_holds_the_height the plane priors leave x, y and the heading free: X_0^-1 X_k and the heights are compared."""
    frames = _frames(0.004)
    odoms, priors, edges, meta, loops, _ = _wrapper_run(frames, True, True)
    assert loops == [] and edges == {str(k - 1 + (k + 1) // 2): [k, k - 1] for k in range(1, N_FRAMES)}  # EdgeSE3 only, ids shared with the priors
    assert [p["node"] for p in priors] == list(range(0, N_FRAMES, 2)) and [p["id"] for p in priors] == [3 * j for j in range(N_FRAMES // 2)]
    for p in priors:
        assert (p["type"], p["kernel"], p["delta"]) == (PC.PLANE, PC.HUBER, 1.0) and np.array_equal(p["information"], np.eye(3) * 0.1)
        assert np.array_equal(p["plane"], [0.0, 0.0, 1.0, 0.0])  # node 0 was still fixed when the plane was made: height 0
        # (the detector's plane is the best three-point draw, not a refit: every floor point lies within its 0.1 m band over a 30 m patch)
        assert np.abs(p["measurement"] - [0.0, 0.0, 1.0, 1.8]).max() < 0.1 and np.abs(p["measurement"][:2]).max() < 0.2 / 30.0
        assert abs(np.linalg.norm(p["measurement"][:3]) - 1.0) < 1e-6
    assert meta["vertex"]["0"]["fix"] is False and len(meta["edge"]) == len(edges)
    assert sorted(odoms) == list(range(N_FRAMES))
    # the replay
    infos = _pair_informations(frames)
    r, odom2map, by_node = PC.Graph(), np.eye(4), {p["node"]: p for p in priors}
    for k, (cloud, pose, accum) in enumerate(frames):
        r.add_node(odom2map @ pose, fixed=(k == 0))
        if k:
            r.add_edge(k, k - 1, GC.inv_T(pose) @ frames[k - 1][1], infos[k])
        if k in by_node:
            p = by_node[k]
            assert r.add_prior(k, p["type"], p["measurement"], p["information"], p["kernel"], p["delta"], plane=p["plane"]) == p["id"]
            r.fixed[0] = False
        if r.optimize(1024)[0] >= 0:
            odom2map = (r.estimates()[-1] @ GC.inv_T(pose)).astype(np.float32).astype(np.float64)
    Y = r.estimates()
    X = [odoms[k] for k in range(N_FRAMES)]
    dp = max(GC.pose_diff(GC.inv_T(X[0]) @ a, GC.inv_T(Y[0]) @ b)[0] for a, b in zip(X, Y))
    da = max(GC.pose_diff(GC.inv_T(X[0]) @ a, GC.inv_T(Y[0]) @ b)[1] for a, b in zip(X, Y))
    dz = max(abs(a[2, 3] - b[2, 3]) for a, b in zip(X, Y))
    drift = abs(frames[-1][1][2, 3] - 1.8)
    print("relative pose", dp, da, "height", dz, "odometry height drift", drift, "corrected", max(abs(a[2, 3] - X[0][2, 3]) for a in X))
    assert dp <= POS_TOL and da <= ROT_TOL and dz <= POS_TOL
    assert max(abs(a[2, 3] - X[0][2, 3]) for a in X) < drift  # the floor edges pull back the height the odometry loses


def test_wrapper_gnss_and_robust_optimization():
    frames = _frames(0.0)
    fix = lambda k: frames[k][1][:3, 3].copy()  # the fixes agree with the odometry, but for the planted one
    OUTLIER = 5

    def after(sw):
        added = []
        assert sw.add_graph_gnss(N_FRAMES, fix(0), 0.05, 3) == [] and sw.add_graph_gnss(-1, fix(0), 0.05, 3) == []  # no such key frame
        for k in range(N_FRAMES):
            xyz = fix(k) + ([0.0, 0.0, 15.0] if k == OUTLIER else [0.0, 0.0, 0.0])
            if k == 3:  # within 10 m of the last accepted fix: the gate refuses it; the key frame can still take a later one
                assert sw.add_graph_gnss(k, fix(2) + [3.0, 0.0, 0.0], 0.05, 3) == []
            if k == 7:  # a 6-D fix: position and orientation
                ids = sw.add_graph_gnss(k, xyz, 0.05, 6, GC.T_to_tq(frames[k][1])[1])
                assert len(ids) == 2 and ids[1] == ids[0] + 1
            else:
                ids = sw.add_graph_gnss(k, xyz, 0.05, 3 if k != 9 else 2)
                assert len(ids) == 1
            assert sw.add_graph_gnss(k, xyz + [500.0, 0.0, 0.0], 0.05, 3) == []  # the key frame has its fix
            added.append(ids)
        before = sw._graph_priors()
        fixed0 = sw.get_graph_meta()["vertex"]["0"]["fix"]
        sw.del_graph_edge(added[1][0])  # a prior's id is ignored
        assert len(sw._graph_priors()) == len(before)
        return added, before, fixed0, sw.run_robust_graph_optimization("mapping"), sw._graph_priors(), sw.get_graph_edges()

    odoms, priors, edges, meta, loops, (added, before, fixed0, result, left, edges_after) = _wrapper_run(frames, True, False, after)
    assert fixed0 is False and len(before) == N_FRAMES + 1 and [p["id"] for p in before] == [i for ids in added for i in ids]
    assert all(p["kernel"] == PC.HUBER and p["delta"] == 1.0 for p in before)
    by_id = {p["id"]: p for p in before}
    p = by_id[added[4][0]]
    assert p["type"] == PC.XYZ and np.array_equal(p["measurement"][:3], fix(4)) and np.array_equal(p["information"], np.eye(3) / 0.05)
    q = by_id[added[7][1]]
    assert q["type"] == PC.QUAT and np.array_equal(q["information"], np.eye(3) / 0.5) and abs(np.linalg.norm(q["measurement"]) - 1.0) < 1e-15
    two = by_id[added[9][0]]
    assert two["measurement"][2] == 0.0 and two["information"][2, 2] == 1.0 / (fix(9)[0] ** 2 + fix(9)[1] ** 2) and two["information"][0, 0] == 1.0 / 0.05
    # the robust optimisation drops the planted fix alone, puts DCS2 on the other positions and returns every key frame's pose
    assert sorted(int(i) for i in result) == list(range(N_FRAMES)) and all(np.array(T).shape == (4, 4) for T in result.values())
    assert [p["id"] for p in left] == [i for i in by_id if i != added[OUTLIER][0]]
    assert all(p["kernel"] == (PC.DCS2 if p["type"] == PC.XYZ else PC.HUBER) for p in left) and edges_after == edges and len(edges) == N_FRAMES - 1
    worst = max(np.linalg.norm(np.array(result[str(k)])[:3, 3] - fix(k)) for k in range(N_FRAMES) if k != 9)
    print("largest distance of a corrected key frame from its fix", worst)
    assert worst < 0.5


def test_wrapper_priors_are_inert_without_the_pose_graph():
    frames = _frames(0.004)[:4]

    def after(sw):
        return sw.add_graph_gnss(0, [1.0, 2.0, 3.0], 0.05, 3), sw.run_robust_graph_optimization("mapping"), sw.run_robust_graph_optimization("localization")

    odoms, priors, edges, meta, loops, (ids, a, b) = _wrapper_run(frames, False, True, after)
    assert odoms == {} and priors == [] and edges == {} and meta == {} and ids == [] and a == {} and b == {}
