"""The pose graph on the device (lio_graph_*) against tests/graph_cases.py's f64 restatement of the rules in include/lio_hip.h, the pair
information of the loop bank against a brute-force nearest neighbour, and the slam_wrapper switch.  Graphs use min_edges = 1 unless a test is
about the minimum."""
import numpy as np
import pytest

import graph_cases as GC
from lsd_amd import capi, lio

pytestmark = pytest.mark.gpu

POS_TOL, ROT_TOL = 1e-4, 1e-5  # the project's parity tolerance (metres, radians)


def _both(spec, remove=(), **params):
    params.setdefault("min_edges", 1)
    return GC.build(spec, lio.PoseGraph(**params), remove), GC.build(spec, GC.Graph(), remove)


@pytest.mark.parametrize("reverse", [False, True])
def test_two_nodes_one_edge(reverse):
    rng = np.random.default_rng(3)
    X0, M = GC.random_pose(rng, 2.0), GC.random_pose(rng, 1.0, angle=0.7)
    want = X0 @ GC.inv_T(M) if reverse else X0 @ M  # the edge 1 -> 0 measures X1^-1 X0
    g = lio.PoseGraph(min_edges=1)
    try:
        g.add_node(X0, fixed=True)
        g.add_node(GC.perturbed(want, rng, 0.3, 0.2))
        g.add_edge(*((1, 0) if reverse else (0, 1)), M, GC.random_info(rng))
        n, rep = g.optimize(50)
        X = g.estimates()
        print("iterations", n, rep)
        assert n >= 1 and rep["chi2_final"] < 1e-20 and g.chi2() == rep["chi2_final"]
        assert np.abs(X[0] - X0).max() < 1e-15 and np.abs(X[1] - want).max() < 1e-12
    finally:
        g.close()


def test_consistent_ring():
    spec = GC.spec_ring()
    g = GC.build(spec, lio.PoseGraph(min_edges=1))
    try:
        n, rep = g.optimize(100)
        print("iterations", n, rep)
        worst = max(GC.pose_diff(X, T)[0] for X, T in zip(g.estimates(), spec["truth"]))
        assert worst < 1e-9 and rep["chi2_final"] < rep["chi2_initial"]
        assert rep["n_active"] == 11 and rep["n_live_edges"] == 12 and 0.0 <= rep["cg_residual"] < 1.0
        t = g.last_times()
        assert all(v > 0 for v in t.values())
    finally:
        g.close()


def _lin_cases():
    loops = GC.spec_chain(257, 2, loops=((256, 4), (200, 60), (130, 129 - 100)), noise=(0.05, 0.02), loop_kernel=GC.HUBER,
                          loop_offset=GC.tq_to_T([0.5, 0.2, -0.1], GC.rotvec_q([0.0, 0.02, 0.1])))
    iso = GC.spec_chain(20, 8, loops=((19, 1),), noise=(0.05, 0.02))
    iso["nodes"].append((np.eye(4), False))                      # no edge at all
    iso["nodes"].append((GC.tq_to_T([1, 2, 3], GC.rotvec_q([0.1, 0, 0])), False))
    iso["edges"].append((21, 5, np.eye(4), np.eye(6), GC.NONE, 1.0))  # its only edge is removed below
    return {
        "65_nodes": (GC.spec_chain(65, 1, noise=(0.05, 0.02)), ()),
        "257_nodes_3_loops": (loops, ()),
        "hub_40": (GC.spec_hub(40), ()),
        "parallel_3": (GC.spec_parallel(), ()),
        "1100_edges": (GC.spec_chain(300, 4, noise=(0.05, 0.02), extra_random_edges=801, fix_first=False), ()),
        "removed_edge": (GC.spec_chain(30, 9, loops=((29, 2), (20, 3)), noise=(0.05, 0.02), loop_kernel=GC.HUBER), (7, 29)),
        "isolated_node": (iso, (20,)),
    }


LIN_CASES = _lin_cases()


@pytest.mark.parametrize("name", list(LIN_CASES))
def test_linearize_against_the_restatement(name):
    spec, remove = LIN_CASES[name]
    g, r = _both(spec, remove)
    try:
        E = len(spec["edges"])
        assert E == {"65_nodes": 64, "257_nodes_3_loops": 259, "hub_40": 40, "parallel_3": 3, "1100_edges": 1100, "removed_edge": 31, "isolated_node": 21}[name]
        got = g.linearize(E)
        want = r.linearize()[:5]
        for what, a, b in zip(("errors", "chi2", "rho1", "b", "Hdiag"), got, want):
            scale = np.abs(b).max()
            print(name, what, "largest entry", scale, "max difference / largest", np.abs(a - b).max() / scale)
            assert np.abs(a - b).max() <= 1e-11 * scale, what
        assert abs(g.chi2() - r.chi2()) <= 1e-11 * r.chi2()
        if name in ("257_nodes_3_loops", "hub_40", "1100_edges"):
            assert (want[2] < 1.0).any() and (want[2] == 1.0).any()  # both Huber branches
        if name == "isolated_node":
            assert not got[3][20].any() and not got[3][21].any() and not got[4][20].any() and got[3][19].any()
        if name == "removed_edge":
            assert not got[0][7].any() and got[0][8].any() and len(g.edges()[2]) == E - 2 and 7 not in g.edges()[2]
    finally:
        g.close()


def test_inconsistent_loops_with_huber():
    """Device against the restatement (exact solve) on 60 nodes with two contradicting Huber loop edges, 100 iterations.
    The chi2 margin is 10 x the relative difference between the restatement with numpy.linalg.solve and the same restatement with the
    conjugate gradients at cg_epsilon = 1e-10 on this graph, measured on the CPU: 3.35e-16 (21.227397197375936 against 21.22739719737593),
    so the margin is 3.35e-15."""
    MARGIN = 10 * 3.35e-16
    spec = GC.spec_huber()
    g, r = _both(spec)
    try:
        n, rep = g.optimize(100)
        rn, rrep = r.optimize(100, min_edges=1)
        X, Y = g.estimates(), r.estimates()
        dp = max(GC.pose_diff(a, b)[0] for a, b in zip(X, Y))
        da = max(GC.pose_diff(a, b)[1] for a, b in zip(X, Y))
        rel = abs(rep["chi2_final"] - rrep["chi2_final"]) / rrep["chi2_final"]
        print("device", n, rep, "restatement", rn, rrep, "pose", dp, da, "chi2 relative difference", rel, "times", g.last_times())
        rho1 = g.linearize(len(spec["edges"]))[2]
        assert rho1[59] < 1.0 and rho1[60] < 1.0 and (rho1[:59] == 1.0).all()  # both loop edges end in Huber's linear branch
        assert dp <= POS_TOL and da <= ROT_TOL
        assert rel <= MARGIN
    finally:
        g.close()


def test_minimum_edge_count():
    spec = GC.spec_chain(10, 12, noise=(0.05, 0.02))  # 9 edges
    g = GC.build(spec, lio.PoseGraph())
    try:
        before = g.estimates().copy()
        n, rep = g.optimize(20)
        assert n == -1 and np.array_equal(before.view(np.uint64), g.estimates().view(np.uint64))
        g.add_edge(9, 0, GC.inv_T(spec["truth"][9]) @ spec["truth"][0], np.eye(6))
        n, rep = g.optimize(20)
        assert n >= 1 and rep["chi2_final"] < rep["chi2_initial"]
    finally:
        g.close()


def test_run_to_run_determinism():
    spec = GC.spec_huber()
    g = lio.PoseGraph(min_edges=1)
    try:
        runs = []
        for _ in range(2):
            g.reset()
            GC.build(spec, g)
            n, rep = g.optimize(30)
            runs.append((n, rep["chi2_final"], rep["trials"], rep["cg_iterations_total"], g.estimates().copy()))
        assert runs[0][:4] == runs[1][:4] and np.array_equal(runs[0][4].view(np.uint64), runs[1][4].view(np.uint64))
    finally:
        g.close()


def test_no_fixed_node():
    spec = GC.spec_chain(20, 31, loops=((19, 2),), noise=(0.02, 0.005), fix_first=False)
    g, r = _both(spec)
    try:
        n, rep = g.optimize(60)
        rn, rrep = r.optimize(60, min_edges=1)
        print("device", n, rep, "restatement", rn, rrep)
        assert rep["n_active"] == 20 and rep["chi2_final"] < rep["chi2_initial"]
        X, Y = g.estimates(), r.estimates()
        for k in range(1, 20):
            dp, da = GC.pose_diff(GC.inv_T(X[0]) @ X[k], GC.inv_T(Y[0]) @ Y[k])
            assert dp <= POS_TOL and da <= ROT_TOL, (k, dp, da)
    finally:
        g.close()


def test_add_edge_refusals():
    g = lio.PoseGraph(min_edges=1)
    try:
        a, b = g.add_node(np.eye(4)), g.add_node(np.eye(4))
        L = capi.lib()
        I, W = np.eye(4), np.eye(6)
        bad = W.copy()
        bad[0, 1] = 1e-6
        f = lambda i, j, w, kern=0, d=1.0: L.lio_graph_add_edge(g.h, i, j, capi.ptr(I, capi.C.c_double), capi.ptr(w, capi.C.c_double), kern, d)
        assert f(a, a, W) == capi.LIO_E_INVALID and f(a, b, bad) == capi.LIO_E_INVALID and f(a, 5, W) == capi.LIO_E_INVALID
        assert f(a, b, W, 7) == capi.LIO_E_INVALID and f(a, b, W, 1, 0.0) == capi.LIO_E_INVALID
        assert f(a, b, W) == 0 and f(b, a, W, 1, 1.0) == 1
        g.remove_edge(0)
        assert L.lio_graph_remove_edge(g.h, 0) == capi.LIO_E_INVALID and f(a, b, W) == 2  # ids are not reused
    finally:
        g.close()


def test_pair_information():
    rng = np.random.default_rng(17)
    c1 = np.concatenate([rng.uniform(-8, 8, (300, 3)), rng.uniform(0, 1, (300, 1))], 1).astype(np.float32)
    c2 = np.concatenate([rng.uniform(-8, 8, (300, 3)), rng.uniform(0, 1, (300, 1))], 1).astype(np.float32)
    c2[:5, :3] += np.float32(40.0)  # nearest neighbours far beyond the detector's own gate of 25 m^2: with max_range = DBL_MAX they count
    rel = GC.tq_to_T([0.4, -0.3, 0.1], GC.rotvec_q([0.02, -0.01, 0.3]))
    d = lio.LoopDetector()
    try:
        assert d.add_keyframe(c1, np.eye(4), 0.0) == 0 and d.add_keyframe(c2, np.eye(4), 1.0) == 1
        score, nr, info = d.pair_information(0, 1, rel)
        T = rel.astype(np.float32)
        p = c2[:, :3]
        moved = np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1)
        assert moved.dtype == np.float32
        dx, dy, dz = (moved[:, None, k] - c1[None, :, k] for k in range(3))
        d2 = ((dx * dx) + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        want = float(np.sum(d2.min(1).astype(np.float64)) / 300.0)
        print("score", score, "brute force", want, "nr", nr)
        assert nr == 300 and abs(score - want) <= 1e-12 * want
        assert (d2.min(1) > 25.0).sum() >= 5
        assert np.array_equal(info.view(np.uint64), lio.LoopDetector.information_matrix(score).view(np.uint64))
        s2, n2, _ = d.pair_information(1, 0, GC.inv_T(rel))
        assert n2 == 300 and s2 != score
    finally:
        d.close()


def _wrapper_drive(frames, graph_on):
    """the key frames of the closed drive through update_odom(): -> (poses of the first and last key frame, edges, loops, odoms seen, status)"""
    import slam_wrapper as sw

    assert sw.init_slam("mapping", "", "FastLIO", ["0-lidar", "IMU"], 0.5, 0.2, 10.0, 60.0) == ["IMU", "0-lidar"]
    try:
        assert sw.get_graph_edges() == {} and sw.run_graph_optimization() == {}
        sw.set_pose_graph(graph_on)
        poses, odoms, n_odoms = {}, {}, []
        for k, (cloud, pose, accum) in enumerate(frames):
            sw._push_keyframe(cloud, pose, 1000 * k, accum)
            d = sw.update_odom()
            assert len(d["keyframes"]) == 1 and np.array_equal(d["keyframes"][0]["pose"], pose.astype(np.float32))
            poses[k] = pose
            n_odoms.append(len(d["odoms"]))
            if d["odoms"]:
                odoms = {int(i): np.array(T) for i, T in d["odoms"].items()}
        edges, loops, status, meta = sw.get_graph_edges(), sw.get_loop_edges(), sw.get_graph_status()["loop_detected"], sw.get_graph_meta()
        again = sw.run_graph_optimization()
        if graph_on:
            assert sorted(int(i) for i in again) == list(range(len(frames))) and all(np.array(T).shape == (4, 4) for T in again.values())
        return poses, odoms, n_odoms, edges, loops, status, meta
    finally:
        sw.deinit_slam()


def test_wrapper_drive_closes_the_loop():
    import loop_cases as LC
    from test_loop_gpu import _drive_frames

    frames = _drive_frames()
    N = len(frames)
    truth = [pose @ GC.inv_T(LC._pose(0.004 * s, -0.003 * s, 0.0004 * s, z=0.0)) for (_, pose, s) in frames]  # loop_cases.drive: estimate = truth drift
    want = GC.inv_T(truth[0]) @ truth[-1]
    poses, odoms, n_odoms, edges, loops, status, meta = _wrapper_drive(frames, False)
    assert edges == {} and odoms == {} and meta == {} and not status and loops == []
    drift_off = GC.pose_diff(GC.inv_T(poses[0]) @ poses[N - 1], want)
    poses, odoms, n_odoms, edges, loops, status, meta = _wrapper_drive(frames, True)
    print("loops", [(e["key1"], e["key2"]) for e in loops], "odoms per call", n_odoms)
    assert status and len(loops) >= 1
    assert len(edges) == N - 1 + len(loops)
    # ids count the edges in creation order: key frame k's edge to k - 1, then the loops found with k as the new frame
    created = []
    for k in range(1, N):
        created.append([k, k - 1])
        created += [[e["key1"], e["key2"]] for e in loops if e["key1"] == k]
    assert edges == {str(i): pair for i, pair in enumerate(created)}
    # fewer than 10 edges: no optimisation, no odoms; from the eleventh key frame on every call returns all key frames so far
    assert n_odoms == [0] * 10 + list(range(11, N + 1)) and sorted(odoms) == list(range(N))
    assert meta["vertex"]["0"]["fix"] is True and meta["vertex"]["1"]["fix"] is False and meta["vertex"]["1"]["edge_num"] >= 2 and len(meta["edge"]) == len(edges)
    drift_on = GC.pose_diff(GC.inv_T(odoms[0]) @ odoms[N - 1], want)
    print("end-to-start error (m, rad): switch off", drift_off, "on", drift_on)
    assert drift_on[0] < drift_off[0]
