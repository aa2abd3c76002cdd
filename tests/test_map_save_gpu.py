"""A map's way to disk from mapping mode, on the device: a vertex leaves the pose graph (lio_graph_remove_node) and the loop bank (lio_loop_retire), the
graph hands back its edges (lio_graph_edge_records), and the module's dump_graph / dump_odometry / del_graph_vertex / get_graph_map write a map that
localisation mode loads, localises in and merges."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import map_save_cases as MC  # noqa: E402
from lsd_amd import capi, lio, synth  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _spd(rng):
    A = rng.normal(size=(6, 6))
    W = A @ A.T + 6 * np.eye(6)
    return 50.0 * (W + W.T) / 2


def _chain(without=None):
    """a chain of 7 nodes, a loop edge 1-5 (Huber) and a GNSS prior on node 3 -> (graph, the binary edges added as (id, from, to, M, W, kernel, delta)).
    The edges that do not touch node 3 come first, so they carry the same ids in the graph built `without` node 3 -- which still adds a placeholder
    node in its place, so that the node ids agree as well."""
    rng = np.random.default_rng(31)
    truth = [MC.pose(2.0 * k, 0.4 * np.sin(0.7 * k), 0.05 * k, [0.01 * k, -0.02 * k, 0.1 * k]) for k in range(7)]
    noise = [MC.pose(*rng.normal(0, 0.2, 3), rng.normal(0, 0.03, 3)) for _ in range(7)]
    pairs = [(0, 1), (1, 2), (4, 5), (5, 6), (1, 5), (2, 3), (3, 4)]
    meas = {p: np.linalg.inv(truth[p[0]]) @ truth[p[1]] @ MC.pose(*rng.normal(0, 0.02, 3), rng.normal(0, 0.004, 3)) for p in pairs}
    info = {p: _spd(rng) for p in pairs}
    g = lio.PoseGraph(min_edges=1)
    added = []
    for k in range(7):
        assert g.add_node(truth[k] if k else np.eye(4) @ truth[0], fixed=(k == 0)) == k
    for k in range(1, 7):  # disturbed estimates (node 3's too: the placeholder never moves, the removed node no longer matters)
        g.set_estimate(k, truth[k] @ noise[k])
    for p in pairs:
        if without is not None and without in p:
            continue
        kernel, delta = (lio.PoseGraph.HUBER, 0.8) if p == (1, 5) else (lio.PoseGraph.NONE, 1.0)
        eid = g.add_edge(p[0], p[1], meas[p], info[p], kernel, delta)
        added.append((eid, p[0], p[1], meas[p], info[p], kernel, delta))
    prior = None
    if without != 3:
        prior = g.add_prior(3, lio.PoseGraph.XYZ, truth[3][:3, 3] + [0.1, -0.1, 0.05], np.diag([4.0, 4.0, 1.0]), lio.PoseGraph.HUBER, 1.0)
    return g, added, prior


def test_remove_node_against_a_graph_that_never_had_the_node():
    """Graph A loses node 3 (two chain edges and the prior go with it); graph B never had them.  The active ordering is the same (nodes 1, 2, 4, 5,
    6 in both: a removed node and an unconnected placeholder are equally inactive), every block is summed in rising edge id over the same live
    edges, and chi2 is folded per 256 ids with the live edges in the same lanes because the surviving edges carry the same ids in both graphs --
    so the estimates of the live nodes and chi2 agree BIT FOR BIT, and that is what is asserted."""
    A, added, prior = _chain()
    B, added_b, _ = _chain(without=3)
    L = capi.lib()
    try:
        assert prior == 7 and [e[0] for e in added] == list(range(7)) and [e[0] for e in added_b] == list(range(5))
        assert A.node_live().tolist() == [True] * 7
        rec = A.edge_records()
        assert len(rec) == 7
        A.remove_node(3)
        assert A.node_live().tolist() == [True, True, True, False, True, True, True] and A.num_nodes == 7
        assert A.fixed().tolist() == [True] + [False] * 6
        # a removed id is as unknown as one never handed out; the other ids have not moved
        assert L.lio_graph_remove_node(A.h, 3) == capi.LIO_E_INVALID and L.lio_graph_remove_node(A.h, 7) == capi.LIO_E_INVALID
        M, W = np.eye(4), np.eye(6)
        f = lambda a, b: L.lio_graph_add_edge(A.h, a, b, lio.ptr(M, lio.C.c_double), lio.ptr(W, lio.C.c_double), 0, 1.0)
        assert f(3, 4) == capi.LIO_E_INVALID and f(2, 3) == capi.LIO_E_INVALID and f(2, 9) == capi.LIO_E_INVALID
        assert L.lio_graph_set_fixed(A.h, 3, 1) == capi.LIO_E_INVALID and L.lio_graph_set_estimate(A.h, 3, lio.ptr(M, lio.C.c_double)) == capi.LIO_E_INVALID
        with pytest.raises(capi.LioError):
            A.add_prior(3, lio.PoseGraph.XYZ, [0, 0, 0], np.eye(3))
        a, b, ids = A.edges()
        assert ids.tolist() == [0, 1, 2, 3, 4] and 3 not in a.tolist() + b.tolist() and A.priors() == []
        # the records: what was added, minus the edges on node 3, bit for bit
        rec = A.edge_records()
        want = [e for e in added if 3 not in (e[1], e[2])]
        assert [(r["id"], r["from"], r["to"], r["kernel"], r["delta"]) for r in rec] == [(e[0], e[1], e[2], e[5], e[6]) for e in want]
        for r, e in zip(rec, want):
            assert np.array_equal(_bits(r["measurement"]), _bits(e[3])) and np.array_equal(_bits(r["information"]), _bits(e[4]))
        assert L.lio_graph_edge_records(A.h, None, None, None, None, None, None, None, 2) == -5  # cap too small: -(count)
        before = A.estimates()
        assert np.array_equal(_bits(A.chi2()), _bits(B.chi2()))
        na, ra = A.optimize(100)
        nb, rb = B.optimize(100)
        print("A", na, ra["stop"], ra["chi2_initial"], ra["chi2_final"], "B", nb, rb["stop"], rb["chi2_final"])
        assert na == nb >= 1 and ra["n_active"] == rb["n_active"] == 5 and ra["n_live_edges"] == rb["n_live_edges"] == 5
        assert ra["chi2_final"] < ra["chi2_initial"]
        ea, eb = A.estimates(), B.estimates()
        live = [0, 1, 2, 4, 5, 6]
        assert np.array_equal(_bits(ea[live]), _bits(eb[live]))
        assert np.array_equal(_bits(ra["chi2_final"]), _bits(rb["chi2_final"])) and np.array_equal(_bits(A.chi2()), _bits(B.chi2()))
        assert np.array_equal(_bits(ea[3]), _bits(before[3]))  # the removed node's row stays as it last was
        assert not np.array_equal(ea[1], before[1])
    finally:
        A.close()
        B.close()


def test_removing_the_only_fixed_node():
    """the header's rule: without a fixed node every connected live node is active, the LM damping alone holds the gauge, chi2 still falls"""
    g, _, _ = _chain()
    try:
        before = g.estimates()
        g.remove_node(0)
        assert g.node_live().tolist() == [False] + [True] * 6 and not g.fixed().any()
        a, b, ids = g.edges()
        assert ids.tolist() == [1, 2, 3, 4, 5, 6, 7]  # edge 0 (0 -> 1) went with the node
        n, rep = g.optimize(100)
        print(n, rep)
        assert n >= 1 and rep["n_active"] == 6 and rep["n_live_edges"] == 7
        assert np.isfinite(rep["chi2_final"]) and rep["chi2_final"] < rep["chi2_initial"]
        est = g.estimates()
        assert np.isfinite(est).all() and np.array_equal(_bits(est[0]), _bits(before[0]))
    finally:
        g.close()


def test_retired_frame_is_never_matched_again():
    """LoopDetector.retire: the frame's slot stays, the stage doors refuse it, detect passes it over as a candidate"""
    scene = MC.scene()
    frames = MC.keyframes(scene, 3)
    d = lio.LoopDetector()
    try:
        for k, (pts, T, _, accum) in enumerate(frames):
            assert d.add_keyframe(pts, T, accum) == k
        assert d.detect() == []
        d.retire(1)
        L = capi.lib()
        assert L.lio_loop_retire(d.h, 1) == capi.LIO_E_INVALID and L.lio_loop_retire(d.h, 3) == capi.LIO_E_INVALID
        assert d.num_keyframes()[0] == 3 and len(d.download_keyframe(1)[0]) == len(frames[1][0])
        with pytest.raises(capi.LioError):
            d.pair_information(0, 1, np.eye(4))
        with pytest.raises(capi.LioError):
            d.pair_information(1, 2, np.eye(4))
        d.pair_information(0, 2, np.linalg.inv(frames[0][1]) @ frames[2][1])
        # a frame at frame 1's pose, far along the drive: frames 0 and 2 are candidates, frame 1 is not
        pts, T, _, _ = MC.keyframes(scene, 2, seed0=900)[1]
        assert d.add_keyframe(pts, T, 60.0) == 3
        d.detect()
        rep = d.last_report()
        print(rep)
        assert rep["new_id"] == 3 and sorted(int(c) for c in rep["candidates"]) == [0, 2]
    finally:
        d.close()


def _session(sw, scene, tmp):
    MC.start_mapping(sw)
    held = dict(points={}, poses={}, stamps={})
    frames = MC.keyframes(scene)
    MC.push(sw, frames, held)
    return frames, held


POSE_TOL = 4 * 2.0 ** -24 * 8.3


def _pose_bound(v):
    """KeyFrame::save (slam/common/keyframe.cpp:118-133) writes the matrix through Eigen's operator<<, 6 significant digits: half a unit of the
    sixth digit of the value, plus the f32 the loaded pose is handed out in"""
    a = np.abs(np.asarray(v, np.float64))
    digit = np.where(a > 0, 0.5 * 10.0 ** (np.floor(np.log10(np.where(a > 0, a, 1.0))) - 5), 0.0)
    return digit + 2.0 ** -23 * a


def test_round_trip_through_disk(tmp_path):
    """mapping mode -> dump_odometry / dump_graph / dump_keyframe (the saving thread's calls) -> localisation mode.  Pose bound: _pose_bound, the
    sixth significant digit of `data`."""
    import slam_wrapper as sw

    scene = MC.scene()
    roots = [str(tmp_path / "map1"), str(tmp_path / "map2")]
    frames, held = _session(sw, scene, tmp_path)
    try:
        live = sw.get_graph_map()  # mapping mode: the key frames handed out so far
        assert sorted(live["stamps"], key=int) == [str(k) for k in range(MC.N_KEYFRAMES)] and live["images"]["0"] == {}
        for k in range(MC.N_KEYFRAMES):
            assert np.array_equal(live["points"][str(k)], held["points"][str(k)]) and live["points"][str(k)].dtype == np.float32
            # the pose is the graph's estimate: odom2map * odometry, and odom2map goes through a Matrix4f (12 entries rounded to 2^-24 relative, a
            # row of three of them against a translation of up to L = 8.3 m), then the f32 it is handed out in: 4 * 2^-24 * L = 2e-6
            assert live["poses"][str(k)].dtype == np.float32 and np.abs(live["poses"][str(k)].astype(np.float64) - frames[k][1]).max() <= POSE_TOL
            assert live["stamps"][str(k)] == frames[k][2]
        saved = [MC.save_map(sw, r, held) for r in roots]
    finally:
        sw.deinit_slam()
    ids = [str(k) for k in range(MC.N_KEYFRAMES)]
    assert saved == [ids, ids]
    g = os.path.join(roots[0], "graph")
    assert sorted(os.listdir(g)) == sorted(["%06d" % k for k in range(MC.N_KEYFRAMES)] + ["graph.g2o", "graph.g2o.kernels", "map_info.txt", "odometrys.txt", "special_nodes.csv"])
    assert open(os.path.join(g, "special_nodes.csv")).read().split() == ["anchor_node", "-1", "anchor_edge", "-1", "floor_node", "-1"]
    rec = sw._read_g2o(os.path.join(g, "graph.g2o"))
    assert sorted(rec["vertices"]) == list(range(MC.N_KEYFRAMES)) and rec["fixed"] == [0] and rec["skipped"] == 0
    assert [(a, b) for a, b, _, _ in rec["edges"]] == [(k, k - 1) for k in range(1, MC.N_KEYFRAMES)]  # key frame -> the one before it
    for k in range(MC.N_KEYFRAMES):  # fewer than 10 edges: never optimised, the vertices are the key frames' poses
        assert np.abs(rec["vertices"][k][:3] - frames[k][1][:3, 3]).max() <= POSE_TOL
    for a, b, m, W in rec["edges"]:
        want = np.linalg.inv(frames[a][1]) @ frames[b][1]
        assert np.abs(m[:3] - want[:3, 3]).max() < 1e-9 and np.array_equal(W, W.T) and np.all(np.linalg.eigvalsh(W) > 0)

    assert sw.init_slam("offline", roots[0], "Localization", ["0-lidar", "IMU"], 0.2, 1.0, 10.0, 50.0) == ["0-lidar", "IMU"]
    sw.set_ins_external_param(0, 0, 0, 0, 0, 0)
    sw.set_imu_external_param(0, 0, 0, 0, 0, 0)
    assert sw.setup_slam() is True
    try:
        gm = sw.get_graph_map()
        assert sorted(gm["stamps"], key=int) == ids
        for i in ids:
            assert np.array_equal(gm["points"][i][:, :3], held["points"][i][:, :3])  # binary PCD: bit for bit
            assert np.array_equal(gm["points"][i][:, 3], held["points"][i][:, 3] * np.float32(255.0))  # dump_keyframe's scale
            assert gm["stamps"][i] == held["stamps"][i]
            err = np.abs(gm["poses"][i].astype(np.float64) - held["poses"][i].astype(np.float64))
            assert np.all(err <= _pose_bound(held["poses"][i])), (i, err.max())
        # the same map saved a second time is a map merge_map takes: every precondition holds (a refusal returns {})
        merged = sw.merge_map(roots[1])
        print("merge:", sw._last_merge())
        assert sorted(merged["points"], key=int) == [str(MC.N_KEYFRAMES + k) for k in range(MC.N_KEYFRAMES)]
        # localisation mode after a merge: the merged graph's record goes out the same way, the odometry list has gained its splitter
        out_dir = tmp_path / "merged"
        out_dir.mkdir()
        assert sw.dump_graph(str(out_dir)) == [str(k) for k in range(2 * MC.N_KEYFRAMES)]
        both = sw._read_g2o(str(out_dir / "graph.g2o"))
        assert sorted(both["vertices"]) == list(range(2 * MC.N_KEYFRAMES)) and 0 in both["fixed"] and len(both["edges"]) >= 2 * (MC.N_KEYFRAMES - 1)
        sw.dump_odometry(str(out_dir))
        assert open(str(out_dir / "odometrys.txt")).read().split() == ["0.000000"] * 7 + ["1.000000"]  # both maps' lists are empty: the zero pose alone
    finally:
        sw.deinit_slam()


def test_localises_in_the_saved_map(tmp_path):
    """A frame taken at key frame 4's pose localises after set_init_pose, to the bound of the walk of tests/test_outer_boundary.py (40 frames, 0.15 m
    after the first second, median 0.08 m), here standing still.  The map is the product-saved one: 8 key frames of 2 200 points in the yard of
    MC.scene(), whose size is worked out there from the localiser's 1 m NDT voxels.  (In the 200 m scene of the other localisation tests a map
    of this size cannot hold a pose whichever way it reached the disk: hand-written maps of 2 200-point frames ended 0.14 - 0.6 m off on an
    MI355X, the same poses with full 64 x 600 scans 7 mm.)"""
    import slam_wrapper as sw

    scene = MC.scene()
    root = str(tmp_path / "map")
    frames, held = _session(sw, scene, tmp_path)
    try:
        assert MC.filled_voxels(frames)[1] >= 100  # walls and boxes the map can hold x, y and yaw by
        MC.save_map(sw, root, held)
    finally:
        sw.deinit_slam()
    assert sw.init_slam("offline", root, "Localization", ["0-lidar", "IMU"], 0.2, 1.0, 10.0, 50.0) == ["0-lidar", "IMU"]
    sw.set_ins_external_param(0, 0, 0, 0, 0, 0)
    sw.set_imu_external_param(0, 0, 0, 0, 0, 0)
    assert sw.setup_slam() is True
    try:
        # a frame taken at key frame 4's pose localises after set_init_pose
        pos, q, T4 = MC.keyframe_pose(4)
        yaw = float(np.arctan2(T4[1, 0], T4[0, 0]))
        tr = synth.Trajectory(p0=tuple(pos), t_static=100.0, heading=yaw, sway=0.0, yaw_amp=0.0, pitch_amp=0.0, roll_amp=0.0)
        imu = synth.imu_stream(tr, 0.0, 4.3, rate=100.0, seed=5, gyr_sigma=1e-3, acc_sigma=1e-2)
        ii, errs, states = 0, [], []
        for k in range(0, 41):  # the walk's 40 frames
            tb = k * 0.1
            rows = []
            while ii < len(imu) and imu[ii][0] <= tb:
                t, gy, ac = imu[ii]
                rows.append([t * 1e6, *(gy * 180.0 / np.pi), *(ac / 9.81)])
                ii += 1
            pts, st = synth.make_sweep(scene, tr, tb, seed=500 + k, n_az=900, fov_deg=(-24.8, 2.0))
            attr = dict(timestamp=int(round(tb * 1e6)), points_attr=np.stack([st.astype(np.float32), np.zeros(len(st), np.float32)], 1))
            out = sw.process({"0-lidar": pts}, {"0-lidar": attr}, {}, {}, {}, {}, np.array(rows, np.float64).reshape(-1, 7), int(round(tb * 1e6)))
            if k == 0:
                assert out["pose"]["state"] == "Initializing"
                sw.set_init_pose(pos[0] + 0.2, pos[1] - 0.15, pos[2], np.degrees(yaw) + 1.0, 0.0, 0.0)
                continue
            errs.append(float(np.linalg.norm(out["pose"]["odom_matrix"][:3, 3] - pos)))
            states.append(out["pose"]["state"])
        print("localisation in the saved map: position error median %.3f m, max after the first second %.3f m, states %s" % (np.median(errs), max(errs[10:]), states[-1]))
        assert max(errs[10:]) < 0.15 and np.median(errs) < 0.08
        assert states[-1] == "Localizing(L)"
    finally:
        sw.deinit_slam()


def test_deleted_vertex_leaves_graph_bank_and_map(tmp_path):
    import slam_wrapper as sw

    scene = MC.scene()
    frames, held = _session(sw, scene, tmp_path)
    try:
        assert [sorted(v) for v in sw.get_graph_edges().values()] == [[k - 1, k] for k in range(1, MC.N_KEYFRAMES)]
        sw.del_graph_vertex(3)
        sw.del_graph_vertex(3)  # a second time, and an id the graph never had: a warning, nothing else
        sw.del_graph_vertex(99)
        keep = [str(k) for k in range(MC.N_KEYFRAMES) if k != 3]
        out_dir = tmp_path / "graph"
        out_dir.mkdir()
        assert sw.dump_graph(str(out_dir)) == keep
        rec = sw._read_g2o(str(out_dir / "graph.g2o"))
        assert sorted(rec["vertices"]) == [int(k) for k in keep] and all(3 not in (a, b) for a, b, _, _ in rec["edges"]) and len(rec["edges"]) == MC.N_KEYFRAMES - 3
        edges, meta = sw.get_graph_edges(), sw.get_graph_meta()
        assert len(edges) == MC.N_KEYFRAMES - 3 and all(3 not in pair for pair in edges.values())
        assert sorted(meta["vertex"], key=int) == keep and all(3 not in (e["prev"], e["next"]) for e in meta["edge"].values()) and sorted(meta["edge"]) == sorted(edges)
        assert meta["vertex"]["2"]["edge_num"] == 1 and meta["vertex"]["4"]["edge_num"] == 1 and meta["vertex"]["0"]["fix"] is True
        gm = sw.get_graph_map()
        assert sorted(gm["stamps"], key=int) == keep and all(np.array_equal(gm["points"][k], held["points"][k]) for k in keep)
        # a further key frame at frame 3's pose, far enough along the drive to be matched against the early frames: frame 3 would be the candidate
        pts, T, _, _ = MC.keyframes(scene, 4, seed0=900)[3]
        n_before = len(sw.get_loop_edges())
        sw._push_keyframe(pts, T, 5_000_000, 60.0)
        d = sw.update_odom()
        assert len(d["keyframes"]) == 1
        loops = sw.get_loop_edges()
        print("loops after the deletion:", [(e["key1"], e["key2"], e["score"]) for e in loops[n_before:]])
        assert all(3 not in (e["key1"], e["key2"]) for e in loops[n_before:])
        edges = sw.get_graph_edges()
        assert [8, 7] in list(edges.values()) and all(3 not in pair for pair in edges.values())  # the new frame's odometry edge goes to the last frame left
        odoms = sw.run_graph_optimization()
        assert sorted(odoms, key=int) == keep + ["8"] and all(np.isfinite(np.asarray(T)).all() for T in odoms.values())
        assert sorted(sw.get_graph_map()["stamps"], key=int) == keep + ["8"]
    finally:
        sw.deinit_slam()


def test_dump_odometry_in_mapping_mode(tmp_path):
    import slam_wrapper as sw
    from test_outer_boundary import _drive

    assert sw.init_slam("mapping", "", "FastLIO", ["0-lidar", "IMU"], 0.5, 1.0, 10.0, 100) == ["IMU", "0-lidar"]
    sw._set_capacity(4_000_000, 1 << 20)
    sw.set_ins_external_param(0.30, 0.10, -0.20, -4.0, 1.0, 2.0)
    sw.set_imu_external_param(0.05, -0.02, 0.10, 3.0, 0.5, -1.0)
    assert sw.setup_slam() is True
    try:
        ends = []

        def process(*a):
            out = sw.process(*a)
            ends.append(sw._last_odometry()[1])
            return out

        _drive(process, n=4)
        sw.dump_odometry(str(tmp_path))
    finally:
        sw.deinit_slam()
    lines = open(str(tmp_path / "odometrys.txt")).read().splitlines()
    assert len(lines) == 4 and all(re.match(r"^\d+\.\d{6}( -?\d+\.\d{6}){7}$", ln) for ln in lines), lines
    for k, (ln, T) in enumerate(zip(lines, ends)):
        v = [float(x) for x in ln.split()]
        assert abs(v[0] - (0.1 * k + 0.1)) < 1e-6  # the end-of-scan stamp
        assert np.abs(np.array(v[1:4]) - T[:3, 3]).max() <= 1e-6  # the format's own rounding (half a unit of the sixth decimal, and the decimal's own f64)
        assert abs(np.linalg.norm(v[4:]) - 1.0) < 2e-6


def test_dump_odometry_in_localisation_mode(tmp_path):
    """the loaded map's graph/odometrys.txt comes back.  The file's quaternions are exact in 6 decimals and of unit length, so reading (no
    normalisation, as MapLoader::loadOdometry) and writing give every number back to the format's rounding, 1e-6"""
    import slam_wrapper as sw

    scene = MC.scene()
    root = str(tmp_path / "map")
    frames, held = _session(sw, scene, tmp_path)
    try:
        MC.save_map(sw, root, held)
    finally:
        sw.deinit_slam()
    rows = [[12.5, 1.25, -2.5, 0.125, 0.0, 0.0, 0.0, 1.0], [12.625, 1.75, -2.25, 0.25, 0.0, 0.0, 0.6, 0.8], [12.75, 2.5, -2.0, 0.375, 0.6, 0.0, 0.0, 0.8],
            [12.875, 3.25, -1.5, 0.5, 0.0, 0.28, 0.0, 0.96]]
    with open(os.path.join(root, "graph", "odometrys.txt"), "w") as f:
        for r in rows:
            f.write(" ".join("%.6f" % v for v in r) + "\n")
    assert sw.init_slam("offline", root, "Localization", ["0-lidar", "IMU"], 0.2, 1.0, 10.0, 50.0) == ["0-lidar", "IMU"]
    sw.set_ins_external_param(0, 0, 0, 0, 0, 0)
    sw.set_imu_external_param(0, 0, 0, 0, 0, 0)
    assert sw.setup_slam() is True
    try:
        sw.dump_odometry(str(tmp_path))
    finally:
        sw.deinit_slam()
    got = np.array([[float(x) for x in ln.split()] for ln in open(str(tmp_path / "odometrys.txt")).read().splitlines()])
    assert got.shape == (4, 8) and np.abs(got - np.array(rows)).max() <= 1e-6
