"""Loop detection on the device (lio_loop_*, csrc/loop.hip): the batched coarse matcher against the single-pair lio.Gicp in voxel mode, against
the vectors the reference's FastVGICP / FastGICP wrote (tests/golden/loop.npz, tools/record_loop_golden.py), the covariance cache, a closed
drive, the corners, and the slam_wrapper switch."""
import os

import numpy as np
import pytest

import keyframe_cases as kc
import loop_cases as LC
from lsd_amd import capi, lio

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "loop.npz"))
I4 = np.eye(4)
_cache = {}


def _five():
    if "five" not in _cache:
        _cache["five"] = LC.five_candidates()
    return _cache["five"]


def _drive_frames():
    if "drive" not in _cache:
        _cache["drive"] = LC.drive()
    return _cache["drive"]


def _single(target, source, guess, max_points):
    g = lio.Gicp(grid_resolution=1.0, max_points=max_points, k=20)
    try:
        g.set_voxel_mode(1.0, 1)
        g.set_target(target)
        g.set_source(source)
        return g.align(guess, transformation_epsilon=0.1, rotation_epsilon_deg=0.1)
    finally:
        g.close()


def _close(T, ref):
    return np.abs(T[:3, 3] - ref[:3, 3]).max() < 1e-4 and np.abs(T[:3, :3] - ref[:3, :3]).max() < 1e-5  # BASELINE.json: 1e-4 m, 1e-5 rad


def test_batch_equals_single():
    tgt, cands, guesses = _five()
    rng = np.random.default_rng(5)
    big = np.concatenate([cands[0], cands[1] + np.array([0.013, 0.007, 0.003, 0], np.float32), cands[2] + np.array([-0.011, 0.009, 0.005, 0], np.float32)])
    srcs = [cands[0][rng.choice(len(cands[0]), 20, replace=False)],  # exactly k points
            cands[1][:128 * 9 + 1],                                    # one more than a multiple of the cost kernel's block (128)
            big,                                                       # much larger than the rest
            cands[3],
            cands[4]]                                                  # the guess 50 m off: no correspondence
    off = guesses[4].copy()
    off[0, 3] += 50.0
    gs = [guesses[0], guesses[1], guesses[0], guesses[3], off]
    M = 16384
    assert len(big) <= M
    d = lio.LoopDetector(max_points=M)
    try:
        t = d.add_keyframe(tgt, I4, 0.0)
        ids = [d.add_keyframe(s, I4, 0.0) for s in srcs]
        want = [_single(tgt, s, g, M) for s, g in zip(srcs, gs)]
        assert any(w[1] for w in want[:4])
        full = d.align_candidates(t, ids, gs)
        for K in (1, 3, 5):
            got = d.align_candidates(t, ids[:K], gs[:K])
            for j in range(K):
                T, conv, it, score, nr = got[j]
                wT, wconv, wit = want[j]
                print(f"K={K} job {j}: n={len(srcs[j])} conv={conv}/{wconv} it={it}/{wit} |dT|={np.abs(T - wT).max():.3e} score={score:.6g} nr={nr}")
                assert conv == wconv and it == wit
                assert np.abs(T - wT).max() < 1e-9
                # a slot's numbers do not depend on the batch it ran in
                assert np.array_equal(T, full[j][0]) and (score, nr) == full[j][3:]
        # permuted slots: every job bit-identical; twice: bit-identical
        perm = [3, 0, 4, 2, 1]
        gp = d.align_candidates(t, [ids[p] for p in perm], [gs[p] for p in perm])
        for slot, p in enumerate(perm):
            assert np.array_equal(gp[slot][0], full[p][0]) and gp[slot][1:] == full[p][1:]
        again = d.align_candidates(t, ids, gs)
        assert all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(again, full))
    finally:
        d.close()


def test_against_reference_vectors():
    tgt, cands, guesses = _five()
    assert [len(tgt)] + [len(c) for c in cands] == GOLD["five/n_points"].tolist()
    d = lio.LoopDetector(max_points=16384)
    try:
        t = d.add_keyframe(tgt, I4, 0.0)
        ids = [d.add_keyframe(c, I4, 0.0) for c in cands]
        got = d.align_candidates(t, ids, guesses)
        conv, scores = [], []
        for j, (T, c, it, score, nr) in enumerate(got):
            print(f"candidate {j}: conv={c} it={it} score={score:.9g} nr={nr} ref it={GOLD['five/iterations'][j]} score={GOLD['five/score'][j]:.9g}")
            assert c == bool(GOLD["five/converged"][j]) and it == int(GOLD["five/iterations"][j])
            assert _close(T, GOLD["five/T"][j].astype(np.float64))
            conv.append(c)
            scores.append(score)
            if c:
                ws, wnr = LC.fitness(tgt, cands[j], T)  # numpy brute force under the project's f32 rule, at the device's own transform
                assert nr == wnr and abs(score - ws) <= 1e-12 * ws
            else:
                assert score == LC.DBL_MAX and nr == 0
            assert nr == int(GOLD["five/nr"][j])  # the count at the reference's own transform
        best, _ = LC.select(conv, scores)
        assert best == int(GOLD["five/best"])
        T, c, it, score, nr = d.align_fine(t, ids[best], got[best][0].astype(np.float32).astype(np.float64))
        print(f"fine: conv={c} it={it} score={score:.9g} ref it={int(GOLD['five/fine_iterations'])} score={float(GOLD['five/fine_score']):.9g}")
        assert c == bool(GOLD["five/fine_converged"]) and _close(T, GOLD["five/fine_T"].astype(np.float64))
        ws, wnr = LC.fitness(tgt, cands[best], T)
        assert nr == wnr and abs(score - ws) <= 1e-12 * ws
        assert nr == int(GOLD["five/fine_nr"])
    finally:
        d.close()


def _rows(dev_pts, pts):
    """perm with dev_pts[i] == pts[perm[i]]; the clouds have no duplicate points"""
    key = lambda a: np.ascontiguousarray(a[:, :3]).view([("x", "f4"), ("y", "f4"), ("z", "f4")]).ravel()
    ka, kb = key(dev_pts), key(pts)
    ob = np.argsort(kb)
    perm = ob[np.searchsorted(kb[ob], ka)]
    assert np.array_equal(pts[perm, :3], dev_pts[:, :3])
    return perm


def test_covariance_cache():
    tgt, cands, guesses = _five()
    M = 8192
    d = lio.LoopDetector(max_points=M)
    g = lio.Gicp(grid_resolution=1.0, max_points=M, k=20)
    try:
        t = d.add_keyframe(tgt, I4, 0.0)
        a = d.add_keyframe(cands[0], I4, 0.0)
        g.set_source(cands[0])
        wp, wc = g.download(1)
        p0, c0 = d.download_keyframe(a)
        # the bank keeps a frame in the order it was added in; lio.Gicp keeps its source in hash-grid order (inside a cell: arrival order, which
        # is any order), so the two are compared row by row: every point with all four fields, every covariance with all its bits
        assert np.array_equal(p0.view(np.uint32), np.ascontiguousarray(cands[0], np.float32).view(np.uint32))
        perm = _rows(wp, p0)
        assert np.array_equal(wp.view(np.uint32), p0[perm].view(np.uint32)) and np.array_equal(wc, c0[perm])
        for _ in range(2):  # a candidate twice (with another frame through the engine in between)
            d.align_candidates(t, [a], [guesses[0]])
            d.add_keyframe(cands[1], I4, 0.0)
        p1, c1 = d.download_keyframe(a)
        assert np.array_equal(p1.view(np.uint32), p0.view(np.uint32)) and np.array_equal(c1, c0)
        with pytest.raises(capi.LioError):
            d.add_keyframe(cands[0][:19], I4, 0.0)  # n < k
    finally:
        g.close()
        d.close()


def _run_drive(d, frames):
    edges, reports = [], []
    for cloud, pose, accum in frames:
        d.add_keyframe(cloud, pose, accum)
        edges += d.detect()
        reports.append(d.last_report())
    return edges, reports


def test_drive():
    frames = _drive_frames()
    assert [len(f[0]) for f in frames] == GOLD["drive/n_points"].tolist()
    want = [tuple(e) for e in GOLD["drive/edges"].tolist()]
    d = lio.LoopDetector(max_points=16384)
    try:
        edges, reports = _run_drive(d, frames)
        print("edges", [(e["key1"], e["key2"], e["score"]) for e in edges], "want", want, GOLD["drive/edge_score"])
        assert [(e["key1"], e["key2"]) for e in edges] == want
        for e, wT, ws in zip(edges, GOLD["drive/edge_pose"], GOLD["drive/edge_score"]):
            assert _close(e["relative_pose"].astype(np.float64), wT.astype(np.float64))
            assert np.array_equal(e["information"], LC.information_matrix(e["score"]))
        # every recorded matching: the same candidates, the same per-candidate outcome, the same choice
        by_id = {r["new_id"]: r for r in reports if r["new_id"] >= 0 and len(r["candidates"])}
        for m, nid in enumerate(GOLD["drive/new_id"].tolist()):
            k = int(GOLD["drive/n_candidates"][m])
            r = by_id[nid]
            assert r["candidates"].tolist() == GOLD["drive/candidates"][m, :k].tolist()
            assert r["converged"].tolist() == GOLD["drive/converged"][m, :k].tolist() and r["iterations"].tolist() == GOLD["drive/iterations"][m, :k].tolist()
            assert r["best"] == int(GOLD["drive/best"][m])
        accum = [f[2] for f in frames]
        first_revisit = min(int(n) for n in GOLD["drive/new_id"])
        assert all(e["key1"] >= first_revisit for e in edges)  # no edge before the start comes back into reach
        k1 = [e["key1"] for e in edges]
        assert all(accum[b] - accum[a] >= 15.0 for a, b in zip(k1, k1[1:]))  # no second edge inside 15 m of travel after one
        assert d.edges() and [(e["key1"], e["key2"]) for e in d.edges()] == want
        # reset, the same drive: the same bits
        d.reset()
        assert d.num_keyframes() == (0, 0) and d.edges() == []
        again, _ = _run_drive(d, frames)
        assert len(again) == len(edges)
        for a, b in zip(again, edges):
            assert (a["key1"], a["key2"], a["score"]) == (b["key1"], b["key2"], b["score"]) and np.array_equal(a["relative_pose"], b["relative_pose"])
    finally:
        d.close()


def test_corners():
    tgt, cands, guesses = _five()
    d = lio.LoopDetector(max_points=8192)
    try:
        # no candidate: nothing is launched, no edge
        d.add_keyframe(tgt, I4, 10.0)
        assert d.detect() == []
        r = d.last_report()
        assert r["new_id"] == 0 and len(r["candidates"]) == 0 and r["reason"] == "no_candidate" and r["coarse_rounds"] == 0
        t = d.last_times()
        assert t["coarse_us"] == 0 and t["fitness_us"] == 0 and t["fine_us"] == 0
        # every candidate not converged (the estimates put the candidate 80 m along x inside the new frame: no point meets a voxel) -> no edge
        d2 = lio.LoopDetector(max_points=8192, distance_thresh=200.0)
        try:
            d2.add_keyframe(tgt, I4, 10.0)
            assert d2.detect() == []
            d2.set_pose(0, np.array([[1, 0, 0, 80.0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]))
            d2.add_keyframe(cands[0], I4, 50.0)
            assert d2.detect() == []
            r = d2.last_report()
            assert r["new_id"] == 1 and r["candidates"].tolist() == [0] and not r["converged"].any() and r["best"] == -1 and r["reason"] == "coarse_score"
            assert r["coarse_rounds"] > 0 and r["best_score"] == LC.DBL_MAX
        finally:
            d2.close()
        # nr = 0: a source 200 m from every target point (every squared distance above 25) scores DBL_MAX
        away = cands[0].copy()
        away[:, 0] += 200.0
        a = d.add_keyframe(away, I4, 60.0)
        T, conv, it, score, nr = d.align_fine(0, a, I4)
        assert nr == 0 and score == LC.DBL_MAX
        # ... and no edge.  Through detect: the estimates put the far frame on top of frame 0, where it is a candidate; no point of it meets a
        # voxel of the new frame, the solver reports the zero pivot (include/lio_hip.h, the third deviation) and the candidate is skipped as not
        # converged with its score left at DBL_MAX -- matching cannot score nr = 0 any other way, a converged alignment has brought points together
        d3 = lio.LoopDetector(max_points=8192)
        try:
            d3.add_keyframe(away, I4, 0.0)
            assert d3.detect() == []
            d3.add_keyframe(tgt, I4, 60.0)
            assert d3.detect() == [] and d3.edges() == []
            r = d3.last_report()
            assert r["new_id"] == 1 and r["candidates"].tolist() == [0] and r["best"] == -1 and r["best_score"] == LC.DBL_MAX and r["reason"] == "coarse_score"
        finally:
            d3.close()
        assert d.detect() == [] and d.edges() == []
    finally:
        d.close()


def test_cap_too_small():
    """a loop out of a detect call that was given no room: -(count), the work is done all the same and the edge is read with lio_loop_edges"""
    frames = _drive_frames()
    want = [tuple(e) for e in GOLD["drive/edges"].tolist()]
    d = lio.LoopDetector(max_points=16384)
    try:
        k1 = want[0][0]
        for cloud, pose, accum in frames[:k1]:
            d.add_keyframe(cloud, pose, accum)
        assert d.detect() == []
        d.add_keyframe(*frames[k1])
        buf = (capi.LoopEdge * 1)()
        assert capi.lib().lio_loop_detect(d.h, None, 0) == -1  # one loop, no room: -(count)
        assert capi.lib().lio_loop_edges(d.h, buf, 1) == 1 and (buf[0].key1, buf[0].key2) == want[0]
        assert d.num_keyframes() == (k1 + 1, 0)
    finally:
        d.close()


def test_wrapper_loop_detection():
    import slam_wrapper as sw
    from test_outer_boundary import _drive as boundary_drive, _rpyt

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device")
    cfg = dict(accum_distance_thresh=0.5, distance_from_last_edge_thresh=0.5, distance_new_keyframe_thresh=0.1, distance_keyframe_thresh=0.1)
    imu_ext, ins_ext = (0.05, -0.02, 0.10, 3.0, 0.5, -1.0), (0.30, 0.10, -0.20, -4.0, 1.0, 2.0)
    assert sw.init_slam("mapping", "", "FastLIO", ["0-lidar", "IMU"], 0.5, 0.2, 10.0, 60.0) == ["IMU", "0-lidar"]
    sw._set_capacity(4_000_000, 1 << 20)
    sw.set_ins_external_param(*ins_ext)
    sw.set_imu_external_param(*imu_ext)
    sw.set_loop_detection(True)
    sw.set_loop_config(cfg)
    assert sw.setup_slam() is True
    fed, groups, status = [], [], []

    def process(points, attr, a, b, c, d, imu, stamp):
        out = sw.process(points, attr, a, b, c, d, imu, stamp)
        fed.append((points["0-lidar"], attr["0-lidar"]["points_attr"][:, 0].astype(np.uint32), attr["0-lidar"]["timestamp"], *sw._last_odometry()))
        groups.append(len(sw.update_odom()["keyframes"]))
        status.append(sw.get_graph_status()["loop_detected"])
        return out

    try:
        boundary_drive(process, n=24)
        got = sw.get_loop_edges()
        assert sw.get_graph_edges() == {}
    finally:
        sw.deinit_slam()
    T_static = _rpyt(*ins_ext)
    print("key frames per call", groups, "loops", [(e["key1"], e["key2"], e["score"]) for e in got])
    assert sum(groups) >= 3 and len(got) >= 1
    assert status[-1] and status == sorted(status)  # turns True and stays
    k = lio.KeyFramer(key_frame_distance=float(np.float32(0.2)), key_frame_degree=10.0, resolution=0.5, key_frame_range=60.0)
    d = lio.LoopDetector(**cfg)
    try:
        want = []
        for (pts, st, header, first, second), n_out in zip(fed, groups):
            k.push(kc.transform_f64(pts, T_static), st, header, first, delta=kc.rigid_inverse(first) @ second)
            assert k.pending() == n_out
            banked = 0
            for _ in range(n_out):
                f = k.pop()
                if len(f["points"]) >= 20:
                    d.add_keyframe(f["points"], f["pose"], f["accum_distance"])
                    banked += 1
            if banked:
                want += d.detect()
        assert [(e["key1"], e["key2"]) for e in got] == [(e["key1"], e["key2"]) for e in want]
        for a, b in zip(got, want):
            assert np.array_equal(a["relative_pose"], b["relative_pose"]) and a["score"] == b["score"] and np.array_equal(a["information"], b["information"])
            assert a["relative_pose"].dtype == np.float32 and a["relative_pose"].shape == (4, 4) and a["information"].shape == (6, 6)
    finally:
        k.close()
        d.close()
