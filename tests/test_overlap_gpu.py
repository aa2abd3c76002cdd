"""Overlap detection on the device (lio_overlap_*, csrc/overlap.hip): the coarse batch over several targets against the loop detector's
per-target batch, the range-gated fitness, the accumulated fine target and one detect() call over the two-map scene, all against the numpy
restatement (tests/overlap_cases.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import keyframe_cases as KC
import loop_cases as LC
import overlap_cases as OC
from lsd_amd import capi, lio

pytestmark = pytest.mark.gpu
I4 = np.eye(4)
_cache = {}


def _five():
    if "five" not in _cache:
        _cache["five"] = LC.five_candidates()
    return _cache["five"]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_align_pairs_equals_per_target_batches():
    tgt, cands, guesses = _five()
    rng = np.random.default_rng(5)
    big = np.concatenate([cands[0], cands[1] + np.array([0.013, 0.007, 0.003, 0], np.float32), cands[2] + np.array([-0.011, 0.009, 0.005, 0], np.float32)])
    inv = np.linalg.inv
    g31 = (inv(guesses[3]) @ guesses[1]).astype(np.float32).astype(np.float64)  # candidate 1 seen from candidate 3
    g30 = (inv(guesses[3]) @ guesses[0]).astype(np.float32).astype(np.float64)
    g02 = (inv(guesses[0]) @ guesses[2]).astype(np.float32).astype(np.float64)
    off = g30.copy()
    off[2, 3] += 50.0  # 50 m above the target: no point meets a voxel (along x the scene's far wall would land on the near one)
    M = 16384
    assert len(big) <= M
    for max_candidates in (64, 2):  # 2: the six pairs go through three launch sets
        d = lio.LoopDetector(max_points=M, max_candidates=max_candidates)
        o = lio.OverlapDetector(d)
        try:
            t0, t1, t2 = d.add_keyframe(tgt, I4, 0.0), d.add_keyframe(cands[3], I4, 0.0), d.add_keyframe(cands[0], I4, 0.0)
            s20 = d.add_keyframe(cands[0][rng.choice(len(cands[0]), 20, replace=False)], I4, 0.0)  # exactly k points
            s1153 = d.add_keyframe(cands[1][:128 * 9 + 1], I4, 0.0)                                  # one more than a multiple of the block
            sbig = d.add_keyframe(big, I4, 0.0)                                                      # three times the rest
            s4 = d.add_keyframe(cands[4], I4, 0.0)
            s2 = d.add_keyframe(cands[2], I4, 0.0)
            # targets with {1, 3, 2} sources; the guess 50 m off meets no voxel; the last pair twice
            pairs = [(t0, s20, guesses[0]), (t1, s1153, g31), (t1, sbig, g30), (t1, s4, off), (t2, s2, g02), (t2, s2, g02)]
            want = []
            for t in (t0, t1, t2):
                mine = [p for p in pairs if p[0] == t]
                want += [r[:3] for r in d.align_candidates(t, [p[1] for p in mine], [p[2] for p in mine])]
            got = o.align_pairs([p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs])
            for j, (g, w) in enumerate(zip(got, want)):
                print(f"max_candidates={max_candidates} pair {j}: conv={g[1]}/{w[1]} it={g[2]}/{w[2]} |dT|={np.abs(g[0] - w[0]).max():.3e}")
            assert all(_same(g, w) for g, w in zip(got, want))
            assert [w[1] for w in want][3] is False and any(w[1] for w in want[:3]) and _same(got[4], got[5])
            tm = o.last_times()
            assert tm["n_pairs"] == 6 and tm["n_targets"] == 3 and tm["coarse_rounds"] > 0 and tm["coarse_us"] > 0
            # any order of the pairs: every pair the same bits; twice: the same bits
            perm = [3, 5, 0, 2, 4, 1]
            gp = o.align_pairs([pairs[p][0] for p in perm], [pairs[p][1] for p in perm], [pairs[p][2] for p in perm])
            assert all(_same(gp[slot], got[p]) for slot, p in enumerate(perm))
            assert all(_same(a, b) for a, b in zip(o.align_pairs([p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs]), got))
            # the bank's own path still answers after its engine served other targets
            assert all(_same(a[:3], b) for a, b in zip(d.align_candidates(t1, [s1153, sbig, s4], [g31, g30, off]), want[1:4]))
        finally:
            o.close()
            d.close()


def _gate_check(got, want, what):
    (s, nr, n_in), (ws, wnr, wn_in) = got, want
    print(f"{what}: score={s:.12g}/{ws:.12g} nr={nr}/{wnr} n_in={n_in}/{wn_in}")
    assert (nr, n_in) == (wnr, wn_in)
    assert (s == ws == LC.DBL_MAX) if wnr == 0 else abs(s - ws) <= 1e-12 * ws  # tests/test_loop_gpu.py's tolerance for the fitness


def test_gate():
    tgt, cands, guesses = _five()
    f = np.float32
    # planted rows: z == 0.5 exactly and sqrtf(x^2 + y^2) == 100 exactly (3600 + 6400) are excluded by the strict comparisons; their neighbours
    # just inside count.  The far rows come as a cluster (a bank frame's covariances search the k nearest of every row)
    far_in = np.array([[59.9 - 0.01 * i, 79.9 - 0.01 * j, 2.0 + 0.1 * i, 1.0] for i in range(5) for j in range(5)], f)
    assert (np.sqrt(far_in[:, 0] ** 2 + far_in[:, 1] ** 2) < f(100)).all()
    planted = np.concatenate([np.array([[60.0, 80.0, 2.0, 1.0], [80.0, 60.0, 3.0, 1.0], [3.0, 3.0, 0.5, 1.0], [-4.0, 2.0, 0.5, 1.0]], f), far_in])
    assert OC.range_filter(planted).tolist() == [False] * 4 + [True] * 25
    tgt_p = np.concatenate([tgt[:700], planted, tgt[700:]])
    src_p = np.concatenate([planted + np.array([0, 0, 0, 0], f), cands[0]])
    floor = tgt.copy()
    floor[:, 2] = -np.abs(floor[:, 2])  # nothing of it passes z > 0.5
    down = I4.copy()
    down[2, 3] = -100.0                 # ... and nothing of a source moved by it
    d = lio.LoopDetector(max_points=16384, max_candidates=3)  # 3: the seven sources go through three launches
    o = lio.OverlapDetector(d)
    try:
        t = d.add_keyframe(tgt_p, I4, 0.0)
        ids = [d.add_keyframe(c, I4, 0.0) for c in cands]
        sp, s257, tf = d.add_keyframe(src_p, I4, 0.0), d.add_keyframe(cands[1][:257], I4, 0.0), d.add_keyframe(floor, I4, 0.0)
        srcs = {**{i: c for i, c in zip(ids, cands)}, sp: src_p, s257: cands[1][:257]}
        jobs = [(i, g) for i, g in zip(ids, guesses)] + [(sp, I4), (s257, guesses[1])]
        for max_range in (1.0, 25.0):
            got = o.gate(t, [j[0] for j in jobs], [j[1] for j in jobs], max_range)
            for (sid, T), g in zip(jobs, got):
                _gate_check(g, OC.gated_fitness(tgt_p, srcs[sid], T, max_range), f"max_range {max_range} source {sid}")
        # the planted source under the identity: the four boundary rows are not among the survivors, the 25 inside rows are, and each of those
        # finds itself in the target (the boundary rows of the target are not there to be found: the far cluster's nearest is 0)
        s, nr, n_in = o.gate(t, [sp], [I4], 1.0)[0]
        assert n_in == 25 + int(OC.range_filter(cands[0]).sum())
        # a filter that empties the target; a filter that empties the source
        assert o.gate(tf, [ids[0]], [guesses[0]], 1.0) == [(LC.DBL_MAX, 0, int(OC.range_filter(KC.transform_f32(cands[0], guesses[0])).sum()))]
        assert o.gate(t, [ids[0]], [down], 1.0) == [(LC.DBL_MAX, 0, 0)]
        assert o.gate(t, [s257], [guesses[1]], 1.0) == o.gate(t, [ids[0], s257], [guesses[0], guesses[1]], 1.0)[1:]
    finally:
        o.close()
        d.close()


def _rows(dev_pts, pts):
    """perm with dev_pts[i] == pts[perm[i]]; the clouds have no duplicate points"""
    key = lambda a: np.ascontiguousarray(a[:, :3]).view([("x", "f4"), ("y", "f4"), ("z", "f4")]).ravel()
    ka, kb = key(dev_pts), key(pts)
    ob = np.argsort(kb)
    perm = ob[np.searchsorted(kb[ob], ka)]
    assert np.array_equal(pts[perm, :3], dev_pts[:, :3])
    return perm


def test_accumulate():
    tgt, cands, _ = _five()
    poses = [LC._pose(0.5, -1.0, 0.2), LC._pose(1.7, -0.2, 0.31) @ LC._pose(0.0, 0.0, 0.0, z=0.07), LC._pose(-0.4, 0.3, 0.05), LC._pose(2.9, 1.1, 0.52)]
    clouds = [tgt, cands[0], cands[1], cands[2]]
    d = lio.LoopDetector(max_points=8192)
    want = OC.accumulate(clouds, poses, 1, [3, 0, 2])  # the order given, not the id order
    o = lio.OverlapDetector(d, max_accum_points=len(want))
    g = lio.Gicp(grid_resolution=1.0, max_points=len(want), k=20)
    try:
        ids = [d.add_keyframe(c, T, 0.0) for c, T in zip(clouds, poses)]
        pts, cov = o.accumulate(ids[1], [ids[3], ids[0], ids[2]])
        assert pts.shape == want.shape and np.array_equal(pts.view(np.uint32), want.view(np.uint32))
        g.set_target(want)
        gp, gc = g.download(0)
        perm = _rows(gp, want)
        assert np.array_equal(cov[perm], gc)
        # the accumulated cloud as the gate's target
        got = o.gate(o.ACCUM, [ids[0]], [OC.rel_pose(poses[1], poses[0])], 25.0)[0]
        _gate_check(got, OC.gated_fitness(want, tgt, OC.rel_pose(poses[1], poses[0]), 25.0), "accumulated target")
        # one point beyond max_accum_points
        extra = d.add_keyframe(cands[3][:20], I4, 0.0)
        nb = np.array([ids[3], ids[0], ids[2], extra], np.int32)
        rc = capi.lib().lio_overlap_accumulate(o.h, ids[1], nb.ctypes.data_as(C.POINTER(C.c_int32)), 4)
        assert rc == capi.LIO_E_CAPACITY
        o2 = lio.OverlapDetector(d, max_accum_points=len(want) - 1)
        try:
            assert capi.lib().lio_overlap_accumulate(o2.h, ids[1], nb.ctypes.data_as(C.POINTER(C.c_int32)), 3) == capi.LIO_E_CAPACITY
        finally:
            o2.close()
        assert o.accumulate(ids[1], [])[0].shape == cands[0].shape  # no neighbour: the best frame alone
    finally:
        g.close()
        o.close()
        d.close()


def _close(T, ref):
    return np.abs(T[:3, 3] - ref[:3, 3]).max() < 1e-4 and np.abs(T[:3, :3] - ref[:3, :3]).max() < 1e-5  # BASELINE.json: 1e-4 m, 1e-5 rad


def _bank(d, sc):
    """both maps into the bank: key-frame id -> bank id"""
    return {k: d.add_keyframe(sc["clouds"][k], sc["poses"][k], 0.0) for k in sc["ref_ids"] + sc["new_ids"]}


def test_detect_two_maps():
    sc, want_edges, recs = OC.scene_restatement()
    d = lio.LoopDetector(max_points=16384)
    o = lio.OverlapDetector(d)
    try:
        runs = []
        for run in range(2):
            bank = _bank(d, sc)
            kf = {b: k for k, b in bank.items()}
            ref, new = [bank[k] for k in sc["ref_ids"]], [bank[k] for k in sc["new_ids"]]
            edges = o.detect(ref, new, sc["edges"], ref_kf=sc["ref_ids"], new_kf=sc["new_ids"])
            runs.append((edges, o.last_report()))
            tm = o.last_times()
            if run == 0:  # the coarse transforms through the stage door: a pair's numbers do not depend on the batch it ran in
                coarse = {}
                for w in recs:
                    if w["candidates"]:
                        g = [OC.make_guess(sc["poses"][w["new_id"]], sc["poses"][c]) for c in w["candidates"]]
                        coarse[w["new_id"]] = o.align_pairs([bank[w["new_id"]]] * len(g), [bank[c] for c in w["candidates"]], g)
            d.reset()
        edges, reports = runs[0]
        for r, w in zip(reports, recs):
            print(kf[r["new_id"]], [kf[c] for c in r["candidates"]], np.round(r["gate_ratio"], 4), r["converged"], r["iterations"], r["scores"], r["best"], r["fine_score"],
                  r["reason"], "want", w["candidates"], np.round(w["ratio"], 4), w["converged"], w["iterations"], w["score"], w["best"], w["fine_score"], w["reason"])
            assert kf[r["new_id"]] == w["new_id"] and [kf[c] for c in r["candidates"]] == w["candidates"]
            assert r["gate_ratio"].tolist() == w["ratio"]  # the same integers, the same quotient
            assert r["converged"].tolist() == w["converged"] and r["iterations"].tolist() == w["iterations"]
            assert r["best"] == w["best"] and r["reason"] == w["reason"] and r["n_neighbours_skipped"] == w["skipped"]
            for k, c in enumerate(w["candidates"]):  # the coarse score: PCL's ungated fitness at the device's own transform
                if w["converged"][k]:
                    T, conv, it = coarse[w["new_id"]][k]
                    assert conv and it == r["iterations"][k] and _close(T, w["T"][k].astype(np.float64))
                    ws, _ = LC.fitness(sc["clouds"][w["new_id"]], sc["clouds"][c], T)
                    assert abs(r["scores"][k] - ws) <= 1e-12 * ws
                else:
                    assert r["scores"][k] == LC.DBL_MAX
        assert [(kf[e["key1"]], kf[e["key2"]]) for e in edges] == [(e["key1"], e["key2"]) for e in want_edges] and len(edges) >= 1
        for e, w in zip(edges, want_edges):
            assert _close(e["relative_pose"].astype(np.float64), w["relative_pose"].astype(np.float64))
            nb = next(r["neighbours"] for r in recs if r["new_id"] == w["key2"])
            acc = OC.accumulate(sc["clouds"], sc["poses"], w["key1"], nb)
            ws, _, _ = OC.gated_fitness(acc, sc["clouds"][w["key2"]], e["relative_pose"], 25.0)  # at the device's own transform
            assert abs(e["score"] - ws) <= 1e-12 * ws
            assert np.array_equal(e["information"], LC.information_matrix(e["score"]))
        # after lio_loop_reset, the same maps: the same bits
        again, rep2 = runs[1]
        assert len(again) == len(edges)
        for a, b in zip(again, edges):
            assert (a["key1"], a["key2"], a["score"]) == (b["key1"], b["key2"], b["score"]) and np.array_equal(a["relative_pose"], b["relative_pose"])
        assert [(r["gate_ratio"].tolist(), r["scores"].tolist(), r["reason"]) for r in rep2] == [(r["gate_ratio"].tolist(), r["scores"].tolist(), r["reason"]) for r in reports]
        assert tm["n_targets"] == sum(1 for r in recs if any(x >= 0.2 for x in r["ratio"])) and tm["n_pairs"] == sum(x >= 0.2 for r in recs for x in r["ratio"])
    finally:
        o.close()
        d.close()


def test_detect_skips_a_neighbour_outside_the_reference_map():
    """OM:189's operator[] corner: a neighbour of the best frame that is a new-map frame (an earlier fragment's overlap edge) is skipped"""
    sc, _, recs = OC.scene_restatement()
    found = [r for r in recs if r["edge"] is not None]
    first, later = found[0], found[-1]
    assert first["new_id"] != later["new_id"]
    best = later["candidates"][later["best"]]
    linked = sc["edges"] + [(best, first["new_id"])]  # the best frame of `later` already carries an overlap edge to another new-map frame
    want_edges, (w,) = OC.detect(sc["clouds"], sc["poses"], sc["ref_ids"], [later["new_id"]], linked)
    assert w["skipped"] == 1 and w["reason"] == "found" and OC.fixture_conditions([w] + recs) == []
    d = lio.LoopDetector(max_points=16384)
    o = lio.OverlapDetector(d)
    try:
        bank = _bank(d, sc)
        edges = o.detect([bank[k] for k in sc["ref_ids"]], [bank[later["new_id"]]], linked, ref_kf=sc["ref_ids"], new_kf=[later["new_id"]])
        r = o.last_report(0)
        print(r, "want", w["candidates"], w["best"], w["neighbours"], w["fine_score"])
        assert [c for c in r["candidates"]] == [bank[c] for c in w["candidates"]] and r["best"] == w["best"]
        assert r["n_neighbours_skipped"] == 1 and r["reason"] == "found"
        assert r["n_accum"] == len(sc["clouds"][w["edge"]["key1"]]) + sum(len(sc["clouds"][c]) for c in w["neighbours"])
        assert len(edges) == 1 and (edges[0]["key1"], edges[0]["key2"]) == (bank[w["edge"]["key1"]], bank[w["edge"]["key2"]])
        assert _close(edges[0]["relative_pose"].astype(np.float64), w["edge"]["relative_pose"].astype(np.float64))
    finally:
        o.close()
        d.close()


def _localization(sw, ref_path):
    assert sw.init_slam("offline", ref_path, "Localization", ["0-lidar", "IMU"], 0.2, 1.0, 10.0, 50.0) == ["0-lidar", "IMU"]
    sw.set_ins_external_param(0, 0, 0, 0, 0, 0)
    sw.set_imu_external_param(0, 0, 0, 0, 0, 0)
    assert sw.setup_slam() is True


def test_merge_map_through_the_wrapper(tmp_path):
    import slam_wrapper as sw

    sc, want = OC.scene_merge()
    ref_path, new_path = OC.write_scene(str(tmp_path / "maps"), sc, extra_lines=["VERTEX_PLANE 2000000 0 0 1 0"])
    # the refusals leave the state as it was: {} and the loaded map alone
    _, no_origin = OC.write_scene(str(tmp_path / "no_origin"), sc, origin=(0, 0, 0, 0, 0, 0))
    _, moved = OC.write_scene(str(tmp_path / "moved"), sc, origin=(OC.ORIGIN[0] + 1e-5,) + OC.ORIGIN[1:])
    _, other = OC.write_scene(str(tmp_path / "other"), sc, coordinate=1)
    _, no_graph = OC.write_scene(str(tmp_path / "no_graph"), sc)
    os.remove(os.path.join(no_graph, "graph", "graph.g2o"))
    assert sw.merge_map(new_path) == {}  # no init_slam: not in localisation mode
    _localization(sw, ref_path)
    try:
        before = sw.get_graph_map()
        assert sorted(before["poses"], key=int) == [str(k) for k in sc["ref_ids"]]
        _, null_q = OC.write_scene(str(tmp_path / "null_q"), sc, extra_lines=["EDGE_SE3:QUAT 0 5 1 0 0 0 0 0 0 " + " ".join(["1"] * 21)])
        for refused in (no_origin, moved, other, no_graph, null_q, str(tmp_path / "nowhere")):
            assert sw.merge_map(refused) == {}
            after = sw.get_graph_map()
            assert sorted(after["poses"]) == sorted(before["poses"]) and all(np.array_equal(after["poses"][k], before["poses"][k]) for k in before["poses"])
        got = sw.merge_map(new_path)
        rep = sw._last_merge()
        print(rep, "want", want["overlaps"])
        assert sorted(got["points"], key=int) == [str(k) for k in want["new_ids"]]  # max + 1 ...
        assert [(a, b) for a, b, _ in rep["overlaps"]] == want["overlaps"] and rep["fragments"] == 2 and rep["skipped_tags"] == 1
        reasons = dict(rep["reasons"])
        assert [lio.OverlapDetector.REASONS[reasons[r["new_id"]]] for r in want["records"]] == [r["reason"] for r in want["records"]]
        full = sw.get_graph_map()
        assert sorted(full["poses"], key=int) == [str(k) for k in sc["ref_ids"] + want["new_ids"]]  # both maps
        for k in want["new_ids"]:
            s = want["scene_of"][k]
            assert np.array_equal(got["points"][str(k)], sc["clouds"][s])  # points as stored
            assert np.array_equal(got["poses"][str(k)], full["poses"][str(k)]) and got["poses"][str(k)].dtype == np.float32
            e0 = np.linalg.norm(sc["poses"][s][:3, 3] - sc["truth"][s][:3, 3])
            e1 = np.linalg.norm(got["poses"][str(k)][:3, 3].astype(np.float64) - sc["truth"][s][:3, 3])
            print(k, s, f"error before {e0:.4f} after {e1:.4f} (restatement {np.linalg.norm(want['poses'][k][:3, 3] - sc['truth'][s][:3, 3]):.4f})")
            assert e1 < e0
            assert np.abs(got["poses"][str(k)].astype(np.float64) - want["poses"][k]).max() < 1e-3  # the restatement's optimum, through f32 poses
        # a second merge builds on the first one's graph (kept as a record, not read from disk again): ids go on from the merged map's largest,
        # and the frames merged before stay where they were to within the optimiser's tolerance (the graph has only gained consistent edges)
        again = sw.merge_map(new_path)
        top = max(want["new_ids"])
        assert sorted(again["points"], key=int) == [str(top + 1 + j) for j in range(len(sc["new_ids"]))]
        both = sw.get_graph_map()
        assert len(both["poses"]) == len(sc["ref_ids"]) + 2 * len(sc["new_ids"]) and all(np.isfinite(v).all() for v in both["poses"].values())
        assert all(np.abs(both["poses"][k].astype(np.float64) - full["poses"][k]).max() < 0.05 for k in full["poses"])
    finally:
        sw.deinit_slam()


def test_against_reference_vectors():
    """the coarse pairs and the fine alignments of the scene against what the reference's own FastVGICP / FastGICP (translation epsilon 0.001)
    returned for them (tests/golden/overlap.npz, tools/record_overlap_golden.py)"""
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlap.npz"))
    sc = OC.scene_restatement()[0]
    assert [len(sc["clouds"][k]) for k in sc["ref_ids"] + sc["new_ids"]] == gold["n_points"].tolist()
    d = lio.LoopDetector(max_points=16384)
    o = lio.OverlapDetector(d)
    try:
        bank = _bank(d, sc)
        kf = {b: k for k, b in bank.items()}
        pairs = gold["coarse/pairs"].tolist()
        guesses = [OC.make_guess(sc["poses"][n], sc["poses"][c]) for n, c in pairs]
        got = o.align_pairs([bank[n] for n, _ in pairs], [bank[c] for _, c in pairs], guesses)
        for j, (T, conv, it) in enumerate(got):
            print(f"pair {pairs[j]}: conv={conv} it={it} ref it={gold['coarse/iterations'][j]} |dt|={np.abs(T[:3, 3] - gold['coarse/T'][j][:3, 3]).max():.2e}")
            assert conv == bool(gold["coarse/converged"][j]) and it == int(gold["coarse/iterations"][j])
            assert _close(T, gold["coarse/T"][j].astype(np.float64))
        edges = o.detect([bank[k] for k in sc["ref_ids"]], [bank[k] for k in sc["new_ids"]], sc["edges"], ref_kf=sc["ref_ids"], new_kf=sc["new_ids"])
        by_new = {kf[e["key2"]]: e for e in edges}
        assert sorted((kf[e["key1"]], kf[e["key2"]]) for e in edges) == sorted(map(tuple, gold["edges"].tolist()))
        reports = {kf[r["new_id"]]: r for r in o.last_report()}
        for j, n in enumerate(gold["fine/new"].tolist()):
            r = reports[n]
            assert kf[int(r["candidates"][r["best"]])] == int(gold["fine/best"][j]) and r["fine_converged"] == bool(gold["fine/converged"][j])
            if n in by_new:
                e = by_new[n]
                print(f"fine {n}: score={e['score']:.9g} ref score={gold['fine/score'][j]:.9g} it={r['fine_iterations']}/{gold['fine/iterations'][j]}")
                assert _close(e["relative_pose"].astype(np.float64), gold["fine/T"][j].astype(np.float64))
    finally:
        o.close()
        d.close()


def test_detect_branches():
    """the outcomes the scene itself does not reach, one new frame each, by overriding a parameter or an estimate: the reason and what the report
    must then hold follow from the rule, not from a run"""
    sc, _, recs = OC.scene_restatement()
    w = recs[0]  # frame 100: three candidates pass the gate and converge, found at a score of 0.18
    assert w["reason"] == "found" and len(w["candidates"]) == 3 and w["fine_score"] > 0.15
    best = w["candidates"][w["best"]]
    d = lio.LoopDetector(max_points=16384)
    try:
        bank = _bank(d, sc)
        ref, new = [bank[k] for k in sc["ref_ids"]], [bank[w["new_id"]]]

        def run(**over):
            o = lio.OverlapDetector(d, **over)
            try:
                edges = o.detect(ref, new, sc["edges"], ref_kf=sc["ref_ids"], new_kf=[w["new_id"]])
                return edges, o.last_report(0)
            finally:
                o.close()

        # a threshold below the found score: the fine stage runs to its end and the score refuses the overlap
        edges, r = run(fitness_score_thresh=0.15)
        assert edges == [] and r["reason"] == "fine_score" and r["fine_converged"] and abs(r["fine_score"] - w["fine_score"]) < 1e-3 * w["fine_score"]
        # a translation epsilon no step can get under: 64 iterations, not converged, no score is taken
        edges, r = run(fine_translation_epsilon=1e-300)
        assert edges == [] and r["reason"] == "fine_not_converged" and not r["fine_converged"] and r["fine_score"] == LC.DBL_MAX and r["best"] == w["best"]
        # a target limited to the best frame and its first neighbour: the second neighbour is left out, the overlap is still found
        n2 = len(sc["clouds"][best]) + len(sc["clouds"][w["neighbours"][0]])
        edges, r = run(max_accum_points=n2)
        assert len(w["neighbours"]) == 2 and r["n_neighbours_dropped"] == 1 and r["n_accum"] == n2 and r["reason"] == "found" and len(edges) == 1
        # the estimate of the new frame 50 m too high, the gate switched off: every candidate's points pass 50 m under the new frame's voxels, H is
        # zero and no alignment converges
        lifted = sc["poses"][w["new_id"]].copy()
        lifted[2, 3] += 50.0
        d.set_pose(new[0], lifted)
        edges, r = run(fitness_inlier_thresh=0.0, distance_thresh=100.0)
        assert edges == [] and r["reason"] == "coarse" and len(r["candidates"]) == 3 and not r["converged"].any() and r["best"] == -1
        assert (r["gate_ratio"] == 0.0).all() and (r["scores"] == LC.DBL_MAX).all()
        # ... and with the gate as it is, the same frame is refused there
        edges, r = run(distance_thresh=100.0)
        assert edges == [] and r["reason"] == "gate"
    finally:
        d.close()
