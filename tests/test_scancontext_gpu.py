"""The Scan Context bank on the device (lio_sc_*, csrc/scancontext.hip) through the C ABI against the numpy restatement (tests/sc_cases.py), to
the last bit: describe at its edges, the keys, the ring-key search and its ties, the distance with its wrap-around, empty columns and NaN cases,
the scene of the localisation test's map with the eight query scans (also against the reference's recorded answers, tests/golden/scancontext.npz),
lio_gicp_fitness_score against the loop detector's score, and two runs byte for byte."""
import os

import numpy as np
import pytest

import loop_cases as LC
import sc_cases as S
from lsd_amd import capi, lio

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "scancontext.npz")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _restate(cloud, shifts):
    d = np.stack([S.describe(cloud, dx, dy) for dx, dy in shifts])
    return d, np.stack([S.ring_key(x) for x in d]), np.stack([S.sector_key(x) for x in d])


@pytest.fixture(scope="module")
def sc():
    h = lio.ScanContext(max_frames=1100, max_points_per_call=1 << 21)
    yield h
    h.close()


def test_describe_edges_and_keys(sc):
    clouds = S.edge_clouds()
    assert sorted(len(c) for c in clouds.values()) == [0, 1, 63, 64, 65, 257, 5000]
    for name, c in clouds.items():
        d, r, s = sc.describe(c, S.SEARCH_SHIFTS)
        wd, wr, ws = _restate(c, S.SEARCH_SHIFTS)
        bad = int((~np.isfinite(c[:, :3]).all(1)).sum())
        print(f"{name}: occupied bins per shift {[(x != 0).sum() for x in wd]} dropped {sc.last_dropped()}/{bad}")
        assert _same(d, wd) and _same(r, wr) and _same(s, ws), name
        assert sc.last_dropped() == bad
        for k, sh in enumerate(S.SEARCH_SHIFTS):  # nine shifts in one call = nine calls of one shift
            d1, r1, s1 = sc.describe(c, [sh])
            assert _same(d1[0], d[k]) and _same(r1[0], r[k]) and _same(s1[0], s[k]), (name, sh)
    lim = S.describe(clouds["limits_axes_64"])
    assert lim[19, 0] == 1.5 and lim[19, 14] == 2.0 and lim[19, 29] == 1.0 and lim[19, 44] == np.float32(np.float64(np.float32(0.7)) + 0.5)  # 80 m is kept
    assert not (lim == 9.5).any() and lim[0, 0] == 3.5 and lim[1, 0] == 1.5  # beyond 80 m is not; the origin lies in ring 1, sector 1
    assert (S.describe(clouds["one_bin_63"]) != 0).sum() == 1 and S.describe(clouds["one_bin_63"]).max() == 3.0


def test_batches_do_not_depend_on_place_or_size(sc):
    clouds = S.edge_clouds()
    probe, other = clouds["three_slices_5000"], [clouds[k] for k in ("random_257", "nonfinite_65", "empty_0", "one_bin_63", "limits_axes_64", "one_1")]
    want = _restate(probe, [(0, 0)])
    for batch, place in (([probe], 0), ([other[0], probe], 1), ([probe, other[1]], 0), (other[:3] + [probe] + other[3:], 3), ([probe] + other, 0), (other + [probe], 6)):
        sc.reset()
        first = sc.add_frames(batch)
        assert first == 0 and sc.num_frames() == len(batch)
        d, r, s = sc.download_frame(place)
        assert _same(d, want[0][0]) and _same(r, want[1][0]) and _same(s, want[2][0]), (len(batch), place)
        for k, c in enumerate(batch):  # and every other frame of the batch is its own
            wd = S.describe(c)
            assert _same(sc.download_frame(k)[0], wd)
    # a second call appends; launch sets of two frames at most give the same bank
    first = sc.add_frames([probe])
    assert first == 7 and _same(sc.download_frame(7)[0], want[0][0])
    small = lio.ScanContext(max_frames=8, max_points_per_call=5300)
    try:
        assert small.add_frames(other + [probe]) == 0
        assert all(_same(small.download_frame(k)[0], sc.download_frame(k)[0]) for k in range(7))
        with pytest.raises(capi.LioError):
            small.add_frames([np.zeros((5301, 4), np.float32)])  # larger than a call stages
        with pytest.raises(capi.LioError):
            small.add_frames([probe, probe])  # beyond max_frames
        assert small.num_frames() == 7
    finally:
        small.close()


def test_ring_key_search(sc):
    tiny = S.tiny_bank(1000)
    bank_d = np.stack([S.describe(c) for c in tiny])
    bank_r = np.stack([S.ring_key(d) for d in bank_d])
    rng = np.random.default_rng(3)
    q_clouds = [tiny[3], tiny[12], tiny[999], np.concatenate([tiny[40][:2], tiny[41][:2]])] + S.tiny_bank(3, seed=11)
    qd = np.stack([S.describe(c) for c in q_clouds])
    qr = np.stack([S.ring_key(d) for d in qd])
    for n in (1, 9, 10, 11, 64, 65, 1000):
        sc.reset()
        assert sc.add_frames(tiny[:n]) == 0
        for k in sorted({0, n // 2, n - 1}):
            d, r, s = sc.download_frame(k)
            assert _same(d, bank_d[k]) and _same(r, bank_r[k]) and _same(s, S.sector_key(bank_d[k]))
        subsets = [None]
        if n >= 11:
            subsets += [rng.permutation(n)[:max(3, n // 3)].astype(np.int32), np.array([7, 3, 5], np.int32)]
        for act in subsets:
            sc.set_active(act)
            ids, dist, sh, nc = sc.search(qd, qr)
            for q in range(len(qd)):
                wi, wdist, ws, _ = S.search(qd[q], qr[q], bank_d[:n], bank_r[:n], act)
                m = len(wi)
                assert nc[q] == m == min(10, n if act is None else len(act))
                assert np.array_equal(ids[q, :m], wi) and _same(dist[q, :m], wdist) and np.array_equal(sh[q, :m], ws), (n, q)
                assert (ids[q, m:] == -1).all() and np.isnan(dist[q, m:]).all() and (sh[q, m:] == -1).all()
            if n >= 8 and act is None:
                assert list(ids[0, :2]) == [3, 7] and dist[0, 0] == dist[0, 1]  # equal ring keys: the smaller id first
            if n == 1000 and act is None:
                assert list(ids[1, :4]) == [12, 20, 21, 500]
    # the empty search set: no candidates, no match
    sc.set_active([])
    ids, dist, sh, nc = sc.search(qd, qr)
    assert (nc == 0).all() and (ids == -1).all()
    g = sc.global_search(tiny[3])
    assert g == dict(match_id=-1, yaw=np.float32(0), score=1.0, shift=0)
    with pytest.raises(capi.LioError):
        sc.set_active([1, 1])
    with pytest.raises(capi.LioError):
        sc.set_active([1000])
    sc.set_active(None)
    assert sc.global_search(tiny[3])["match_id"] == 3


def test_distance(sc):
    a, b, what = S.distance_pairs()
    wd, ws, _ = S.distance(a, b)
    d, s = sc.distance(a, b)
    for k, w in enumerate(what):
        print(f"{w}: dist {d[k]!r} / {wd[k]!r} shift {s[k]} / {ws[k]}")
    assert _same(d, wd) and np.array_equal(s, ws)
    byname = dict(zip(what, zip(wd, ws)))
    for k in (0, 1, 2, 57, 58, 59, 30):
        assert byname[f"shift_{k}"][1] == k and abs(byname[f"shift_{k}"][0]) < 1e-15
    for w in ("first_all_empty", "second_all_empty", "both_all_empty"):
        assert byname[w] == (S.BIG, 0)  # every count 0: NaN wins no <
    assert byname["every_shift_ties"][1] == 0 and byname["even_shifts_tie"][1] == 0
    # pair by pair = in one call, and the reverse pairs
    d1, s1 = sc.distance(a[3:4], b[3:4])
    assert _same(d1, d[3:4]) and s1[0] == s[3]
    wd2, ws2, _ = S.distance(b, a)
    d2, s2 = sc.distance(b, a)
    assert _same(d2, wd2) and np.array_equal(s2, ws2)


def _scene_run():
    sc = lio.ScanContext(max_frames=30, max_points_per_call=1 << 21)
    try:
        scn = S.scene()
        assert sc.add_frames(scn["frames"]) == 0
        bank = [sc.download_frame(k) for k in range(30)]
        res = [sc.global_search(q) for q in scn["queries"]]
        t = sc.last_times()
        return bank, res, t
    finally:
        sc.close()


@pytest.fixture(scope="module")
def scene_run():
    return _scene_run()


def test_scene_against_the_restatement(scene_run):
    bank, res, t = scene_run
    scn = S.scene()
    print("times of the last global search (us):", t)
    for k in range(30):
        assert _same(bank[k][0], scn["desc"][k]) and _same(bank[k][1], scn["ring"][k]) and _same(bank[k][2], scn["sector"][k]), k
    for q, (got, want) in enumerate(zip(res, scn["search"])):
        print(f"query {S.QUERIES[q]}: frame {got['match_id']} shift {got['shift']} score {got['score']:.6f}")
        assert got["match_id"] == want["match_id"] and got["shift"] == want["shift"] and got["score"] == want["score"]
        assert _same(np.array([got["yaw"]], np.float32), np.array([want["yaw"]], np.float32))
    assert tuple(r["match_id"] for r in res[:5]) == S.POSITIVE_FRAMES and tuple(r["shift"] for r in res[:5]) == S.POSITIVE_SHIFTS


def test_scene_against_the_reference(scene_run):
    """the rule of tests/test_scancontext_cpu.py, with the device in the restatement's place"""
    _, res, _ = scene_run
    g = np.load(GOLD)
    scn = S.scene()
    assert [S.cloud_hash(c) for c in scn["queries"]] == list(g["query_hash"])
    skipped = 0
    for q, got in enumerate(res):
        if S.search_gap(scn["search"][q]) <= 1e-12:
            skipped += 1
            continue
        assert got["match_id"] == int(g["gs_id"][q]) and abs(got["score"] - float(g["gs_score"][q])) <= 1e-12
        assert _same(np.array([got["yaw"]], np.float32), g["gs_yaw"][q:q + 1])
    assert skipped / len(res) <= 0.02


def test_two_runs_are_byte_equal(scene_run):
    bank, res, _ = scene_run
    bank2, res2, _ = _scene_run()
    for a, b in zip(bank, bank2):
        assert all(_same(x, y) for x, y in zip(a, b))
    assert [(r["match_id"], r["shift"], r["score"], float(r["yaw"])) for r in res] == [(r["match_id"], r["shift"], r["score"], float(r["yaw"])) for r in res2]


def test_gicp_fitness_score_is_the_loop_detectors():
    tgt, cands, guesses = LC.five_candidates()
    M = 16384
    d = lio.LoopDetector(max_points=M)
    g = lio.Gicp(grid_resolution=1.0, max_points=M, k=20)
    try:
        ids = [d.add_keyframe(c, np.eye(4), 0.0) for c in [tgt] + list(cands[:2])]
        g.set_target(tgt)
        with pytest.raises(capi.LioError):
            g.fitness_score(np.eye(4))  # no source yet
        for src in (1, 2):
            T, conv, it, score, nr = d.align_candidates(ids[0], [ids[src]], [guesses[src - 1]])[0]
            g.set_source(cands[src - 1])
            got = g.fitness_score(T, d.params.fitness_score_max_range)
            print(f"source {src}: loop score {score!r} nr {nr}; gicp {got}")
            assert nr > 0 and got == (score, nr)
        # another target: the index follows it
        T, conv, it, score, nr = d.align_candidates(ids[1], [ids[2]], [np.eye(4)])[0]
        g.set_target(cands[0])
        assert g.fitness_score(T, d.params.fitness_score_max_range) == (score, nr)
        assert g.fitness_score(T, 0.0)[1] <= nr
        with pytest.raises(capi.LioError):
            g.fitness_score(np.full((4, 4), np.nan))
    finally:
        g.close()
        d.close()
