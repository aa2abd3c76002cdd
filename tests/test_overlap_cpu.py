"""Overlap detection, the host side (lio_overlap_*, csrc/overlap.hip): the ABI revision and symbols, find_candidates and connection_count against
the numpy restatement (tests/overlap_cases.py) on seeded random graphs, and the conditions the two-map scene of the GPU test must meet."""
import os
import re

import numpy as np

import overlap_cases as OC
from lsd_amd import capi, lio

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "lio_hip.h")


def test_abi_revision_and_symbols():
    hdr = open(HEADER).read()
    rev = int(re.search(r"#define LIO_ABI_VERSION (\d+)", hdr).group(1))
    assert rev >= 16 and capi.lib().lio_abi_version() == rev
    names = ["lio_overlap_default_params", "lio_overlap_connection_count", "lio_overlap_find_candidates", "lio_overlap_create", "lio_overlap_destroy",
             "lio_overlap_gate_batch", "lio_overlap_align_pairs", "lio_overlap_accumulate", "lio_overlap_download_accum", "lio_overlap_detect",
             "lio_overlap_last_report", "lio_overlap_last_times"]
    for n in names:
        assert n in capi.SYMBOLS and re.search(r"\b%s\(" % n, hdr) and hasattr(capi.lib(), n)
    p = lio.OverlapDetector.default_params()
    got = {k: getattr(p, k) for k in OC.DEFAULTS}
    assert got == OC.DEFAULTS and p.max_accum_points == 8 * 65536
    assert p.fine_translation_epsilon == 0.001  # OM:60, not the loop detector's 0.01


def _random_graph(rng, kind):
    """(positions, ids, edges, new id, new position): two components -- the key frames (ids 0 ..) and the new map (ids 1000 ..)"""
    n = int(rng.integers(0, 9)) if kind == "few" else int(rng.integers(10, 40))
    ids = rng.permutation(n).astype(np.int32)  # the key-frame list is not in id order
    pos = rng.uniform(-25, 25, (n, 3))
    pos[:, 2] *= 0.05
    if n > 3 and kind == "ties":  # frames at exactly the same place, and at mirrored places: equal f32 distances
        pos[1] = pos[0]
        pos[2] = pos[3] * [1, 1, 1]
    edges = [(int(ids[i]), int(ids[i + 1])) for i in range(n - 1) if rng.random() < (0.6 if kind == "disconnected" else 1.0)]
    m = int(rng.integers(1, 9)) if kind == "short" else int(rng.integers(1, 30))
    new = list(range(1000, 1000 + m))
    edges += [(new[i], new[i + 1]) for i in range(m - 1)]
    if kind == "cyclic" and m > 2:
        edges += [(new[0], new[-1])] + [(new[int(rng.integers(m))], new[int(rng.integers(m))]) for _ in range(3)]
    if kind == "linked" and n:  # an earlier overlap edge between the maps
        edges += [(new[int(rng.integers(m))], int(ids[int(rng.integers(n))]))]
    rng.shuffle(edges)
    k = int(rng.integers(m))
    q = rng.uniform(-25, 25, 3)
    if n and kind == "ties":
        q = pos[0] + [3.0, 0, 0]
    return pos, ids, edges, new[k], q


def test_candidates_and_connection_count_random_graphs():
    rng = np.random.default_rng(2024)
    kinds = ["chain", "disconnected", "cyclic", "short", "few", "linked", "ties"]
    n_cand = 0
    for trial in range(500):
        kind = kinds[trial % len(kinds)]
        pos, ids, edges, new_id, q = _random_graph(rng, kind)
        conn = OC.connection_map(edges)
        p = dict(OC.DEFAULTS)
        prm = lio.OverlapDetector.default_params()
        if trial % 5 == 0:  # other thresholds, max_count = 0 among them (the walk then only ends when the queue runs dry)
            p.update(candidate_link_dist=int(rng.integers(0, 6)), distance_thresh=float(rng.uniform(5, 40)), max_candidate_num=int(rng.integers(1, 5)), knn=int(rng.integers(1, 14)))
            prm.candidate_link_dist, prm.distance_thresh, prm.max_candidate_num, prm.knn = p["candidate_link_dist"], p["distance_thresh"], p["max_candidate_num"], p["knn"]
        want = OC.find_candidates(pos, ids, conn, new_id, q, p)
        got = lio.OverlapDetector.find_candidates(pos, ids, edges, new_id, q, prm).tolist()
        assert got == want, (trial, kind)
        n_cand += len(want)
        nodes = sorted(conn) + [new_id, 5000]
        for _ in range(6):
            s, t = int(rng.choice(nodes)), int(rng.choice(nodes))
            mc = int(rng.choice([0, 1, 3, 10, 10, 50]))
            assert lio.OverlapDetector.connection_count(edges, s, t, mc) == OC.connection_count(conn, s, t, mc), (trial, kind, s, t, mc)
    assert n_cand > 200  # the graphs do produce candidates


def test_connection_count_counts_levels():
    chain = [(i, i + 1) for i in range(11)]  # 12 frames
    # from frame 3 the walk runs dry after 9 levels, from frames 0-2 and 9-11 it reaches 10: only they can have candidates
    assert [lio.OverlapDetector.connection_count(chain, s, 999, 10) for s in range(12)] == [10, 10, 10, 9, 8, 7, 7, 8, 9, 10, 10, 10]
    assert lio.OverlapDetector.connection_count(chain, 0, 4, 10) == 4 and lio.OverlapDetector.connection_count(chain, 0, 11, 10) == 10
    assert lio.OverlapDetector.connection_count(chain, 0, 11, 0) == 11 and lio.OverlapDetector.connection_count([], 3, 4, 10) == 1


def test_scene_fixture_conditions():
    sc, edges, recs = OC.scene_restatement()
    for r in recs:
        print(r["new_id"], r["candidates"], np.round(r["ratio"], 3), r["converged"], r["score"], r["best"], r["fine_score"], r["reason"], np.sqrt(r["cand_d2"]))
    assert OC.fixture_conditions(recs) == []
    deep = [r["new_id"] for r in recs if r["candidates"]]
    assert set(deep) <= {100, 101, 102, 109, 110, 111} and any(r["reason"] == "gate" for r in recs) and len(edges) >= 1


def test_merge_fixture_conditions():
    """the fragment loop of the merge on the same scene: the second fragment is matched at the poses the first optimisation left"""
    sc, m = OC.scene_merge()
    assert OC.fixture_conditions(m["records"], content=False) == []
    assert m["new_ids"] == list(range(max(sc["ref_ids"]) + 1, max(sc["ref_ids"]) + 1 + len(sc["new_ids"]))) and len(m["overlaps"]) >= 1
    for k in m["new_ids"]:  # every new frame ends nearer to the truth than its estimate began
        s = m["scene_of"][k]
        assert np.linalg.norm(m["poses"][k][:3, 3] - sc["truth"][s][:3, 3]) < np.linalg.norm(sc["poses"][s][:3, 3] - sc["truth"][s][:3, 3])


def test_read_g2o_round_trip(tmp_path):
    import pytest

    import graph_cases as GC
    import slam_wrapper as sw

    rng = np.random.default_rng(3)
    vertices = {int(k): GC.random_pose(rng, 5.0) for k in (0, 3, 4, 17, 1000)}
    edges = [(0, 3, GC.random_pose(rng), GC.random_info(rng)), (3, 4, GC.random_pose(rng), GC.random_info(rng)), (17, 0, GC.random_pose(rng), OC.ODOM_INFO)]
    extra = ["VERTEX_PLANE 2000000 0 0 1 0", "EDGE_SE3_PLANE 3 2000000 0 0 1 0 1 0 0 1 0 1", "# a comment", "", "EDGE_SE3_PRIORXYZ 4 1 2 3 1 0 0 1 0 1"]
    OC.write_map(str(tmp_path), {}, vertices, edges, fixed=[0, 17], extra_lines=extra)
    path = str(tmp_path / "graph" / "graph.g2o")
    got = sw._read_g2o(path)
    assert sorted(got["vertices"]) == sorted(vertices) and got["fixed"] == [0, 17] and got["skipped"] == 3  # the comment and the empty line are no tags
    for k, T in vertices.items():
        t, q = GC.T_to_tq(T)
        assert np.array_equal(got["vertices"][k], np.concatenate([t, q]))  # repr round-trips a double
    assert len(got["edges"]) == 3
    for (a, b, M, info), (ga, gb, gm, ginfo) in zip(edges, got["edges"]):
        t, q = GC.T_to_tq(M)
        assert (ga, gb) == (a, b) and np.array_equal(gm, np.concatenate([t, q])) and ginfo.shape == (6, 6)
        assert np.array_equal(np.triu(ginfo), np.triu(info)) and np.array_equal(ginfo, ginfo.T)
    # a truncated line is an error, whichever tag it carries
    text = open(path).read().splitlines()
    for tag, keep in (("EDGE_SE3:QUAT", 25), ("VERTEX_SE3:QUAT", 8), ("FIX", 1)):
        bad = [(" ".join(l.split()[:keep]) if l.startswith(tag) else l) for l in text]
        p2 = tmp_path / f"bad_{keep}.g2o"
        p2.write_text("\n".join(bad) + "\n")
        with pytest.raises(RuntimeError, match="truncated"):
            sw._read_g2o(str(p2))
    with pytest.raises(RuntimeError):
        sw._read_g2o(str(tmp_path / "missing.g2o"))
    # a quaternion that cannot be normalised is an error too (the merge then refuses the map); a token that is no number ("nan") does not parse
    # and reads as a truncated line
    for k, (old, new, msg) in enumerate(((" ".join(text[0].split()[5:9]), "0 0 0 0", "null quaternion"), (text[0].split()[2], "nan", "truncated"))):
        p3 = tmp_path / f"null_{k}.g2o"
        p3.write_text("\n".join([text[0].replace(old, new, 1)] + text[1:]) + "\n")
        with pytest.raises(RuntimeError, match=msg):
            sw._read_g2o(str(p3))
