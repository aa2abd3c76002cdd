"""The cases of tests/gicp_edge_cases.py without the library: every builder runs, the structural claims of the cases hold (ties, cell
occupancies, distances in cells, d2 == 4.0f), E of every case is measured and printed (pytest -s shows it), the numpy restatement of the
kernels' search rule agrees with brute force on them, and every seeded mistake in that rule changes what at least one case expects."""
import numpy as np
import pytest

import gicp_edge_cases as GC

F32 = np.float32


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in GC.all_cases() + [GC.overflow_source()]}


def _cells_apart(P, res, i, j):
    return int(np.abs(GC.cell_of(P[i], res) - GC.cell_of(P[j], res)).max())


def test_case_claims(cases):
    # 1: occupancies above 32 at the coarse grid, many rings at the fine one
    c = cases["k_edges/k32/g4.0"]
    occ = np.unique(GC.cell_of(c["target"], 4.0), axis=0, return_counts=True)[1]
    assert occ.max() > 32 and (occ > 16).sum() >= 2
    c = cases["k_edges/k32/g0.25"]
    idx, _ = GC.expected_lists(c["target"], 32)
    rings = [_cells_apart(c["target"], 0.25, i, idx[i, -1]) for i in range(0, 600, 37)]
    assert min(rings) >= 3 and max(rings) >= 6, rings
    assert all(cases[f"k_edges/k{k}/g{g}"]["k"] == k for k in GC.K_EDGE_KS for g in GC.K_EDGE_GRIDS)
    # 2: n = k and k + 1 over several cells
    for k in (20, 32):
        for e in (0, 1):
            c = cases[f"n_edges/k{k}/n{k + e}"]
            assert len(c["target"]) == k + e and len(np.unique(GC.cell_of(c["target"], 1.0), axis=0)) >= 8
    # 3: on the faces, ties at the k-th place, |x / res| out to 333 at res 0.3
    for res, k in ((1.0, 7), (1.0, 20), (0.3, 7), (0.3, 20)):
        c = cases[f"lattice/g{res}/k{k}"]
        P = c["target"]
        order, d2 = GC.sorted_keys(P, P)
        assert (d2[:, k - 1] == d2[:, k]).sum() > len(P) // 4  # the k-th and the (k + 1)-th at the same f32 distance
        on_face = (P[:, :3] / F32(res) - F32(0.5)) == np.round(P[:, :3] / F32(res) - F32(0.5))
        assert on_face.all(axis=1).sum() >= len(P) // 3
        assert (P[:, :3] > 0).any() and (P[:, :3] < 0).any()
        if res == 0.3:
            assert np.abs(P[:, :3] / F32(res)).max() > 333 and np.abs(P[:, :3]).max() > 100
        w, sq = GC.expected_pairs(c["source"], P, c["T"], c["maxd"])
        d = GC.d2_f32(c["source"][:, :3], P)
        assert ((d == sq[:, None]).sum(1) >= 2).mean() >= 0.1 and (w >= 0).all()  # a part of the pairs are ties of the f32 distance
    # 4: duplicates: 2, k and k + 3 copies; all-zero C
    c = cases["duplicates/k10"]
    _, cnt = np.unique(c["target"][:, :3], axis=0, return_counts=True)
    assert {2, 10, 13} <= set(cnt.tolist())
    idx, _ = GC.expected_lists(c["target"], 10)
    C = GC.cov_exact(c["target"], idx)
    assert (np.abs(C).max((1, 2)) == 0).sum() == 2 * 10 + 2 * 13
    # 5: the nearest lies in another cell while the own cell is occupied
    c = cases["near_beats_home"]
    P = c["target"]
    idx, _ = GC.expected_lists(P, 3)
    kinds = set()
    for g in range(len(GC.NEAR_DIRS)):
        q = 6 * g  # the query of k-NN group g as built: four points of the k-NN group, then two of the 1-NN group
        home = [j for j in range(len(P)) if j != q and _cells_apart(P, 1.0, q, j) == 0]
        assert len(home) == 2 and _cells_apart(P, 1.0, q, idx[q, 1]) == 1 and set(idx[q]) != {q, *home}
        kinds.add(int(np.abs(GC.cell_of(P[q], 1.0) - GC.cell_of(P[idx[q, 1]], 1.0)).sum()))
    assert kinds == {1, 2, 3}  # face, edge, corner
    w, _ = GC.expected_pairs(c["source"], P, c["T"], c["maxd"])
    for s in range(len(GC.NEAR_DIRS)):
        cs = GC.cell_of(c["source"][s], 1.0)
        assert any((GC.cell_of(P[j], 1.0) == cs).all() for j in range(len(P))) and np.abs(GC.cell_of(P[w[s]], 1.0) - cs).max() == 1
    # 6: 40 cells, and past the last ring
    for name, far, lo in (("sparse/lone", [200], 40), ("sparse/beyond", [200], 40), ("sparse/beyond", [201, 202, 203, 204, 205], GC.COV_RINGS + 1)):
        c = cases[name]
        idx, _ = GC.expected_lists(c["target"], 20)
        for i in far:
            assert lo <= _cells_apart(c["target"], 0.5, i, idx[i, 19]) < lo + 12
    # 7: the threshold itself
    c = cases["threshold/exact"]
    w, sq = GC.expected_pairs(c["source"], c["target"], c["T"], 2.0)
    assert sq[0] == F32(4.0) and w[0] == -1 and (w == -1).all()
    c = cases["threshold/below"]
    w, sq = GC.expected_pairs(c["source"], c["target"], c["T"], 2.0)
    assert sq[0] < F32(4.0) and sq[0] == np.nextafter(F32(2.0), F32(0)) ** 2 and w[0] == 2
    c = cases["threshold/tie"]
    w, sq = GC.expected_pairs(c["source"], c["target"], c["T"], 2.0)
    assert (GC.d2_f32(c["source"][:1, :3], c["target"])[0] == sq[0]).sum() == 4 and w[0] == 2
    # 8, 9, 10
    assert cases["no_pairs"]["maxd"] == 0.0
    assert [len(cases[f"cost_sizes/{n}"]["source"]) for n in GC.COST_SIZES] == [127, 128, 129, 4097] and -(-4097 // 128) == 33
    R = cases["cost_sizes/127"]["T"][:3, :3]
    assert np.abs(R - np.eye(3)).max() > 0.2 and np.allclose(R @ R.T, np.eye(3), atol=1e-14)
    c = cases["far_source"]
    w, sq = GC.expected_pairs(c["source"], c["target"], c["T"], np.inf)
    assert (w >= 0).all() and (np.sqrt(sq[-4:]) / 0.5 >= 20).all() and GC.CORR_RINGS < 20
    c = cases["overflow_source"]
    with np.errstate(over="ignore", invalid="ignore"):
        q = GC.OG.transform_f(c["T"], c["source"])
    assert np.isfinite(c["source"]).all() and np.isfinite(c["T"]).all() and not np.isfinite(q[c["row"]]).all() and np.isfinite(np.delete(q, c["row"], 0)).all()
    w, _ = GC.expected_pairs(c["source"], c["target"], c["T"], np.inf)
    assert w[c["row"]] == -1 and (np.delete(w, c["row"]) >= 0).all()


def test_E_of_every_case(cases):
    """E, the oracle's own distance from the long-double covariance, per case (input order; the GPU file measures it again in device order)"""
    for name, c in cases.items():
        E = []
        for P in (c["target"], c["source"]):
            idx, _ = GC.expected_lists(P, c["k"])
            E.append(GC.oracle_E(P, idx))
        print(f"E  {name:24s} target {E[0]:.2e}  source {E[1]:.2e}")
        assert all(np.isfinite(E))


def _subset(n, step):
    return list(range(0, n, step))


def test_standin_agrees_with_brute_force(cases):
    """the restated search rule, unmutated, gives the expected lists and pairs: the uniform clouds on every tenth query"""
    for name, c in cases.items():
        if name.startswith("k_edges") and c["k"] not in (16, 17, 32) or name.startswith("cost_sizes"):
            continue
        P, k = c["target"], c["k"]
        qs = _subset(len(P), 10 if name.startswith("k_edges") else 1)
        st = GC.standin_knn(P, k, c["res"], queries=qs)
        want, _ = GC.expected_lists(P, k)
        assert np.array_equal(st[qs, :k], want[qs]), name
        S = c["source"][:: 3 if len(c["source"]) > 100 else 1]
        assert np.array_equal(GC.standin_corr(S, P, c["T"], c["maxd"], c["res"]), GC.expected_pairs(S, P, c["T"], c["maxd"])[0]), name


# the cases that catch each mistake: (case, "knn" | "corr" | "cov")
CATCHES = {
    "tie_high": [("threshold/tie", "corr"), ("lattice/g1.0/k7", "knn")],
    "corr_le": [("threshold/exact", "corr")],
    "ring_early": [("near_beats_home", "knn"), ("near_beats_home", "corr")],
    "gap_unshrunk": [("lattice/g0.3/k7", "knn")],
    "tie_stop": [("lattice/g1.0/k7", "knn"), ("lattice/g0.3/k7", "knn")],
    "no_carry": [("n_edges/k20/n21", "knn"), ("n_edges/k32/n32", "knn")],
    "kth_at_k": [("k_edges/k16/g1.0", "knn"), ("k_edges/k32/g4.0", "knn")],
    "mean_by_found": [("k_edges/k3/g4.0", "cov")],
    "cov_by_found": [("k_edges/k3/g4.0", "cov")],
    "no_sweep": [("sparse/beyond", "knn"), ("far_source", "corr")],
}


@pytest.mark.parametrize("mut", GC.MUTATIONS)
def test_every_seeded_mistake_changes_an_expectation(cases, mut):
    assert mut in CATCHES
    for name, what in CATCHES[mut]:
        c = cases[name]
        P, k = c["target"], c["k"]
        if what == "corr":
            want = GC.expected_pairs(c["source"], P, c["T"], c["maxd"])[0]
            assert np.array_equal(GC.standin_corr(c["source"], P, c["T"], c["maxd"], c["res"]), want)
            assert not np.array_equal(GC.standin_corr(c["source"], P, c["T"], c["maxd"], c["res"], mut), want), (mut, name)
            continue
        qs = _subset(len(P), 6 if name.startswith("k_edges") else 1) if name != "sparse/beyond" else list(range(190, len(P)))
        want, _ = GC.expected_lists(P, k)
        good = GC.standin_knn(P, k, c["res"], queries=qs)
        assert np.array_equal(good[qs, :k], want[qs])
        if what == "knn":
            got = GC.standin_knn(P, k, c["res"], mut, queries=qs)
            assert not np.array_equal(got[qs, :k], want[qs]), (mut, name)
        else:
            C = GC.cov_exact(P, want)[qs]
            assert np.abs(GC.standin_cov(P, k, good, None, qs)[qs] - C).max() < 1e-17
            Cm = GC.standin_cov(P, k, good, mut, qs)[qs]
            assert np.abs(Cm - C).max() > 1e-3, (mut, name)
