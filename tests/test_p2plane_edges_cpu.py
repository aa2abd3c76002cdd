"""The cases of tests/p2plane_edge_cases.py against the CPU oracle: the cases meet the conditions they were built for (these are assertions: a
case that misses one gets fixed, not skipped), the numpy restatements of the gate, of map_incremental's rule and of the degeneracy sums reproduce
the oracle, and the neighbour sets of the plane-threshold and rank cases are pinned to the reference's own esti_plane where it is built."""
import numpy as np
import pytest

import p2plane_edge_cases as E


@pytest.fixture(scope="module")
def W(oracle_mod):
    return E.world(esti_plane=oracle_mod.esti_plane)


@pytest.fixture(scope="module")
def Wref(oracle_mod, W):
    return E.oracle_search(oracle_mod, W)[1]


@pytest.fixture(scope="module")
def P(oracle_mod):
    return E.world(state=E.pose6_state())


@pytest.fixture(scope="module")
def Pref(oracle_mod, P):
    return E.oracle_search(oracle_mod, P)[1]


@pytest.fixture(scope="module")
def T(oracle_mod):
    steps = E.thresh_steps(oracle_mod.esti_plane)
    return steps, [E.oracle_search(oracle_mod, c)[1] for c in steps]


def test_five_neighbours_where_meant(W, Wref, P, Pref, T):
    for case, ref in [(W, Wref), (P, Pref)] + list(zip(*T)):
        assert np.all(ref["nn_cnt"][case.want5] == 5), case.name
    for k in E.COUNTS:
        assert np.all(Wref["nn_cnt"][W.idx("count:%d" % k)] == min(k, 5)), k
    assert np.all(Wref["nn_cnt"][W.idx("count:0")] == 0)


def test_gate_sweeps_hold_both_outcomes(W, Wref, P, Pref):
    """every +-32 ulp sweep of the residual gate flips inside the sweep, under the identity pose and through the pose of case 6; over a plane
    through the world origin (A n = -1 has no solution) the fit is rejected throughout"""
    for case, ref in ((W, Wref), (P, Pref)):
        sweeps = case.sweeps("gate")
        assert len(sweeps) >= 10
        norms = []
        for sw in sweeps:
            assert len(sw) == 65
            s = ref["selected"][sw]
            assert 0 < s.sum() < 65, (case.name, case.group[sw[0]], s)
            norms.append(np.linalg.norm(case.ds[sw[0], :3]))
        assert min(norms) < 1.8 and max(norms) > 13.0  # |p_body| from about 1 m to about 14 m
        assert {np.sign(case.height[sw[0]]) for sw in sweeps} == {-1.0, 1.0}  # above and below the plane
        for sw in case.sweeps("gate0"):
            assert not ref["selected"][sw].any()
        assert len(case.sweeps("gate0")) == 3
    # the body origin: sqrt(|p|) = 0 divides by zero; never selected, whatever the plane
    for case, ref in ((W, Wref), (P, Pref)):
        i = case.idx("origin")
        assert len(i) == 1 and not np.any(case.ds[i, :3]) and ref["nn_cnt"][i[0]] == 5 and not ref["selected"][i[0]]


def test_plane_threshold_sweeps_hold_both_outcomes(oracle_mod, T):
    steps, refs = T
    sel = np.array([r["selected"] for r in refs])  # [41 steps, 9 (node, orientation) + the tie sweep]
    assert sel.shape == (41, len(E.THRESH_NODES) + 1)
    for j in range(sel.shape[1]):
        assert 0 < sel[:, j].sum() < 41, (j, sel[:, j])
    assert sel[20].all() and not sel[21].any()  # step 0 is the last lift the bisection saw accepted, step 1 the first it saw rejected
    # the tie sweep: at some accepted step a neighbour's |v| EQUALS 0.1f (the comparison is `>`: equal is accepted)
    ties = 0
    for r in refs:
        ok, plane = oracle_mod.esti_plane(r["nn"][-1])
        ties += bool(ok and r["selected"][-1] and np.any(np.abs(E.plane_residuals(plane, r["nn"][-1])) == np.float32(0.1)))
    assert ties >= 1


def test_counts_below_five_are_never_selected(W, Wref):
    for k in E.COUNTS:
        s = Wref["selected"][W.idx("count:%d" % k)]
        assert len(s) == 4 and (s.all() if k >= 5 else not s.any()), k


def test_reference_rule_on_degenerate_sets(oracle_mod, W, Wref):
    """Pins what the REFERENCE's esti_plane does with neighbour sets one might expect it to refuse (behaviour to keep, not to fix): collinear
    neighbours, two / three / five coincident neighbours are ACCEPTED with a finite plane; a set symmetric about the world origin gives the normal
    0, the plane (nan, nan, nan, inf), which passes the `fabs(v) > 0.1` test (every comparison with nan is false) and is stopped by the gate."""
    for name in ("collinear", "coincident2", "coincident3", "coincident5", "tie_x", "tie_y", "tie_z", "far0", "far1", "far2"):
        i = W.idx("rank:" + name)
        assert len(i) == 4 and Wref["selected"][i].all(), name
        assert np.all(np.isfinite(Wref["normvec"][i])), name
    i = W.idx("rank:origin")
    fits = [oracle_mod.esti_plane(Wref["nn"][j]) for j in i]  # (which rounding the rows meet depends on the order the search hands them over in)
    assert any(ok and np.all(np.isnan(pl[:3])) and np.isinf(pl[3]) for ok, pl in fits), fits
    assert not Wref["selected"][i].any()
    far = W.map[np.abs(W.map[:, 0]) > 50]
    assert len(far) == 15 and np.all(np.abs(far[:, :2]) >= 60) and np.all(np.abs(far[:, :2]) <= 90)


def test_tails_end_in_a_selected_point(oracle_mod, W):
    last = W.idx("tilt")[0]
    o = E.oracle_engine(oracle_mod, W.map, W.state)
    for n in E.TAIL_SIZES:
        ds = E.tail_cloud(W.ds, n, last)
        assert len(ds) == n and np.array_equal(ds[-1], W.ds[last])
        o.set_ds(ds)
        r = o.linearize(True)
        assert r["selected"][n - 1] == 1 and abs(r["normvec"][n - 1, 3]) > 0.05, n
    assert sorted({-(-n // 64) for n in E.TAIL_SIZES}) == [1, 2, 32, 33, 224, 225, 256, 257, 481, 482]


def test_gate_restatement(oracle_mod, W, Wref, P, Pref, T):
    """the numpy gate applied to the oracle's planes gives the oracle's `selected` and, where selected, its residual bits"""
    for case, ref in [(W, Wref), (P, Pref)] + list(zip(*T)):
        five = np.flatnonzero(ref["nn_cnt"] == 5)
        fit = [oracle_mod.esti_plane(ref["nn"][i]) for i in five]
        ok = np.array([f[0] for f in fit])
        plane = np.array([f[1] for f in fit])
        sel, pd2 = E.gate(plane, ref["world"][five], case.ds[five])
        want = np.zeros(len(case), bool)
        want[five] = ok & sel
        assert np.array_equal(want, ref["selected"].astype(bool)), case.name
        s = ok & sel
        got = np.c_[plane[s, :3], pd2[s]].astype(np.float32)
        assert np.array_equal(got.view(np.uint32), ref["normvec"][five[s]].view(np.uint32)), case.name


@pytest.mark.parametrize("n", E.CLASSIFY_SIZES)
def test_classify_restatement_and_branches(oracle_mod, n):
    mp, ds, r = E.classify_oracle(oracle_mod, n)
    cls, branch = E.classify_rule(r["world"], r["nn"], r["nn_cnt"])
    assert r["n_add"] == int((cls > 0).sum())
    added = r["dump"][r["dump"][:, 3] >= 1000.0]
    assert len(added) == r["n_add"] and len(r["dump"]) == len(mp) + r["n_add"]
    assert np.array_equal(E.rows_u32(added), E.rows_u32(r["world"][cls > 0]))
    if n >= 255:  # room for every branch
        for b in E.BRANCHES:
            assert int((branch == b).sum()) >= 8, (n, b)
        for k in (1, 2, 3, 4):
            assert int(((branch == "lt5_kept") & (r["nn_cnt"] == k)).sum()) >= 8, (n, k)
        assert set(np.unique(cls[branch == "exact_half"])) == {0} and set(np.unique(cls[branch == "far_all_axes"])) == {2}
        assert set(np.unique(cls[branch == "five_tie_kept"])) == {1}
    assert -(-max(E.CLASSIFY_SIZES) // 256) > 256  # the second trip of the scatter's prefix loop


def test_classify_before_the_filter_is_initialised(oracle_mod):
    mp, ds, r = E.classify_oracle(oracle_mod, 257, ekf_inited=False)
    cls, branch = E.classify_rule(r["world"], r["nn"], r["nn_cnt"], ekf_inited=False)
    assert r["n_add"] == 257 and cls.all() and np.all(branch == "not_inited")


def test_degeneracy_restatement(oracle_mod, W, P):
    """the six sums against the oracle's own (f32 running sums there: 2e-2 absolute, the allowance tests/test_degenerate.py gives them)"""
    for case in (W, P):
        o, ref = E.oracle_search(oracle_mod, case)
        sel = ref["selected"].astype(bool)
        nv = ref["normvec"][sel]
        r3 = nv[:, :3].astype(np.float64)
        hth = np.cumsum(r3[:, :, None] * r3[:, None, :], axis=0)[-1]  # the oracle's order of addition
        _, V = oracle_mod.eig3(hth)
        contri, strong, dot = E.degeneracy_sums(nv, V)
        d = o.last_degeneracy()
        assert np.abs(contri - d["contri"]).max() < 2e-2 and np.abs(strong - d["strong"]).max() < 2e-2, (contri, strong, d)
        assert contri.min() > 50.0  # varied normals: every direction gathers something


def test_neighbour_sets_pinned_to_the_reference(oracle_mod, W, Wref, T):
    """cases 2 and 3 through the reference's own esti_plane (oracle/_ref): same decision, same bits where both planes are finite"""
    import ref as refmod

    if not refmod.available():
        pytest.skip("oracle/_ref/libref_harness.so not built (needs /root/reference)")
    sets = [Wref["nn"][i] for i in np.concatenate([W.idx("rank:"), W.idx("thresh")])]
    for case, ref in zip(*T):
        sets += list(ref["nn"])
    n_ok = 0
    for pts in sets:
        ok_r, p_r = refmod.esti_plane(pts)
        ok_o, p_o = oracle_mod.esti_plane(pts)
        assert ok_r == ok_o, pts
        if np.all(np.isfinite(p_r)) and np.all(np.isfinite(p_o)):
            assert np.array_equal(p_r.view(np.uint32), p_o.view(np.uint32)), (pts, p_r, p_o)
        n_ok += ok_r
    assert len(sets) >= 41 * 9 + 44 and 100 < n_ok < len(sets) - 100
