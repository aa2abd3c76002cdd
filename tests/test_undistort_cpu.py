"""The references of tests/undistort_cases.py against each other and against the oracle: nothing here needs a GPU.  The float64
restatement of undistort_point equals the oracle bit for bit, the long-double value and the oracle agree to the error budget E the
module's docstring records, every builder delivers the branches it promises, and (where oracle/_ref is built) the reference's own
headers agree on a sample that takes both sides of |gyr| dt = 0.5."""
import re

import numpy as np
import pytest

import ref
import undistort_cases as UC


@pytest.fixture(scope="module")
def cases():
    return UC.all_imu_cases()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_float64_restatement_equals_the_oracle_bit_for_bit(oracle_mod, cases):
    """every single-pass point of every case: (float) of the numpy restatement == orc_undistort_point, so that the restatement's value
    BEFORE the cast is the oracle's"""
    total = 0
    for c in cases:
        w = UC.walk(c)
        sel = UC.single_pass(c, w)
        if len(sel) == 0:
            continue
        fl = UC.flow(c, oracle_mod, w)
        r = UC.restate64(c, sel, w).astype(np.float32)
        assert np.array_equal(_bits(r), _bits(fl[sel, :3])), c["name"]
        total += len(sel)
    # the wrapper the oracle publishes is the function flow() calls
    c, w = cases[2], UC.walk(cases[2])
    for i in UC.single_pass(c, w)[:50]:
        hd, tl = c["poses"][w["h"][i]], c["poses"][w["h"][i] + 1]
        o = oracle_mod.undistort_point(hd[13:22], hd[7:10], hd[10:13], tl[1:4], tl[4:7], w["t"][i] - hd[0], c["pts"][i, :3], c["end_pos"], c["end_rot"], c["ril"], c["til"])
        assert np.array_equal(_bits(o), _bits(UC.restate64(c, np.array([i]), w).astype(np.float32)[0]))
    assert total > 60000


def test_long_double_and_oracle_agree_to_the_recorded_budget(cases):
    """E per case, printed; the figures recorded in the module's docstring hold to their leading digit; no case is far from the handful of
    f64 roundings E stands for (a coordinate of <= ~100 m: ulp 1.4e-14)"""
    worst = {}
    for c in cases:
        E = UC.error_budget(c)
        worst[c["name"]] = E
        print("E[%s] = %.2e" % (c["name"], E))
        assert E < 4e-13, c["name"]
    rec = {m.group(1): float(m.group(2)) for m in re.finditer(r"^    ([a-z][\w-]+)\s+([0-9.]+e[-+]\d+)$", UC.__doc__, re.M)}
    assert set(rec) == set(worst)
    for name, E in worst.items():  # to the leading digit: within one unit of it
        assert abs(E - rec[name]) < (10.0 ** np.floor(np.log10(rec[name])) if rec[name] > 0 else 1e-300), (name, E, rec[name])
    # the flow reference's cast agrees with the rounded long-double value except where the two straddle an f32 rounding boundary
    c = cases[2]
    sel = UC.single_pass(c)
    ex = UC.exact(c, sel)
    r64 = UC.restate64(c, sel)
    assert np.all(np.abs(r64.astype(np.float32).astype(np.longdouble) - ex) <= UC.ulp_f32(ex.astype(np.float64)) / 2 + worst["rotating"])


def test_builders_deliver_their_branches(cases):
    by = {c["name"]: c for c in cases}
    cnt = lambda c: np.bincount(UC.labels(c), minlength=6)  # noqa: E731
    # the no-rotation case: every compensated point is STILL; its twin one f64 step above the threshold takes the trig path everywhere
    a, b = cnt(by["still"]), cnt(by["still-above"])
    assert a[UC.STILL] > 19000 and a[UC.TAYLOR] == a[UC.LIBRARY] == 0 and a[UC.FILTERED] == 1 and a[UC.UNTOUCHED] >= 1
    assert b[UC.TAYLOR] == a[UC.STILL] and b[UC.STILL] == 0
    g = np.linalg.norm(by["still"]["poses"][1:, 4:7], axis=1)
    assert set(np.unique(g > 0)) == {False, True} and (g == 1e-7).sum() >= 3 and ((g > 0) & (g < 1e-7)).sum() >= 3 and g.max() == 1e-7
    assert np.all(np.linalg.norm(by["still-above"]["poses"][1:, 4:7], axis=1) == np.nextafter(1e-7, 1.0))
    # rotating: both sin_versin branches a thousand times, |gyr| dt over [0, 0.7], the three boundary groups on their sides of 0.5
    c = by["rotating"]
    r, th, lab = cnt(c), UC.gyr_dt(c), UC.labels(c)
    assert r[UC.TAYLOR] >= 1000 and r[UC.LIBRARY] >= 1000 and r[UC.REPEATED] == 0
    assert np.nanmax(th) <= 0.7 and np.nanmax(th) > 0.69 and np.nanmin(th) < 1e-3
    hist = np.histogram(th[~np.isnan(th)], bins=7, range=(0, 0.7))[0]
    assert hist.min() >= 300, hist
    bd = c["boundary"]
    assert np.all((th[bd["below"]] < 0.5) & (th[bd["below"]] > 0.5 - 1e-6)) and np.all(lab[bd["below"]] == UC.TAYLOR)
    assert np.all((th[bd["above"]] > 0.5) & (th[bd["above"]] < 0.5 + 1e-6)) and np.all(lab[bd["above"]] == UC.LIBRARY)
    assert np.all(th[bd["exact"]] == 0.5) and np.all(lab[bd["exact"]] == UC.LIBRARY)
    mags = np.linalg.norm(c["poses"][1:, 4:7], axis=1)
    assert np.isclose(mags, 0.3).any() and np.isclose(mags, 2.0).any() and ((mags >= 4) & (mags <= 8)).sum() >= 8
    # the repeated point: who, and how many passes
    for v in UC.REPEAT_VARIANTS:
        c = by["repeat-" + v]
        w = UC.walk(c)
        who, passes = UC.REPEAT_EXPECT[v]
        assert w["passes"] == passes, (v, w["passes"])
        rep = np.nonzero(UC.labels(c, w) == UC.REPEATED)[0]
        assert list(rep) == ([] if who is None else [who]), (v, rep)
    assert len(by["repeat-tail_wg"]["pts"]) == 16385 + 200 and UC.walk(by["repeat-tail_wg"])["first"] // 256 == 64
    assert cnt(by["repeat-blind"])[UC.FILTERED] == 1 and cnt(by["repeat-decimated"])[UC.FILTERED] == 2000
    assert cnt(by["repeat-zero"])[UC.UNTOUCHED] == 1 and cnt(by["repeat-head0"])[UC.UNTOUCHED] == 0
    # a stamp on a pose offset belongs to the earlier segment; stamps beyond the last pose use the last segment
    c = by["sizes-n900-p6-onoffset"]
    w = UC.walk(c)
    on = np.isin(w["t"][:10], c["poses"][:, 0])
    assert on.all() and np.all(c["poses"][w["h"][:10] + 1, 0] == w["t"][:10])
    c = by["sizes-n900-p6-beyond"]
    w = UC.walk(c)
    assert (w["t"] > c["poses"][-1, 0]).sum() > 200 and np.all(w["h"][w["t"] > c["poses"][-1, 0]] == 4)
    for p in (2, 3, 127, 128):
        assert len(by["sizes-n700-p%d" % p]["poses"]) == p
    # filters: the points on the radius are dropped, their outward neighbours kept
    for fn in (1, 2, 3, 7):
        c = UC.case_filters(fn)
        w = UC.walk(c)
        e = c["edge"]
        assert not w["keep"][e["on"]].any() and not w["keep"][e["inside"]].any()
        assert np.array_equal(w["keep"][e["outside"]], e["outside"] % fn == 0) and (fn > 2 or w["keep"][e["outside"]].any())
        assert UC.labels(c, w).max() <= UC.UNTOUCHED


def test_pose_list_segment_restatement_is_the_oracles_walk(oracle_mod):
    """the pure-translation cases: the oracle's output equals 'every point moved by its own interval's translation', the interval being
    the prefix maximum pose_list_segments() states -- so a bit-exact device result pins the segment of every point"""
    for layout in UC.POSE_LAYOUTS:
        c = UC.pose_list_case(4097, layout)
        seg = UC.pose_list_segments(c)
        out = oracle_mod.undistort_poses(c["pts"], c["stamp"], c["header"], c["pose_stamps"], c["pose_T"])
        n_poses = len(c["pose_stamps"])
        exp = c["pts"].copy()
        for i in range(1, n_poses):
            m = seg == i
            assert not (c["stamp"][m].astype(np.uint64) > c["pose_stamps"][i] - np.uint64(c["header"])).any()
            # two poses: interval i alone, which covers every stamp handed to it
            exp[m] = oracle_mod.undistort_poses(c["pts"][m], c["stamp"][m], c["header"], c["pose_stamps"][[0, i]], c["pose_T"][[0, i]])
        assert np.array_equal(_bits(exp), _bits(out)), layout
        assert (seg < n_poses).sum() >= 300 and (layout != "past_last_early" or (seg == n_poses).sum() > 3000)
        if layout != "sorted":
            assert (seg != 1 + np.searchsorted((c["pose_stamps"][1:] - np.uint64(c["header"])), c["stamp"].astype(np.uint64), side="left")).any(), layout


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libref_harness.so not built (needs /root/reference)")
def test_reference_headers_agree_on_both_sides_of_one_half(oracle_mod, cases):
    c = cases[2]
    w, lab = UC.walk(c), UC.labels(c)
    rng = np.random.default_rng(5)
    pick = np.concatenate([rng.choice(np.nonzero(lab == UC.LIBRARY)[0], 150, replace=False), rng.choice(np.nonzero(lab == UC.TAYLOR)[0], 150, replace=False),
                           c["boundary"]["below"][:5], c["boundary"]["exact"][:5], c["boundary"]["above"][:5]])
    assert (UC.gyr_dt(c, w)[pick] > 0.5).sum() >= 150
    for i in pick:
        hd, tl = c["poses"][w["h"][i]], c["poses"][w["h"][i] + 1]
        a = [hd[13:22], hd[7:10], hd[10:13], tl[1:4], tl[4:7], w["t"][i] - hd[0], c["pts"][i, :3], c["end_pos"], c["end_rot"], c["ril"], c["til"]]
        assert np.array_equal(_bits(oracle_mod.undistort_point(*a)), _bits(ref.undistort_point(*a))), i
