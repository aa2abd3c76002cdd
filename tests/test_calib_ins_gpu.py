"""The lidar-INS calibration on the device against the restatement of tests/calib_ins_cases.py.

Shapes: 3 scans of about 700 points give several tree levels and leaves that are not full; the edge inputs are a handful of points each.

Bounds.  The combined cloud and the n x K terms are compared on every bit with numpy's f32 in the stated operation order.  The device's cost
against the f64 sum of those same terms: rtol 1e-12 (the same f64 addends in another order: n K <= 1e4 addends, each rounding 1.1e-16).
End to end, J is the restated local-metric cost (cKDTree, f64) and the condition is the issue's:
J(result) <= J(yardstick) + 0.05 (J(init) - J(yardstick)); the x, y and yaw errors of the result are each smaller than the initial ones.
Measured on an MI355X (profiles/calib_ins_bench.json holds the run): J(init) 785.13, J(truth) 254.91, J(yardstick) 261.18, J(twin) 257.89,
J(result) 257.89 against the bound 287.38, 989 evaluations; x / y / yaw errors 0.40 m / 0.34 m / 0.025 rad before and 0.009 m / 0.017 m /
0.004 rad after; z 0.05 m before and 0.36 m after (the yardstick: 0.49 m), roll / pitch 0.035 / 0.035 rad before and 0.0004 / 0.0003 after."""
import numpy as np
import pytest

import calib_ins_cases as CI
from lsd_amd import capi, lio

pytestmark = pytest.mark.gpu
STAMP0 = 1_700_000_000_000_000
X = np.array([0.3, -0.2, 0.15, 0.05, -0.04, 0.2])


def _odom(cal, m=6, shift=0):
    stamps, Ts = [], []
    for i in range(m):
        T = CI.se3_matrix(CI.se3_exp(np.array([1.5 * i, 0.2 * i * i, 0.02 * i, 0.01 * i, -0.015 * i, 0.12 * i])))
        stamps.append(STAMP0 + 100_000 * i + shift)
        Ts.append(T.astype(np.float32))
        cal.add_odom(Ts[-1], stamps[-1])
    return stamps, Ts


def _surface(n, seed):
    """points on a floor, two walls and a box, seen from near the origin"""
    rng = np.random.default_rng(seed)
    k = n // 4
    floor = np.stack([rng.uniform(-6, 6, k), rng.uniform(-6, 6, k), rng.normal(0, 0.01, k)], 1)
    wall1 = np.stack([np.full(k, 6.0) + rng.normal(0, 0.01, k), rng.uniform(-6, 6, k), rng.uniform(0, 3, k)], 1)
    wall2 = np.stack([rng.uniform(-6, 6, k), np.full(k, -6.0) + rng.normal(0, 0.01, k), rng.uniform(0, 3, k)], 1)
    m = n - 3 * k
    box = np.stack([rng.uniform(2, 3, m), rng.uniform(1, 2, m), np.full(m, 1.0)], 1)
    return np.concatenate([floor, wall1, wall2, box]).astype(np.float32)


@pytest.fixture(scope="module")
def base():
    """3 scans of 690 / 700 / 713 points, 6 odometry entries; the combined cloud and both metrics' terms from the restatement, computed once"""
    cal = lio.InsCalib(init=np.eye(4))
    _odom(cal)
    scans, stamps = [_surface(n, 20 + i) for i, n in enumerate((690, 700, 713))], [STAMP0 + 120_000, STAMP0 + 250_000, STAMP0 + 410_000]
    for s, st in zip(scans, stamps):
        assert cal.add_scan(s, st) == len(s)  # fewer than 6000 points: the ratio is 1, all are kept
    cal.set_transform(X)
    mats = cal.scan_matrices(0.0)
    cloud = CI.combined_f32(mats, scans)
    ref = {m: CI.terms_brute_f32(cloud, m) for m in (0, 1)}
    for v in ref.values():
        v.setflags(write=False)
    return dict(cal=cal, scans=scans, stamps=stamps, mats=mats, cloud=cloud, terms=ref)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_scan_matrices_follow_the_restated_interpolation(base):
    cal = base["cal"]
    ostamps = [STAMP0 + 100_000 * i for i in range(6)]
    oT = [CI.se3_exp(np.array([1.5 * i, 0.2 * i * i, 0.02 * i, 0.01 * i, -0.015 * i, 0.12 * i])) for i in range(6)]
    for off in (0.0, 0.03, -0.2):
        cal.set_transform(X)
        got = cal.scan_matrices(off).astype(np.float64)
        want = [CI.se3_matrix(CI.se3_mul(P, CI.se3_exp(X.astype(np.float32).astype(np.float64)))) for P in CI.scan_poses(ostamps, oT, base["stamps"], off)]
        assert np.abs(got - np.array(want)).max() <= 32 * 2.0 ** -23 * 8.0  # f32 roundings at translations of up to 8 m, through exp / log / two products
    cal.scan_matrices(0.0)


def test_combined_cloud_bit_for_bit(base):
    got = base["cal"].combined(X)
    assert got.shape == base["cloud"].shape and np.array_equal(_bits(got), _bits(base["cloud"]))


@pytest.mark.parametrize("metric", [0, 1])
def test_terms_bit_for_bit_and_their_sum(base, metric):
    cal, want = base["cal"], base["terms"][metric]
    got = cal.error_terms(X, metric)
    assert got.shape == want.shape == (len(base["cloud"]), CI.METRICS[metric][0])
    assert np.array_equal(_bits(got), _bits(want))
    assert np.all(got[:, 0] == 0) and np.all(np.diff(got, axis=1) >= 0)  # the point itself first, ascending
    e = cal.error(X, metric)
    s = float(want.astype(np.float64).sum())
    print(f"metric {metric}: device {e!r} f64 sum of the restated terms {s!r} rel {abs(e - s) / s:.2e}")
    assert abs(e - s) <= 1e-12 * s
    assert cal.error(X, metric | lio.InsCalib.UNCAPPED) == e  # the walk from +inf finds the same terms


@pytest.mark.parametrize("metric", [0, 1])
def test_the_capped_walk_loses_nothing(base, metric):
    """the same cloud through the public k-NN index (uncapped, an independent device path), capped in numpy"""
    K, cap = CI.METRICS[metric]
    idx = lio.KnnIndex()
    assert idx.build(base["cloud"]) == len(base["cloud"])
    _, d2 = idx.query(base["cloud"], K)
    assert np.array_equal(_bits(np.minimum(d2, np.float32(cap))), _bits(base["cal"].error_terms(X, metric)))
    idx.close()


def _fresh(scans, stamps=None, shift=0):
    cal = lio.InsCalib(init=np.eye(4))
    _odom(cal, shift=shift)
    kept = [cal.add_scan(s, (STAMP0 + 150_000 + 70_000 * i if stamps is None else stamps[i]) + shift) for i, s in enumerate(scans)]
    return cal, kept


def _check(cal, scans, metrics=(0, 1)):
    cal.set_transform(X)
    cloud = CI.combined_f32(cal.scan_matrices(0.0), scans)
    assert np.array_equal(_bits(cal.combined(X)), _bits(cloud))
    out = {}
    for m in metrics:
        want = CI.terms_brute_f32(cloud, m)
        got = cal.error_terms(X, m)
        assert np.array_equal(_bits(got), _bits(want)), m
        assert abs(cal.error(X, m) - float(want.astype(np.float64).sum())) <= 1e-12 * max(1.0, float(want.sum()))
        out[m] = got
    return out


def test_a_scan_added_twice(base):
    s = base["scans"][0][:300]
    cal, _ = _fresh([s, s], stamps=[STAMP0 + 200_000, STAMP0 + 200_000])
    t = _check(cal, [s, s])
    assert np.all(t[1][:, 1] == 0) and np.all(t[0][:, 1] == 0)  # every point has its copy at distance 0


def test_isolated_points_pay_the_cap():
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * 4.0  # 4 m apart: d2 = 16 > 10
    cal, _ = _fresh([g[:40], g[40:]], stamps=[STAMP0 + 200_000, STAMP0 + 200_000])  # one pose for both: the grid stays a grid
    t = _check(cal, [g[:40], g[40:]])
    assert np.all(t[0][:, 1:] == 10.0) and np.all(t[1][:, 1] == 1.0) and np.all(t[0][:, 0] == 0)


def test_the_squared_distance_equal_to_the_cap():
    cal = lio.InsCalib(init=np.eye(4))
    for i in range(2):
        cal.add_odom(np.eye(4), STAMP0 + 100_000 * i)
    pair = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    assert cal.add_scan(pair, STAMP0 + 50_000) == 2
    cal.scan_matrices(0.0)
    z = np.zeros(6)
    assert np.array_equal(cal.error_terms(z, 1), [[0, 1], [0, 1]]) and cal.error(z, 1) == 2.0  # d2 == cap exactly
    with pytest.raises(capi.LioError) as ei:  # two points, the global metric needs K = 4
        cal.error(z, 0)
    assert f"error {capi.LIO_E_STATE}" in str(ei.value)


@pytest.mark.parametrize("n,metric", [(4, 0), (2, 1), (32, 0), (33, 0), (32, 1), (33, 1), (3, 0), (1, 1)])
def test_totals_at_the_edges(base, n, metric):
    """exactly K points, one full leaf, one leaf + 1; K - 1 points is LIO_E_STATE"""
    pts = base["scans"][1][:n]
    a = n // 2
    cal, kept = _fresh([pts[:a], pts[a:]])
    assert kept == [a, n - a]
    if n < CI.METRICS[metric][0]:
        cal.scan_matrices(0.0)
        for call in (cal.error, cal.error_terms):
            with pytest.raises(capi.LioError) as ei:
                call(X, metric)
            assert f"error {capi.LIO_E_STATE}" in str(ei.value)
        return
    _check(cal, [pts[:a], pts[a:]], metrics=(metric,))


def test_an_empty_scan_between_two_others(base):
    a, b = base["scans"][0][:150], base["scans"][2][:170]
    e = np.zeros((0, 3), np.float32)
    cal, kept = _fresh([a, e, b])
    assert kept == [150, 0, 170] and cal.counts() == (3, 6, 320)
    _check(cal, [a, e, b])


def test_non_finite_points_are_drawn_for_and_dropped():
    n, stamp = 7000, STAMP0 + 222_222  # more than 6000: the draws decide, so a shifted draw sequence would show
    pts = _surface(n, 31)
    bad = pts.copy()
    bad[10, 0], bad[500, 1], bad[6999, 2], bad[3000, 0] = np.nan, np.inf, -np.inf, np.nan
    keep = CI.keep_mask(n, stamp)
    want = pts[keep & np.isfinite(bad).all(1)]
    cal = lio.InsCalib(init=np.eye(4))
    assert cal.add_scan(bad, stamp) == len(want)
    for i in range(2):
        cal.add_odom(np.eye(4), STAMP0 + 400_000 * i)
    cal.scan_matrices(0.0)
    assert np.array_equal(_bits(cal.combined(np.zeros(6))), _bits(want))  # identity poses: the kept points themselves, in input order
    with pytest.raises(capi.LioError):
        cal.add_scan(np.zeros((5, 2), np.float32), stamp)  # a stride below 3


def test_two_entries_with_one_stamp_are_refused(base):
    cal = lio.InsCalib(init=np.eye(4))
    for _ in range(2):
        cal.add_odom(np.eye(4), STAMP0)
    cal.add_scan(base["scans"][0][:50], STAMP0 + 10)
    with pytest.raises(capi.LioError) as ei:
        cal.error(np.concatenate([X, [0.0]]), 1)
    assert f"error {capi.LIO_E_INVALID}" in str(ei.value)
    one = lio.InsCalib(init=np.eye(4))
    one.add_odom(np.eye(4), STAMP0)
    one.add_scan(base["scans"][0][:50], STAMP0 + 10)
    with pytest.raises(capi.LioError) as ei:
        one.scan_matrices(0.0)
    assert f"error {capi.LIO_E_STATE}" in str(ei.value)


@pytest.mark.parametrize("delta", [0.031, -0.1999])
def test_the_time_offset_is_a_shift_of_the_scan_stamps(base, delta):
    cal = base["cal"]
    shift = int(1000000.0 * delta)
    other = lio.InsCalib(init=np.eye(4))
    _odom(other)
    for s, st in zip(base["scans"], base["stamps"]):
        other.add_scan(s, st + shift)
    other.scan_matrices(0.0)
    for m in (0, 1):
        assert cal.error(np.concatenate([X, [delta]]), m) == other.error(X, m)
    cal.scan_matrices(0.0)


def test_no_state_leaks_between_evaluations(base):
    cal = base["cal"]
    x7 = np.concatenate([X, [0.0]])
    first = {m: np.float64(cal.error(x7, m)).tobytes() for m in (0, 1)}
    cal.error(np.concatenate([X + 0.3, [0.11]]), 0)
    cal.error(X * -1.0, 1)
    cal.error_terms(X * 0.5, 0)
    for m in (1, 0):
        assert np.float64(cal.error(x7, m)).tobytes() == first[m]
    assert np.float64(cal.error(X, 1)).tobytes() == first[1]  # six parameters: the scan poses as the last call left them (offset 0)
    t = cal.last_times()
    assert all(v > 0 for v in t)


def test_end_to_end(base):
    """Six key scans of 32 x 400 rays in a small yard, odometry at 100 Hz, the initial transform off by 0.5 m and 3 degrees.
    The figures of the recorded run are in profiles/calib_ins_bench.json (tools/calib_ins_bench.py writes them)."""
    g = np.load(CI.GOLDEN)
    scans, stamps, odom, ostamps = CI.e2e_inputs()
    assert CI.checksum(scans) == str(g["checksum"]), "the generated scans are not the ones the golden costs were recorded for"
    truth, init = g["truth"], g["init"]
    j_init, j_truth, j_y, j_twin = float(g["J_init"]), float(g["J_truth"]), float(g["J_yardstick"]), float(g["J_twin"])
    assert j_init >= 3 * j_truth
    cal = lio.InsCalib(init=CI.se3_matrix(CI.se3_exp(init)))
    R = CI.e2e_restated(scans, stamps, odom, ostamps)
    for s, st, r in zip(scans, stamps, R.scans):
        assert cal.add_scan(s, st) == len(r)
    for M, st in zip(odom, ostamps):
        cal.add_odom(M, st)
    cal.scan_matrices(0.0)
    T = cal.calibrate().astype(np.float64)
    evals, best, finished = cal.progress()
    x = CI.se3_log(CI.se3_from_matrix(T))
    j_res = R.cost(np.concatenate([x, [0.0]]), 1)
    (dt0, dr0), (dt1, dr1) = CI.pose_errors(init, truth), CI.pose_errors(x, truth)
    bound = j_y + 0.05 * (j_init - j_y)
    print(f"J(init) {j_init:.3f} J(truth) {j_truth:.3f} J(yardstick) {j_y:.3f} J(twin) {j_twin:.3f} J(result) {j_res:.3f} bound {bound:.3f} evals {evals} "
          f"device best {best:.3f}\n  |dxyz| init {dt0} result {dt1}\n  |drot| init {dr0} result {dr1}")
    assert finished and evals <= 2 * 501
    assert j_res <= bound
    assert dt1[0] < dt0[0] and dt1[1] < dt0[1] and dr1[2] < dr0[2]  # x, y and yaw; z, roll and pitch are printed, a planar drive need not observe them
