"""Key frames of the mapping mode on the device (csrc/keyframe.hip) against the numpy restatement of tests/keyframe_cases.py: the radius outlier
filter bit for bit, the range filter's edges, the fitness score, the local map's ring, a 40-frame drive through both undistortion branches, and
the slam_wrapper switch."""
import numpy as np
import pytest

import keyframe_cases as kc
from lsd_amd import capi, lio

pytestmark = pytest.mark.gpu

# the relative tolerance tests/test_overlap_merge_gpu.py holds lio_ndt_overlap_score's score to (written there as `< 0.02 * score`)
OVERLAP_SCORE_RTOL = 0.02


@pytest.fixture(scope="module")
def kf():
    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device")
    k = lio.KeyFramer()
    yield k
    k.close()


def _xyzi(xyz):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return np.concatenate([xyz, np.arange(len(xyz), dtype=np.float32)[:, None]], 1)


def _check_radius(kf, pts, radius=1.0, min_nb=3):
    got, dropped, n_rad = kf.radius_outlier(pts, radius, min_nb)
    want, wdropped = kc.radius_keep(pts, radius, min_nb)
    assert got.dtype == np.uint32 and np.array_equal(got, want), (len(pts), len(got), len(want))
    assert dropped == wdropped and n_rad == len(want)
    return got


@pytest.mark.parametrize("n", [1, 3, 4, 31, 32, 33, 1025])
def test_radius_filter_sizes_at_leaf_and_level_edges(kf, n):
    rng = np.random.default_rng(n)
    pts = _xyzi(rng.uniform(-1.5, 1.5, (n, 3)) * (1.0 if n < 100 else 4.0))
    got = _check_radius(kf, pts)
    if n == 1025:
        assert 0 < len(got) < n


def test_radius_filter_clusters_ties_and_non_finite_rows(kf):
    far = [(50.0, 50.0, 0.0), (50.1, 50.0, 0.0), (50.0, 50.1, 0.0), (50.1, 50.1, 0.0)]
    assert _check_radius(kf, _xyzi([(0, 0, 0), (0.1, 0, 0), (0, 0.1, 0), *far])).tolist() == [3, 4, 5, 6]        # a cluster of exactly 3 goes
    assert _check_radius(kf, _xyzi([(0, 0, 0), (0.1, 0, 0), (0, 0.1, 0), (0, 0, 0.1), *far])).tolist() == list(range(8))  # of exactly 4 stays
    assert _check_radius(kf, _xyzi([(1, 2, 3)] * 4)).tolist() == [0, 1, 2, 3]                                    # coincident points count
    assert _check_radius(kf, _xyzi([(1, 2, 3)] * 3)).tolist() == []
    edge = _xyzi([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)])
    assert _check_radius(kf, edge).tolist() == [0]                                                               # d2 == 1.0f is within
    edge[1, 0] = np.nextafter(np.float32(1), np.float32(2))
    assert _check_radius(kf, edge).tolist() == []                                                                # one ulp above is not
    nan = _xyzi([(0, 0, 0), (0.1, 0, 0), (np.nan, 0, 0), (0, 0.1, 0), (0, np.inf, 0), (0, 0, 0.1), (-np.inf, np.nan, 1)])
    got, dropped, _ = kf.radius_outlier(nan)
    assert got.tolist() == [0, 1, 3, 5] and dropped == 3
    got, dropped, _ = kf.radius_outlier(_xyzi([(np.nan, 0, 0)] * 5))
    assert got.tolist() == [] and dropped == 5
    assert _check_radius(kf, _xyzi([(0, 0, 0), (9, 9, 9)]), 1.0, 0).tolist() == [0, 1]                          # min_neighbours = 0


def test_radius_filter_lattice_with_exact_ties(kf):
    rng = np.random.default_rng(11)
    pts = _xyzi(rng.integers(0, 80, (2000, 3)).astype(np.float32) * np.float32(8.0 / 256.0))   # on the 1/256 m lattice: every d2 is exact
    r = 9.0 / 32.0                                # r2 = 81/1024 exactly: 102 lattice offsets lie ON the sphere
    a = _check_radius(kf, pts, r, 8)
    b = _check_radius(kf, pts, r, 14)
    _check_radius(kf, pts, 1.0, 3)
    assert 0 < len(b) < len(a) < len(pts)
    q = pts[:, :3]
    on_sphere = sum(int((kc.d2_f32(q[i], q) == np.float32(r * r)).sum()) for i in range(0, 2000, 10))
    assert on_sphere > 40                         # (the ties are there: neighbours at d2 == r2 exactly, in a tenth of the queries)


def test_range_filter_edges(kf):
    five = np.float32(5.0)
    rows = [(0.0, 1, 0), (-0.0, 1, 0), (5.0, 1, 0), (-5.0, 1, 0), (1, np.nextafter(five, np.float32(0)), 0), (1, -5.0, 0), (1e-30, -1e-30, 0), (2, 2, 900.0),
            (np.nextafter(five, np.float32(0)), -np.nextafter(five, np.float32(0)), 0)]
    pts = _xyzi(np.repeat(np.array(rows, np.float32), 4, axis=0))   # four coincident copies each: the radius filter keeps every row
    got, _, n_rad = kf.radius_outlier(pts, 1.0, 3, key_frame_range=5.0)
    want, w_rad, _ = kc.filters(pts, 1.0, 3, 5.0)
    assert n_rad == w_rad == len(pts) and np.array_equal(got, want)
    assert sorted(set((got // 4).tolist())) == [4, 6, 7, 8]


def test_fitness_score(kf):
    rng = np.random.default_rng(5)
    target = np.concatenate([rng.uniform(10, 30, (4999, 3)), [[0, 0, 0]]]).astype(np.float32)
    target = np.concatenate([target, np.ones((5000, 1), np.float32)], 1)
    kf.reset()
    assert kf.append_local_map(target, np.eye(4)) == 5000
    assert np.array_equal(kf.local_map().view(np.uint32), target.view(np.uint32))
    src = target[rng.integers(0, 4999, 3000)].copy()
    src[:, :3] += rng.normal(0, 0.05, (3000, 3)).astype(np.float32)
    T = np.eye(4)
    T[:3, 3] = [0.02, -0.01, 0.03]
    for cloud, pose in ((src, T), (src, np.eye(4))):
        score, nr = kf.fitness(cloud, pose)
        ws, wn = kc.fitness(target, cloud, pose, 1.0, gated=False)
        print("fitness: device %.17g restatement %.17g nr %d" % (score, ws, nr))
        assert nr == wn == 3000 and abs(score - ws) <= OVERLAP_SCORE_RTOL * ws
    Tfar = np.eye(4)
    Tfar[0, 3] = 1000.0
    assert kf.fitness(src, Tfar) == (kc.DBL_MAX, 0)                                        # none in range
    one = np.array([[1, 0, 0, 1], [0, -1, 0, 1], [np.nextafter(np.float32(1), np.float32(2)), 0, 0, 1], [500, 0, 0, 1]], np.float32)
    score, nr = kf.fitness(one, np.eye(4))                                                 # d2 == 1.0f exactly is in range, an ulp above is not
    assert nr == 2 and score == 1.0 and kc.fitness(target, one, np.eye(4), 1.0, gated=False) == (1.0, 2)


def test_ring_crosses_the_cap_by_a_partial_frame():
    k = lio.KeyFramer(local_map_cap=1000)
    try:
        rng = np.random.default_rng(9)
        want = np.zeros((0, 4), np.float32)
        for i, n in enumerate((400, 400, 400, 250, 1300)):
            cloud = rng.uniform(-20, 20, (n, 4)).astype(np.float32)
            T = np.eye(4)
            c, s = np.cos(0.3 * i), np.sin(0.3 * i)
            T[:2, :2], T[:3, 3] = [[c, -s], [s, c]], [i, -2.0 * i, 0.5]
            want = kc.ring_append(want, cloud, T, 1000)
            assert k.append_local_map(cloud, T) == len(want) == min(1000, 400 * (i + 1))
            assert np.array_equal(k.local_map().view(np.uint32), want.view(np.uint32)), i   # the front is dropped, the order kept
            q = want[::37].copy()
            assert k.fitness(q, np.eye(4))[1] == len(q)                                    # the tree is the new map's
    finally:
        k.close()


@pytest.fixture(scope="module")
def frames():
    return kc.drive_frames()


def _drive(k, ref, frames, branch):
    reports = []
    for pts, st, header, odom, delta, pstamps, plist in frames:
        kw = dict(delta=delta) if branch == "delta" else dict(pose_stamps_us=pstamps, poses=plist)
        got = k.push(pts, st, header, odom, **kw)
        reports.append(got)
        if ref is None:
            continue
        want = ref.push(pts, st, header, odom, **({"delta": delta} if branch == "delta" else {"pose_stamps": pstamps, "poses": plist}))
        for key in ("first", "need", "must", "elected", "emitted", "nr", "n_downsampled", "local_map_size"):
            assert got[key] == want[key], (len(reports), key, got, want)
        assert got["dx"] == want["dx"] or abs(got["dx"] - want["dx"]) <= 1e-6 * want["dx"]
        assert abs(got["accum_distance"] - want["accum_distance"]) <= 1e-12 * max(1.0, want["accum_distance"])
        if want["nr"]:
            assert abs(got["score"] - want["score"]) <= OVERLAP_SCORE_RTOL * want["score"]
        else:
            assert got["score"] == want["score"]
    return reports


@pytest.mark.parametrize("D,branch", [(2.0, "delta"), (1.0, "poses")])
def test_drive_emits_the_restatements_key_frames(frames, D, branch):
    cfg = dict(key_frame_distance=D, resolution=0.5)
    k = lio.KeyFramer(**cfg)
    ref = kc.RefKeyFramer(D=D, resolution=0.5)
    try:
        assert k.push(np.zeros((0, 4), np.float32), np.zeros(0, np.uint32), 0, np.eye(4), delta=np.eye(4))["first"] == 0   # an empty cloud: nothing
        reports = _drive(k, ref, frames, branch)
        assert ref.step == (1 if D == 2.0 else 2)
        # the condition the comparison rests on: no election of the restatement is decided by less than 1e-9 relative
        for lhs, rhs in ref.contests:
            assert abs(lhs - rhs) > 1e-9 * max(abs(lhs), abs(rhs)), (lhs, rhs)
        emitted = [i for i, r in enumerate(reports) if r["emitted"]]
        candidates = [i for i, r in enumerate(reports) if r["need"]]
        assert len(emitted) >= 4 and len(candidates) >= 2 * len(emitted) and k.pending() == len(emitted) == len(ref.out)
        first_bytes = []
        for want in ref.out:
            got = k.pop()
            assert got["stamp"] == want["stamp"] and got["n_before_filters"] == want["n_before_filters"] and got["n_after_radius"] == want["n_after_radius"]
            assert np.array_equal(got["points"].view(np.uint32), want["points"].view(np.uint32))
            assert 0 < len(got["points"]) <= got["n_after_radius"] <= got["n_before_filters"]
            assert np.abs(got["pose"] - want["pose"]).max() <= 1e-12 and abs(got["accum_distance"] - want["accum_distance"]) <= 1e-12 * want["accum_distance"]
            first_bytes.append(got["points"].tobytes())
        assert k.pop() is None
        assert np.array_equal(k.local_map().view(np.uint32), ref.local_map.view(np.uint32))
        # reset, then the same drive again: the same bytes
        k.reset()
        assert k.pending() == 0 and len(k.local_map()) == 0
        again = _drive(k, None, frames, branch)
        assert [r["emitted"] for r in again] == [r["emitted"] for r in reports] and [r["score"] for r in again] == [r["score"] for r in reports]
        assert [k.pop()["points"].tobytes() for _ in range(k.pending())] == first_bytes
    finally:
        k.close()


def _wrapper_drive(sw, on):
    from test_outer_boundary import _drive as boundary_drive, _rpyt

    imu_ext, ins_ext = (0.05, -0.02, 0.10, 3.0, 0.5, -1.0), (0.30, 0.10, -0.20, -4.0, 1.0, 2.0)
    assert sw.init_slam("mapping", "", "FastLIO", ["0-lidar", "IMU"], 0.5, 0.2, 10.0, 60.0) == ["IMU", "0-lidar"]
    sw._set_capacity(4_000_000, 1 << 20)
    sw.set_ins_external_param(*ins_ext)
    sw.set_imu_external_param(*imu_ext)
    if on:
        sw.set_keyframe_output(True)
    assert sw.setup_slam() is True
    fed = []

    def process(points, attr, a, b, c, d, imu, stamp):
        out = sw.process(points, attr, a, b, c, d, imu, stamp)
        fed.append((points["0-lidar"], attr["0-lidar"]["points_attr"][:, 0].astype(np.uint32), attr["0-lidar"]["timestamp"], *sw._last_odometry()))
        return out

    try:
        boundary_drive(process, n=24)
        return sw.update_odom(), fed, _rpyt(*ins_ext)
    finally:
        sw.deinit_slam()


def test_wrapper_switch_off_and_on():
    import slam_wrapper as sw

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device")
    off, _, _ = _wrapper_drive(sw, False)
    assert off == {"odoms": {}, "keyframes": []}
    on, fed, T_static = _wrapper_drive(sw, True)
    assert on["odoms"] == {} and len(on["keyframes"]) >= 1
    k = lio.KeyFramer(key_frame_distance=float(np.float32(0.2)), key_frame_degree=10.0, resolution=0.5, key_frame_range=60.0)
    try:
        for pts, st, header, first, second in fed:
            k.push(kc.transform_f64(pts, T_static), st, header, first, delta=kc.rigid_inverse(first) @ second)
        assert k.pending() == len(on["keyframes"])
        for f in on["keyframes"]:
            want = k.pop()
            assert set(f) == {"points", "image", "pose", "stamp"} and f["image"] == {}
            assert f["points"].dtype == np.float32 and f["points"].ndim == 2 and f["points"].shape[1] == 4
            assert f["pose"].dtype == np.float32 and f["pose"].shape == (4, 4) and f["stamp"] == want["stamp"]
            assert np.array_equal(f["points"].view(np.uint32), want["points"].view(np.uint32))
            assert np.array_equal(f["pose"], want["pose"].astype(np.float32))
    finally:
        k.close()
