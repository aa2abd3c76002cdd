"""Ground extraction on the device (csrc/ground.hip, lio_ground_*; slam_wrapper.set_ground_extraction, _detect_ground and
accumulate_cloud(extract_ground=True)) against the CPU restatement of tests/ground_cases.py.

The clip is held index for index; the normals to numpy.linalg.eigh within 0.05 degrees where the eigen-gap is at least 0.01, and the filter's
verdict wherever the f64 angle is not within 0.1 degrees of the threshold (band and small-gap points together may be at most 1 % of the
clipped cloud); the RANSAC bit for bit on the device's own filtered set: triples, counts, the replayed loop, the winning draw, the
coefficients and the inlier list."""
import numpy as np
import pytest

import ground_cases as gc

pytestmark = pytest.mark.gpu


def _need_gpu():
    from lsd_amd import capi

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")


def _module():
    import slam_wrapper

    assert slam_wrapper.__file__.endswith(".so")
    return slam_wrapper


@pytest.fixture
def ground_switch():
    sw = _module()
    yield sw
    sw.set_ground_extraction(False)


@pytest.fixture(scope="module")
def scene_pts():
    p = gc.scene()
    # the clip's edge cases, in the middle of the cloud: NaN, +-inf, z exactly on the lower end (kept) and on the upper end (dropped)
    edge = np.array([[np.nan, 0, 0, 1], [0, np.inf, 0, 1], [0, 0, -np.inf, 1], [3, 4, -1.5, 1], [3, 4, 1.5, 1],
                     [3, 4, np.nextafter(np.float32(1.5), np.float32(0)), 1], [3, 4, np.nextafter(np.float32(-1.5), np.float32(-2)), 1]], np.float32)
    return np.concatenate([p[:50_000], edge, p[50_000:]])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_ransac(det, pts, prm, res):
    """the RANSAC of the last call, bit for bit, on the device's own filtered set; returns the restated run and the filtered indices"""
    from lsd_amd import lio

    fidx = det.indices(1).astype(np.int64)
    assert len(fidx) == res["n_filtered"]
    tri, counts, planes = det.draws()
    run = det.last_run()
    if len(fidx) < prm.min_points or len(fidx) < 3:
        assert len(counts) == 0 and not res["found"] and run["winner"] == -1 and res["n_inliers"] == 0
        return None, fidx
    P = pts[fidx, :3]
    assert len(counts) % 64 == 0 and len(counts) >= 64
    rt, rc, rp, rrun = gc.ransac(P, prm.seed, len(counts), np.float32(prm.distance_threshold), prm.max_iterations, prm.probability)
    assert np.array_equal(tri.astype(np.int64), rt)                      # the triples
    assert np.array_equal(rt, lio.ground_draw(prm.seed, np.arange(len(counts)), len(P)))  # (the numpy form of the rule agrees)
    assert np.array_equal(counts, rc)                                    # every scored hypothesis's count (and which draws are bad)
    good = counts != gc.BAD
    assert np.array_equal(_bits(planes[good]), _bits(rp[good])) and np.isnan(planes[~good]).all()
    assert run == rrun, (run, rrun)                                      # the replayed loop and the winning draw
    assert len(counts) - run["draws_used"] < 64                          # no batch beyond the one the loop ended in
    win = rp[run["winner"]]
    inl = np.nonzero(gc.residual_ok(P, win, np.float32(prm.distance_threshold)))[0]
    assert res["n_inliers"] == len(inl) == int(counts[run["winner"]])
    assert np.array_equal(det.indices(2).astype(np.int64), fidx[inl])    # the inlier list
    assert np.array_equal(_bits(det.inliers()), _bits(pts[fidx[inl]]))
    refuse = len(inl) < prm.min_points or abs(float(win[2])) < np.cos(np.radians(prm.floor_normal_thresh_deg))
    assert res["found"] == (not refuse)
    if res["found"]:
        want = -win if win[2] < 0 else win
        assert np.array_equal(_bits(res["coeffs"]), _bits(want)) and res["coeffs"][2] >= 0
    return dict(run=rrun, win=win, inliers=fidx[inl]), fidx


def test_clip_normals_filter_and_ransac_on_the_scene(scene_pts):
    _need_gpu()
    from lsd_amd import lio

    pts = scene_pts
    det = lio.GroundDetector()
    prm = det.params(0, seed=11)
    res = det.detect_host(pts, prm)
    # 1. the clip, index for index
    cidx = gc.clip(pts)
    assert np.array_equal(det.indices(0).astype(np.int64), cidx) and res["n_clipped"] == len(cidx)
    z_of = {float(pts[i, 2]) for i in cidx if pts[i, 0] == 3 and pts[i, 1] == 4}
    assert -1.5 in z_of and 1.5 not in z_of and len(z_of) == 2
    # 2. the normals and the filter
    C = pts[cidx, :3]
    nn, tie = gc.self_knn(C)
    assert not tie.any()                                         # no exact 10th / 11th neighbour tie on this scene
    assert (nn[:, 0] == np.arange(len(C))).all()                 # every point is its own first neighbour
    n_ref, gap, ang = gc.normals(C, nn)
    n_dev = det.normals().astype(np.float64)
    assert n_dev.shape == n_ref.shape and np.isfinite(n_dev).all()
    assert np.abs(np.linalg.norm(n_dev, axis=1) - 1).max() < 1e-6
    small_gap = gap < 0.01
    band = np.abs(ang - 20.0) <= 0.1
    dev_ang = np.degrees(np.arccos(np.clip(np.abs((n_dev * n_ref).sum(1)), 0, 1)))
    print(f"clipped {len(cidx)}  band {band.mean():.5f}  small gap {small_gap.mean():.5f}  worst normal angle (gap >= 0.01) {dev_ang[~small_gap].max():.2e} deg")
    assert (band | small_gap).mean() <= 0.01                     # the cap on points the test leaves open
    assert dev_ang[~small_gap].max() < 0.05
    fidx = det.indices(1).astype(np.int64)
    kept_dev = np.isin(cidx, fidx)
    kept_ref = ang < 20.0
    sure = ~band & ~small_gap
    assert np.array_equal(kept_dev[sure], kept_ref[sure])
    assert np.array_equal(fidx, np.sort(fidx)) and res["n_filtered"] == len(fidx)
    print(f"filtered {len(fidx)} (restated {int(kept_ref.sum())})")
    # 3. RANSAC, bit for bit on the device's filtered set
    out, _ = _check_ransac(det, pts, prm, res)
    assert res["found"] and out["run"]["winner"] >= 0
    a, b, c, d = res["coeffs"].astype(np.float64)
    assert abs(-a / c - 0.02) < 2e-3 and abs(-b / c + 0.01) < 2e-3 and abs(-d / c + 1.0) < 0.05  # z = -1 + 0.02 x - 0.01 y
    f_us, r_us = det.last_times()
    print(f"device time: clip + k-NN + normals + filter {f_us:.0f} us, RANSAC + inliers {r_us:.0f} us; inliers {res['n_inliers']}")
    assert f_us > 0 and r_us > 0
    # the same seed again: bit-identical; preset 1 clips 2.0 / 1.0
    first = (det.indices(1), det.indices(2), res["coeffs"].copy())
    res2 = det.detect_host(pts, prm)
    assert np.array_equal(det.indices(1), first[0]) and np.array_equal(det.indices(2), first[1]) and np.array_equal(_bits(res2["coeffs"]), _bits(first[2]))
    p1 = det.params(1, seed=11)
    det.detect_host(pts, p1)
    assert np.array_equal(det.indices(0).astype(np.int64), gc.clip(pts, 0.0, 2.0, 1.0))
    det.close()


def _plain(det, **over):
    """RANSAC on the cloud as it is: no normal filter, a clip that keeps everything finite"""
    return det.params(0, use_normal_filter=0, clip_low=1000.0, clip_high=1000.0, **over)


def test_ransac_cases_bit_for_bit():
    _need_gpu()
    from lsd_amd import capi, lio

    det = lio.GroundDetector()
    rng = np.random.default_rng(21)

    def cloud(xyz):
        return np.column_stack([xyz, rng.uniform(0, 255, len(xyz))]).astype(np.float32)

    # duplicated and collinear draws: a third of the points are one point, a third sit on a line with integer coordinates
    flat = np.column_stack([rng.uniform(-20, 20, (1500, 2)), rng.normal(0, 0.02, 1500)])
    dup = np.tile([[1.0, 1.0, 0.0]], (1500, 1))
    t = rng.integers(-500, 500, 1500).astype(np.float64)
    line = np.column_stack([t, t, np.zeros(1500)])
    pts = cloud(np.concatenate([flat, dup, line])[rng.permutation(4500)])
    skipped = 0
    for seed in range(4):
        prm = _plain(det, seed=seed)
        res = det.detect_host(pts, prm)
        out, fidx = _check_ransac(det, pts, prm, res)
        assert len(fidx) == 4500 and res["n_clipped"] == 4500
        skipped += out["run"]["skipped"]
        assert (det.draws()[1] == gc.BAD).any()
    assert skipped > 0  # the loop met bad draws and counted them as skipped samples
    # fewer than 1024 filtered points: none, nothing scored
    few = cloud(np.column_stack([rng.uniform(-5, 5, (500, 2)), rng.normal(0, 0.01, 500)]))
    prm = _plain(det, seed=1)
    res = det.detect_host(few, prm)
    _check_ransac(det, few, prm, res)
    assert not res["found"] and res["n_filtered"] == 500 and res["coeffs"] is None
    # fewer than 1024 inliers: points spread over a cube; the loop runs to max_iterations (+1, as ransac.hpp's `>` lets it)
    cube = cloud(rng.uniform(-25, 25, (2000, 3)))
    res = det.detect_host(cube, prm)
    out, _ = _check_ransac(det, cube, prm, res)
    assert not res["found"] and 0 < res["n_inliers"] < 1024 and out["run"]["iterations"] == 1001
    # a floor tilted by 30 degrees: enough inliers, refused by the verticality check
    xy = rng.uniform(-20, 20, (5000, 2))
    tilt = cloud(np.column_stack([xy, np.tan(np.radians(30.0)) * xy[:, 0] + rng.normal(0, 0.02, 5000)]))
    res = det.detect_host(tilt, prm)
    out, _ = _check_ransac(det, tilt, prm, res)
    assert not res["found"] and res["n_inliers"] > 4000 and abs(out["win"][2]) < np.cos(np.radians(10.0))
    # the upward flip: the sign of a draw's normal follows the order of its three points; both signs occur over a few seeds
    signs = set()
    flat_cloud = cloud(flat)
    for seed in range(8):
        prm = _plain(det, seed=seed)
        res = det.detect_host(flat_cloud, prm)
        out, _ = _check_ransac(det, flat_cloud, prm, res)
        assert res["found"] and res["coeffs"][2] > 0.99
        signs.add(bool(out["win"][2] < 0))
        if out["win"][2] < 0:
            assert np.array_equal(_bits(res["coeffs"]), _bits(-out["win"]))
    assert signs == {True, False}
    # an inverted cloud (the floor above the sensor, seen from below) is a floor too once the normal is made upward
    up = cloud(np.column_stack([flat[:, :2], 1.2 - flat[:, 2]]))
    prm = det.params(0, use_normal_filter=0, seed=3)
    res = det.detect_host(up, prm)
    _check_ransac(det, up, prm, res)
    assert res["found"] and res["coeffs"][2] > 0.99 and abs(res["coeffs"][3] + 1.2) < 0.05
    # what the entry points refuse
    with pytest.raises(capi.LioError, match="k = 5"):
        det.detect_host(up, det.params(0, k=5))
    det.close()


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def test_detect_scan_replace_then_append(scene_pts):
    _need_gpu()
    from lsd_amd import lio

    pts = scene_pts
    det, sc, cl = lio.GroundDetector(), lio.Scan(max_raw=1 << 17, max_ds=1 << 10), lio.Cloud()
    prm = det.params(0, seed=4)
    sc.upload(pts)
    res = det.detect_scan(sc, prm, replace=False)
    assert res["found"] and _same(sc.download_raw(), pts)  # replace = 0 leaves the scan alone
    out, _ = _check_ransac(det, pts, prm, res)
    res = det.detect_scan(sc, prm, replace=True)
    assert res["found"] and _same(sc.download_raw(), pts[out["inliers"]])
    T = np.eye(4)
    a = np.radians(25.0)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = [10.5, -3.25, 0.75]
    cl.append_scan(sc, T)
    assert _same(cl.download(), lio.transform_cloud_f64(pts[out["inliers"]], T))
    # no floor: the scan stays as it is even with replace
    high = pts.copy()
    high[:, 2] += 10.0
    sc.upload(high)
    res = det.detect_scan(sc, prm, replace=True)
    assert not res["found"] and res["n_clipped"] < 1024 and _same(sc.download_raw(), high)
    for h in (det, sc, cl):
        h.close()


def _read_pcd(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"DATA binary\n", 1)
    n = int([ln for ln in head.decode().splitlines() if ln.startswith("POINTS")][0].split()[1])
    return np.frombuffer(body, np.float32).reshape(n, 4).copy()


def _frames(scene_pts):
    """three frames of a short drive: (points, points_attr, TUM rows); the middle one is lifted out of the clip and has no floor"""
    rng = np.random.default_rng(31)
    out = []
    for f in range(3):
        pts = scene_pts[np.isfinite(scene_pts).all(1)][rng.permutation(90_000)[:80_000]].copy()
        if f == 1:
            pts[:, 2] += 10.0
        n = len(pts)
        attr = np.stack([np.sort(rng.integers(0, 100_000, n)).astype(np.float32), np.zeros(n, np.float32)], 1)
        header = 1_700_000_000_000_000 + 100_000 * f
        rows = []
        for k in range(5):
            yaw = np.radians(2.0 * f + 0.2 * k)
            rows.append([header + 25_000 * k, 1.0 * f + 0.02 * k, 0.3 + 0.005 * k, 0.01 * k, 0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)])
        out.append((pts, {"points_attr": attr, "timestamp": header}, np.array(rows, np.float64)))
    return out


def test_accumulate_cloud_with_ground_extraction(ground_switch, scene_pts, tmp_path):
    """graph_utils.cpp:420-429 with extract_ground: undistort, detect_ground in the sensor frame, nothing appended when there is no floor,
    else the inliers moved by odometrys[0].T -- against the composition of the pieces (lio.Scan.undistort_poses, lio.GroundDetector with
    the same seed, the f64 transform), whose parts the tests above hold to the restatement"""
    _need_gpu()
    from lsd_amd import lio

    sw = ground_switch
    frames = _frames(scene_pts)
    with pytest.raises(ValueError, match="extract_ground"):  # off: the old refusal
        sw.accumulate_cloud(frames[0][0], frames[0][1], frames[0][2], "TUM", True)
    det, sc = lio.GroundDetector(), lio.Scan(max_raw=1 << 17, max_ds=1 << 10)
    want, founds = [], []
    for pts, pa, rows in frames:
        T0, rel = sw._tum_relative_poses(rows)
        sc.upload(pts)
        sc.undistort_poses(pa["points_attr"][:, 0].astype(np.uint32), pa["timestamp"], rows[:, 0].astype(np.uint64), np.stack([np.asarray(r) for r in rel]).reshape(-1, 16))
        und = sc.download_raw()
        prm = det.params(0, seed=9)
        res = det.detect_scan(sc, prm, replace=True)
        founds.append(res["found"])
        if res["found"]:
            out, _ = _check_ransac(det, und, prm, res)
            want.append(lio.transform_cloud_f64(und[out["inliers"]], np.asarray(T0)))
    assert founds == [True, False, True]

    def run(path):
        sw.set_ground_extraction(True, 9)
        for pts, pa, rows in frames:
            sw.accumulate_cloud(pts, pa, rows, "TUM", True)
        sw.save_accumulate_cloud(str(path), 0.0)
        return _read_pcd(path)

    got = run(tmp_path / "ground.pcd")
    assert len(got) > 2 * 1024 and _same(got, np.concatenate(want))
    assert _same(run(tmp_path / "again.pcd"), got)  # the same seed: bit-identical
    sw.set_ground_extraction(False)
    with pytest.raises(ValueError, match="extract_ground"):
        sw.accumulate_cloud(frames[0][0], frames[0][1], frames[0][2], "TUM", True)
    f = tmp_path / "none.pcd"
    sw.save_accumulate_cloud(str(f), 0.0)
    assert not f.exists()  # the refused call accumulated nothing
    det.close()
    sc.close()


def test_full_size_ring_scan_through_detect_ground():
    """a full-size ring-structured sweep (64 x 1875 = 120 000 rays): ring neighbourhoods are ill-conditioned, so only properties are held"""
    _need_gpu()
    from lsd_amd import synth

    sw = _module()
    scn = synth.Scene(half=60.0, n_boxes=20, seed=3)
    raw, _ = synth.make_scan(scn, np.array([0.5, 1.0, 1.2]), synth.quat_from_rotvec([0, 0, 0.2]), seed=5, n_az=1875)
    pts = raw[:, :4].astype(np.float32)
    assert len(pts) > 100_000  # 64 x 1875 = 120 000 rays; the ones that hit nothing within range are not in the scan
    coeffs, inl = sw._detect_ground(pts, 0, 2)
    assert coeffs is not None and coeffs.dtype == np.float32 and coeffs[2] > np.cos(np.radians(10.0))
    assert len(inl) >= 1024 and gc.residual_ok(inl[:, :3], coeffs).all()  # (the flip negates all four: the `<` test is the same)
    assert abs(coeffs[3] - 1.2) < 0.05
    # the count is the restatement's for that plane over the filtered points; every inlier is a point of the input
    from lsd_amd import lio

    det = lio.GroundDetector()
    res = det.detect_host(pts, det.params(0, seed=2))
    fidx = det.indices(1).astype(np.int64)
    assert res["found"] and _same(res["coeffs"], coeffs) and _same(det.inliers(), inl)
    assert int(gc.residual_ok(pts[fidx, :3], coeffs).sum()) == len(inl) == res["n_inliers"]
    f_us, r_us = det.last_times()
    print(f"120 000-point sweep: clipped {res['n_clipped']} filtered {res['n_filtered']} inliers {res['n_inliers']}; filter {f_us:.0f} us, RANSAC {r_us:.0f} us")
    det.close()
