"""The motion-compensation kernels of csrc/undistort.hip alone, at their branch edges: the IMU backward propagation through
lio_scan_undistort_imu (the launcher the engine runs, on caller-supplied poses), the pose-list kernels across tile borders, the
constant-velocity kernel at small sizes.  References and cases: tests/undistort_cases.py (nothing there calls the library).

IMU kernel, per point by its label:
  filtered    NaN pattern 0x7fc00000 in x y z, the intensity's bits kept
  untouched   the uploaded bits
  single pass |device - exact| <= ulp_f32(exact) / 2 + 8 E, exact = the long-double value, E = the oracle's own distance from it (measured
              on the CPU per case and printed).  The 8: the device's Taylor series / sincos and the host libm are each a few f64 ulp from the
              true value and sit behind the same dozen roundings; it was fixed before the device was run and is not tuned on its output.
  repeated    the flow reference's value, or within h f32 ulp of the point's largest coordinate, h = the passes it took
Where no sine is taken the whole cloud equals the flow reference bit for bit."""
import numpy as np
import pytest

import undistort_cases as UC

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scan():
    from lsd_amd import capi, lio

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    sc = lio.Scan(max_raw=1 << 15, max_ds=1 << 14)
    yield sc
    sc.close()


def run_imu(sc, c):
    sc.upload(c["pts"])
    sc.undistort_imu(c["stamp"], c["poses"], c["end_pos"], c["end_rot"], c["ril"], c["til"], blind=c["blind"], filter_num=c["filter_num"], undistort=c["undistort"])
    out = sc.download_raw()
    assert out.shape == c["pts"].shape
    return out


def check_imu(c, out, oracle):
    """every point of the case by its label; returns (E, worst (|device - exact| - ulp / 2) / E over the single-pass coordinates)"""
    w = UC.walk(c)
    lab = UC.labels(c, w)
    ob, ib = _bits(out), _bits(c["pts"])
    assert np.array_equal(ob[:, 3], ib[:, 3]), c["name"]  # intensities
    f = lab == UC.FILTERED
    assert np.all(ob[f, :3] == UC.NAN_BITS), c["name"]
    u = lab == UC.UNTOUCHED
    assert np.array_equal(ob[u], ib[u]), c["name"]
    E, ratio = UC.error_budget(c, w), 0.0
    sel = UC.single_pass(c, w)
    if len(sel):
        ex = UC.exact(c, sel, w)
        err = np.abs(out[sel, :3].astype(np.longdouble) - ex).astype(np.float64)
        half = UC.ulp_f32(ex.astype(np.float64)) / 2
        r = (err - half) / E
        ratio = float(r.max())
        bad = np.argwhere(err > half + 8 * E)
        th = UC.gyr_dt(c, w)
        msg = ["%s: point %d coordinate %d branch %s |gyr| dt %.9g: |device - exact| %.3e > %.3e" %
               (c["name"], sel[i], a, UC.LABELS[lab[sel[i]]], th[sel[i]], err[i, a], half[i, a] + 8 * E) for i, a in bad[:10]]
        assert len(bad) == 0, "\n".join(msg)
    if w["passes"] > 1:
        i = w["first"]
        fl = UC.flow(c, oracle, w, rows=[i])[i, :3]
        tol = w["passes"] * UC.ulp_f32(np.abs(fl).max())
        assert np.all(np.abs(out[i, :3].astype(np.float64) - fl.astype(np.float64)) <= tol), (c["name"], i, out[i, :3], fl, w["passes"])
    print("%-28s n %6d  E %.2e  worst ratio %+.3f  %s" % (c["name"], len(out), E, ratio, dict(zip(UC.LABELS, np.bincount(lab, minlength=6).tolist()))))
    return E, ratio


# ---------------------------------------------------------------------------------------------------------------- IMU kernel
def test_imu_no_rotation_is_bit_exact(scan, oracle_mod):
    """2 cases.  |gyr| of every tail is 0, exactly 1e-7 or a normal value below it: no sine is taken, every f64 operation is the oracle's, the
    whole cloud equals the flow reference as uint32 (NaN pattern and intensities included).  The twin case at nextafter(1e-7, 1) takes the
    trig path: held to the bound, which an identity rotation there would miss (|gyr| dt |p| reaches 8e-7 m at E of 1e-13).
    Measured worst ratio (|device - exact| - ulp / 2) / E, one run: still -34.8, still-above -10.9 (negative: no coordinate lay within E of
    its f32 rounding boundary on the far side)"""
    c = UC.case_still()
    out = run_imu(scan, c)
    fl = UC.flow(c, oracle_mod)
    assert np.array_equal(_bits(out), _bits(fl))
    check_imu(c, out, oracle_mod)
    c2 = UC.case_still(above=True)
    out2 = run_imu(scan, c2)
    check_imu(c2, out2, oracle_mod)
    # the threshold is where it is: one f64 step above it the cloud is NOT the identity-rotation cloud
    assert np.array_equal(_bits(c["pts"]), _bits(c2["pts"])) and (_bits(out2) != _bits(out)).any()


def test_imu_rotating_segments_within_the_error_budget(scan, oracle_mod):
    """1 case, 20000 points: |gyr| of 0.3, 2 and 4-8 rad/s, |gyr| dt over [0, 0.7], both sin_versin branches >= 1000 times, |gyr| dt = 0.5
    exactly and within 1e-6 on either side.  Every single-pass coordinate: |device - exact| <= ulp_f32(exact) / 2 + 8 E.
    Measured worst ratio (|device - exact| - ulp / 2) / E, one run: -9.7 (E = 3.9e-14 m)"""
    c = UC.case_rotating()
    cnt = np.bincount(UC.labels(c), minlength=6)
    assert cnt[UC.TAYLOR] >= 1000 and cnt[UC.LIBRARY] >= 1000  # the builder's promise (a CPU matter, checked here as well)
    out = run_imu(scan, c)
    check_imu(c, out, oracle_mod)


@pytest.mark.parametrize("variant", UC.REPEAT_VARIANTS)
def test_imu_repeated_point(scan, oracle_mod, variant):
    """9 cases: who the earliest kept point is (blind and decimated points take no part, a tie goes to the lowest index, the last partial
    workgroup of 65, index 0) and that every earlier segment compensates it again.  Measured worst ratios of the other points, one run: -754.7 ... -3.4 (tail_wg)"""
    c = UC.case_repeat(variant)
    who, passes = UC.REPEAT_EXPECT[variant]
    w = UC.walk(c)
    assert w["passes"] == passes and (who is None or w["first"] == who)
    out = run_imu(scan, c)
    check_imu(c, out, oracle_mod)
    if variant == "tie3":  # the other two of the tie are single-pass points: their one-pass value, not the repeated one
        for i in (1234, 2000):
            assert UC.labels(c, w)[i] == UC.TAYLOR and w["t_ms"][i] == w["t_ms"][700]
    if who is not None:  # the repeat changes the point: a kernel that skipped it would not pass by accident
        once = UC.restate64(c, np.array([who]), w).astype(np.float32)[0]
        assert np.abs(once - out[who, :3]).max() > 100 * UC.ulp_f32(np.abs(once).max())


@pytest.mark.parametrize("n,n_poses,kw", [(1, 5, {}), (255, 5, {}), (256, 5, {}), (257, 5, {}), (700, 2, {}), (700, 3, {}), (700, 127, {}), (700, 128, {}),
                                          (900, 6, dict(on_offset=True)), (300, 2, dict(on_offset=True)), (900, 6, dict(beyond=True))])
def test_imu_sizes_and_tables(scan, oracle_mod, n, n_poses, kw):
    """11 cases: 1 / 255 / 256 / 257 points, 2 / 3 / 127 / 128 poses (the LDS table full), stamps whose t IS a pose offset (the earlier
    segment's: strict >), stamps beyond the last pose.  Measured worst ratios, one run: -9472.7 ... -19.1"""
    c = UC.case_sizes(n, n_poses, **kw)
    out = run_imu(scan, c)
    check_imu(c, out, oracle_mod)
    if kw.get("on_offset"):
        w = UC.walk(c)
        k = min(n, 10)
        assert np.all(c["poses"][w["h"][:k] + 1, 0] == w["t"][:k])  # the point sits on its segment's END


@pytest.mark.parametrize("n_poses", [129, 1])
def test_imu_refuses_pose_tables_it_cannot_hold(scan, n_poses):
    from lsd_amd import capi

    rng = np.random.default_rng(9)
    c = UC.case_sizes(300, 4)
    poses = UC.make_poses(rng, np.arange(n_poses) * 0.001, [rng.uniform(-1, 1, 3) for _ in range(n_poses - 1)])
    scan.upload(c["pts"])
    with pytest.raises(capi.LioError):
        scan.undistort_imu(c["stamp"], poses, c["end_pos"], c["end_rot"], c["ril"], c["til"])
    assert np.array_equal(_bits(scan.download_raw()), _bits(c["pts"]))


@pytest.mark.parametrize("filter_num", [1, 2, 3, 7])
def test_imu_filters_only(scan, oracle_mod, filter_num):
    """undistort = 0: decimation and the blind radius, bit-exact; a point at r^2 == blind^2 is dropped, its nextafter neighbour kept"""
    c = UC.case_filters(filter_num)
    out = run_imu(scan, c)
    assert np.array_equal(_bits(out), _bits(UC.flow(c, oracle_mod)))
    e, ob = c["edge"], _bits(out)
    assert np.all(ob[e["on"], :3] == UC.NAN_BITS) and np.all(ob[e["inside"], :3] == UC.NAN_BITS)
    kept = e["outside"][e["outside"] % filter_num == 0]
    assert np.array_equal(ob[kept], _bits(c["pts"])[kept]) and (filter_num > 2 or len(kept))
    assert np.isnan(out[:, 0]).sum() == (~UC.walk(c)["keep"]).sum()


def test_imu_repeatable_and_read_by_the_downsample(scan, oracle_mod):
    c = UC.case_repeat("middle")
    a = run_imu(scan, c)
    b = run_imu(scan, c)
    assert np.array_equal(_bits(a), _bits(b))
    n_ds = scan.voxel_downsample(0.5)
    ds = oracle_mod.voxel_downsample(b[np.isfinite(b[:, 0])], 0.5)
    assert n_ds == len(ds) > 100
    got = scan.get_ds()  # the compensated cloud, not the uploaded one (which lies metres away)
    assert np.allclose(np.sort(got[:, 0]), np.sort(ds[:, 0]), atol=1e-3) and not np.allclose(np.sort(got[:, 0])[:2000], np.sort(c["pts"][:, 0])[:2000], atol=1e-2)


# ---------------------------------------------------------------------------------------------------------------- pose-list kernels
def run_poses(sc, c):
    sc.upload(c["pts"])
    sc.undistort_poses(c["stamp"], c["header"], c["pose_stamps"], c["pose_T"])
    return sc.download_raw(cap=len(c["pts"]))


@pytest.mark.parametrize("layout", UC.POSE_LAYOUTS)
@pytest.mark.parametrize("n", UC.POSE_SIZES)
def test_pose_list_pure_translation_is_bit_exact(scan, oracle_mod, n, layout):
    """identity rotations, power-of-two translations: oracle and device do the same f32 operations and no sine is taken, so a wrong
    segment for one point is a wrong bit pattern"""
    c = UC.pose_list_case(n, layout)
    ref = oracle_mod.undistort_poses(c["pts"], c["stamp"], c["header"], c["pose_stamps"], c["pose_T"])
    assert np.array_equal(_bits(run_poses(scan, c)), _bits(ref))
    assert (_bits(ref) != _bits(c["pts"])).any(axis=1).sum() > (100 if layout == "past_last_early" else n // 4)


@pytest.mark.parametrize("layout", UC.POSE_LAYOUTS_STRIDED)
def test_pose_list_more_than_256_tiles(oracle_mod, layout):
    """257 * 2048 + 3 points: the fold over the tiles before takes its strided second trip; the one late stamp sits in tile 1 (first trip)
    or in tile 256 (second trip) and everything after it is carried"""
    from lsd_amd import capi, lio

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    n = UC.POSE_SIZE_STRIDED
    c = UC.pose_list_case(n, layout)
    seg = UC.pose_list_segments(c)
    at = UC.POSE_TILE * (1 if layout == "late_at_tile1" else 256)
    assert seg[at - 1] < len(c["pose_stamps"]) - 1 and np.all(seg[at + 5:] == len(c["pose_stamps"]) - 1)
    ref = oracle_mod.undistort_poses(c["pts"], c["stamp"], c["header"], c["pose_stamps"], c["pose_T"])
    sc = lio.Scan(max_raw=n, max_ds=1024)
    try:
        assert np.array_equal(_bits(run_poses(sc, c)), _bits(ref))
    finally:
        sc.close()


@pytest.mark.parametrize("n_poses", [2, 63, 64, 65])
def test_pose_list_pose_counts(scan, oracle_mod, n_poses):
    from lsd_amd import capi

    for layout in ("sorted", "shuffled", "late_at_tile1"):
        c = UC.pose_list_case(4097, layout, n_poses=n_poses)
        if n_poses == 65:
            scan.upload(c["pts"])
            with pytest.raises(capi.LioError):
                scan.undistort_poses(c["stamp"], c["header"], c["pose_stamps"], c["pose_T"])
            continue
        ref = oracle_mod.undistort_poses(c["pts"], c["stamp"], c["header"], c["pose_stamps"], c["pose_T"])
        assert np.array_equal(_bits(run_poses(scan, c)), _bits(ref)), layout


def test_pose_list_rotating_across_three_tiles(scan, oracle_mod):
    """rotating poses, 3 * 2048 + 5 shuffled points with a stamp past the last pose in the third tile: what the walk never reaches is
    bit-equal, the rest within the bound of test_hip_undistort_poses (8 ulp of the point's largest coordinate, < 1 % differing)"""
    rng = np.random.default_rng(77)
    n_poses = 12
    _, T = UC.pose_list_translations(n_poses)
    T = T.reshape(n_poses, 4, 4).copy()
    for i in range(1, n_poses):
        T[i, :3, :3] = UC.quat_to_R(UC.rand_quat(rng, 0.02 * i))
        T[i, :3, 3] = rng.uniform(-0.3, 0.3, 3)
    c = UC.pose_list_case(3 * 2048 + 5, "shuffled", n_poses=n_poses, T=T.reshape(n_poses, 16))
    c["stamp"][2 * 2048 + 900] = (n_poses - 1) * 1000 + 50
    ref = oracle_mod.undistort_poses(c["pts"], c["stamp"], c["header"], c["pose_stamps"], c["pose_T"])
    out = run_poses(scan, c)
    never = UC.pose_list_segments(c) == n_poses
    assert never.sum() == 2048 + 5 - 900 and np.array_equal(_bits(out[never]), _bits(c["pts"][never]))
    assert np.array_equal(_bits(out[:, 3]), _bits(ref[:, 3]))
    d = np.abs(out[:, :3] - ref[:, :3])
    scale = np.maximum(np.abs(ref[:, :3]).max(axis=1, keepdims=True), 1e-3)
    assert (d / (scale * 2.0 ** -23)).max() <= 8.0 and (d > 0).mean() < 1e-2, ((d / (scale * 2.0 ** -23)).max(), (d > 0).mean())


# ---------------------------------------------------------------------------------------------------------------- constant velocity
def _delta(rotvec, t):
    D = np.eye(4, dtype=np.float32)
    a = np.linalg.norm(rotvec)
    if a > 0:
        q = np.r_[np.sin(a / 2) * np.asarray(rotvec) / a, np.cos(a / 2)]
        D[:3, :3] = UC.quat_to_R(q).astype(np.float32)
    D[:3, 3] = t
    return D


def test_delta_small_sizes(scan, oracle_mod):
    """n = 1, 255, 257.  Identity rotation: bit-exact against the oracle.  Rotations whose scaled norm falls on both sides of 1e-8 (a 1e-6 rad
    delta: stamps below 1 ms stay under it) and stamps up to twice the scan period: the bound of test_hip_undistort_delta"""
    rng = np.random.default_rng(8)
    worst, differing, total = 0.0, 0, 0
    for n in (1, 255, 257):
        pts = UC.cloud(rng, n, 2.0, 60.0)
        st = rng.integers(0, 200001, n).astype(np.uint32)
        st[: n // 3] = rng.integers(0, 1500, n // 3)
        st[-1] = 200000  # twice the period
        D = _delta(np.zeros(3), [0.4, -0.25, 0.0625])
        scan.upload(pts)
        scan.undistort_delta(st, D, 0.1)
        assert np.array_equal(_bits(scan.download_raw()), _bits(oracle_mod.undistort_delta(pts, st, D, 0.1))), n
        for rv in ([1e-6, 0, 0], [3e-7, -8e-7, 5e-7], [0.02, -0.03, 0.05], [0.0, 0.0, -0.4]):
            D = _delta(np.array(rv), rng.uniform(-0.5, 0.5, 3))
            ref = oracle_mod.undistort_delta(pts, st, D, 0.1)
            scan.upload(pts)
            scan.undistort_delta(st, D, 0.1)
            out = scan.download_raw()
            assert np.array_equal(_bits(out[:, 3]), _bits(ref[:, 3]))
            d = np.abs(out[:, :3] - ref[:, :3])
            scale = np.abs(ref[:, :3]).max(axis=1, keepdims=True)
            worst, differing, total = max(worst, float((d / (scale * 2.0 ** -23)).max())), differing + int((d > 0).sum()), total + d.size
            assert d.max() < 2e-5
    assert worst <= 8.0 and differing <= 1e-2 * total, (worst, differing, total)
