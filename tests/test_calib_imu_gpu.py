"""The device half of the lidar-IMU calibration (lio_calib_imu_lidar_pose / _add_frame): the odometry with its map in HBM against a twin
built here from the public entries with a host round trip per stage (tests/calib_imu_cases.py: Twin), against the map bookkeeping restated
over the oracle's pcl::VoxelGrid, and one frame pair against oracle/gicp.py's Vgicp.

Scans: 16 beams x 360 azimuths of a small scene (about 5 000 points), 8 frames 0.43 m and under 3 degrees apart, three of them key frames.
Poses, map and target are compared bit for bit: every stage is sequential IEEE arithmetic and the header promises the same bits from either
side.  The one allowance is the Vgicp pair (docs/kernels.md, "calib_imu"): on an MI355X the device's pose and the oracle's were EQUAL (0 m, 0 rad:
both deliver a Matrix4f's values, and the f64 difference between the two engines vanished in that rounding).  Ten times nothing is no
allowance, so the number format gives it: one f32 step per entry, where a last-bit tie may fall either way -- 2^-23 m for a translation
below 1 m, 2^-22 rad for a rotation whose entries move by at most 2^-24 each."""
import ctypes as C

import numpy as np
import pytest

import calib_imu_cases as CM
from lsd_amd import capi, lio

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY, E_STATE = -1, -2, -4
KEYS = (2, 4, 6)
ALLOW_VGICP_T, ALLOW_VGICP_R = 2.0 ** -23, 2.0 ** -22  # m, rad
I4 = np.eye(4)


@pytest.fixture(scope="module")
def drive():
    return CM.scan_drive(n_frames=8, n_az=360)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def pose_rc(c, pts):
    T = np.full((4, 4), 7.0)
    p = capi.f32(pts)
    return capi.lib().lio_calib_imu_lidar_pose(c.h, capi.ptr(p, C.c_float), len(p), 4, capi.ptr(T, C.c_double)), T


def frame_rc(c, stamp, pts, gT, dT):
    p, g, d = capi.f32(pts), capi.f64(gT), capi.f64(dT)
    return capi.lib().lio_calib_imu_add_frame(c.h, stamp, capi.ptr(p, C.c_float), len(p), 4, capi.ptr(g, C.c_double), capi.ptr(d, C.c_double))


def state(c):
    return c.counts(), c.map_download(), c.target_download()


def same_state(a, b):
    return a[0] == b[0] and same(a[1], b[1]) and same(a[2], b[2])


@pytest.fixture(scope="module")
def run(drive):
    """the whole drive once through the product, the twin and the bookkeeping; what each test needs is kept"""
    c, tw, book = lio.ImuCalib(0, 1 << 13, 1 << 16), CM.Twin(), CM.MapBook()
    rec = dict(poses=[], twin=[], maps=[], targets=[], want_maps=[], want_targets=[], times=[], counts=[])
    prev = I4
    for i, (pts, _) in enumerate(drive):
        T, Tt = c.lidar_pose(pts), tw.lidar_pose(pts)
        rec["poses"].append(T)
        rec["twin"].append(Tt)
        rec["times"].append(c.last_times())
        if i == 0:
            book.first(pts)
            rec["first"] = (c.counts(), c.map_download(), c.target_download())
        if i in KEYS:
            c.add_frame(1_000_000 + 100_000 * i, T, np.linalg.inv(prev) @ T, pts)
            tw.add_frame(pts, Tt)
            book.key_frame(pts, T)
            prev = T
            rec["maps"].append(c.map_download())
            rec["targets"].append(c.target_download())
            rec["want_maps"].append(book.map())
            rec["want_targets"].append(book.target())
            rec["twin_targets"] = rec.get("twin_targets", []) + [tw.target.copy()]
            rec["counts"].append(c.counts())
            rec["map_time"] = c.last_times()["map_update_us"]
    rec["c"], rec["tw"] = c, tw
    return rec


def test_first_call(run, drive):
    counts, m, t = run["first"]
    n = len(drive[0][0])
    assert same(run["poses"][0], I4)
    assert counts["map_points"] == counts["target_points"] == n and counts["no_rtk"] and counts["frames"] == 0
    assert same(m, drive[0][0])  # the RAW scan, in input order
    assert same(CM.sorted_rows(t), CM.sorted_rows(drive[0][0]))  # the target holds the raw scan's points (the matcher's internal order)


def test_every_pose_equals_the_twin(run, drive):
    for i in range(1, len(drive)):
        T, Tt = run["poses"][i], run["twin"][i]
        d = float(np.abs(T - Tt).max())
        print(f"frame {i}: largest element difference to the twin {d:.3e}; to the true pose "
              f"{np.linalg.norm(T[:3, 3] - (np.linalg.inv(drive[0][1]) @ drive[i][1])[:3, 3]):.3e} m")
        assert not same(T, I4), i  # it converged
        assert same(T, CM.f32_round(T))  # a Matrix4f's values
        assert same(T, Tt), i
    t = run["times"][3]
    assert t["stage_us"] > 0 and t["filter_us"] > 0 and t["align_us"] > 0 and run["map_time"] > 0


def test_map_and_target_after_each_key_frame(run):
    for k in range(len(KEYS)):
        m, t, wm, wt = run["maps"][k], run["targets"][k], run["want_maps"][k], run["want_targets"][k]
        assert run["counts"][k]["frames"] == k + 1 and run["counts"][k]["map_points"] == len(wm) and run["counts"][k]["target_points"] == len(wt)
        assert same(m, wm), k  # [raw scan 0; filter(T_k scan_k) ...], append order
        assert same(CM.sorted_rows(t), CM.sorted_rows(wt)), k  # the target as a set = filter(map)
        assert same(CM.sorted_rows(t), CM.sorted_rows(run["twin_targets"][k])), k
    assert len(run["maps"][0]) < len(run["maps"][1]) < len(run["maps"][2])


def test_one_pair_against_the_oracles_vgicp():
    import gicp as ogicp  # oracle/gicp.py (brute force)

    (p0, T0), (p1, T1) = CM.scan_drive(n_frames=2, n_az=96)
    assert 1200 < len(p0) < 1700
    c = lio.ImuCalib(0, 1 << 12, 1 << 13)
    c.lidar_pose(p0)
    T = c.lidar_pose(p1)
    o = ogicp.Vgicp()
    o.set_target(p0)
    o.set_source(CM.voxel_filter(p1))
    To, it, conv = o.align(I4)
    assert conv and not same(T, I4)
    To = To.astype(np.float64)
    dt = float(np.linalg.norm(T[:3, 3] - To[:3, 3]))
    dr = CM.rot_angle(T[:3, :3], To[:3, :3])
    print(f"vgicp pair: {len(p0)} / {len(p1)} points, {it + 1} iterations; translation difference {dt:.3e} m, angle {dr:.3e} rad")
    assert dt <= ALLOW_VGICP_T and dr <= ALLOW_VGICP_R


def test_non_convergence_keeps_the_last_pose(drive):
    c, tw = lio.ImuCalib(0, 1 << 13, 1 << 16), CM.Twin()
    for pts, _ in drive[:2]:
        T1, Tt1 = c.lidar_pose(pts), tw.lidar_pose(pts)
    far = CM.transform_f64(np.block([[CM.euler_R(0, 0, 20.0), np.array([[3.0], [0.0], [0.0]])], [np.zeros((1, 3)), np.ones((1, 1))]]), drive[2][0])
    c.set_max_iterations(1)
    assert same(c.lidar_pose(far), I4)  # not converged: I
    assert b"converge" in capi.lib().lio_last_warning()
    c.set_max_iterations(64)
    T3, Tt3 = c.lidar_pose(drive[2][0]), tw.lidar_pose(drive[2][0])  # from the OLD last pose
    assert same(T3, Tt3) and not same(T3, I4)


def test_empty_cloud_sets_only_the_flag():
    c = lio.ImuCalib(0, 64, 64)
    assert c.counts()["no_rtk"] is False
    assert same(c.lidar_pose(np.zeros((0, 4), np.float32)), I4)
    assert c.counts() == dict(frames=0, imus=0, aligned=0, map_points=0, target_points=0, no_rtk=True)
    # the flag is set and there is no map: the reference dereferences null
    assert frame_rc(c, 5, np.ones((30, 4), np.float32), I4, I4) == E_STATE and c.counts()["frames"] == 0


def test_refused_calls_leave_the_object_unchanged(drive):
    c = lio.ImuCalib(0, 6000, 12000)
    pts = drive[0][0]
    bad = pts.copy()
    bad[17, 1] = np.nan
    rc, T = pose_rc(c, bad)
    assert rc == E_INVALID and np.all(T == 7.0) and c.counts()["no_rtk"] is False and c.counts()["map_points"] == 0
    c.lidar_pose(pts)
    c.lidar_pose(drive[1][0])
    before = state(c)
    bad = drive[2][0].copy()
    bad[-1, 0] = np.inf
    assert pose_rc(c, bad)[0] == E_INVALID and same_state(state(c), before)
    assert frame_rc(c, 7, bad, I4, I4) == E_INVALID and same_state(state(c), before)
    big = np.tile(pts, (2, 1))[:6001]
    assert pose_rc(c, big)[0] == E_CAPACITY and frame_rc(c, 7, big, I4, I4) == E_CAPACITY and same_state(state(c), before)
    # the map's capacity: 12 000 points hold the raw scan and one filtered key frame, not a second one far away
    c.add_frame(8, I4, I4, drive[1][0])
    mid = state(c)
    away = np.eye(4)
    away[0, 3] = 500.0
    assert mid[0]["frames"] == 1
    rcs = [frame_rc(c, 9 + k, drive[2][0], away, I4) for k in range(3)]
    assert E_CAPACITY in rcs and all(r in (0, E_CAPACITY) for r in rcs)
    k = rcs.index(E_CAPACITY)
    after = state(c)
    assert after[0]["frames"] == 1 + k and after[0]["map_points"] <= 12000
    assert frame_rc(c, 20, drive[2][0], away, I4) == E_CAPACITY and same_state(state(c), after)
    T = c.lidar_pose(drive[2][0])  # and it still aligns
    assert not same(T, I4)


def test_rtk_path_leaves_the_map_alone(drive):
    c = lio.ImuCalib(0, 1 << 13, 1 << 14)
    c.add_frame(1, I4, I4, drive[0][0])  # no lidar_pose before: no flag, the frame alone (no device work)
    assert c.counts() == dict(frames=1, imus=0, aligned=0, map_points=0, target_points=0, no_rtk=False)
    assert len(c.map_download()) == 0 and len(c.target_download()) == 0


def test_tails():
    rng = np.random.default_rng(11)

    def cloud(n, spread=40.0):
        return np.concatenate([rng.uniform(-spread, spread, (n, 3)), rng.uniform(0, 255, (n, 1))], 1).astype(np.float32)

    # 20 points far apart survive the filter as 20: the matcher's minimum; 19 are refused as lio_gicp_set_source_device refuses them
    c = lio.ImuCalib(0, 4096, 8192)
    base = cloud(2049)  # one past the filter's tile of 2048
    c.lidar_pose(base)
    assert c.counts()["map_points"] == 2049
    assert len(CM.voxel_filter(base[:20])) == 20 and pose_rc(c, base[:20])[0] == 0
    before = state(c)
    rc, T = pose_rc(c, cloud(19))
    assert rc == E_INVALID and np.all(T == 7.0) and same_state(state(c), before)
    # a first scan of 19 points cannot be a target either
    c2 = lio.ImuCalib(0, 4096, 8192)
    assert pose_rc(c2, cloud(19))[0] == E_INVALID and c2.counts()["map_points"] == 0 and c2.counts()["no_rtk"] is False
    # a map of 2049 points + a key frame: the whole-map filter over a size that is no multiple of the tile
    key = cloud(2048, spread=20.0)
    c.add_frame(3, I4, I4, key)
    book = CM.MapBook()
    book.first(base)
    book.key_frame(key, I4)
    assert same(c.map_download(), book.map())
    assert same(CM.sorted_rows(c.target_download()), CM.sorted_rows(book.target()))
    # a map whose size is exactly one past a multiple of the tile when the whole-map filter runs
    c3 = lio.ImuCalib(0, 4096, 8192)
    first = cloud(2 * 2048 + 1 - 24, spread=60.0)
    c3.lidar_pose(first)
    key = cloud(24, spread=60.0)
    assert len(CM.voxel_filter(key)) == 24
    c3.add_frame(4, I4, I4, key)
    assert c3.counts()["map_points"] == 2 * 2048 + 1
    b3 = CM.MapBook()
    b3.first(first)
    b3.key_frame(key, I4)
    assert same(c3.map_download(), b3.map()) and same(CM.sorted_rows(c3.target_download()), CM.sorted_rows(b3.target()))
