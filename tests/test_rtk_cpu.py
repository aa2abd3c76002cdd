"""The GNSS side of mapping mode, the parts that need no device: the UTM projection against tests/golden/rtk.npz (the reference's own
UTMProjector), both computeRTKTransform forms, the RTK track and the graph's GNSS queue against the restatement of tests/rtk_cases.py, RTKM's
sensor list.  Bounds: projection |d| <= 1e-6 m forward (the evaluation is about 60 f64 operations on values up to 1e7 m, ulp 1.9e-9 m; another
compiler's libm can move it some tens of ulp; 20 x that, 100 x under the project's 1e-4 m), <= 1e-11 degrees inverse, <= 1e-12 degrees
convergence; poses 1e-9 m and 1e-12 rad (both sides f64 from the same statements)."""
import os
import re

import numpy as np
import pytest

import rtk_cases as R
from lsd_amd import capi, lio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "rtk.npz"))
CODE = {capi.RTK_INTERPOLATED: R.INTERPOLATED, capi.RTK_EXACT: R.EXACT, capi.RTK_NO_ORIGIN: R.NO_ORIGIN, capi.RTK_TOO_FEW: R.TOO_FEW, capi.RTK_EARLY: R.EARLY,
        capi.RTK_LATE: R.LATE}


def rot_angle(A, B):
    c = (np.trace(A[:3, :3].T @ B[:3, :3]) - 1.0) / 2.0
    s = np.linalg.norm(A[:3, :3].T @ B[:3, :3] - (A[:3, :3].T @ B[:3, :3]).T) / (2.0 * np.sqrt(2.0))  # |sin| from the skew part: exact near 0
    return float(np.arctan2(s, c))


def assert_pose(A, B, what=""):
    assert np.abs(A[:3, 3] - B[:3, 3]).max() <= 1e-9 and rot_angle(A, B) <= 1e-12, (what, np.abs(A[:3, 3] - B[:3, 3]).max(), rot_angle(A, B))
    assert np.array_equal(A[3], [0, 0, 0, 1])


def test_abi_revision_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "lio_hip.h")).read()
    rev = int(re.search(r"#define LIO_ABI_VERSION (\d+)", hdr).group(1))
    assert rev >= 22 and capi.lib().lio_abi_version() == rev >= capi.ABI_VERSION == 22
    for s in ("lio_utm_forward", "lio_rtk_track_interpolate", "lio_gnss_queue_flush", "lio_scan_merge_run_host", "lio_interpolate_transform"):
        assert s in capi.SYMBOLS and hasattr(capi.lib(), s)


def _project(make_fresh, make_pinned):
    """the golden's six recordings through a pair of projector factories: forward fresh / pinned (x, y, zone, lon0, convergence), four inverses"""
    lat, lon, off = GOLDEN["lat"], GOLDEN["lon"], float(GOLDEN["pin_offset"])
    n = len(lat)
    fresh, pinned, inv = np.zeros((n, 5)), np.zeros((n, 5)), np.zeros((n, 4, 3))
    for k in range(n):
        la, lo = float(lat[k]), float(lon[k])
        p = make_fresh()
        fresh[k, :2] = p.forward(la, lo)
        fresh[k, 2:] = p.zone, p.longitude0(), p.convergence(la, lo)
        q = make_pinned(la, lo + off)
        pinned[k, :2] = q.forward(la, lo)
        pinned[k, 2:] = q.zone, q.longitude0(), q.convergence(la, lo)
        for j, (proj, src) in enumerate([(make_fresh(), fresh), (make_pinned(la, lo + off), pinned), (make_fresh(), pinned), (make_pinned(la, lo + off), fresh)]):
            inv[k, j, :2] = proj.inverse(src[k, 0], src[k, 1])
            inv[k, j, 2] = proj.zone
    return fresh, pinned, inv


class _LibProj:
    def __init__(self):
        self.u = lio.Utm()

    zone = property(lambda self: self.u.zone)
    forward = lambda self, la, lo: self.u.forward(la, lo)
    inverse = lambda self, x, y: self.u.inverse(x, y)
    longitude0 = lambda self: self.u.longitude0()
    convergence = lambda self, la, lo: lio.grid_convergence(self.u.longitude0(), la, lo)


class _RefProj(R.UtmRef):
    zone = property(lambda self: self.project_no)
    convergence = lambda self, la, lo: R.grid_convergence(self.longitude0(), la, lo)


def _pinned(cls):
    def make(la, lo):
        p = cls()
        p.forward(la, lo)
        return p
    return make


@pytest.mark.parametrize("side", ["library", "restatement"])
def test_projection_against_the_reference(side):
    cls = _LibProj if side == "library" else _RefProj
    fresh, pinned, inv = _project(cls, _pinned(cls))
    lat = GOLDEN["lat"]
    assert len(lat) >= 390 and lat.min() == -60 and lat.max() == 60 and (lat == 0).any() and (GOLDEN["lon"] < 0).any()
    worst = {}
    for name, got in (("fresh", fresh), ("pinned", pinned)):
        ref = GOLDEN[name]
        assert np.array_equal(got[:, 2], ref[:, 2]) and np.array_equal(got[:, 3], ref[:, 3]), name  # zone, longitude0: exact
        worst[name + " forward m"] = np.abs(got[:, :2] - ref[:, :2]).max()
        worst[name + " convergence deg"] = np.abs(got[:, 4] - ref[:, 4]).max()
    assert np.array_equal(inv[:, :, 2], GOLDEN["inverse"][:, :, 2])
    worst["inverse deg"] = np.abs(inv[:, :, :2] - GOLDEN["inverse"][:, :, :2]).max()
    print(side, {k: float(v) for k, v in worst.items()})
    assert worst["fresh forward m"] <= 1e-6 and worst["pinned forward m"] <= 1e-6
    assert worst["inverse deg"] <= 1e-11
    assert worst["fresh convergence deg"] <= 1e-12 and worst["pinned convergence deg"] <= 1e-12
    # what the golden must show for the quirks to be covered: a pinned zone that differs from the point's own, a zone west of Greenwich that
    # does not stick (the pinned projector answers like the fresh one there), a point on a central meridian
    ref_f, ref_p = GOLDEN["fresh"], GOLDEN["pinned"]
    east = GOLDEN["lon"] > 0
    assert (ref_f[east, 2] != ref_p[east, 2]).any() and np.array_equal(ref_f[~east, :2], ref_p[~east, :2]) and (ref_f[:, 2] < 0).any()
    assert (np.abs(ref_f[:, 0] - (1000000 * (ref_f[:, 2] + 1) * 0.9996 + 500000)) < 1e-6).any()  # false easting 1000000 (zone + 1) + 500000, scaled about 500000


def test_fresh_handle_and_bad_arguments():
    u = lio.Utm()
    assert u.zone == -1 and u.longitude0() == -1 * 6 + 3
    x, y = u.forward(31.0, 121.0)
    assert u.zone == 20 and u.longitude0() == 123.0 and 21e6 < x < 22e6
    assert u.forward(31.0, 127.5)[0] > x and u.zone == 20  # the zone sticks
    assert not capi.lib().lio_utm_create(0)
    L = capi.lib()
    assert L.lio_utm_forward(None, 0.0, 0.0, None, None) == capi.LIO_E_INVALID and L.lio_rtk_track_feed(None, 1, None) == capi.LIO_E_INVALID
    assert L.lio_gnss_queue_flush(None, None, None, 0, None, None, 0) == capi.LIO_E_INVALID and L.lio_rtk_track_interpolate(None, 0, None) == capi.LIO_E_INVALID


def test_rpyt_and_interpolation_against_the_restatement():
    rng = np.random.default_rng(5)
    for k in range(200):
        a = rng.uniform(-1, 1, 6) * [500, 500, 30, 180, 89, 89]
        b = a + rng.uniform(-1, 1, 6) * [3, 3, 0.5, 20, 5, 5] * (0 if k % 50 == 0 else 1)  # (every 50th: no motion at all -> the kEpsilon branch)
        A, B = lio.transform_from_rpyt(*a), lio.transform_from_rpyt(*b)
        assert_pose(A, R.transform_from_rpyt(*a), "rpyt")
        r = float(rng.uniform(0, 1))
        assert_pose(lio.interpolate_transform(A, B, r), R.interpolate_transform(A, B, r), "interpolate")
    assert_pose(lio.interpolate_transform(A, B, 0.0), A)
    assert_pose(lio.interpolate_transform(A, B, 1.0), B)


def test_both_rtk_transform_forms_against_the_restatement():
    for seed in range(200):
        fixes = R.seeded_fixes(seed, n=4)
        u, v = lio.Utm(), R.UtmRef()
        zero = np.array(R.UtmRef().forward(fixes[0]["latitude"], fixes[0]["longitude"]) + (fixes[0]["altitude"],))
        for f in fixes:
            assert_pose(u.rtk_transform_utm(f, zero), R.rtk_transform_utm(v, f, zero), "zero_utm form")
        u, v = lio.Utm(), R.UtmRef()
        for f in fixes:
            assert_pose(u.rtk_transform_origin(fixes[0], f), R.rtk_transform_origin(v, fixes[0], f), "origin form")
    # the origin's own pose sits at the origin with the heading less the convergence; the two forms agree when zero_utm is the origin's projection
    f0 = fixes[0]
    T = lio.Utm().rtk_transform_origin(f0, f0)
    assert np.array_equal(T[:3, 3], [0, 0, 0])
    assert_pose(T, lio.Utm().rtk_transform_utm(f0, zero))


def _tracks(seed):
    fixes = R.seeded_fixes(seed)
    a, b = lio.RtkTrack(), R.TrackRef()
    return fixes, a, b


def _same_answer(a, b, stamp, expect=None):
    code, T = a.interpolate(stamp)
    rcode, RT = b.interpolate(stamp)
    assert CODE[code] == rcode and (expect is None or rcode == expect), (CODE[code], rcode, expect)
    assert (T is None) == (RT is None)
    if T is not None:
        assert_pose(T, RT, rcode)
    return rcode


def test_track_against_the_restatement():
    seen = set()
    for seed in range(200):
        fixes, a, b = _tracks(seed)
        rng = np.random.default_rng(9000 + seed)
        assert a.feed(fixes[0]) is False and b.feed(fixes[0]) is False  # dropped: no origin yet
        took, T0 = a.set_origin(fixes[0])
        rtook, RT0 = b.set_origin(fixes[0])
        assert took and rtook
        assert_pose(T0, RT0, "origin")
        assert a.set_origin(fixes[1]) == (False, None)  # the first one wins
        for f in fixes:
            valid = rng.random() > 0.1
            assert a.feed(f, valid) == b.feed(f, valid) == valid
        assert len(a) == len(b.data)
        lo, hi = fixes[0]["stamp_us"], fixes[-1]["stamp_us"]
        for stamp in list(rng.integers(lo - 100000, hi + 100000, 12)) + [f["stamp_us"] for f in fixes[:3]]:
            seen.add(_same_answer(a, b, int(stamp)))
    assert {R.INTERPOLATED, R.EXACT, R.EARLY, R.LATE} <= seen


def test_track_refusals_exact_hit_and_last_fix():
    fixes = R.seeded_fixes(77, n=6, jitter=False)
    a, b = lio.RtkTrack(), R.TrackRef()
    mid = fixes[2]["stamp_us"] + 12345
    _same_answer(a, b, mid, R.NO_ORIGIN)                                   # 1. no origin
    a.set_origin(fixes[0]), b.set_origin(fixes[0])
    _same_answer(a, b, mid, R.TOO_FEW)                                     # 2. fewer than two fixes: none ...
    a.feed(fixes[1]), b.feed(fixes[1])
    _same_answer(a, b, mid, R.TOO_FEW)                                     #    ... and one
    _same_answer(a, b, fixes[1]["stamp_us"], R.EXACT)                      # the exact hit answers before the count is looked at
    for f in fixes[2:]:
        a.feed(f), b.feed(f)
    _same_answer(a, b, fixes[1]["stamp_us"] - 1, R.EARLY)                  # 3. before the first fix
    _same_answer(a, b, fixes[-1]["stamp_us"] + 1, R.LATE)                  # 4. after the last
    _same_answer(a, b, fixes[-1]["stamp_us"], R.EXACT)                     # a stamp on the last fix
    _same_answer(a, b, fixes[-1]["stamp_us"] - 1, R.INTERPOLATED)
    code, T = a.interpolate(mid)
    assert code == capi.RTK_INTERPOLATED
    # the ratio has no + 1: halfway between two fixes is the half-way pose
    half = (fixes[2]["stamp_us"] + fixes[3]["stamp_us"]) // 2
    P, N = a.interpolate(fixes[2]["stamp_us"])[1], a.interpolate(fixes[3]["stamp_us"])[1]
    assert_pose(a.interpolate(half)[1], R.interpolate_transform(P, N, 0.5))
    # a fix with a stamp already held replaces it
    moved = dict(fixes[3], altitude=fixes[3]["altitude"] + 5.0)
    a.feed(moved), b.feed(moved)
    assert len(a) == 5 and abs(a.interpolate(fixes[3]["stamp_us"])[1][2, 3] - N[2, 3] - 5.0) < 1e-9


def _run_queue(origin, fixes, kf, has, z, last=None):
    a, b = lio.GnssQueue(), R.GnssQueueRef()
    if last is not None:
        a.last_xyz[:] = last
        b.last_xyz = np.array(last, float)
    za, zb = a.set_origin(origin, z), b.set_origin(origin, z)
    assert np.abs(za - zb).max() <= 1e-9
    for f in fixes:
        a.push(f), b.push(f)
    ha, hb = has.copy(), has.copy()
    ma, mb = a.flush(kf, ha), b.flush(kf, hb)
    assert [(m["keyframe"], m["first"], m["second"], m["dimension"], m["precision"]) for m in ma] == \
           [(m["keyframe"], m["first"], m["second"], m["dimension"], m["precision"]) for m in mb]
    for x, y in zip(ma, mb):
        assert np.abs(x["xyz"] - y["xyz"]).max() <= 1e-9
        assert min(np.abs(x["quat"] - y["quat"]).max(), np.abs(x["quat"] + y["quat"]).max()) <= 1e-12 and abs(np.linalg.norm(x["quat"]) - 1) < 1e-14
    assert np.array_equal(ha, hb) and np.array_equal(a.stamps(), b.stamps()) and len(a) == len(b.queue)
    assert np.abs(a.last_xyz - b.last_xyz).max() <= 1e-9
    return ma, ha, a, b


def test_gnss_queue_flush_against_the_restatement():
    n_matches = n_refused = 0
    for seed in range(300):
        origin, fixes, kf, has, z = R.seeded_queue(seed)
        m, h, a, _ = _run_queue(origin, fixes, kf, has, z)
        n_matches += len(m)
        n_refused += int((h == 0).sum())
    assert n_matches > 150 and n_refused > 150  # the seeded set exercises both outcomes


def _line(n, step_us, t0=1_000_000_000_000, dlat=2e-4, **kw):
    """n fixes northwards, about 22 m apart"""
    return [R.fix(t0 + k * step_us, 31.0 + k * dlat, 121.0, 10.0 + k, 45.0, **kw) for k in range(n)]


def test_gnss_queue_named_cases():
    f = _line(6, 1_000_000, precision=0.05, dimension=3)
    t0 = f[0]["stamp_us"]
    # a key frame before the first fix is passed over, the others take their pairs; the erase leaves the fixes after the last key frame
    kf = np.array([t0 - 10, t0 + 500_000, t0 + 2_250_000], np.uint64)
    m, h, a, b = _run_queue(f[0], f, kf, np.zeros(3, np.uint8), None)
    assert [x["keyframe"] for x in m] == [1, 2] and list(h) == [0, 1, 1]
    assert (m[0]["first"], m[0]["second"]) == (t0, t0 + 1_000_000) and (m[1]["first"], m[1]["second"]) == (t0 + 2_000_000, t0 + 3_000_000)
    assert list(a.stamps()) == [t0 + 3_000_000, t0 + 4_000_000, t0 + 5_000_000]
    # the ratio's denominator carries a + 1: halfway in time is a hair short of halfway in space
    half = R.interpolate_transform(R.rtk_transform_utm(b.proj, f[0], b.zero_utm), R.rtk_transform_utm(b.proj, f[1], b.zero_utm), 0.5)[:3, 3]
    assert 0 < np.linalg.norm(half - m[0]["xyz"]) < 1e-4
    # a bracket of exactly 2.0 s is refused (dt2 - dt < 2.0), one of 1.999999 s is taken
    for step, want in ((2_000_000, []), (1_999_999, [0])):
        g = _line(3, step, precision=0.05, dimension=3)
        m, h, a, _ = _run_queue(g[0], g, np.array([g[0]["stamp_us"] + 700_000], np.uint64), np.zeros(1, np.uint8), None)
        assert [x["keyframe"] for x in m] == want
    # unequal precisions pass the key frame over; the walk goes on to the next key frame
    g = _line(4, 1_000_000, dimension=3, precision=0.05)
    g[1]["precision"] = 150.0
    kf = np.array([t0 + 500_000, t0 + 2_500_000], np.uint64)
    m, h, _, _ = _run_queue(g[0], g, kf, np.zeros(2, np.uint8), None)
    assert [x["keyframe"] for x in m] == [1] and list(h) == [0, 1]
    # a fix inside the gate of the last accepted one (10 m at this precision) is refused, one outside is taken
    g = _line(4, 1_000_000, dlat=3e-5, precision=0.05, dimension=3)  # about 3.3 m apart
    kf = np.array([t0 + 500_000, t0 + 1_500_000, t0 + 2_900_000], np.uint64)
    m, h, _, _ = _run_queue(g[0], g, kf, np.zeros(3, np.uint8), None)
    assert [x["keyframe"] for x in m] == [0] and list(h) == [1, 0, 0]
    m, h, _, _ = _run_queue(g[0], g, kf, np.zeros(3, np.uint8), None, last=[500.0, 0.0, 0.0])
    assert [x["keyframe"] for x in m] == [0] and np.linalg.norm(m[0]["xyz"] - [500.0, 0, 0]) > 10
    for prec, thr in ((150.0, 20.0), (2000.0, 50.0)):
        g = _line(3, 1_000_000, dlat=1.35e-4, precision=prec, dimension=3)  # about 15 m apart: inside 20 and 50
        m, h, _, _ = _run_queue(g[0], g, np.array([t0 + 500_000, t0 + 1_500_000], np.uint64), np.zeros(2, np.uint8), None)
        assert [x["keyframe"] for x in m] == [0], (prec, thr)
    # dimension 2: z = 0 whatever the altitude says; dimension 3 keeps it (less the origin's, less the last key frame's z)
    for dim, z in ((2, None), (3, None), (3, 1.25)):
        g = _line(3, 1_000_000, precision=0.05, dimension=dim)
        m, _, _, _ = _run_queue(g[0], g, np.array([t0 + 1_500_000], np.uint64), np.zeros(1, np.uint8), z)
        assert len(m) == 1 and m[0]["dimension"] == dim
        assert m[0]["xyz"][2] == 0.0 if dim == 2 else abs(m[0]["xyz"][2] - (1.5 + (z or 0.0))) < 1e-5
    # a key frame that already has a fix keeps it
    g = _line(4, 1_000_000, precision=0.05, dimension=3)
    m, h, _, _ = _run_queue(g[0], g, np.array([t0 + 500_000, t0 + 2_500_000], np.uint64), np.array([1, 0], np.uint8), None)
    assert [x["keyframe"] for x in m] == [1]
    # nothing without key frames or without fixes: the queue stays as it is
    q = lio.GnssQueue()
    q.set_origin(g[0])
    for x in g:
        q.push(x)
    assert q.flush(np.zeros(0, np.uint64), np.zeros(0, np.uint8)) == [] and len(q) == 4
    # a key frame later than every fix ends the walk, and the erase takes the whole queue
    assert q.flush(np.array([t0 + 10_000_000], np.uint64), np.zeros(1, np.uint8)) == [] and len(q) == 0


def test_rtkm_sensor_list():
    import slam_wrapper as sw

    cases = [(["0-lidar", "RTK", "IMU", "1-lidar"], ["RTK", "IMU", "0-lidar", "1-lidar"]),
             (["0-lidar", "IMU"], ["IMU"]),                                   # no RTK: no lidar
             (["camera_front", "1-lidar", "RTK", "0-lidar"], ["RTK", "camera_front", "1-lidar", "0-lidar"]),  # camera names pass; the first n- name is the base
             (["RTK"], ["RTK"])]
    for given, want in cases:
        try:
            assert sw.init_slam("mapping", "", "RTKM", given, 0.5, 0.2, 10.0, 60.0) == want
        finally:
            sw.deinit_slam()
    with pytest.raises(RuntimeError):
        sw.init_slam("mapping", "", "NoSuchMethod", ["RTK"], 0.5, 0.2, 10.0, 60.0)


def test_wrapper_gnss_switch_is_off_by_default():
    import slam_wrapper as sw

    sw.init_slam("mapping", "", "FastLIO", ["RTK", "IMU", "0-lidar"], 0.5, 0.2, 10.0, 60.0)
    try:
        assert sw._gnss_state()["enabled"] is False
        sw._push_gnss(dict(timestamp=1_000_000, latitude=31.0, longitude=121.0, altitude=4.0, heading=90.0, pitch=0.0, roll=0.0, Status=1, Ve=0.0))
        st = sw._gnss_state()
        assert st["origin_set"] is False and st["queued"] == 0 and np.array_equal(sw.get_map_origin(), np.zeros((1, 7)))
    finally:
        sw.deinit_slam()
