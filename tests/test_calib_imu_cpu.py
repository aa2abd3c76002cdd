"""The lidar-IMU calibration, the parts that need no device: the ABI, the two outer surfaces against the reference's files, and every host
entry point (integrate, interpolate, time_align, solve, calibrate, the pose lists) against the numpy restatement of tests/calib_imu_cases.py.

Allowances (docs/kernels.md, "calib_imu"): the largest difference to the restatement measured over the cases below, times ten.
integrate is the same IEEE operations in the same order on both sides and is compared for equality.  interpolate and time_align go through
sin, cos and atan2 of two libraries: 2.22e-16 per quaternion element measured, ALLOW_Q = 2.3e-15.  solve and calibrate differ in method
(one-sided Jacobi here, LAPACK's SVD in the restatement): the rotation angle between the two answers was at most 9.5e-15 rad (8 pairs, and
the same 8 pairs twice), ALLOW_ANGLE = 9.5e-14.  The pose lists are products of up to 59 matrices, summed by BLAS in the restatement:
2.22e-15 per element measured, ALLOW_POSE = 2.3e-14.  Against the TRUE extrinsic the restatement itself is off by 3.7e-6 .. 6.3e-5 rad on
the noise-free cases (trapezoid integration at 200 Hz, interpolation between samples) and the product by the same figures; the product's
distance to the truth is held to 10 x ALLOW_ANGLE around the restatement's, there is no separate bound against truth."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import calib_imu_cases as CM
from lsd_amd import capi, lio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_WRAPPER = "/root/reference/sensor_driver/calibration/calib_wrapper.cpp"
REF_DRIVER = "/root/reference/sensor_driver/calibration/calib_driver.py"
NEW = ["lio_calib_imu_integrate", "lio_calib_imu_interpolate", "lio_calib_imu_time_align", "lio_calib_imu_solve", "lio_calib_imu_create",
       "lio_calib_imu_destroy", "lio_calib_imu_reset", "lio_calib_imu_add_imu", "lio_calib_imu_add_frame", "lio_calib_imu_lidar_pose",
       "lio_calib_imu_calibrate", "lio_calib_imu_lidar_poses", "lio_calib_imu_imu_poses", "lio_calib_imu_map_download",
       "lio_calib_imu_target_download", "lio_calib_imu_counts", "lio_calib_imu_last_times", "lio_calib_imu_set_max_iterations"]
ALLOW_ANGLE = 9.5e-14  # rad
ALLOW_Q = 2.3e-15      # per quaternion element (unit quaternions)
ALLOW_POSE = 2.3e-14   # per element of a 4 x 4 whose entries are below 2 in size
f64p, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
E_STATE, E_INVALID = -4, -1


def _p(a):
    return capi.ptr(a, C.c_double)


def p_integrate(t, g):
    t, g = capi.f64(t), capi.f64(np.asarray(g, np.float64).reshape(-1, 3))
    out = np.zeros((max(len(t), 1), 4))
    assert capi.lib().lio_calib_imu_integrate(_p(t), _p(g), len(t), _p(out)) == 0
    return out[:len(t)]


def p_interpolate(qs, qe, scale):
    out = np.zeros(4)
    assert capi.lib().lio_calib_imu_interpolate(_p(capi.f64(qs)), _p(capi.f64(qe)), float(scale), _p(out)) == 0
    return out


def p_time_align(it, irot, ft):
    it, irot, ft = capi.f64(it), capi.f64(irot), capi.f64(ft)
    out = np.zeros((max(len(ft), 1), 4))
    first, n = C.c_uint32(0), C.c_uint32(0)
    rc = capi.lib().lio_calib_imu_time_align(_p(it), _p(irot), len(it), _p(ft), len(ft), C.byref(first), C.byref(n), _p(out))
    assert rc == 0, rc
    return first.value, out[:n.value]


def p_solve(pairs):
    pairs = capi.f64(np.asarray(pairs, np.float64).reshape(-1, 8))
    out = np.zeros(4)
    assert capi.lib().lio_calib_imu_solve(_p(pairs), len(pairs), _p(out)) == 0
    return out


class Product:
    """lio.ImuCalib behind the restatement's method names"""

    def __init__(self):
        self.c = lio.ImuCalib(0, 1 << 10, 1 << 12)  # (no device is opened: no call below handles a cloud)

    def add_imu(self, rows):
        self.c.add_imu(rows)

    def add_frame(self, s, g, d):
        self.c.add_frame(s, g, d)

    def calibrate(self):
        return self.c.calibrate()

    def lidar_poses(self):
        return self.c.lidar_poses()

    def imu_poses(self):
        return self.c.imu_poses()


WORST = {}


def close(got, want, allow, what):
    """the largest element difference, printed and kept per kind before it is held against the allowance"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    d = float(np.abs(got - want).max()) if got.size else 0.0
    if d > WORST.get(what, -1.0):
        WORST[what] = d
        print(f"{what}: largest element difference so far {d:.3e}")
    return d <= allow


def both(case, n_calibrate=1):
    r, p = CM.Restated(), Product()
    return r, p, CM.run(r, case, n_calibrate), CM.run(p, case, n_calibrate)


def test_abi_revision_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "lio_hip.h")).read()
    rev = int(re.search(r"#define LIO_ABI_VERSION (\d+)", hdr).group(1))
    assert rev >= 27 and capi.lib().lio_abi_version() == rev
    assert " * 27 = lio_calib_imu_*" in hdr
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(capi.lib(), s) and s in hdr, s
        assert getattr(capi.lib(), s).argtypes is not None, s
    assert not capi.lib().lio_calib_imu_create(-1, 16, 16) and not capi.lib().lio_calib_imu_create(0, 0, 16)


def _module_block(text):
    return re.findall(r'm\.def\("(calib_imu_\w+)"[^;]*;', text), {
        name: re.findall(r'py::arg\("(\w+)"\)', stmt) for name, stmt in re.findall(r'm\.def\("(calib_imu_\w+)"([^;]*);', text)}


def test_module_surface_is_the_references():
    import calib_imu_ext as ext

    names = ["calib_imu_reset", "calib_imu_set_points", "calib_imu_set_imu", "calib_imu_calibrate", "calib_imu_get_lidar_poses",
             "calib_imu_get_imu_poses", "calib_imu_get_lidar_T_R"]
    assert sorted(n for n in dir(ext) if n.startswith("calib_imu_")) == sorted(names)
    assert not [n for n in dir(ext) if n.startswith("calib_ins_")]
    mine = open(os.path.join(ROOT, "lidar-slam-detection_amd", "csrc", "calib_imu_wrapper.cpp")).read()
    got_names, got_args = _module_block(mine)
    assert got_names == names
    for n in names:  # the argument names as pybind11 prints them
        for a in got_args[n]:
            assert f"{a}:" in getattr(ext, n).__doc__, (n, a)
    if not os.path.exists(REF_WRAPPER):
        pytest.skip("the reference tree is not mounted")
    ref_names, ref_args = _module_block(open(REF_WRAPPER).read())
    assert ref_names == got_names and ref_args == got_args


def test_calib_driver_holds_the_thirteen_names():
    from lsd_amd import calib_driver

    mine = sorted(n for n, f in vars(calib_driver).items() if inspect.isfunction(f) and not n.startswith("_"))
    assert len(mine) == 13 and sum(n.startswith("calib_ins_") for n in mine) == 6 and sum(n.startswith("calib_imu_") for n in mine) == 7
    if not os.path.exists(REF_DRIVER):
        pytest.skip("the reference tree is not mounted")
    ref = re.findall(r"^def (\w+)\(([^)]*)\)", open(REF_DRIVER).read(), re.M)
    assert sorted(n for n, _ in ref) == mine
    for n, args in ref:
        assert list(inspect.signature(getattr(calib_driver, n)).parameters) == [a.strip() for a in args.split(",") if a.strip()], n


def test_module_host_flow_without_a_device():
    """set_imu, set_points on the RTK path (no get_lidar_T_R before), calibrate and the pose lists never open the device"""
    from lsd_amd import calib_driver as drv
    import calib_imu_ext as ext

    case = CM.host_case()
    drv.calib_imu_reset()
    assert np.array_equal(drv.calib_imu_calibrate(), np.zeros((3, 3), np.float32))  # no IMU sample: zeros and a warning
    drv.calib_imu_add_imu(case["imu"])
    assert np.array_equal(drv.calib_imu_calibrate(), np.zeros((3, 3), np.float32))  # no frame
    pts = np.zeros((0, 4), np.float32)
    for s, g, d in case["frames"]:
        drv.calib_imu_add_points(pts, s, d.astype(np.float32), g.astype(np.float32))
    assert ext._counts()[:2] == (len(case["frames"]), len(case["imu"]))
    R = drv.calib_imu_calibrate()
    assert R.dtype == np.float32 and R.shape == (3, 3)
    r = CM.Restated()
    r.add_imu(case["imu"])
    for s, g, d in case["frames"]:
        r.add_frame(s, g.astype(np.float32), d.astype(np.float32))  # array2Eigen: the f32 values
    want = r.calibrate()
    assert np.abs(R - want.astype(np.float32)).max() <= 2.0 ** -23
    lp, ip = drv.calib_imu_get_lidar_poses(), drv.calib_imu_get_imu_poses()
    assert len(lp) == len(ip) == len(case["frames"]) - 1 and lp[0].dtype == np.float32 and lp[0].shape == (4, 4)
    assert np.abs(np.array(lp) - r.lidar_poses().astype(np.float32)).max() <= 2.0 ** -22
    drv.calib_imu_reset()
    assert ext._counts() == (0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("rate,n", [(200.0, 320), (97.0, 50), (200.0, 1), (200.0, 0)])
def test_integrate(rate, n):
    traj = CM.drive()
    rows = CM.imu_rows(traj, 0.4, 0.4 + n / rate - 1e-6 if n else 0.4, rate)
    assert len(rows) == n
    t, g = rows[:, 0] / 1e6, rows[:, 1:4] / 180.0 * np.pi
    got, want = p_integrate(t, g), CM.integrate(t, g)
    assert np.array_equal(got, want)
    if n > 100:
        assert abs(np.linalg.norm(want[-1]) - 1.0) > 1e-6  # the running product is NOT unit: the inverse divides by the squared norm


def test_interpolate_edges():
    rng = np.random.default_rng(5)
    for _ in range(50):
        qs, qe = rng.normal(size=4), rng.normal(size=4)  # not unit, as the integrated quaternions
        for scale in (0.0, 1e-300, 0.25, 1.0, np.nextafter(1.0, 2.0), 3.0, -0.5):
            got, want = p_interpolate(qs, qe, scale), CM.interpolate(qs, qe, scale)
            assert close(got, want, ALLOW_Q, "interpolate"), (qs, qe, scale)
            if scale == 0.0 or scale > 1.0:
                assert np.array_equal(got, CM.EYE_Q)  # the reference's answer there, whatever q_s is
    # a difference quaternion with w < 0: the axis is negated, the angle stays below pi
    qs = CM.EYE_Q
    qe = np.array([-np.cos(0.2), 0.0, 0.0, np.sin(0.2)])
    d = CM.q_normalized(CM.q_mul(CM.q_inv(qs), qe))
    assert d[0] < 0
    got = p_interpolate(qs, qe, 0.5)
    assert close(got, CM.interpolate(qs, qe, 0.5), ALLOW_Q, "interpolate")
    assert CM.rot_angle(CM.q_to_R(got), CM.euler_R(0, 0, np.degrees(-0.2))) < 1e-15  # half of the SHORT rotation (-0.4 rad about z)
    # equal attitudes (|v| = 0) and the largest-diagonal branch of Quaterniond(Matrix3d) (an angle near pi)
    assert close(p_interpolate(qs, qs, 0.5), CM.interpolate(qs, qs, 0.5), ALLOW_Q, "interpolate")
    for axis in np.eye(3):
        qe = np.concatenate([[np.cos(1.5)], np.sin(1.5) * axis])
        assert close(p_interpolate(qs, qe, 1.0), CM.interpolate(qs, qe, 1.0), ALLOW_Q, "interpolate")


def _align_inputs(case):
    it = case["imu"][:, 0] / 1e6
    rot = CM.integrate(it, case["imu"][:, 1:4] / 180.0 * np.pi)
    ft = np.array([f[0] for f in case["frames"]]) / 1e6
    return it, rot, ft


@pytest.mark.parametrize("name,kw,first,n_aligned", [
    ("covered", dict(), 0, 12),
    ("first frame on the first sample", dict(t0=0.4, offset_us=0), 0, 12),
    ("three frames before the first sample", dict(t0=0.15), 3, 9),
    ("the stream ends before the last two frames", dict(imu_t1=1.503), 0, 10),
    ("every frame before the stream", dict(t0=0.0, n_frames=3, dt_us=10000), 3, 0),
    ("one sample", dict(imu_t1=0.4049), 0, 0),
])
def test_time_align(name, kw, first, n_aligned):
    case = CM.host_case(**kw)
    it, rot, ft = _align_inputs(case)
    gf, gq = p_time_align(it, rot, ft)
    wf, wq = CM.time_align(it, rot, ft)
    assert (gf, len(gq)) == (wf, len(wq)) == (first, n_aligned), name
    assert close(gq, wq, ALLOW_Q, "time_align")
    if name.startswith("first frame"):
        assert np.array_equal(gq[0], CM.EYE_Q)  # scale == 0
    out = np.zeros((4, 4))
    n = C.c_uint32(0)
    assert capi.lib().lio_calib_imu_time_align(_p(it), _p(rot), 0, _p(ft), len(ft), C.byref(n), C.byref(n), _p(out)) == E_STATE


def test_time_align_keeps_the_iterator_across_frames():
    """two frames inside one IMU interval, then one a few intervals on: the stepped-back iterator is where the walk resumes"""
    it = np.arange(10) * 0.005
    rot = CM.integrate(it, np.tile([0.3, -0.2, 0.5], (10, 1)))
    ft = np.array([0.0061, 0.0062, 0.0063, 0.0301, 0.0451])
    gf, gq = p_time_align(it, rot, ft)
    wf, wq = CM.time_align(it, rot, ft)
    assert gf == wf == 0 and len(gq) == len(wq) == 4 and close(gq, wq, ALLOW_Q, "time_align")  # 0.0451 is past the last sample (0.045): left out


def _pairs_of(case):
    r = CM.Restated()
    CM.run(r, case)
    return r.pairs()


CASES = {
    "identity": dict(ext=(0.0, 0.0, 0.0)),
    "general": dict(ext=CM.GENERAL),
    "three before": dict(t0=0.15),
    "stream ends early": dict(imu_t1=1.503),
    "long": dict(n_frames=60, dt_us=50000, imu_t1=4.0),
}


def test_solve_against_the_restatement():
    worst = 0.0
    for name, kw in CASES.items():
        pairs = _pairs_of(CM.host_case(**kw))
        got, want = p_solve(pairs), CM.solve(pairs)
        assert abs(np.linalg.norm(got) - 1.0) < 1e-15
        a = CM.rot_angle(CM.q_to_R(CM.q_normalized(got)), CM.q_to_R(CM.q_normalized(want)))
        worst = max(worst, a)
        print(f"solve {name}: {len(pairs)} pairs, angle to the restatement {a:.3e}")
        assert a <= ALLOW_ANGLE, name
    print(f"solve: largest angle {worst:.3e}")
    assert np.array_equal(p_solve(np.zeros((0, 8))), CM.EYE_Q)


def test_solve_huber_branch():
    """one pair 10 degrees off: equal to the restatement, and different from the unweighted solve"""
    pairs = _pairs_of(CM.host_case())
    off = CM.q_from_R(CM.euler_R(0.0, 10.0, 0.0))
    pairs[4, :4] = CM.q_mul(pairs[4, :4], off)
    assert 180 / np.pi * CM.angular_distance(pairs[4, 4:], pairs[4, :4]) > 2.0
    got, want, plain = p_solve(pairs), CM.solve(pairs), CM.solve(pairs, weighted=False)
    Rg = CM.q_to_R(CM.q_normalized(got))
    a = CM.rot_angle(Rg, CM.q_to_R(CM.q_normalized(want)))
    b = CM.rot_angle(Rg, CM.q_to_R(CM.q_normalized(plain)))
    print(f"huber: angle to the restatement {a:.3e}, to the unweighted solve {b:.3e}")
    assert a <= ALLOW_ANGLE and b > 1e-4


@pytest.mark.parametrize("name", list(CASES))
def test_calibrate_and_poses(name):
    case = CM.host_case(**CASES[name])
    r, p, Rr, Rp = both(case)
    a = CM.rot_angle(Rp, Rr)
    truth = CM.rot_angle(Rr, case["R"])
    print(f"calibrate {name}: angle to the restatement {a:.3e}; the restatement to the truth {truth:.3e}, the product {CM.rot_angle(Rp, case['R']):.3e}")
    assert a <= ALLOW_ANGLE
    assert abs(CM.rot_angle(Rp, case["R"]) - truth) <= 10 * ALLOW_ANGLE  # recovery: held around the restatement
    assert truth < 2e-3  # (the case is a calibration at all: the restatement finds the extrinsic)
    n = len(r.aligned) - 1
    assert p.c.counts()["aligned"] == len(r.aligned) and p.c.counts()["frames"] == len(r.frames)
    lp, ip = p.lidar_poses(), p.imu_poses()
    assert len(lp) == len(ip) == n
    assert close(lp, r.lidar_poses(), ALLOW_POSE, "lidar_poses")
    d = np.abs(ip - r.imu_poses()).max()
    print(f"imu_poses {name}: largest element difference {d:.3e}")
    assert d <= ALLOW_POSE


def test_second_calibrate_appends_the_pairs_again():
    case = CM.host_case(t0=0.15)  # with erased frames: they stay erased, the kept ones are aligned twice
    r, p, Rr, Rp = both(case, n_calibrate=2)
    assert len(r.aligned) == 18 and p.c.counts()["aligned"] == 18 and p.c.counts()["frames"] == 9
    assert CM.rot_angle(Rp, Rr) <= ALLOW_ANGLE
    assert len(p.lidar_poses()) == 17 and close(p.lidar_poses(), r.lidar_poses(), ALLOW_POSE, "lidar_poses")
    assert np.abs(p.imu_poses() - r.imu_poses()).max() <= ALLOW_POSE
    p.c.reset()
    assert p.c.counts() == dict(frames=0, imus=0, aligned=0, map_points=0, target_points=0, no_rtk=False)


def test_frame_cap():
    case = CM.host_case(n_frames=205, dt_us=10000, imu_t1=3.0)
    r, p, Rr, Rp = both(case)
    assert p.c.counts()["frames"] == len(r.frames) == 200 and p.c.counts()["aligned"] == 200
    assert CM.rot_angle(Rp, Rr) <= ALLOW_ANGLE


def test_error_returns():
    L = capi.lib()
    c = lio.ImuCalib(0, 64, 64)
    R = np.full((3, 3), 7.0)
    assert L.lio_calib_imu_calibrate(c.h, _p(R)) == E_STATE and np.all(R == 7.0)  # no IMU sample
    case = CM.host_case(t0=0.0, n_frames=3, dt_us=10000)
    c.add_imu(case["imu"])
    assert L.lio_calib_imu_calibrate(c.h, _p(R)) == E_STATE  # no frame at all
    for s, g, d in case["frames"]:
        c.add_frame(s, g, d)
    assert L.lio_calib_imu_calibrate(c.h, _p(R)) == E_STATE and np.all(R == 7.0)  # every frame before the first sample: erased, none left
    assert c.counts()["frames"] == 0 and c.counts()["aligned"] == 0
    assert b"IMU" in L.lio_last_error()
    assert L.lio_calib_imu_calibrate(None, _p(R)) == E_INVALID and L.lio_calib_imu_calibrate(c.h, None) == E_INVALID
    assert L.lio_calib_imu_lidar_poses(c.h, None, 0) == 0 and L.lio_calib_imu_set_max_iterations(c.h, 0) == E_INVALID
    out = np.zeros(4)
    assert L.lio_calib_imu_solve(None, 1, _p(out)) == E_INVALID and L.lio_calib_imu_interpolate(None, _p(out), 0.5, _p(out)) == E_INVALID
    c2 = lio.ImuCalib(0, 64, 64)
    good = CM.host_case()
    c2.add_imu(good["imu"])
    for s, g, d in good["frames"]:
        c2.add_frame(s, g, d)
    c2.calibrate()
    small = np.zeros((2, 4, 4))
    assert L.lio_calib_imu_lidar_poses(c2.h, _p(small), 2) == -11 and L.lio_calib_imu_imu_poses(c2.h, _p(small), 2) == -11
