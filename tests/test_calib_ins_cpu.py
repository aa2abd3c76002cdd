"""The lidar-INS calibration, the parts that need no device: Scan's subsampling against the five-line restatement of its generator, the f32
Transform and the odometry interpolation against the f64 restatement (tests/calib_ins_cases.py), the two derivative-free minimisers on analytic
functions, the ABI, and the outer module's surface against the reference's PYBIND11_MODULE block.

Bounds.  SE3 and interpolation: |delta| <= 16 * 2^-23 * max(1, max|t|) per matrix entry, a handful of f32 roundings at the size of the
translations.  DIRECT-L after 500 evaluations on the global box must land inside the local stage's box around the minimiser (+-10 m, +-1 m,
+-1 rad): that is what the global stage owes the local one.  Nelder-Mead must reach f <= 1e-6 f(x0) within 500 evaluations on a separable
quadratic of condition number 100 in 7 dimensions (scipy's reaches 5e-12 there; the margin covers a restated variant)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import calib_ins_cases as CI
from lsd_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_WRAPPER = "/root/reference/sensor_driver/calibration/calib_wrapper.cpp"
NEW = ["lio_calib_subsample", "lio_se3f_exp", "lio_se3f_log", "lio_se3f_mul", "lio_se3f_inverse", "lio_se3f_matrix", "lio_se3f_from_matrix",
       "lio_calib_interpolate", "lio_dfo_default_params", "lio_dfo_direct_l", "lio_dfo_nelder_mead", "lio_calib_default_params",
       "lio_calib_ins_create", "lio_calib_ins_destroy", "lio_calib_ins_reset", "lio_calib_ins_add_scan", "lio_calib_ins_add_odom",
       "lio_calib_ins_counts", "lio_calib_ins_set_transform", "lio_calib_ins_scan_matrices", "lio_calib_ins_combined", "lio_calib_ins_error",
       "lio_calib_ins_error_terms", "lio_calib_ins_calibrate", "lio_calib_ins_progress", "lio_calib_ins_result", "lio_calib_ins_last_times"]
f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)


def test_abi_revision_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "lio_hip.h")).read()
    rev = int(re.search(r"#define LIO_ABI_VERSION (\d+)", hdr).group(1))
    assert rev >= 24 and capi.lib().lio_abi_version() == rev
    assert capi.ABI_VERSION == 22 and capi.ABI_REQUIRED == 23
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(capi.lib(), s) and s in hdr, s
        assert getattr(capi.lib(), s).argtypes is not None, s


def test_param_structs_match_the_header(tmp_path):
    import subprocess

    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lio_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(lio_dfo_params), sizeof(lio_dfo_report), sizeof(lio_calib_params), offsetof(lio_calib_params, nm_step), "
                   "offsetof(lio_dfo_params, step)); return 0; }\n")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(capi.DfoParams), C.sizeof(capi.DfoReport), C.sizeof(capi.CalibParams), capi.CalibParams.nm_step.offset, capi.DfoParams.step.offset]
    p = capi.CalibParams()
    capi.lib().lio_calib_default_params(C.byref(p))
    assert (p.local_only, p.time_cal, p.max_time_offset, p.max_evals, p.knn_batch_size, p.xtol) == (0, 1, 0.2, 500, 1000, 0.0001)
    assert (p.local_knn_k, p.global_knn_k, p.local_knn_max_dist, p.global_knn_max_dist) == (1, 3, 1.0, 10.0)
    assert not capi.lib().lio_calib_ins_create(-1)  # no such device: NULL, like every *_create


STAMPS = [0, 1, 2147483647, 3 * 2147483647, 1700000000123456, 1699999999999999]


@pytest.mark.parametrize("n", [0, 1, 5999, 6000, 6001, 50000])
def test_subsample_is_the_restated_generator(n):
    L = capi.lib()
    for stamp in STAMPS if n <= 6001 else STAMPS[3:5]:
        keep = np.zeros(max(n, 1), np.uint8)
        got = L.lio_calib_subsample(n, stamp, capi.ptr(keep, C.c_uint8))
        want = CI.keep_mask(n, stamp)
        assert got == int(want.sum()) and np.array_equal(keep[:n].astype(bool), want), (n, stamp)
    if n == 50000:
        assert 5500 < got < 6500  # about 6000 of 50 000
    if 0 < n <= 5999:
        assert got == n  # the ratio is 1 and every draw is below 1


def _T7(a):
    return capi.f32(a)


def _call7(name, *args, out=7):
    o = np.zeros(out, np.float32)
    getattr(capi.lib(), name)(*[capi.ptr(_T7(a), C.c_float) for a in args], capi.ptr(o, C.c_float))
    return o


def _tol(*Ts):
    return 16 * 2.0 ** -23 * max(1.0, max(float(np.abs(np.asarray(T)[:3]).max()) for T in Ts))


def _matrix_close(T_lib, T_ref64, tol):
    M = _call7("lio_se3f_matrix", T_lib, out=16).reshape(4, 4).astype(np.float64)
    assert np.abs(M - CI.se3_matrix(T_ref64)).max() <= tol, (M, CI.se3_matrix(T_ref64))


def _random_vecs():
    rng = np.random.default_rng(5)
    v = [np.concatenate([rng.uniform(-50, 50, 3), rng.normal(size=3)]) for _ in range(12)]
    v += [np.array([1.0, -2.0, 3.0, 0, 0, 0]), np.array([0.5, 0.5, 0.5, 5e-9, 0, 0]), np.array([0.5, 0.5, 0.5, 2e-8, 0, 0]),
          np.array([0, 0, 0, np.pi - 1e-3, 0, 0]), np.array([3.0, 1.0, 2.0, 0, 0, 4.0])]  # the last: half angle 2 rad, w < 0
    return v


def test_se3_functions_against_the_f64_restatement():
    vs = _random_vecs()
    Ts = []
    for v in vs:
        T = _call7("lio_se3f_exp", v[:6].astype(np.float32))
        T64 = CI.se3_exp(v.astype(np.float32).astype(np.float64))
        _matrix_close(T, T64, _tol(T64))
        # the f32 restatement follows the same statements: equal to a few ulp (libm's sinf / cosf may differ from numpy's in the last place)
        assert np.abs(T - CI.se3_exp(v, np.float32)).max() <= 4 * 2.0 ** -23 * max(1.0, np.abs(v[:3]).max())
        Ts.append((T, T64))
    for (a, a64), (b, b64) in zip(Ts, Ts[1:] + Ts[:1]):
        _matrix_close(_call7("lio_se3f_mul", a, b), CI.se3_mul(a64, b64), _tol(a64, b64, CI.se3_mul(a64, b64)))
        inv = _call7("lio_se3f_inverse", a)
        _matrix_close(inv, CI.se3_inverse(a64), _tol(a64))
        _matrix_close(_call7("lio_se3f_mul", a, inv), CI.se3_exp(np.zeros(6)), 2 * _tol(a64))
        back = _call7("lio_se3f_from_matrix", _call7("lio_se3f_matrix", a, out=16))
        _matrix_close(back, a64, _tol(a64))


def test_exp_log_round_trips_at_the_gate_near_pi_and_for_negative_w():
    for v in _random_vecs():
        T = _call7("lio_se3f_exp", v.astype(np.float32))
        lg = _call7("lio_se3f_log", T, out=6)
        T2 = _call7("lio_se3f_exp", lg)
        _matrix_close(T2, CI.se3_exp(v.astype(np.float32).astype(np.float64)), _tol(v))
        ang = np.linalg.norm(v[3:])
        if ang < 1e-8:
            assert np.array_equal(T[3:], [1, 0, 0, 0]) and np.array_equal(lg[3:], [0, 0, 0])  # below the gate: the identity rotation
        elif ang <= np.pi:
            assert np.abs(lg[3:] - v[3:]).max() <= 8 * 2.0 ** -23 * np.pi  # a few f32 roundings of an angle up to pi
    # w < 0: the angle comes from |w| and the axis is flipped -- the same rotation with an angle in [0, pi]
    T = _call7("lio_se3f_exp", np.array([0, 0, 0, 0, 0, 4.0], np.float32))
    assert T[3] < 0
    lg = _call7("lio_se3f_log", T, out=6)
    assert abs(lg[5] - (4.0 - 2 * np.pi)) < 1e-5 and lg[3] == 0 and lg[4] == 0
    z = _call7("lio_se3f_log", np.array([1, 2, 3, 1, 0, 0, 0], np.float32), out=6)
    assert np.array_equal(z, [1, 2, 3, 0, 0, 0])


def _track(m=6):
    rng = np.random.default_rng(9)
    stamps = np.array([1_700_000_000_000_000 + 10_000 * i + (i % 2) * 137 for i in range(m)], np.int64)
    T = np.stack([CI.se3_exp(np.concatenate([[3.0 * i, 0.4 * i * i, 0.1 * i], 0.05 * i * np.array([0.2, -0.1, 1.0]) + 0.01 * rng.normal(size=3)]))
                  for i in range(m)]).astype(np.float32)
    return stamps, T


def _interp(stamps, T, stamp, start=0):
    out, idx = np.zeros(7, np.float32), C.c_uint32(99)
    rc = capi.lib().lio_calib_interpolate(stamps.ctypes.data_as(C.POINTER(C.c_int64)), capi.ptr(T, C.c_float), len(stamps), int(stamp), start,
                                          capi.ptr(out, C.c_float), C.byref(idx))
    return rc, out, idx.value


@pytest.mark.parametrize("case", ["inside", "before", "after", "on_entry", "start_past", "two_entries"])
def test_interpolation_with_its_quirks(case):
    stamps, T = _track(2 if case == "two_entries" else 6)
    T64 = T.astype(np.float64)
    stamp, start = {"inside": lambda: (stamps[2] + 3333, 0), "before": lambda: (stamps[0] - 4000, 0), "after": lambda: (stamps[-1] + 6000, 0),
                    "on_entry": lambda: (stamps[3], 0), "start_past": lambda: (stamps[1] + 100, 4), "two_entries": lambda: (stamps[0] + 2500, 0)}[case]()
    rc, out, idx = _interp(stamps, T, stamp, start)
    want, widx = CI.interpolate(list(stamps), T64, int(stamp), start)
    assert rc == capi.LIO_OK and idx == widx
    _matrix_close(out, want, _tol(want, *T64))
    if case == "before":
        assert idx == 0  # ratio < 0: extrapolated backwards from the first pair
    if case == "after":
        assert idx == len(stamps) - 2  # ratio > 1
    if case == "on_entry":
        assert idx == 2  # stamp == entry 3: the search stops at 3 and steps back; ratio 1
    if case == "start_past":
        assert idx == 3  # the search cannot go back: the pair (3, 4) extrapolates to a stamp between 1 and 2


def test_interpolation_needs_two_entries():
    stamps, T = _track(2)
    assert _interp(stamps[:1], T[:1], stamps[0])[0] == capi.LIO_E_STATE


# ---- the optimisers ---------------------------------------------------------------------------------------------------------------------------
GLOBAL_LB = np.array([-100.0, -100.0, -10.0, -np.pi, -np.pi, -np.pi])
GLOBAL_UB = -GLOBAL_LB


class Counted:
    def __init__(self, f, lb, ub, budget):
        self.f, self.lb, self.ub, self.budget, self.xs, self.fs, self.hooked = f, np.asarray(lb), np.asarray(ub), budget, [], [], 0
        self.cb = capi.DFO_FN(self._call)
        self.hook = capi.DFO_HOOK(self._hook)

    def _call(self, x, n, _):
        v = np.array([x[i] for i in range(n)])
        assert np.all(v >= self.lb) and np.all(v <= self.ub), v  # never outside the box
        self.xs.append(v)
        assert len(self.xs) <= self.budget  # never beyond the budget
        self.fs.append(float(self.f(v)))
        return self.fs[-1]

    def _hook(self, evals, x, n, f, _):
        self.hooked += 1
        assert evals == len(self.xs) and f == self.fs[-1]
        return 0


def _run(method, fn, lb, ub, x0=None, max_evals=500, steps=None):
    L = capi.lib()
    p, rep = capi.DfoParams(), capi.DfoReport()
    L.lio_dfo_default_params(C.byref(p))
    assert (p.max_evals, p.xtol_abs, p.epsilon) == (500, 1e-4, 1e-4)
    p.max_evals = max_evals
    for i, s in enumerate(steps or []):
        p.step[i] = s
    lb, ub, out = capi.f64(lb), capi.f64(ub), np.zeros(len(lb))
    c = Counted(fn, lb, ub, max_evals)
    if method == "direct":
        rc = L.lio_dfo_direct_l(c.cb, None, len(lb), capi.ptr(lb, C.c_double), capi.ptr(ub, C.c_double), C.byref(p), c.hook, None, capi.ptr(out, C.c_double), C.byref(rep))
    else:
        rc = L.lio_dfo_nelder_mead(c.cb, None, len(lb), capi.ptr(capi.f64(x0), C.c_double), capi.ptr(lb, C.c_double), capi.ptr(ub, C.c_double), C.byref(p),
                                   c.hook, None, capi.ptr(out, C.c_double), C.byref(rep))
    assert rc == capi.LIO_OK and rep.evals == len(c.xs) == c.hooked <= max_evals
    assert rep.f_best == min(c.fs) and np.array_equal(out, c.xs[int(np.argmin(c.fs))])
    return c, out, rep


XMIN = np.array([4.0, -3.0, 1.5, 0.3, -0.2, 0.5])  # a few metres off-centre


def _bowl(x):
    return float((((x - XMIN) / (GLOBAL_UB - GLOBAL_LB)) ** 2).sum())


def test_direct_l_starts_at_the_centre_and_samples_a_third_of_the_side():
    c, _, _ = _run("direct", _bowl, GLOBAL_LB, GLOBAL_UB, max_evals=40)
    centre, side = (GLOBAL_LB + GLOBAL_UB) / 2, GLOBAL_UB - GLOBAL_LB
    assert np.array_equal(c.xs[0], centre)
    for i in range(6):
        e = np.zeros(6)
        e[i] = side[i] / 3
        assert np.allclose(c.xs[1 + 2 * i], centre + e, rtol=0, atol=1e-12) and np.allclose(c.xs[2 + 2 * i], centre - e, rtol=0, atol=1e-12)


def test_direct_l_hands_the_local_stage_its_box():
    c, best, rep = _run("direct", _bowl, GLOBAL_LB, GLOBAL_UB)
    d = np.abs(best - XMIN)
    print("DIRECT-L: evals", rep.evals, "best", best, "|best - minimiser|", d)
    assert rep.evals <= 500 and np.all(d < [10.0, 10.0, 1.0, 1.0, 1.0, 1.0])


def test_direct_l_stops_on_a_hook_and_on_a_tiny_budget():
    L = capi.lib()
    p, rep, out = capi.DfoParams(), capi.DfoReport(), np.zeros(2)
    L.lio_dfo_default_params(C.byref(p))
    seen = []
    cb = capi.DFO_FN(lambda x, n, u: seen.append(1) or float(x[0] ** 2 + x[1] ** 2))
    hook = capi.DFO_HOOK(lambda e, x, n, f, u: int(e >= 7))
    lb, ub = capi.f64([-1, -2]), capi.f64([3, 1])
    assert L.lio_dfo_direct_l(cb, None, 2, capi.ptr(lb, C.c_double), capi.ptr(ub, C.c_double), C.byref(p), hook, None, capi.ptr(out, C.c_double), C.byref(rep)) == 0
    assert rep.evals == len(seen) == 7 and rep.stop == capi.DFO_STOP_HOOK
    p.max_evals = 1
    assert L.lio_dfo_direct_l(cb, None, 2, capi.ptr(lb, C.c_double), capi.ptr(ub, C.c_double), C.byref(p), capi.DFO_HOOK(), None, capi.ptr(out, C.c_double), C.byref(rep)) == 0
    assert rep.evals == 1 and np.array_equal(out, [1.0, -0.5])
    assert L.lio_dfo_direct_l(cb, None, 9, capi.ptr(lb, C.c_double), capi.ptr(ub, C.c_double), C.byref(p), capi.DFO_HOOK(), None, None, None) == capi.LIO_E_INVALID


def test_nelder_mead_on_an_ill_conditioned_quadratic():
    centre = np.array([0.8, -0.6, 0.05, 0.07, -0.02, 0.16, 0.0])
    half = np.array([10.0, 10.0, 1.0, 1.0, 1.0, 1.0, 0.2])
    xmin = centre + half * np.array([0.04, -0.03, 0.2, -0.05, 0.03, 0.06, 0.25])
    w = np.logspace(0, 2, 7)  # condition number 100 in the box's own units

    def f(x):
        return float((w * ((x - xmin) / half) ** 2).sum())

    c, best, rep = _run("nm", f, centre - half, centre + half, x0=centre)
    print("Nelder-Mead: evals", rep.evals, "f(x0)", f(centre), "f(best)", rep.f_best, "ratio", rep.f_best / f(centre))
    assert np.array_equal(c.xs[0], centre) and rep.evals <= 500
    assert rep.f_best <= 1e-6 * f(centre)


def test_nelder_mead_projects_onto_the_box():
    # the minimiser lies outside: the best point ends on the face, and no evaluation leaves the box (Counted checks every one)
    c, best, rep = _run("nm", lambda x: float(((x - np.array([5.0, 0.2])) ** 2).sum()), [-1, -1], [1, 1], x0=[0.9, 0.0], max_evals=200)
    assert abs(best[0] - 1.0) < 1e-3 and abs(best[1] - 0.2) < 1e-2 and rep.evals <= 200


# ---- the outer module's surface -----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(REF_WRAPPER), reason="the reference tree is not mounted")
def test_module_surface_is_the_references_ins_half():
    block = open(REF_WRAPPER).read().split("PYBIND11_MODULE(calib_driver_ext", 1)[1]
    ref = {m.group(1): re.findall(r'py::arg\("(\w+)"\)', m.group(2)) for m in re.finditer(r'm\.def\("(\w+)",([^;]*);', block)}
    ins = {k: v for k, v in ref.items() if k.startswith("calib_ins_")}
    assert len(ins) == 6
    import calib_driver_ext as ext

    for name, args in ins.items():
        doc = getattr(ext, name).__doc__
        got = re.findall(r"(\w+): ", doc.split("->")[0])
        assert got == args, (name, got, args)
    assert not [n for n in dir(ext) if n.startswith("calib_imu_")]  # the lidar-IMU calibration is out of scope: no no-op stand-ins
    assert sorted(n for n in dir(ext) if n.startswith("calib_ins_")) == sorted(ins)
