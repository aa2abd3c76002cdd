"""The outer boundary of the lidar-INS calibration: the reference's calling sequence through the pybind11 module calib_driver_ext
(sensor_driver/calibration/calib_wrapper.cpp:41-115), and the reference's own calib_driver.py on top of it when the reference tree is there.
Small scans and a reduced evaluation budget (the module's test hook) keep a run at a fraction of a second."""
import importlib.util
import os
import time

import numpy as np
import pytest

import calib_ins_cases as CI
from lsd_amd import lio

pytestmark = pytest.mark.gpu
STAMP0 = 1_700_000_000_000_000
REF_DRIVER = "/root/reference/sensor_driver/calibration/calib_driver.py"
DEADLINE_S = 60.0


def _inputs():
    rng = np.random.default_rng(3)
    init = CI.se3_matrix(CI.se3_exp(np.array([0.2, -0.1, 0.05, 0.02, -0.01, 0.05]))).astype(np.float32)
    scans = []
    for i in range(21):
        k = 150
        floor = np.stack([rng.uniform(-5, 5, k), rng.uniform(-5, 5, k), rng.normal(0, 0.01, k), rng.uniform(0, 255, k)], 1)
        wall = np.stack([np.full(k, 5.0), rng.uniform(-5, 5, k), rng.uniform(0, 2, k), rng.uniform(0, 255, k)], 1)
        scans.append((np.concatenate([floor, wall]).astype(np.float32), STAMP0 + 100_000 + 40_000 * i))  # N x 4: the intensity column is not read
    odom = [(CI.se3_matrix(CI.se3_exp(np.array([0.5 * i, 0.05 * i * i, 0.0, 0.0, 0.0, 0.1 * i]))).astype(np.float32), STAMP0 + 100_000 * i) for i in range(12)]
    return init, scans, odom


def _drive(reset, set_points, set_odom, calibrate, get, get_T, ext, max_evals=40):
    init, scans, odom = _inputs()
    reset(init)
    ext._set_max_evals(max_evals)
    for p, st in scans:
        set_points(p, st)
    assert ext._counts()[0] == 20  # the 21st scan is ignored
    for T, st in odom:
        set_odom(T, st)
    assert ext._counts() == (20, 12, 20 * 300)
    t0 = time.monotonic()
    calibrate()
    assert time.monotonic() - t0 < 5.0  # returns at once: the optimisation runs on its own thread
    set_points(scans[20][0], scans[20][1])  # while it runs (and after, until the next reset): ignored
    set_odom(odom[0][0], odom[0][1] + 5)
    last, deadline = -1.0, time.monotonic() + DEADLINE_S
    while True:
        r = get()
        assert set(r) == {"finish", "percent"} and r["percent"] >= last
        last = r["percent"]
        if r["finish"]:
            break
        assert time.monotonic() < deadline, "the calibration did not finish in time"
    assert last == 100.0 and get()["percent"] == 100.0
    assert ext._counts() == (20, 12, 20 * 300)
    T = get_T()
    assert T.shape == (4, 4) and T.dtype == np.float32
    return init, scans, odom, T


def test_the_references_calling_sequence():
    import calib_driver_ext as ext

    init, scans, odom, T = _drive(ext.calib_ins_reset, ext.calib_ins_set_points, ext.calib_ins_set_odom, ext.calib_ins_calibrate,
                                  ext.calib_ins_get_calibration, ext.calib_ins_get_calibration_transform, ext)
    cal = lio.InsCalib(init=init)
    for p, st in scans[:20]:
        cal.add_scan(p, st)
    for M, st in odom:
        cal.add_odom(M, st)
    cal.scan_matrices(0.0)
    p = lio.InsCalib.default_params()
    p.max_evals = 40
    assert np.array_equal(cal.calibrate(p), T)  # the same inputs through the class: the same bits
    assert not np.array_equal(T, init)
    # a reset during a run joins it
    ext.calib_ins_reset(init)
    ext._set_max_evals(500)
    for pts, st in scans[:4]:
        ext.calib_ins_set_points(pts, st)
    for M, st in odom:
        ext.calib_ins_set_odom(M, st)
    ext.calib_ins_calibrate()
    ext.calib_ins_reset(np.eye(4, dtype=np.float32))
    assert ext._counts() == (0, 0, 0) and np.array_equal(ext.calib_ins_get_calibration_transform(), np.eye(4, dtype=np.float32))
    assert ext.calib_ins_get_calibration() == {"finish": False, "percent": 0.0}


@pytest.mark.skipif(not os.path.exists(REF_DRIVER), reason="the reference tree is not mounted")
def test_the_references_driver_runs_on_it_unchanged():
    import calib_driver_ext as ext

    spec = importlib.util.spec_from_file_location("ref_calib_driver", REF_DRIVER)
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)  # `import calib_driver_ext as driver` resolves to this project's module
    assert drv.driver is ext
    _drive(drv.calib_ins_reset, drv.calib_ins_add_points, drv.calib_ins_add_odom, drv.calib_ins_calibrate, drv.calib_ins_get_calibration,
           drv.calib_ins_get_calibration_transform, ext)
    ext.calib_ins_reset(np.eye(4, dtype=np.float32))
