#!/usr/bin/env python3
"""Records tests/golden/calib_ins_e2e.npz for the end-to-end case of the lidar-INS calibration.  Runs on the CPU: no device is touched.

For the scene and drive of tests/calib_ins_cases.py it evaluates the restated cost (cKDTree, f64, local metric) at the truth and at the initial
transform, and at the results of
  * the yardstick: scipy.optimize.direct(locally_biased=True, maxfun=500) over the global box, then scipy.optimize.minimize(Nelder-Mead,
    maxfev=500) over the local box, driven by the protocol of Aligner::lidarOdomTransform (the best evaluation across both stages, the local box
    around log(best), one more evaluation after each stage), and
  * the CPU twin: the product's own lio_dfo_direct_l / lio_dfo_nelder_mead over the same restated cost through a ctypes callback, under the same
    protocol.  This is where the simplex steps of lio_calib_params.nm_step are settled.
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lidar-slam-detection_amd", "python"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import calib_ins_cases as CI  # noqa: E402
from lsd_amd import capi  # noqa: E402

GLOBAL_LB = np.array([-100.0, -100.0, -10.0, -np.pi, -np.pi, -np.pi])
LOCAL_HALF = np.array([10.0, 10.0, 1.0, 1.0, 1.0, 1.0])
MAX_EVALS, XTOL, MAX_OFFSET = 500, 1e-4, 0.2


class Protocol:
    """Aligner's bookkeeping around an optimiser: error_, the best transform, the evaluation count"""

    def __init__(self, R, init):
        self.R, self.best, self.error, self.evals, self.local = R, np.asarray(init, np.float64), 1e8, 0, False

    def f(self, x):
        x = np.asarray(x, np.float64)
        e = self.R.cost(x, 1 if self.local else 0)
        if self.error > e:
            self.error, self.best = e, x[:6].copy()
        self.evals += 1
        return e

    def run(self, global_opt, local_opt):
        self.R.poses = CI.scan_poses(self.R.odom_stamps, self.R.odom_T7, self.R.scan_stamps, 0.0)
        self.error = self.R.cost(self.best, 0)
        xg = global_opt(self.f, GLOBAL_LB, -GLOBAL_LB)
        self.f(xg)
        x = self.best.copy()
        self.local = True
        lb, ub = np.concatenate([x - LOCAL_HALF, [-MAX_OFFSET]]), np.concatenate([x + LOCAL_HALF, [MAX_OFFSET]])
        xl = local_opt(self.f, np.concatenate([x, [0.0]]), lb, ub)
        self.f(xl)
        return self.best.copy()


def scipy_direct(f, lb, ub):
    from scipy.optimize import direct

    return direct(f, list(zip(lb, ub)), locally_biased=True, maxfun=MAX_EVALS, maxiter=100000).x


def scipy_nm(f, x0, lb, ub):
    from scipy.optimize import minimize

    return minimize(f, x0, method="Nelder-Mead", bounds=list(zip(lb, ub)), options=dict(maxfev=MAX_EVALS, xatol=XTOL, fatol=0.0)).x


def product_opt(kind, steps):
    L = capi.lib()

    def run(f, *args):
        x0, lb, ub = (None, *args) if kind == "direct" else args
        p, rep = capi.DfoParams(), capi.DfoReport()
        L.lio_dfo_default_params(C.byref(p))
        p.max_evals, p.xtol_abs = MAX_EVALS, XTOL
        for i, s in enumerate(steps):
            p.step[i] = s
        cb = capi.DFO_FN(lambda x, n, u: float(f([x[i] for i in range(n)])))
        lb, ub, out = capi.f64(lb), capi.f64(ub), np.zeros(len(lb))
        if kind == "direct":
            rc = L.lio_dfo_direct_l(cb, None, len(lb), capi.ptr(lb, C.c_double), capi.ptr(ub, C.c_double), C.byref(p), capi.DFO_HOOK(), None,
                                    capi.ptr(out, C.c_double), C.byref(rep))
        else:
            rc = L.lio_dfo_nelder_mead(cb, None, len(lb), capi.ptr(capi.f64(x0), C.c_double), capi.ptr(lb, C.c_double), capi.ptr(ub, C.c_double), C.byref(p),
                                       capi.DFO_HOOK(), None, capi.ptr(out, C.c_double), C.byref(rep))
        assert rc == 0
        return out

    return run


def main():
    t0 = time.time()
    scans, stamps, odom, ostamps = CI.e2e_inputs()
    R = CI.e2e_restated(scans, stamps, odom, ostamps)
    truth, init = np.array(CI.E2E["truth"]), np.array(CI.E2E["init"])
    J = lambda x: R.cost(np.concatenate([x[:6], [0.0]]), 1)  # noqa: E731
    j_truth, j_init = J(truth), J(init)
    print(f"points kept {[len(s) for s in R.scans]}  J(truth) {j_truth:.4f}  J(init) {j_init:.4f}  ratio {j_init / j_truth:.2f}  [{time.time() - t0:.0f} s]")
    assert j_init >= 3 * j_truth, "choose inputs with J(init) >= 3 J(truth)"
    cp = capi.CalibParams()
    capi.lib().lio_calib_default_params(C.byref(cp))
    steps = list(cp.nm_step)
    py = Protocol(R, init)
    x_y = py.run(scipy_direct, scipy_nm)
    j_y = J(x_y)
    print(f"yardstick: evals {py.evals}  x {x_y}  J {j_y:.4f}  [{time.time() - t0:.0f} s]")
    pt = Protocol(R, init)
    x_t = pt.run(product_opt("direct", steps), product_opt("nm", steps))
    j_t = J(x_t)
    bound = j_y + 0.05 * (j_init - j_y)
    print(f"twin: evals {pt.evals}  x {x_t}  J {j_t:.4f}  bound {bound:.4f}  steps {steps}  [{time.time() - t0:.0f} s]")
    for name, x in (("init", init), ("yardstick", x_y), ("twin", x_t)):
        dt, dr = CI.pose_errors(x, truth)
        print(f"  {name:10s} |dxyz| {dt}  |drot| {dr}")
    assert j_t <= bound, "the CPU twin misses the end-to-end condition"
    np.savez(CI.GOLDEN, e2e=np.array(repr(sorted(CI.E2E.items()))), checksum=np.array(CI.checksum(scans)), truth=truth, init=init, J_truth=j_truth, J_init=j_init,
             J_yardstick=j_y, x_yardstick=x_y, J_twin=j_t, x_twin=x_t, evals_yardstick=py.evals, evals_twin=pt.evals, nm_step=np.array(steps))
    print("wrote", CI.GOLDEN)


if __name__ == "__main__":
    main()
