#!/usr/bin/env python
"""The lidar-INS calibration on one device (lio_calib_ins_*, csrc/calib.hip), measured: milliseconds per evaluation of the cost for both metrics
at 20 scans x about 6000 points (wall clock of the call, and the stage split assemble / build / terms + fold from lio_calib_ins_last_times, HIP
events), the share of the walk's time that starting it from the cap removes (the same evaluation with kd started at +inf), the whole
calibration's wall time, and on the same inputs the restatement's evaluation on the host (scipy's cKDTree, tests/calib_ins_cases.py).  Then the
end-to-end case of tests/test_calib_ins_gpu.py with its figures.  A warm-up, then the median of 10.  Writes profiles/calib_ins_bench.json (or
the path given).  The host figure is scipy on whatever host this runs on: a scale, not a race.  No threshold: the record is the result."""
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "lidar-slam-detection_amd", "python"), os.path.join(ROOT, "tests")]
import calib_ins_cases as CI  # noqa: E402
from lsd_amd import lio  # noqa: E402


def load(cal, scans, stamps, odom, ostamps):
    kept = [cal.add_scan(s, st) for s, st in zip(scans, stamps)]
    for M, st in zip(odom, ostamps):
        cal.add_odom(M, st)
    cal.scan_matrices(0.0)
    return kept


def median_eval(cal, x, metric, reps=11):
    rows = []
    for _ in range(reps):
        t0 = time.perf_counter()
        e = cal.error(x, metric)
        rows.append(((time.perf_counter() - t0) * 1e3,) + tuple(v / 1e3 for v in cal.last_times()))
    r = np.median(np.array(rows[1:]), axis=0)
    return dict(cost=e, wall_ms=float(r[0]), assemble_ms=float(r[1]), build_ms=float(r[2]), terms_and_fold_ms=float(r[3]))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "calib_ins_bench.json")
    e2e = copy.deepcopy(CI.E2E)
    CI.E2E.update(n_scans=20, dt_scan=0.4)
    scans, stamps, odom, ostamps = CI.e2e_inputs()
    CI.E2E.update(e2e)
    init = np.array(CI.E2E["init"])
    x7 = np.concatenate([init, [0.0]])
    cal = lio.InsCalib(init=CI.se3_matrix(CI.se3_exp(init)))
    kept = load(cal, scans, stamps, odom, ostamps)
    out = dict(scans=len(scans), points=int(sum(kept)), metrics={})
    R = CI.e2e_restated(scans, stamps, odom, ostamps)
    for name, m in (("global", 0), ("local", 1)):
        d = median_eval(cal, x7, m)
        u = median_eval(cal, x7, m | lio.InsCalib.UNCAPPED)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            hc = R.cost(x7, m)
            host.append((time.perf_counter() - t0) * 1e3)
        d.update(uncapped_terms_and_fold_ms=u["terms_and_fold_ms"], share_of_the_walk_the_cap_removes=1.0 - d["terms_and_fold_ms"] / u["terms_and_fold_ms"],
                 same_cost_uncapped=bool(u["cost"] == d["cost"]), restatement_ckdtree_on_this_host_ms=float(np.median(host)), restatement_cost=hc,
                 host_over_device=float(np.median(host)) / d["wall_ms"])
        out["metrics"][name] = d
        print(name, d, flush=True)
    t0 = time.perf_counter()
    cal.calibrate()
    out["calibration_wall_s"] = time.perf_counter() - t0
    out["calibration_evaluations"] = cal.progress()[0]
    print("calibration", out["calibration_wall_s"], "s", out["calibration_evaluations"], "evaluations", flush=True)
    # the end-to-end case of the tests
    g = np.load(CI.GOLDEN)
    scans, stamps, odom, ostamps = CI.e2e_inputs()
    assert CI.checksum(scans) == str(g["checksum"])
    cal = lio.InsCalib(init=CI.se3_matrix(CI.se3_exp(init)))
    load(cal, scans, stamps, odom, ostamps)
    t0 = time.perf_counter()
    T = cal.calibrate().astype(np.float64)
    wall = time.perf_counter() - t0
    x = CI.se3_log(CI.se3_from_matrix(T))
    R = CI.e2e_restated(scans, stamps, odom, ostamps)
    (dt0, dr0), (dt1, dr1) = CI.pose_errors(init, g["truth"]), CI.pose_errors(x, g["truth"])
    j = dict(J_init=float(g["J_init"]), J_truth=float(g["J_truth"]), J_yardstick=float(g["J_yardstick"]), J_twin=float(g["J_twin"]),
             J_result=R.cost(np.concatenate([x, [0.0]]), 1))
    j["bound"] = j["J_yardstick"] + 0.05 * (j["J_init"] - j["J_yardstick"])
    out["end_to_end"] = dict(j, wall_s=wall, evaluations=cal.progress()[0], result=x.tolist(), truth=g["truth"].tolist(), init=init.tolist(),
                             yardstick=g["x_yardstick"].tolist(), twin=g["x_twin"].tolist(), xyz_error_init_m=dt0.tolist(), xyz_error_result_m=dt1.tolist(),
                             rot_error_init_rad=dr0.tolist(), rot_error_result_rad=dr1.tolist())
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
