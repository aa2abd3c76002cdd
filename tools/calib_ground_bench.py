#!/usr/bin/env python
"""Lidar ground calibration on one MI355X: lsd_amd.calib_lidar.align_points_to_xyplane (lio_calib_ground_*, csrc/calib_ground.hip) on a
seeded synthetic 120 000-point scan whose five-vertex ROI keeps a few tens of thousands of points, 100 iterations, against the same rules
written as the reference writes them -- scalar Python loops over every point (tests/calib_ground_cases.py: crop_loop, fit_loop) -- on the same
input and host, run once.  The reference itself is not timed here.

    python tools/calib_ground_bench.py [--points 120000] [--repeats 3] [--no-cpu] [--out FILE]

Prints one JSON record.  Device times come from HIP events on the handle's stream (lio_calib_ground_last_times): the crop (count kernel, scan,
write kernel), and within the fit the plane and the score kernels summed over its batches; median of the repeats after one warm-up call (which
allocates).  Wall times are perf_counter around calls that end in a stream synchronise, uploads included."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lidar-slam-detection_amd", "python"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

ROI = [[-18.0, -16.0], [21.0, -19.0], [22.0, 17.0], [2.0, 4.0], [-19.0, 15.0]]


def scan(n, seed):
    """a tilted floor (sigma 2 cm) over 60 m x 60 m with a fifth of the points raised by 0.2 .. 2 m, x y z intensity"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-30, 30, (n, 2))
    z = -1.8 + 0.02 * xy[:, 0] - 0.015 * xy[:, 1] + rng.normal(0, 0.02, n)
    up = rng.choice(n, n // 5, replace=False)
    z[up] += rng.uniform(0.2, 2.0, len(up))
    return np.column_stack([xy, z, rng.uniform(0, 255, n)]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import calib_ground_cases as CG
    from lsd_amd import calib_lidar as CL

    pts = scan(a.points, a.seed)
    g = CL._handle()
    T = CL.align_points_to_xyplane(pts, ROI, seed=a.seed)  # warm-up: allocates
    crop, fit, planes, score, wall = [], [], [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        T = CL.align_points_to_xyplane(pts, ROI, seed=a.seed)
        wall.append(time.perf_counter() - t0)
        c, f, p, s = g.last_times()
        crop.append(c); fit.append(f); planes.append(p); score.append(s)
    run, kept = g.last_run(), int(len(g.indices()))
    n_scored = int(len(g.draws()[2]))
    rec = dict(tool="calib_ground_bench", points=a.points, kept=kept, vertices=len(ROI), num_iteration=CG.NUM_ITERATION, seed=a.seed, repeats=a.repeats,
               run=run, attempts_scored=n_scored, T=[float(v) for v in T.reshape(-1)],
               device_us=dict(crop=float(np.median(crop)), fit_incl_host_replay=float(np.median(fit)), plane_kernels=float(np.median(planes)),
                              score_kernels=float(np.median(score)), crop_min=float(np.min(crop)), score_kernels_min=float(np.min(score))),
               align_points_to_xyplane_wall_ms=1e3 * float(np.median(wall)), align_points_to_xyplane_wall_ms_all=[1e3 * w for w in wall],
               not_taken="rocprofv3 kernel statistics; the reference's own time at this size")
    if not a.no_cpu:
        t0 = time.perf_counter()
        keep = CG.crop_loop(pts, ROI)
        t1 = time.perf_counter()
        coef, winner = CG.fit_loop(pts[keep, :3], CG.SIGMA, CG.NUM_ITERATION, CG.THRESH, a.seed)
        t2 = time.perf_counter()
        rec["python_loop_restatement_run_once"] = dict(crop_s=t1 - t0, fit_s=t2 - t1, total_s=t2 - t0, kept=len(keep), winner=winner,
                                                      same_transform=bool(np.array_equal(CL.plane_to_transform(coef), T)))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
