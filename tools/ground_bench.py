#!/usr/bin/env python
"""Ground extraction on one MI355X: the detector (lio_ground_*, csrc/ground.hip) on a seeded 120 000-point scan -- a ring-structured sweep
of lsd_amd.synth's scene and, for comparison, an unstructured sample of the same surface -- against the numpy / cKDTree restatement of
tests/ground_cases.py on the host (PCL is not available to time).

    python tools/ground_bench.py [--points 120000] [--repeats 20] [--no-cpu] [--out FILE]

Prints one JSON record.  Device times come from HIP events on the detector's stream (lio_ground_last_times): clip + index build + k-NN walk
+ normals + filter, and RANSAC (plane batches, the host's replay between them, the inlier selection); median of the repeats after one
warm-up call (which allocates the scratch)."""
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


def clouds(n):
    from lsd_amd import synth

    scn = synth.Scene(half=60.0, n_boxes=20, seed=3)
    n_az = max(1, n // 64)
    raw, _ = synth.make_scan(scn, np.array([0.5, 1.0, 1.2]), synth.quat_from_rotvec([0, 0, 0.2]), seed=5, n_az=n_az)
    surf = scn.sample_surface(n, seed=6, sigma=0.02)
    surf[:, 2] -= 1.2  # the sensor frame of a sensor 1.2 m above the ground
    return {"ring_sweep": raw[:, :4].astype(np.float32), "surface_sample": surf.astype(np.float32)}


def cpu_restatement(pts, seed):
    import ground_cases as gc

    t0 = time.perf_counter()
    cidx = gc.clip(pts)
    C = pts[cidx, :3]
    t1 = time.perf_counter()
    nn, _ = gc.self_knn(C)
    t2 = time.perf_counter()
    _, _, ang = gc.normals(C, nn)
    fidx = cidx[ang < 20.0]
    t3 = time.perf_counter()
    _, counts, planes, run = gc.ransac(pts[fidx, :3], seed, 64)
    inl = int(gc.residual_ok(pts[fidx, :3], planes[run["winner"]]).sum()) if run["winner"] >= 0 else 0
    t4 = time.perf_counter()
    return dict(clip_ms=1e3 * (t1 - t0), knn_ckdtree_16_workers_ms=1e3 * (t2 - t1), normals_eigh_ms=1e3 * (t3 - t2), ransac_64_draws_ms=1e3 * (t4 - t3),
                total_ms=1e3 * (t4 - t0), n_clipped=int(len(cidx)), n_filtered=int(len(fidx)), n_inliers=inl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from lsd_amd import lio

    det = lio.GroundDetector()
    rec = dict(tool="ground_bench", points=a.points, repeats=a.repeats, seed=a.seed, scans={})
    for name, pts in clouds(a.points).items():
        prm = det.params(0, seed=a.seed)
        res = det.detect_host(pts, prm)  # warm-up: allocates
        f_us, r_us, wall = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            res = det.detect_host(pts, prm)
            wall.append(time.perf_counter() - t0)
            f, r = det.last_times()
            f_us.append(f)
            r_us.append(r)
        run = det.last_run()
        e = dict(points=int(len(pts)), found=res["found"], n_clipped=res["n_clipped"], n_filtered=res["n_filtered"], n_inliers=res["n_inliers"],
                 coeffs=None if res["coeffs"] is None else [float(x) for x in res["coeffs"]], iterations=run["iterations"], draws_used=run["draws_used"],
                 device_us=dict(clip_knn_normals_filter=float(np.median(f_us)), ransac_and_inliers=float(np.median(r_us)),
                                clip_knn_normals_filter_min=float(np.min(f_us)), ransac_and_inliers_min=float(np.min(r_us))),
                 host_wall_ms_incl_h2d=1e3 * float(np.median(wall)))
        if not a.no_cpu:
            e["cpu_restatement"] = cpu_restatement(pts, a.seed)
        rec["scans"][name] = e
    det.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
