#!/usr/bin/env python
"""Bird's-eye intensity image on one MI355X: lio_bev_* (csrc/bev.hip) on a seeded synthetic ground cloud of a square map at the reference's
defaults (25 px/m, 50 m window).

    python tools/bev_bench.py [--points 20000000] [--side 1000] [--ppm 25] [--window 50] [--repeats 3] [--out FILE]

Prints one JSON record.  Device times come from HIP events on the handle's stream (lio_bev_last_times): preprocess = bounds + noise filter
(4 radix passes) + pixel keys + second sort + heads + per-pixel means, the two host read-backs included; convert = row ranges + one
workgroup per equalisation node + render.  Median of the repeats after one warm-up call (which allocates the scratch).  The reference's
numpy version is not timed at this size (its work is nodes x pixels x steps)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lidar-slam-detection_amd", "python"),):
    if p not in sys.path:
        sys.path.insert(0, p)


def cloud(n, side, seed=7):
    """ground of side x side metres: a brightness ramp, lane-like bright stripes every 25 m and a square hole in the middle"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, side, n).astype(np.float32), rng.uniform(0, side, n).astype(np.float32)
    inten = (0.04 + 0.10 * x / side + rng.normal(0, 0.012, n)).astype(np.float32)
    stripe = (np.abs(np.mod(y, 25.0) - 12.5) < 0.15) | (np.abs(np.mod(x, 25.0) - 12.5) < 0.15)
    inten = np.where(stripe, 0.55 + rng.normal(0, 0.05, n), inten).clip(0.001, 1.0).astype(np.float32)
    z = (0.02 * np.sin(x / 7.0)).astype(np.float32)
    pts = np.stack([x, y, z, inten], 1)
    hole = (np.abs(x - side / 2) < side * 0.1) & (np.abs(y - side / 2) < side * 0.1)
    return np.ascontiguousarray(pts[~hole])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--side", type=float, default=1000.0)
    ap.add_argument("--ppm", type=int, default=25)
    ap.add_argument("--window", type=float, default=50.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from lsd_amd import lio

    pts = cloud(a.points, a.side)
    h = lio.BevImage()
    h.preprocess_host(pts, a.ppm)  # warm-up: allocates
    h.convert(a.window, a.ppm)
    pre, con, wall = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        h.preprocess_host(pts, a.ppm)
        lib_t = time.perf_counter()
        lio.lib().lio_bev_convert(h.h, float(a.window), float(a.ppm))
        wall.append((lib_t - t0, time.perf_counter() - lib_t))
        p, c = h.last_times()
        pre.append(p)
        con.append(c)
    info = h.info()
    count, step, clip = h.nodes()
    run = step >= 0
    rec = dict(tool="bev_bench", points=int(len(pts)), side_m=a.side, pixel_per_meter=a.ppm, window_m=a.window, repeats=a.repeats,
               image=[info["padded_w"], info["padded_h"]], occupied_pixels=info["n_pixels"], kept_points=info["n_kept"],
               nodes=int(len(step)), nodes_running=int(run.sum()), steps_max=int(step.max()), clip_min=float(clip[run].min()) if run.any() else None,
               clip_max=float(clip.max()), pixels_per_window_max=int(count.max()),
               device_us=dict(preprocess=float(np.median(pre)), convert=float(np.median(con)), preprocess_min=float(np.min(pre)), convert_min=float(np.min(con))),
               host_wall_ms=dict(preprocess_incl_h2d=1e3 * float(np.median([w[0] for w in wall])), convert=1e3 * float(np.median([w[1] for w in wall]))))
    h.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
