#!/usr/bin/env python
"""Colour map on one MI355X: lio_render_* (csrc/render.hip) on a seeded synthetic road.

    python tools/render_bench.py [--points 120000] [--frames 200] [--images 3] [--rows 1080] [--cols 1920] [--out profiles/render_bench.json]

A vehicle drives 0.5 m per frame along a 16 m wide floor; every frame is `--points` points (floor plus a tenth of clutter above it) through the
ground test into the map, without images, for `--frames` frames.  Then ONE more frame is timed against `--images` images of rows x cols:
the wall time of the call (ground test, uploads and the wait included) and the device times of its stages from HIP events
(lio_render_last_times: the insert chain, all images, finish + read-back).

The yardstick is the numpy restatement of tests/render_cases.py on the host, the only one there is: the reference cannot be built here (PCL,
OpenCV, Boost) and the parent commit has no such path.  It is interpreted Python, not the reference's OpenMP code.  Its map is loaded from
the device's read-backs before the timed frame, it is handed the floor inliers of the device's detector (the ground test is not restated),
and it paints the same frame with the same images; `same_result` tells whether its map then equals the device's bit for bit.  The bench
asserts nothing."""
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


def frame_points(n, seed):
    """the body frame: floor 1 m below the sensor on x in [1, 25], y in [-8, 8], a tenth of the points scattered above it"""
    rng = np.random.default_rng(seed)
    m = n - n // 10
    fl = np.stack([rng.uniform(1, 25, m), rng.uniform(-8, 8, m), -1.0 + rng.normal(0, 0.004, m), np.full(m, 0.5)], 1)
    cl = np.stack([rng.uniform(1, 25, n - m), rng.uniform(-8, 8, n - m), rng.uniform(-0.8, 1.4, n - m), np.full(n - m, 0.5)], 1)
    return np.concatenate([fl, cl]).astype(np.float32)


def load(painter, vox, pts):
    """the restatement's map from the device's read-backs"""
    import render_cases as rc

    painter.clear()
    _, box, centre, cell, key = rc.voxel_of(pts["xyz"])
    for v, b in enumerate(vox["box"]):
        painter.vox_id[tuple(int(x) for x in b)] = v
        painter.box.append(tuple(int(x) for x in b))
        painter.hits.append(int(vox["hits"][v]))
        painter.vkeys.append({})
        painter.vpts.append([])
        painter.centre.append(None)
    for s in range(len(pts["xyz"])):
        v = int(pts["voxel"][s])
        painter.centre[v] = tuple(int(c) for c in centre[s])
        painter.vkeys[v][int(key[s])] = tuple(int(c) for c in cell[s])
        painter.vpts[v].append(s)
    painter.pos = list(pts["xyz"])
    painter.vox = [int(v) for v in pts["voxel"]]
    painter.rgb = list(pts["rgb"])
    painter.score = list(pts["score"])
    painter.depth = list(pts["depth"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--images", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=1920)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import render_cases as rc
    from lsd_amd import lio

    f = 0.94 * a.cols  # about 56 degrees across, as f = 300 is for 320 columns
    K = (f, f, a.cols / 2.0, a.rows / 2.0)
    yaws = [0.0, 25.0, -25.0, 50.0, -50.0][: a.images]
    cams = {"cam%d" % i: (K, rc.mount(yaw=y, pitch=12.0)) for i, y in enumerate(yaws)}
    cm = lio.ColourMap(max_voxels=1 << 18, max_points=1 << 24)
    cm.set_cameras(cams)
    t0 = time.perf_counter()
    outcomes = {}
    for k in range(a.frames):
        out = cm.frame(frame_points(a.points, k), rc.se3(None, (0.5 * (k + 1), 0.0, 0.0)), {}, use_ground=True, seed=k)
        outcomes[out] = outcomes.get(out, 0) + 1
    grow_s = time.perf_counter() - t0
    before = cm.size()
    pose = rc.se3(None, (0.5 * (a.frames + 1), 0.0, 0.0))
    pts = frame_points(a.points, a.frames)
    images = {n: (rc.image(a.rows, a.cols, 50 + i), pose) for i, n in enumerate(cams)}
    host = None
    if not a.no_host:
        host = rc.Painter(cams)
        load(host, cm.voxels(), cm.points())
        host.last_pose = rc.se3(None, (0.5 * a.frames, 0.0, 0.0))
        det = lio.GroundDetector()
        r = det.detect_host(pts, det.params(0, distance_threshold=rc.GROUND_THRESHOLD, seed=a.frames))
        inliers = det.inliers() if r["found"] else None
    t0 = time.perf_counter()
    out = cm.frame(pts, pose, images, use_ground=True, seed=a.frames)
    wall = time.perf_counter() - t0
    times = cm.last_times()
    after = cm.size()
    rec = dict(tool="render_bench", points=a.points, grown_by_frames=a.frames, grow_outcomes=outcomes, grow_wall_s=grow_s, images=a.images, image=[a.rows, a.cols],
               map_before=dict(voxels=before[0], points=before[1]), map_after=dict(voxels=after[0], points=after[1]), outcome=out,
               frame_wall_ms=1e3 * wall, device_us=times, exported_points=int(len(cm.colour_map())),
               yardstick="numpy restatement (tests/render_cases.py) on the host: interpreted Python, the only yardstick there is -- the reference cannot be "
                         "built here and the parent commit has no such path")
    if host is not None:
        t0 = time.perf_counter()
        hout = host.frame(pts, pose, images, (lambda q: inliers))
        rec["host_restatement_ms"] = 1e3 * (time.perf_counter() - t0)
        rec["host_outcome"] = hout
        want, got = host.state(), cm.points()
        rec["same_result"] = bool(out == hout and cm.size() == (len(want["hits"]), len(want["score"])) and
                                  all(np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)) for k in ("xyz", "rgb", "score", "depth")))
        rec["host_stats"] = {k: (float(v) if isinstance(v, float) else int(v)) for k, v in host.stats.items() if not k.startswith("min_")}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
