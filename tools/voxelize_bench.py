#!/usr/bin/env python
"""The detection front end on one MI355X (lio.Voxelizer; csrc/voxelize.hip) at the configuration's own size
(sensor_inference/cfgs/detection_object.yaml: range +-64 / +-64 / -2..4, voxel 0.1 / 0.1 / 0.15, 5 points per voxel, 300 000 voxels, 2 sweeps,
room for 500 000 points): two sweeps of 120 000 and of 250 000 synthetic lidar points from lsd_amd.synth, the second sweep a realtime call
with a small ego motion, so that the window holds both and every stage runs.

    python tools/voxelize_bench.py [--sizes 120000 250000] [--repeats 20] [--warmup 3] [--no-cpu] [--out FILE]

Prints one JSON record.  Per size: the stage times of the second call from HIP events on the handle's stream (lio_voxelizer_last_times: window
move + sweep copy, table clear + insert, head ranking, slots, means, first launch to last; medians and minima over the repeats after the
warm-up calls), the wall time of the call (perf_counter, the upload and the one host wait included), the counts, and the bytes every stage
must move once.  Beside them, FOR INFORMATION ONLY: the host time of the numpy restatement of tests/voxelize_cases.py on the same window (run
once, numpy's own threads, at most 16) with the check that the device's output equals it, and lio_cloud_voxel_downsample -- the project's
sort-based voxel stage, PCL's centroid filter, another result -- on the same points at leaf 0.1.  The reference itself is not timed here and
nothing of it is read.  There is no pass / fail threshold: this is the first measurement and the parent commit has no such path."""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lidar-slam-detection_amd", "python"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

P, MAX_VOXELS, MAX_POINTS, FRAMES = 5, 300_000, 500_000, 2


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)))


def sweeps(n, seed):
    """two sweeps of exactly n rows (x y z intensity 0, the sensor's frame: the ground near z = -1.8) from two poses 0.8 m apart, and the motion
    from the first pose's frame to the second's"""
    from lsd_amd import synth

    scene = synth.Scene(half=100.0, n_boxes=40, seed=1)
    beams, az = (64, 2600) if n <= 140_000 else (128, 2800)
    out = []
    for k, x in enumerate((0.0, 0.8)):
        raw, _ = synth.make_scan(scene, np.array([x, 0.0, 1.8]), synth.quat_from_rotvec([0.0, 0.0, 0.0]), seed=seed + k, n_beams=beams, n_az=az, max_range=100.0)
        if len(raw) < n:
            raise SystemExit(f"the synthetic scan has {len(raw)} returns, {n} are needed")
        pick = np.sort(np.random.default_rng(seed + 10 + k).choice(len(raw), n, replace=False))
        rows = np.zeros((n, 5), np.float32)
        rows[:, :4] = raw[pick]
        out.append(rows)
    motion = np.eye(4, dtype=np.float32)
    motion[0, 3] = -0.8  # a point of the first frame seen from the second
    return out, motion


def bytes_once(n0, n1, table, in_range, voxels, kept):
    m = n0 + n1
    return dict(window=2 * 20 * n0, sweep_copy=2 * 20 * n1, table_clear=2 * 4 * table, insert=12 * m + 4 * m + 8 * in_range, rank=2 * (4 * m + 4 * in_range) + 16 * voxels + 4 * P * voxels,
                slots=4 * m + 4 * in_range + 4 * in_range + 4 * P * voxels, mean=20 * kept + 4 * P * voxels + 14 * voxels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[120_000, 250_000])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import voxelize_cases as vc
    from lsd_amd import lio

    p = vc.params(max_voxels=MAX_VOXELS, P=P, max_points=MAX_POINTS, frames=FRAMES, **vc.YAML)
    v = lio.Voxelizer(p["min"], p["max"], p["size"], MAX_VOXELS, P, MAX_POINTS, FRAMES, vc.ZYX)
    rec = dict(tool="voxelize_bench", config=dict(range=[-64, -64, -2, 64, 64, 4], voxel=[0.1, 0.1, 0.15], max_points_per_voxel=P, max_voxels=MAX_VOXELS, max_points=MAX_POINTS,
                                                  frames=FRAMES, grid=lio.Voxelizer.grid_size(p["min"], p["max"], p["size"])), repeats=a.repeats, warmup=a.warmup, sizes=[])
    names = ("window_us", "insert_us", "rank_us", "slots_us", "mean_us", "total_us")
    for n in a.sizes:
        (s0, s1), motion = sweeps(n, a.seed)
        t, wall = [], []
        for r in range(a.warmup + a.repeats):
            v.forward(s0, None, False)
            w0 = time.perf_counter()
            v.forward(s1, motion, True)
            w1 = time.perf_counter()
            if r >= a.warmup:
                t.append(v.last_times())
                wall.append((w1 - w0) * 1e6)
        t = np.asarray(t)
        real, in_range, kept = v.last_counts()
        feat, idx, cnt = v.output()
        table = 64
        while table < 4 * n:
            table <<= 1
        one = dict(points_per_sweep=n, window_rows=2 * n, points_in_range=in_range, real_voxels=real, voxels=v.num_voxels, points_kept=kept, table_slots=table,
                   device={k: stats(t[:, i]) for i, k in enumerate(names)}, wall_us=stats(wall),
                   bytes_once=bytes_once(n, n, table, in_range, v.num_voxels, kept))
        if not a.no_cpu:
            w = vc.Window(MAX_POINTS, FRAMES)
            w.forward(s0, vc.EYE, False)
            c0 = time.perf_counter()
            win = w.forward(s1, motion, True)
            c1 = time.perf_counter()
            r = vc.voxelize(win, p)
            c2 = time.perf_counter()
            one["restatement_host_us"] = dict(window=(c1 - c0) * 1e6, voxelize=(c2 - c1) * 1e6)
            one["equals_restatement"] = bool(np.array_equal(feat.view(np.uint16), r["features"]) and np.array_equal(idx, r["indices"]) and np.array_equal(cnt, r["counts"])
                                             and np.array_equal(v.window().view(np.uint32), win.view(np.uint32)) and real == r["real"])
        # for information: the sort-based voxel stage (pcl::VoxelGrid centroids at leaf 0.1) over the same 2n points
        cloud = lio.Cloud(reserve=2 * n)
        win4 = np.ascontiguousarray(v.window()[:, :4])
        vt = []
        for r in range(a.warmup + 5):
            cloud.clear()
            cloud.append_host(win4)
            out_n = cloud.voxel_downsample(0.1)
            if r >= a.warmup:
                vt.append(cloud.last_times()[1])
        cloud.close()
        one["cloud_voxel_downsample"] = dict(leaf=0.1, points_out=out_n, device_us=stats(vt))
        rec["sizes"].append(one)
    v.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
