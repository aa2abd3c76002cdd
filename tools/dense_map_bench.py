#!/usr/bin/env python
"""Dense-map export on one MI355X: a seeded synthetic drive through accumulate_cloud's device path (frame upload, pose-list undistortion,
lio_cloud_append_scan with the frame's absolute pose), then the whole-cloud VoxelGrid (lio_cloud_voxel_downsample) at several leaf sizes,
against the CPU oracle's VoxelGrid on the same cloud (the reference's PCL is not available to time; the oracle is the project's own
restatement of it, oracle/lio_oracle.cpp).

    python tools/dense_map_bench.py [--frames 600] [--points 120000] [--leaves 0.1,0.2,0.5] [--no-oracle] [--out FILE]

Prints one JSON record.  Device times come from HIP events on the cloud's stream (lio_cloud_last_times); the frame's host-to-device copy is
timed on the host (it is synchronous from pageable memory) and reported apart.  The bytes the chain must move are computed from the shapes
(see chain_bytes); frac_of_8TBps = those bytes / voxel time / 8 TB/s."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lidar-slam-detection_amd", "python"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_BPS = 8.0e12
# (a loop of 300 m radius puts the 0.1 m grid past PCL's int32 voxel-count guard: the filter then returns its input, as PCL does)
RADIUS = 100.0


def rot(q):  # (x, y, z, w) -> R
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def drive(n_frames, n_points, seed):
    """frames of a 2 km drive, three times round a loop of 100 m radius, through a synthetic scene: the frame's points in the sensor frame (a random sample of the scene's
    surface in the 120 m x 120 m around the sensor, with noise), per-point stamps over 100 ms, five TUM poses per frame"""
    from lsd_amd import synth

    rng = np.random.default_rng(seed)
    scene = synth.Scene(half=400.0, n_boxes=400, seed=seed)
    surf = scene.sample_surface(6_000_000, seed=seed + 1)[:, :3].astype(np.float64)
    cell = np.floor(surf[:, :2] / 40.0).astype(np.int64)  # 40 m bins: a frame's neighbourhood without a pass over the whole surface
    key = (cell[:, 0] + 1000) * 4096 + (cell[:, 1] + 1000)
    order = np.argsort(key, kind="stable")
    keys_sorted = key[order]
    for f in range(n_frames):
        s = 2000.0 * f / max(n_frames, 1)
        ang = s / RADIUS
        pos = np.array([RADIUS * np.cos(ang), RADIUS * np.sin(ang), 1.8])
        c0 = np.floor(pos[:2] / 40.0).astype(np.int64)
        near = np.concatenate([order[np.searchsorted(keys_sorted, k, "left"):np.searchsorted(keys_sorted, k, "right")]
                               for dx in (-1, 0, 1) for dy in (-1, 0, 1) for k in [(c0[0] + dx + 1000) * 4096 + (c0[1] + dy + 1000)]])
        idx = rng.choice(near, n_points, replace=len(near) < n_points)
        q = synth.quat_from_rotvec([0, 0, ang + np.pi / 2])
        R = rot(q)
        body = (surf[idx] - pos) @ R  # world -> sensor
        pts = np.concatenate([body + rng.normal(0, 0.02, body.shape), rng.uniform(0, 1, (n_points, 1))], 1).astype(np.float32)
        stamps = np.sort(rng.integers(0, 100_000, n_points)).astype(np.uint32)
        header = 1_700_000_000_000_000 + 100_000 * f
        rows = []
        for k in range(5):
            a = ang + 0.0005 * k
            qk = synth.quat_from_rotvec([0, 0, a + np.pi / 2])
            rows.append([header + 25_000 * k, RADIUS * np.cos(a), RADIUS * np.sin(a), 1.8, *qk])
        yield pts, stamps, header, np.array(rows)


def chain_bytes(n, n_valid, n_vox, passes):
    """bytes the voxel chain must move, from its shapes: bbox read 16/pt; keys read 16, write key + value 8; per radix pass a histogram read
    of the keys (not in the first pass: fused into the keys) 4, the scatter's read and write of key + value 16, the [digit][tile] table
    (256 words per 2048-point tile: written, scanned = read twice and written, read) 20 * 256 / 2048 per point; head count read 4; head write
    read key + value 8, the gather read 16 and write 16 (finite points); centroid read 16 (finite points), write 16 per voxel"""
    per_pass_table = 20.0 * 256 / 2048
    b = 16.0 * n + 24.0 * n
    b += passes * (16.0 * n + per_pass_table * n) + max(passes - 1, 0) * 4.0 * n
    b += 4.0 * n + 8.0 * n + 32.0 * n_valid + 16.0 * n_valid + 16.0 * n_vox
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--leaves", default="0.1,0.2,0.5")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import slam_wrapper as sw

    from lsd_amd import lio

    scan = lio.Scan(max_raw=a.points, max_ds=1024)
    cloud = lio.Cloud(reserve=a.frames * a.points)
    h2d_s = und_s = 0.0
    app_us = []
    wall0 = time.perf_counter()
    for pts, stamps, header, rows in drive(a.frames, a.points, a.seed):
        T0, rel = sw._tum_relative_poses(rows)
        Ts = np.stack([np.asarray(r) for r in rel]).reshape(-1, 16)
        t0 = time.perf_counter()
        scan.upload(pts)
        t1 = time.perf_counter()
        scan.undistort_poses(stamps, header, rows[:, 0].astype(np.uint64), Ts)
        t2 = time.perf_counter()
        cloud.append_scan(scan, np.asarray(T0))
        app_us.append(cloud.last_times()[0])
        h2d_s += t1 - t0
        und_s += t2 - t1
    wall = time.perf_counter() - wall0
    n = cloud.size
    whole = cloud.download()
    fin = np.isfinite(whole[:, :3]).all(1)
    rec = dict(tool="dense_map_bench", frames=a.frames, points_per_frame=a.points, points=int(n), cloud_bytes=int(n) * 16,
               accumulate=dict(append_device_us_per_frame=float(np.mean(app_us)), append_device_us_p50=float(np.median(app_us)),
                               h2d_plus_enqueue_host_ms_per_frame=1e3 * h2d_s / a.frames, undistort_host_ms_per_frame=1e3 * und_s / a.frames,
                               append_points_per_s=float(a.points / (np.mean(app_us) * 1e-6)),
                               note="append = transform + copy into the cloud (device events); h2d = scan upload from pageable memory, host wall; "
                                    "undistort = lio_scan_undistort_poses incl. the stamps' copy, host wall"),
               voxel=[])
    for leaf in [float(x) for x in a.leaves.split(",") if x]:
        cloud.clear()
        cloud.append_host(whole)
        scratch = cloud.scratch_bytes()
        t0 = time.perf_counter()
        m = cloud.voxel_downsample(leaf)
        wall_v = time.perf_counter() - t0
        vus = cloud.last_times()[1]
        inv = np.float32(1.0) / np.float32(leaf)
        mn, mx = whole[fin, :3].min(0), whole[fin, :3].max(0)
        cells = np.prod((np.floor(mx * inv).astype(np.int64) - np.floor(mn * inv).astype(np.int64) + 1).astype(np.float64))
        passes = int((int(cells).bit_length() + 7) // 8)
        b = chain_bytes(n, int(fin.sum()), m, passes)
        e = dict(leaf=leaf, points_out=int(m), radix_passes=passes, device_ms=vus / 1e3, wall_ms_incl_scratch_alloc=wall_v * 1e3,
                 points_per_s=n / (vus * 1e-6), ms_per_1e8_points=vus / 1e3 * 1e8 / n, chain_bytes=b, bytes_per_point=b / n,
                 frac_of_8TBps=b / (vus * 1e-6) / PEAK_BPS, scratch_bytes=int(scratch))
        if not a.no_oracle:
            import oracle

            t0 = time.perf_counter()
            ref = oracle.voxel_downsample(whole, leaf)
            e["cpu_oracle_ms"] = (time.perf_counter() - t0) * 1e3
            got = cloud.download()
            e["bit_equal_to_oracle"] = bool(len(ref) == len(got) and np.array_equal(ref.view(np.uint32), got.view(np.uint32)))
        rec["voxel"].append(e)
    rec["drive_wall_s"] = wall
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
