#!/usr/bin/env python
"""Lidar-IMU calibration's odometry on one MI355X at the tool's real shape: 64 x 1875 scans of a seeded scene along an arc (0.5 m and 1.8
degrees per frame), every frame a key frame, 200 key frames -- lio_calib_imu_lidar_pose + lio_calib_imu_add_frame (csrc/calib_imu.hip, the map
resident in HBM) against the same sequence done through the public entries with a host round trip per stage (tests/calib_imu_cases.py: Twin:
lio_scan_voxel_downsample, lio_cloud_append_host + filter, a host concatenation and a lio_cloud filter of the whole map, lio_gicp_set_target /
_set_source / _align).

    python tools/calib_imu_bench.py [--frames 200] [--no-twin] [--out FILE]

Prints one JSON record.  Stage times of the resident path are HIP events (lio_calib_imu_last_times: staging, frame filter, matcher, map update);
wall times are perf_counter around calls that end in a synchronise, uploads included.  The scans are made on the host before the device is
opened (worker processes that never touch it).  Nobody has measured either path before; the record says what was seen, no bar is set."""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lidar-slam-detection_amd", "python"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEP, STEP_DEG = (0.5, 0.0, 0.0), (0.0, 0.0, 1.8)


def pose_of(i):
    """an arc: 0.5 m along the heading per frame, the heading turning by 1.8 degrees"""
    import calib_imu_cases as CM

    T = np.eye(4)
    pos = np.array([0.0, -16.0, 1.8])
    for k in range(i):
        yaw = np.radians(STEP_DEG[2] * k)
        pos = pos + STEP[0] * np.array([np.cos(yaw), np.sin(yaw), 0.0])
    T[:3, :3] = CM.euler_R(0.0, 0.0, STEP_DEG[2] * i)
    T[:3, 3] = pos
    return T


def make(i):
    import calib_imu_cases as CM
    from lsd_amd import synth

    scene = synth.Scene(half=100.0, n_boxes=40, seed=1)
    T = pose_of(i)
    pts, _ = synth.make_scan(scene, T[:3, 3], CM.quat_xyzw_of_R(T[:3, :3]), seed=1000 + i)
    return pts


def stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), mean=float(v.mean()), first=float(v[0]), last=float(v[-1]), max=float(v.max())) if len(v) else {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--no-twin", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    t0 = time.perf_counter()
    with multiprocessing.get_context("fork").Pool(a.workers) as pool:
        scans = pool.map(make, range(a.frames + 1))
    gen_s = time.perf_counter() - t0
    import calib_imu_cases as CM
    from lsd_amd import lio

    c = lio.ImuCalib(0, 1 << 17, 1 << 24)
    st = dict(stage=[], filt=[], align=[], map_update=[], pose_wall=[], frame_wall=[], map_points=[], target_points=[])
    converged, prev = 0, np.eye(4)
    t_all = time.perf_counter()
    for i, pts in enumerate(scans):
        t0 = time.perf_counter()
        T = c.lidar_pose(pts)
        t1 = time.perf_counter()
        lt = c.last_times()
        if i == 0:
            continue  # the first call makes the map from the raw scan (and allocates)
        converged += int(not np.array_equal(T, np.eye(4)))
        c.add_frame(1_000_000 + 100_000 * i, T, np.linalg.inv(prev) @ T, pts)
        t2 = time.perf_counter()
        prev = T
        cn = c.counts()
        st["stage"].append(lt["stage_us"]); st["filt"].append(lt["filter_us"]); st["align"].append(lt["align_us"])
        st["map_update"].append(c.last_times()["map_update_us"])
        st["pose_wall"].append(1e3 * (t1 - t0)); st["frame_wall"].append(1e3 * (t2 - t1))
        st["map_points"].append(cn["map_points"]); st["target_points"].append(cn["target_points"])
    resident_s = time.perf_counter() - t_all
    err = float(np.linalg.norm((np.linalg.inv(pose_of(0)) @ pose_of(a.frames))[:3, 3] - T[:3, 3]))
    rec = dict(tool="calib_imu_bench", beams=64, azimuths=1875, key_frames=a.frames, points_per_scan=int(np.median([len(s) for s in scans])),
               converged=converged, last_pose_error_m=err, scan_generation_s=gen_s,
               resident=dict(total_s=resident_s, device_us=dict(stage=stats(st["stage"]), frame_filter=stats(st["filt"]), matcher=stats(st["align"]),
                                                                map_update=stats(st["map_update"])),
                             wall_ms=dict(lidar_pose=stats(st["pose_wall"]), add_frame=stats(st["frame_wall"])),
                             map_points_last=st["map_points"][-1], target_points_last=st["target_points"][-1]),
               not_taken="rocprofv3 kernel statistics; the reference's own time at this size")
    last_T = T
    c.close()
    if not a.no_twin:
        tw = CM.Twin(max_points=1 << 24, max_scan=1 << 17)
        pw, fw = [], []
        t_all = time.perf_counter()
        for i, pts in enumerate(scans):
            t0 = time.perf_counter()
            T = tw.lidar_pose(pts)
            t1 = time.perf_counter()
            if i == 0:
                continue
            tw.add_frame(pts, T)
            t2 = time.perf_counter()
            pw.append(1e3 * (t1 - t0)); fw.append(1e3 * (t2 - t1))
        rec["host_round_trips"] = dict(total_s=time.perf_counter() - t_all, wall_ms=dict(lidar_pose=stats(pw), add_frame=stats(fw)),
                                       same_last_pose=bool(np.array_equal(T, last_T)))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
