#!/usr/bin/env python
"""Times of one operator's pose hint (lio_localmap_estimate_pose, csrc/localmap.hip) at the workload's size on one device: five key frames of
100 000 points near the hint, a 30 000-point scan as the source.

  device   the call itself: its wall clock and the stage times of its report (HIP events; the matcher's stages include the host side of the LM loop)
  host     the same answer the only way there was before the device entries: the key frames concatenated on the host, both mean heights taken
           on the host, lio_gicp_set_target / lio_gicp_set_source from host memory, then the same align and fitness score -- same GPU, same
           matcher, same guess rule (wall clock per stage)

A warm-up, then the median of 3 for every figure.  Writes profiles/estimate_pose_bench.json (--out for another place).  No ratio is demanded: the
record is the result.  NOT measured: the reference's own CPU path (PCL kd-tree, fast_gicp on the host), a map with more than five key frames in
reach (the call takes five at most), and the module's frame hand-over."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-slam-detection_amd", "python"))
from lsd_amd import capi, lio, synth  # noqa: E402

N_KEYFRAMES, N_KF_POINTS, N_SOURCE = 5, 100_000, 30_000
FOV = (-24.8, 2.0)


def _exactly(cloud, n, seed):
    assert len(cloud) >= n, (len(cloud), n)
    return np.ascontiguousarray(cloud[np.sort(np.random.default_rng(seed).permutation(len(cloud))[:n])])


def _hint(x, y, yaw):
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1], T[0, 3], T[1, 3] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), x, y
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimate_pose_bench.json"))
    args = ap.parse_args()
    scene = synth.Scene(half=100.0, n_boxes=40, seed=1)
    frames, positions = [], []
    for k in range(N_KEYFRAMES):
        pos = np.array([-4.0 + 2.0 * k, 0.2, 1.8])
        raw, _ = synth.make_scan(scene, pos, synth.quat_from_rotvec([0, 0, 0]), seed=700 + k, n_az=1800, fov_deg=FOV)
        raw = _exactly(raw, N_KF_POINTS, k)
        raw[:, :3] = (raw[:, :3].astype(np.float64) + pos).astype(np.float32)
        frames.append(raw)
        positions.append(pos.astype(np.float32))
    true_pos, true_yaw = np.array([0.3, 0.1, 1.8]), 0.02
    src, _ = synth.make_scan(scene, true_pos, synth.quat_from_rotvec([0, 0, true_yaw]), seed=800, n_az=600, fov_deg=FOV)
    src = _exactly(src, N_SOURCE, 9)
    hint = _hint(true_pos[0] + 0.2, true_pos[1] - 0.15, true_yaw + np.radians(2.0))

    lp, prm = capi.LoopParams(), capi.NdtParams()
    capi.lib().lio_loop_default_params(C.byref(lp))
    capi.lib().lio_estimate_matcher_params(C.byref(prm))
    lm = lio.LocalMap(max_total_points=N_KEYFRAMES * N_KF_POINTS + 16, max_local_points=200_000, max_keyframe_points=N_KF_POINTS)
    for f, p in zip(frames, positions):
        lm.add_keyframe(f, p)
    holder = lio.LocalMap(max_total_points=N_SOURCE + 16, max_local_points=8, max_keyframe_points=N_SOURCE)  # puts the scan in HBM, as the module's last frame is
    holder.add_keyframe(src, [0.0, 0.0, 0.0])
    holder.gather([0])
    holder.store_frame(0, *holder.gather_device())
    d_src, n_src = holder.frame(0)
    gd, gh = (lio.Gicp(lp.grid_resolution, N_KEYFRAMES * N_KF_POINTS, lp.k_correspondences) for _ in range(2))
    for g in (gd, gh):
        g.set_voxel_mode(lp.voxel_resolution, 1)
    align_kw = dict(rotation_epsilon_deg=prm.rotation_epsilon_deg, transformation_epsilon=prm.transformation_epsilon, max_iterations=prm.max_iterations,
                    max_process_time_ms=prm.max_process_time_ms)

    device, host = [], []
    for rep in range(4):
        t0 = time.perf_counter()
        out, r = lm.estimate_pose(gd, d_src, n_src, hint)
        wall = time.perf_counter() - t0
        row = dict(wall_ms=wall * 1e3, **{k[:-3] + "_ms": r[k] / 1e3 for k in ("nearest_us", "gather_us", "set_target_us", "set_source_us", "z_source_us", "align_us", "fitness_us")})
        row.update(result=r["result"], iterations=r["iterations"], score=r["score"], n_target=r["n_target"])
        device.append(row)

        t = [time.perf_counter()]
        ids, d2 = lm.nearest((hint[0, 3], hint[1, 3]), 5)
        target = np.concatenate([frames[int(i)] for i, d in zip(ids, d2) if d <= 400.0])
        guess = hint.copy()
        guess[2, 3] = float(np.mean(target[:, 2], dtype=np.float64)) - float(np.mean(src[:, 2], dtype=np.float64))
        guess = guess.astype(np.float32).astype(np.float64)
        t.append(time.perf_counter())
        gh.set_target(target)
        t.append(time.perf_counter())
        gh.set_source(src)
        t.append(time.perf_counter())
        T, conv, it = gh.align(guess, max_corr_dist=1.0, **align_kw)
        t.append(time.perf_counter())
        score = gh.fitness_score(T, lp.fitness_score_max_range)[0] if conv else 0.0
        t.append(time.perf_counter())
        d = np.diff(t) * 1e3
        host.append(dict(wall_ms=(t[-1] - t[0]) * 1e3, assemble_ms=d[0], set_target_ms=d[1], set_source_ms=d[2], align_ms=d[3], fitness_ms=d[4], iterations=it, score=score))
        print(rep, device[-1], host[-1], flush=True)

    med = lambda rows, k: float(np.median([x[k] for x in rows[1:]]))
    res = dict(keyframes=N_KEYFRAMES, points_per_keyframe=N_KF_POINTS, source_points=N_SOURCE, target_points=device[-1]["n_target"],
               device={k: med(device, k) for k in device[0] if k.endswith("_ms")}, host_path={k: med(host, k) for k in host[0] if k.endswith("_ms")},
               result=device[-1]["result"], iterations=dict(device=device[-1]["iterations"], host_path=host[-1]["iterations"]),
               score=dict(device=device[-1]["score"], host_path=host[-1]["score"]), position_error_m=float(np.linalg.norm(out[:3, 3] - true_pos)),
               not_measured=["the reference's own CPU path (PCL kd-tree search, fast_gicp on the host)", "the module's frame hand-over",
                             "more than five key frames within 20 m (the call takes five at most)"],
               note="the host path's z means are numpy's pairwise sums, the device's the chunked sum: the guesses differ in the last bits, so may the iterations")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
