"""Times loop detection for ONE new key frame against K = 16 candidates (lio.LoopDetector) beside the same coarse alignments done one after the
other with the single-pair matcher.  The key frame is the keyframer bench's: a 120 000-point synthetic scan downsampled at 0.2 m; the candidates
are scans of the same scene from poses around it.

  detect        the whole lio_loop_detect call for the new frame (wall clock around the synchronous call) and its stages from lio_loop_last_times
                (HIP events): target build, coarse batch, fitness, fine step; bank insert from the insert of the new frame
  (a) baseline  K sequential lio.Gicp voxel-mode alignments (set_voxel_mode(1.0, 1), epsilons 0.1 / 0.1), each with its set_source, against one
                set_target: the code path as it was before the batch existed.  Wall clock around synchronous calls (that path records no events).
  (b) reference RefVgicp on 4 threads on the same pairs, where oracle/_ref/libref_gicp.so is present

A warm-up, then the median of 3.  Writes profiles/loop_bench.json.  No threshold: the record is the result."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-slam-detection_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from lsd_amd import lio, synth  # noqa: E402

K = 16


def med(f, runs=3):
    f()
    out = [f() for _ in range(runs)]
    return {k: float(np.median([o[k] for o in out])) for k in out[0]}


def pose_of(x, y, yaw):
    T = np.eye(4)
    T[:3, :3] = synth.quat_to_R(synth.quat_from_rotvec([0, 0, yaw]))
    T[:3, 3] = [x, y, 1.8]
    return T


def main():
    import oracle
    import loop_cases as LC

    scene = synth.Scene(half=80.0, n_boxes=40, seed=2)
    rng = np.random.default_rng(1)

    def frame(T, seed):
        raw, _ = synth.make_scan(scene, T[:3, 3], synth.quat_from_rotvec([0, 0, np.arctan2(T[1, 0], T[0, 0])]), seed=seed)
        return oracle.voxel_downsample(np.ascontiguousarray(raw[:120_000, :4], np.float32), 0.2)

    Tn = pose_of(1.0, 0.5, 0.0)
    new = frame(Tn, 3)
    poses = [pose_of(1.0 + rng.uniform(-3, 3), 0.5 + rng.uniform(-3, 3), rng.uniform(-0.3, 0.3)) for _ in range(K)]
    cands = [frame(T, 10 + k) for k, T in enumerate(poses)]
    est = [T @ pose_of(rng.normal() * 0.1, rng.normal() * 0.1, rng.normal() * 0.01) @ np.linalg.inv(pose_of(0, 0, 0)) for T in poses]  # drifted estimates
    guesses = [LC.make_guess(Tn, e) for e in est]
    M = 1 << 16
    assert max(len(new), *(len(c) for c in cands)) <= M
    rec = dict(workload=dict(new_frame_points=len(new), candidates=K, candidate_points=[len(c) for c in cands], resolution=0.2))

    d = lio.LoopDetector(max_points=M)

    def t_detect():
        d.reset()
        for k, c in enumerate(cands):
            d.add_keyframe(c, est[k], 2.0 * k)
        d.detect()
        d.add_keyframe(new, Tn, 100.0)
        t_ins = d.last_times()["insert_us"]
        t0 = time.perf_counter()
        loops = d.detect()
        wall = (time.perf_counter() - t0) * 1e6
        r = d.last_report()
        assert len(r["candidates"]) == K, len(r["candidates"])
        t = d.last_times()
        return dict(detect_wall_us=wall, bank_insert_us=t_ins, target_us=t["target_us"], coarse_batch_us=t["coarse_us"], fitness_us=t["fitness_us"], fine_us=t["fine_us"],
                    loops=len(loops), coarse_rounds=r["coarse_rounds"], converged=int(r["converged"].sum()))

    rec["detect"] = med(t_detect)

    def t_stage_door():
        ids = list(range(K))
        t0 = time.perf_counter()
        d.align_candidates(K, ids, guesses)
        return dict(align_candidates_wall_us=(time.perf_counter() - t0) * 1e6, coarse_batch_us=d.last_times()["coarse_us"])

    rec["stage_door"] = med(t_stage_door)
    d.close()

    g = lio.Gicp(grid_resolution=1.0, max_points=M, k=20)
    g.set_voxel_mode(1.0, 1)

    def t_single():
        t0 = time.perf_counter()
        g.set_target(new)
        t1 = time.perf_counter()
        conv = 0
        for c, gs in zip(cands, guesses):
            g.set_source(c)
            conv += g.align(gs, transformation_epsilon=0.1, rotation_epsilon_deg=0.1)[1]
        t2 = time.perf_counter()
        return dict(set_target_wall_us=(t1 - t0) * 1e6, sequential_alignments_wall_us=(t2 - t1) * 1e6, converged=conv)

    rec["baseline_single_pair"] = med(t_single)
    g.close()
    rec["batch_vs_baseline"] = rec["baseline_single_pair"]["sequential_alignments_wall_us"] / rec["stage_door"]["align_candidates_wall_us"]

    import ref_gicp

    if ref_gicp.available():
        def t_ref():
            m = ref_gicp.RefVgicp(k=20, resolution=1.0, search_method=1, transformation_epsilon=0.1, rotation_epsilon=0.1, max_iterations=64, num_threads=4)
            m.set_target(new)
            t0 = time.perf_counter()
            for c, gs in zip(cands, guesses):
                m.set_source(c)
                m.align(gs.astype(np.float32))
            dt = (time.perf_counter() - t0) * 1e6
            m.close()
            return dict(sequential_alignments_wall_us=dt)

        rec["reference_vgicp_4_threads"] = med(t_ref, runs=3)
    else:
        rec["reference_vgicp_4_threads"] = "oracle/_ref/libref_gicp.so is not built here"
    out = os.path.join(ROOT, "profiles", "loop_bench.json")
    if len(sys.argv) > 1:
        out = sys.argv[1]
    json.dump(rec, open(out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
