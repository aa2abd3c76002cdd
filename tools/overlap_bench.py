"""Times one detect() call of the map merge (lio.OverlapDetector) for a fragment of 10 new key frames with 3 candidates each, beside the only way
the same coarse alignments could be done before: ten lio_loop_align_candidates calls of three sources each.  The key frames are the keyframer
bench's: 120 000-point synthetic scans downsampled at 0.2 m (about 38 000 points).  The reference map is a 16-frame drive, the fragment runs
beside it; the new map's graph is a chain of 30 whose frames 10-19 are the fragment, so that every frame of it is 10 levels deep.

  detect     the stages of lio_overlap_detect from lio_overlap_last_times (HIP events): gate, targets (voxel builds + pool copies), coarse (the
             one set of rounds), fitness, accumulate, fine; and the wall clock around the synchronous call
  baseline   per new frame one lio_loop_align_candidates over the pairs the gate let through, from the same guesses: the target build (which
             also builds the fitness index), the coarse batch and the fitness from lio_loop_last_times, summed over the ten calls
  ratios     like with like: baseline (target + coarse + fitness) over detect (targets + coarse + fitness) -- both sides then hold the voxel
             builds, the rounds, the exact index of every new frame and the fitness launch; above 1 the single batch is faster.  And the rounds
             alone: baseline coarse over detect coarse

A warm-up, then the median of 3.  Writes profiles/overlap_bench.json.  No threshold: the record is the result."""
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

N_REF, N_NEW = 16, 10


def pose_of(x, y, yaw):
    T = np.eye(4)
    T[:3, :3] = synth.quat_to_R(synth.quat_from_rotvec([0, 0, yaw]))
    T[:3, 3] = [x, y, 1.8]
    return T


def main():
    import oracle
    import overlap_cases as OC

    scene = synth.Scene(half=80.0, n_boxes=40, seed=2)
    rng = np.random.default_rng(1)

    def frame(T, seed):
        raw, _ = synth.make_scan(scene, T[:3, 3], synth.quat_from_rotvec([0, 0, np.arctan2(T[1, 0], T[0, 0])]), seed=seed)
        return oracle.voxel_downsample(np.ascontiguousarray(raw[:120_000, :4], np.float32), 0.2)

    ref_T = [pose_of(-15.0 + 2.0 * k, 0.0, 0.02 * k) for k in range(N_REF)]
    new_T = [pose_of(-9.0 + 2.0 * j, 1.0, 0.05) for j in range(N_NEW)]
    ref = [frame(T, 10 + k) for k, T in enumerate(ref_T)]
    print("reference frames done", flush=True)
    new = [frame(T, 100 + j) for j, T in enumerate(new_T)]
    print("fragment frames done", flush=True)
    new_est = [T @ pose_of(rng.normal() * 0.1, rng.normal() * 0.1, rng.normal() * 0.01) @ np.linalg.inv(pose_of(0, 0, 0)) for T in new_T]  # drifted estimates
    M = 1 << 16
    assert max(len(c) for c in ref + new) <= M
    ref_kf, chain = list(range(N_REF)), list(range(1000, 1030))
    new_kf = chain[10:20]
    edges = [(a, a + 1) for a in ref_kf[:-1]] + [(a, a + 1) for a in chain[:-1]]
    rec = dict(workload=dict(reference_frames=N_REF, fragment_frames=N_NEW, points=[len(c) for c in ref + new], resolution=0.2))

    d = lio.LoopDetector(max_points=M)
    o = lio.OverlapDetector(d)
    ref_b = [d.add_keyframe(c, T, 0.0) for c, T in zip(ref, ref_T)]
    new_b = [d.add_keyframe(c, T, 0.0) for c, T in zip(new, new_est)]
    pairs = {}

    def t_detect():
        t0 = time.perf_counter()
        found = o.detect(ref_b, new_b, edges, ref_kf=ref_kf, new_kf=new_kf)
        wall = (time.perf_counter() - t0) * 1e6
        t = o.last_times()
        reps = o.last_report()
        for r in reps:
            pairs[r["new_id"]] = [int(c) for c, ratio in zip(r["candidates"], r["gate_ratio"]) if ratio >= 0.2]
        assert all(len(r["candidates"]) == 3 for r in reps), [len(r["candidates"]) for r in reps]
        return dict(detect_wall_us=wall, candidates_us=t["candidates_us"], gate_us=t["gate_us"], targets_us=t["targets_us"], coarse_us=t["coarse_us"], fitness_us=t["fitness_us"],
                    accumulate_us=t["accumulate_us"], fine_us=t["fine_us"], coarse_rounds=t["coarse_rounds"], pairs=t["n_pairs"], targets=t["n_targets"], overlaps=len(found),
                    converged=int(sum(r["converged"].sum() for r in reps)))

    rec["detect"] = med(t_detect)
    print("detect", rec["detect"], flush=True)
    pose = {b: T for b, T in zip(ref_b + new_b, ref_T + new_est)}

    def t_baseline():
        tgt = coarse = fit = wall = 0.0
        conv = 0
        for nb in new_b:
            ids = pairs[nb]
            if not ids:
                continue
            g = [OC.make_guess(pose[nb], pose[c]) for c in ids]
            t0 = time.perf_counter()
            out = d.align_candidates(nb, ids, g)
            wall += (time.perf_counter() - t0) * 1e6
            t = d.last_times()
            tgt += t["target_us"]
            coarse += t["coarse_us"]
            fit += t["fitness_us"]
            conv += sum(r[1] for r in out)
        return dict(calls_wall_us=wall, target_us=tgt, coarse_us=coarse, fitness_us=fit, converged=conv)

    rec["baseline_ten_calls"] = med(t_baseline)
    b, t = rec["baseline_ten_calls"], rec["detect"]
    rec["coarse_stage_like_with_like_ratio"] = (b["target_us"] + b["coarse_us"] + b["fitness_us"]) / (t["targets_us"] + t["coarse_us"] + t["fitness_us"])
    rec["coarse_rounds_only_ratio"] = rec["baseline_ten_calls"]["coarse_us"] / rec["detect"]["coarse_us"]
    o.close()
    d.close()
    out = os.path.join(ROOT, "profiles", "overlap_bench.json")
    if len(sys.argv) > 1:
        out = sys.argv[1]
    json.dump(rec, open(out, "w"), indent=1)
    print(json.dumps(rec))


def med(f, runs=3):
    f()
    out = [f() for _ in range(runs)]
    return {k: float(np.median([o[k] for o in out])) for k in out[0]}


if __name__ == "__main__":
    main()
