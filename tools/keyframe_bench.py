"""Times the key-frame stages on the device (lio.KeyFramer) on one workload: a 120 000-point synthetic scan, resolution 0.2, a full
100 000-point local map.  Median of 3 runs after a warm-up per stage, beside the numpy / cKDTree restatement's time on the same data when
scipy is importable.  Writes profiles/keyframe_bench.json.  No threshold: the record is the result."""
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


def med(f, runs=3):
    f()
    out = []
    for _ in range(runs):
        out.append(f())
    return float(np.median(out))


def main():
    scene = synth.Scene(half=80.0, n_boxes=40, seed=2)
    pose = np.eye(4)
    pose[:3, 3] = [1.0, 0.5, 1.8]
    raw, _ = synth.make_scan(scene, pose[:3, 3], synth.quat_from_rotvec([0, 0, 0]), seed=3)
    raw = np.ascontiguousarray(raw[:120_000, :4], np.float32)
    stamps = np.linspace(0, 99_999, len(raw)).astype(np.uint32)
    world = scene.sample_surface(100_000, seed=4).astype(np.float32)
    world = np.concatenate([world[:, :3], np.ones((len(world), 1), np.float32)], 1)
    k = lio.KeyFramer(resolution=0.2, key_frame_distance=1.0)
    import oracle

    ds = oracle.voxel_downsample(raw, 0.2)
    rec = dict(workload=dict(scan_points=len(raw), downsampled=len(ds), resolution=0.2, local_map_points=len(world)), device_us={}, host_s={})

    def t_radius():
        k.radius_outlier(ds, 1.0, 3, key_frame_range=50.0)
        return k.last_times()["filters_us"]

    def t_ring():
        k.append_local_map(ds, pose)
        return k.last_times()["ring_us"]

    def t_fitness():
        k.fitness(ds, pose)
        return k.last_times()["fitness_us"]

    def t_push():
        k.reset()
        k.push(raw, stamps, 0, np.eye(4), delta=np.eye(4))
        k.append_local_map(world, np.eye(4))
        far = pose.copy()
        far[0, 3] += 3.0   # past 1.5 D: a candidate that is elected and emitted
        t0 = time.perf_counter()
        r = k.push(raw, stamps, 100_000, far, delta=np.eye(4))
        dt = time.perf_counter() - t0
        assert r["emitted"] == 1
        return dt * 1e6

    k.append_local_map(world, np.eye(4))
    rec["device_us"]["radius_and_range_filter"] = med(t_radius)
    rec["device_us"]["fitness"] = med(t_fitness)
    rec["device_us"]["ring_append_and_rebuild"] = med(t_ring)
    rec["wall_us_whole_push_with_emission"] = med(t_push)
    try:
        import scipy  # noqa: F401
        import keyframe_cases as kc

        t0 = time.perf_counter()
        kc.fitness(world, ds, pose, 1.0)
        rec["host_s"]["fitness_ckdtree_restatement"] = time.perf_counter() - t0
        from scipy.spatial import cKDTree

        t0 = time.perf_counter()
        tree = cKDTree(ds[:, :3].astype(np.float64))
        cnt = tree.query_ball_point(ds[:, :3].astype(np.float64), 1.0, return_length=True)
        rec["host_s"]["radius_filter_ckdtree_f64"] = time.perf_counter() - t0
        rec["host_s"]["note"] = "cKDTree counts in f64 (timing only; the f32 rule is the restatement's brute force); kept %d" % int((cnt > 3).sum())
    except ImportError:
        rec["host_s"]["note"] = "scipy is not importable here: no host comparison was made"
    k.close()
    out = os.path.join(ROOT, "profiles", "keyframe_bench.json")
    if len(sys.argv) > 1:
        out = sys.argv[1]
    json.dump(rec, open(out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
