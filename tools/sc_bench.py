#!/usr/bin/env python
"""Times of the Scan Context bank (lio_sc_*, csrc/scancontext.hip) on one device:

  build    lio_sc_add_frames_host of 2 000 frames x 30 000 points (the map load): the wall clock of the call and the device time of its launch
           sets (upload + describe + finish) from lio_sc_last_times
  search   one lio_sc_global_search_host of a 30 000-point scan over that bank: the wall clock, and describe / ring-key search / distances from
           lio_sc_last_times (HIP events)

A warm-up, then the median of 3.  Writes profiles/sc_bench.json.  Beside the device's numbers goes the reference's own time per described frame
as tools/record_sc_golden.py measured it on the recording host (tests/golden/scancontext.npz) -- ANOTHER MACHINE, a CPU: a scale, not a race.
No threshold: the record is the result."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-slam-detection_amd", "python"))
from lsd_amd import lio  # noqa: E402

N_FRAMES, N_POINTS = 2000, 30_000


def main():
    rng = np.random.default_rng(1)
    base = np.concatenate([rng.normal(0, 30, (N_POINTS, 2)), rng.uniform(-1.5, 8, (N_POINTS, 1)), np.zeros((N_POINTS, 1))], 1).astype(np.float32)
    frames = []
    for k in range(N_FRAMES):  # every frame its own cloud: the base turned and thinned differently
        a = 2 * np.pi * k / N_FRAMES
        c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
        f = base.copy()
        f[:, 0], f[:, 1] = c * base[:, 0] - s * base[:, 1], s * base[:, 0] + c * base[:, 1]
        f[:, 2] *= np.float32(0.5 + (k % 7) / 7.0)
        frames.append(f)
    query = frames[N_FRAMES // 3] + np.array([0.3, -0.2, 0.0, 0.0], np.float32)
    sc = lio.ScanContext(max_frames=N_FRAMES, max_points_per_call=1 << 22)
    build, search = [], []
    for rep in range(4):
        sc.reset()
        t0 = time.perf_counter()
        sc.add_frames(frames)
        wall = time.perf_counter() - t0
        build.append(dict(wall_ms=wall * 1e3, device_ms=sc.last_times()["describe_us"] / 1e3))
        t0 = time.perf_counter()
        r = sc.global_search(query)
        wall = time.perf_counter() - t0
        t = sc.last_times()
        search.append(dict(wall_ms=wall * 1e3, describe_ms=t["describe_us"] / 1e3, ringkey_ms=t["ringkey_us"] / 1e3, distance_ms=t["distance_us"] / 1e3, match_id=r["match_id"],
                           score=r["score"]))
        print(rep, build[-1], search[-1], flush=True)
    med = lambda rows, k: float(np.median([x[k] for x in rows[1:]]))
    out = dict(frames=N_FRAMES, points_per_frame=N_POINTS,
               build={k: med(build, k) for k in ("wall_ms", "device_ms")},
               search={k: med(search, k) for k in ("wall_ms", "describe_ms", "ringkey_ms", "distance_ms")}, match_id=search[-1]["match_id"], score=search[-1]["score"])
    out["build"]["device_us_per_frame"] = out["build"]["device_ms"] * 1e3 / N_FRAMES
    gold = os.path.join(ROOT, "tests", "golden", "scancontext.npz")
    if os.path.exists(gold):
        g = np.load(gold)
        out["reference_on_the_recording_host"] = dict(describe_ms_per_frame=float(g["ref_describe_ms_per_frame"]), host=str(g["ref_host"]),
                                                       note="another machine (a CPU), ~34 000 points per frame: a scale, not a comparison")
    path = os.path.join(ROOT, "profiles", "sc_bench.json")
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
