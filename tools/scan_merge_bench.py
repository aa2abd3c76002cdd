#!/usr/bin/env python
"""Stage times of one merge of 6 x 120 000 points on one device (lio_scan_merge_*, csrc/scanmerge.hip): the uploads and the merge itself
(count + scan + write + the count's read-back) from lio_scan_merge_last_times (HIP events), the download, and the wall clock of the call --
next to the numpy restatement of tests/rtk_cases.py on the host.  A warm-up, then the median of 3.  Writes profiles/scan_merge_bench.json.
The restatement is numpy on one core of whatever host this runs on: a scale, not a race.  No threshold: the record is the result."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "lidar-slam-detection_amd", "python"), os.path.join(ROOT, "tests")]
import rtk_cases as R  # noqa: E402
from lsd_amd import lio  # noqa: E402

N_CLOUDS, N_POINTS, PERIOD = 6, 120_000, 100_000


def main():
    rng = np.random.default_rng(1)
    clouds, stamps, headers = [], [], []
    for l in range(N_CLOUDS):
        p = np.concatenate([rng.uniform(-80, 80, (N_POINTS, 3)), rng.uniform(0, 255, (N_POINTS, 1))], 1).astype(np.float32)
        clouds.append(p), stamps.append(np.sort(rng.integers(0, PERIOD + 1, N_POINTS)).astype(np.uint32)), headers.append((1 << 40) + (l - 2) * 4000)
    T = R.transform_from_rpyt(1.0, 0.5, 1.2, 3.0, 1.0, -2.0)
    m = lio.ScanMerge(max_clouds=N_CLOUDS, max_points=N_CLOUDS * N_POINTS)
    m.set_transform(T)
    rows = []
    for rep in range(4):
        t0 = time.perf_counter()
        n, kept, early, late = m.run(clouds, stamps, headers, PERIOD)
        wall = time.perf_counter() - t0
        up, merge = m.last_times()
        t0 = time.perf_counter()
        pts, st = m.download()
        down = time.perf_counter() - t0
        rows.append(dict(run_wall_ms=wall * 1e3, upload_ms=up / 1e3, merge_ms=merge / 1e3, download_wall_ms=down * 1e3))
        print(rep, rows[-1], flush=True)
    host = []
    for rep in range(4):
        t0 = time.perf_counter()
        want = R.merge_points(clouds, stamps, headers, PERIOD, T)
        host.append((time.perf_counter() - t0) * 1e3)
    same = bool(np.array_equal(pts.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(st, want[1]))
    med = lambda k: float(np.median([x[k] for x in rows[1:]]))
    out = dict(clouds=N_CLOUDS, points_per_cloud=N_POINTS, points_out=int(n), kept=[int(x) for x in kept], early=[int(x) for x in early], late=[int(x) for x in late],
               device={k: med(k) for k in rows[0]}, numpy_restatement_on_this_host_ms=float(np.median(host[1:])), identical_to_the_restatement=same,
               bytes_moved_by_the_kernels=int(N_CLOUDS * N_POINTS * (4 + 16 + 4) + n * 20),
               note="merge_ms = count + scan + write kernels and the read-back of the count; upload_ms = 12 host-to-device copies from pageable memory")
    out["merge_gb_per_s"] = out["bytes_moved_by_the_kernels"] / (out["device"]["merge_ms"] * 1e-3) / 1e9
    path = os.path.join(ROOT, "profiles", "scan_merge_bench.json")
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
