#!/usr/bin/env python
"""Detection boxes on one MI355X: the fused post-process (lio.Boxes.postprocess: filter, order, prepare, mask, sweep, gather; csrc/boxes.hip) at
N = 2048 candidates of which about 250 are kept, and the tracker's GIoU3D matrix (lio.Boxes.pairwise) at 256 x 256, each beside the vectorised
numpy restatement of tests/boxes_cases.py on the same input and host (numpy's own threads, at most 16).  The reference itself is not timed
here and nothing of it is read.

    python tools/boxes_bench.py [--n 2048] [--clusters 12] [--repeats 200] [--warmup 20] [--no-cpu] [--out FILE]

Prints one JSON record.  Device times come from HIP events on the handle's stream (lio_boxes_last_times): filter + order, prepare + mask,
sweep, and first launch to last; medians and minima over the repeats after the warm-up calls (the first allocates).  Wall times are
perf_counter around calls that end in a stream synchronise, uploads and the one download included.  There is no pass / fail threshold."""
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

CLASS_THRESH = [0.10, 0.10, 0.10, 0.10]
NMS_THRESH, POST_MAX = 0.25, 256


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)))


def restated_postprocess(bc, b, s, lab):
    """tests/boxes_cases.py's postprocess with the IoU matrix built 64 rows at a time (the pair arrays of 2048 x 2048 at once do not fit a
    cache, nor comfortably a host)"""
    idx = np.flatnonzero(bc.passes(s, lab, CLASS_THRESH))
    order = idx[bc.stable_order(s[idx])]
    ob = b[order]
    iou = np.concatenate([bc.pairwise(ob[r:r + 64], ob, ("iou_bev",))["iou_bev"] for r in range(0, len(ob), 64)]) if len(ob) else np.zeros((0, 0))
    return order[bc.nms_from_iou(iou, NMS_THRESH, None, POST_MAX)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--clusters", type=int, default=12)
    ap.add_argument("--pair", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import boxes_cases as bc
    from lsd_amd import lio

    b = bc.clustered(a.seed, a.n, clusters=a.clusters, span=120.0)
    s, lab = bc.scored(a.seed, a.n)
    # detections against tracks: the same boxes moved a little, as a tracker's predictions lie beside the next frame's detections
    da = bc.clustered(a.seed + 1, a.pair, clusters=24, span=60.0)
    r = np.random.default_rng(a.seed + 2)
    db = (da + np.column_stack([r.normal(0, 0.3, (a.pair, 2)), r.normal(0, 0.05, (a.pair, 4)), r.normal(0, 0.05, a.pair)])).astype(np.float32)[r.permutation(a.pair)]
    bx = lio.Boxes(max(a.n, a.pair))
    order, mask, sweep, total, wall = [], [], [], [], []
    for k in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        out = bx.postprocess(b, s, lab, CLASS_THRESH, NMS_THRESH, POST_MAX)
        t1 = time.perf_counter()
        if k >= a.warmup:
            o, m, w, t = bx.last_times()
            order.append(o); mask.append(m); sweep.append(w); total.append(t); wall.append(1e6 * (t1 - t0))
    kept = bx.last_indices()
    passing = int(bc.passes(s, lab, CLASS_THRESH).sum())
    ptotal, pwall = [], []
    for k in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        gi = bx.pairwise(da, db, what=("giou3d",))["giou3d"]
        t1 = time.perf_counter()
        if k >= a.warmup:
            ptotal.append(bx.last_times()[3]); pwall.append(1e6 * (t1 - t0))
    rec = dict(tool="boxes_bench", n=a.n, clusters=a.clusters, seed=a.seed, passing=passing, kept=int(len(kept)), post_max=POST_MAX, nms_thresh=NMS_THRESH,
               repeats=a.repeats, warmup=a.warmup,
               postprocess_device_us=dict(filter_order=stats(order), prepare_mask=stats(mask), sweep=stats(sweep), first_launch_to_last=stats(total)),
               postprocess_wall_us=stats(wall),
               giou3d=dict(shape=[a.pair, a.pair], overlapping_pairs=int((bx.pairwise(da, db, what=("overlap",))["overlap"] > 0).sum()), device_us=stats(ptotal), wall_us=stats(pwall)),
               not_taken="rocprofv3 kernel statistics; the reference's own time at these sizes")
    if not a.no_cpu:
        t0 = time.perf_counter()
        keep = restated_postprocess(bc, b, s, lab)
        t1 = time.perf_counter()
        ref = bc.pairwise(da, db, ("giou3d",))["giou3d"]
        t2 = time.perf_counter()
        rec["numpy_restatement_run_once"] = dict(postprocess_s=t1 - t0, same_kept=bool(np.array_equal(keep, kept)), giou3d_s=t2 - t1,
                                                 giou3d_largest_difference=float(np.abs(ref - gi).max()), threads=os.environ["OMP_NUM_THREADS"])
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
