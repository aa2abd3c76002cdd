#!/usr/bin/env python
"""texture_mesh on one MI355X: a seeded synthetic coloured surface (the ground-plus-boxes scene of lsd_amd.synth, random colours, a few hundred
outlier points 5 km out) and mesh vertices jittered onto it, 1 % of them displaced 5-50 m off it ("bubbles").

    python tools/texture_mesh_bench.py [--points 20000000] [--vertices 2000000] [--outliers 300] [--no-cpu] [--no-files] [--out FILE]

Prints one JSON record:
  - device: lio_knn_index build and colour (k = 3) in microseconds from HIP events (lio_knn_index_last_times; no host copies), median of
    --reps; the colour pass for the on-surface vertices alone and for all of them (bubbles included);
  - texture_mesh: its wall time on the PCD / OBJ written here, and the split measured through the module's own pieces (_read_rgb_pcd,
    _read_obj, the device pass with its copies, _write_mesh_ply);
  - cpu_baseline: scipy.spatial.cKDTree build + query(k=3, workers=16) on the same data."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-slam-detection_amd", "python"))


def make_data(n_points, n_vertices, n_out=300, seed=21):
    from lsd_amd import synth

    rng = np.random.default_rng(seed)
    scene = synth.Scene(half=100.0, n_boxes=40, seed=1)
    P = np.empty((n_points, 3), np.float32)
    P[: n_points - n_out] = scene.sample_surface(n_points - n_out, seed=seed + 1, sigma=0.01)[:, :3]
    d = rng.normal(size=(n_out, 3))
    P[n_points - n_out:] = (d / np.linalg.norm(d, axis=1, keepdims=True) * 5000.0).astype(np.float32)
    P = P[rng.permutation(n_points)]
    rgb = rng.integers(0, 1 << 24, n_points).astype(np.uint32)
    V = scene.sample_surface(n_vertices, seed=seed + 2, sigma=0.02)[:, :3].copy()
    nb = n_vertices // 100
    b = rng.choice(n_vertices, nb, replace=False)
    u = rng.normal(size=(nb, 3))
    V[b] += (u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(5, 50, (nb, 1))).astype(np.float32)
    on = np.ones(n_vertices, bool)
    on[b] = False
    return P, rgb, V, on


def write_files(d, P, rgb, V):
    pcd, obj = os.path.join(d, "cloud.pcd"), os.path.join(d, "mesh.obj")
    with open(pcd, "wb") as f:
        f.write(("VERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\n"
                 f"WIDTH {len(P)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(P)}\nDATA binary\n").encode())
        rec = np.empty((len(P), 4), np.float32)
        rec[:, :3] = P
        rec[:, 3] = rgb.view(np.float32)
        f.write(rec.tobytes())
    nf = len(V) // 3
    with open(obj, "w") as f:
        f.write("".join("v %r %r %r\n" % (float(a), float(b), float(c)) for a, b, c in V))
        f.write("".join("f %d %d %d\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3) for i in range(nf)))
    return pcd, obj, nf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--vertices", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--outliers", type=int, default=300)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-files", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    from lsd_amd import lio

    P, rgb, V, on = make_data(a.points, a.vertices, a.outliers)
    rec = {"points": a.points, "vertices": a.vertices, "bubbles": int((~on).sum()), "outliers": a.outliers, "k": 3}
    x = lio.KnnIndex()
    builds, q_on, q_all, walls = [], [], [], []
    for _ in range(a.reps):
        t = time.perf_counter()
        nf = x.build(P, rgb)
        walls.append(time.perf_counter() - t)
        builds.append(x.last_times()[0])
        x.colour(V[on], 3)
        q_on.append(x.last_times()[1])
        x.colour(V, 3)
        q_all.append(x.last_times()[1])
    rec["n_finite"] = nf
    rec["device"] = {"build_us": float(np.median(builds)), "colour_on_surface_us": float(np.median(q_on)), "colour_all_us": float(np.median(q_all)),
                     "bubble_cost_ratio": float(np.median(q_all) / np.median(q_on)), "build_wall_s_with_upload": float(np.median(walls)),
                     "build_us_all": builds, "colour_all_us_all": q_all}
    if not a.no_files:
        import slam_wrapper

        with tempfile.TemporaryDirectory() as d:
            pcd, obj, nfaces = write_files(d, P, rgb, V)
            t0 = time.perf_counter()
            slam_wrapper.texture_mesh(obj, pcd, d)
            t1 = time.perf_counter()
            xyz, c = slam_wrapper._read_rgb_pcd(pcd)
            t2 = time.perf_counter()
            v, faces = slam_wrapper._read_obj(obj)
            t3 = time.perf_counter()
            y = lio.KnnIndex()
            y.build(xyz, c)
            col = y.colour(v, 3)
            t4 = time.perf_counter()
            slam_wrapper._write_mesh_ply(os.path.join(d, "again.ply"), v, col, faces)
            t5 = time.perf_counter()
            same = open(os.path.join(d, "again.ply"), "rb").read() == open(os.path.join(d, "texture_mesh.ply"), "rb").read()
        rec["texture_mesh"] = {"wall_s": t1 - t0, "faces": nfaces, "split_s": {"pcd_read": t2 - t1, "obj_read": t3 - t2, "device_with_copies": t4 - t3,
                                                                              "ply_write_with_face_list_conversion": t5 - t4},
                               "pieces_reproduce_the_file": bool(same)}
    if not a.no_cpu:
        from scipy.spatial import cKDTree

        t0 = time.perf_counter()
        tree = cKDTree(P)
        t1 = time.perf_counter()
        tree.query(V, k=3, workers=16)
        t2 = time.perf_counter()
        rec["cpu_baseline"] = {"what": "scipy.spatial.cKDTree(points) + query(vertices, k=3, workers=16)", "build_s": t1 - t0, "query_s": t2 - t1}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
