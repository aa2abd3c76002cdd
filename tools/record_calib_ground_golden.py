#!/usr/bin/env python3
"""Records tests/golden/calib_ground.npz with the reference's own crop_points, fit_plane and align_points_to_xyplane
(calibration/lidar_calibration).  Runs on the CPU: no device is touched; needs the reference tree, numpy and scipy.

    python tools/record_calib_ground_golden.py [--reference /root/reference]

np.random.choice is wrapped while the reference runs, so every triple it drew (rejected ones included) is recorded; the plane of every
accepted triple comes from fit_plane(..., num_iteration=1) with that draw forced.  Per fit case <c>: <c>_points (n x 4 f32), <c>_polygon,
<c>_mask, <c>_triples, <c>_planes (NaN rows: the reference rejected the triple as colinear), <c>_best_coef, <c>_T.  `edges_*`: the crop alone.
`pq_*`, `ap_*`, `euler_*`, `rot_*`: the host functions.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import calib_ground_cases as CG  # noqa: E402


class Choice:
    """np.random.choice, recording what it returns or handing out a forced list"""

    def __init__(self):
        self.real, self.log, self.forced = np.random.choice, [], None

    def __call__(self, a, size=None, replace=True, p=None):
        if self.forced is not None:
            out = np.array(self.forced.pop(0))
        else:
            out = self.real(a, size, replace=replace, p=p)
        self.log.append([int(v) for v in out])
        return out


def floor(rng, n, half, tilt, noise, n_out):
    xy = rng.uniform(-half, half, (n, 2))
    z = -1.7 + tilt[0] * xy[:, 0] + tilt[1] * xy[:, 1] + rng.normal(0, noise, n)
    z[rng.choice(n, n_out, replace=False)] += rng.uniform(0.2, 1.5, n_out)
    return np.column_stack([xy, z, rng.uniform(0, 255, n)]).astype(np.float32)


def fit_cases():
    rng = np.random.default_rng(2026)
    concave = [[-6.0, -5.5], [7.0, -6.5], [7.5, 6.0], [0.5, 1.0], [-6.5, 5.0]]
    base = floor(rng, 3000, 10.0, (0.03, -0.02), 0.02, 480)
    early = floor(rng, 1500, 10.0, (-0.01, 0.02), 0.004, 60)
    skipped = floor(rng, 1200, 10.0, (0.02, 0.01), 0.01, 150)
    rep = rng.choice(len(skipped), 500, replace=False)  # enough repeated points that some draws hold one twice
    skipped[rep] = np.array([1.0, -2.0, -1.7, 9.0], np.float32)
    ties = np.zeros((90, 4), np.float32)  # an exact floor (z = x / 4) and a third of outliers: many accepted draws share the best count
    ties[:, :2] = rng.uniform(-3, 3, (90, 2)).astype(np.float32)
    ties[:, 2] = ties[:, 0] * np.float32(0.25)
    ties[::3, 2] += rng.uniform(0.5, 2.0, 30).astype(np.float32)
    square = [[-2.5, -2.5], [2.5, -2.5], [2.5, 2.5], [-2.5, 2.5]]
    return dict(base=(base, concave, 11), early=(early, concave, 12), skipped=(skipped, concave, 13), ties=(ties, square, 14))


def edge_case():
    """points on a quarter-unit lattice against an integer polygon with a horizontal and vertical edges: y equal to a vertex's y, x on an edge"""
    poly = [[0, 0], [4, 0], [4, 3], [2, 1], [0, 3]]
    g = np.arange(-1.0, 5.25, 0.25)
    xy = np.array([[x, y] for y in g for x in g])
    pts = np.column_stack([xy, np.zeros(len(xy)), np.ones(len(xy))]).astype(np.float32)
    return pts, poly


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=CG.GOLDEN)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.reference, "calibration"))
    import lidar_calibration as LC
    from lidar_calibration import calib, filter as flt, fit as fitmod

    out = {}
    choice = Choice()
    np.random.choice = choice
    try:
        for name, (pts, poly, seed) in fit_cases().items():
            np.random.seed(seed)
            choice.log, choice.forced = [], None
            T = LC.align_points_to_xyplane(pts.copy(), poly)
            triples = np.array(choice.log, np.uint32)
            xyz = pts[:, :3]
            mask = np.array([bool(flt.test_point_in_polygon(p, np.array(poly))) for p in xyz])
            crop = np.array(flt.crop_points(xyz, np.array(poly)))
            assert np.array_equal(crop, xyz[mask])
            choice.forced = [list(t) for t in triples]
            best = fitmod.fit_plane(crop, sigma=CG.SIGMA, num_iteration=CG.NUM_ITERATION, thresh=CG.THRESH)
            assert not choice.forced, "the replay consumed other draws than the run"
            assert best[2] > 0 and T[2, 3] == best[3] / best[2]
            pl = np.full((len(triples), 4), np.nan, np.float32)
            for j, t in enumerate(triples):
                if not fitmod.is_colinear(crop[t[0]], crop[t[1]], crop[t[2]]):
                    choice.forced = [list(t)]
                    coef = fitmod.fit_plane(crop, sigma=CG.SIGMA, num_iteration=1, thresh=CG.THRESH)
                    assert coef.any(), "a plane without an inlier"
                    pl[j] = coef.astype(np.float32)
                    assert np.array_equal(pl[j].astype(np.float64), coef)
            out.update({f"{name}_points": pts, f"{name}_polygon": np.array(poly, np.float64), f"{name}_mask": mask, f"{name}_triples": triples,
                        f"{name}_planes": pl, f"{name}_best_coef": best, f"{name}_T": T})
            # what the case is there for, by the restatement's counts
            r = CG.fit(crop, draws=triples)
            acc = r["counts"][~r["colinear"]]
            print(f"{name}: kept {mask.sum()} of {len(pts)}, {len(triples)} draws, skipped {r['skipped']}, early {r['early_exit']}, "
                  f"best {acc.max()} x{np.count_nonzero(acc == acc.max())}, restated best_coef equal: "
                  f"{np.array_equal(r['coef'].astype(np.float64), best)}")
            assert dict(base=not r["early_exit"] and len(triples) == 100, early=r["early_exit"], skipped=r["skipped"] > 0,
                        ties=not r["early_exit"] and np.count_nonzero(acc == acc.max()) > 1)[name]
    finally:
        np.random.choice = choice.real

    pts, poly = edge_case()
    out.update(edges_points=pts, edges_polygon=np.array(poly, np.float64),
               edges_mask=np.array([bool(flt.test_point_in_polygon(p, np.array(poly))) for p in pts[:, :3]]))
    print(f"edges: kept {out['edges_mask'].sum()} of {len(pts)}")

    rng = np.random.default_rng(7)
    pq = rng.uniform(-20, 20, (5, 4, 3))
    R, t = zip(*[calib.align_pq_to_known(*c) for c in pq])
    out.update(pq_in=pq, pq_R=np.array(R), pq_t=np.array(t))
    for i, m in enumerate((2, 3, 6)):
        p0 = rng.uniform(-20, 20, (m, 3))
        ang, sh = rng.uniform(-3, 3), rng.uniform(-5, 5, 2)
        p1 = p0.copy()
        p1[:, 0] = np.cos(ang) * p0[:, 0] - np.sin(ang) * p0[:, 1] + sh[0] + rng.normal(0, 0.01, m)
        p1[:, 1] = np.sin(ang) * p0[:, 0] + np.cos(ang) * p0[:, 1] + sh[1] + rng.normal(0, 0.01, m)
        out.update({f"ap{i}_p0": p0, f"ap{i}_p1": p1, f"ap{i}_T": calib.align_points(p0, p1)})
    # x y z roll pitch yaw, degrees; pitch (the middle angle) kept away from +-90: no gimbal lock
    eul = np.column_stack([rng.uniform(-5, 5, (8, 3)), rng.uniform(-179, 179, 8), rng.uniform(-80, 80, 8), rng.uniform(-179, 179, 8)])
    eul[0, 3:] = 0.0
    out.update(euler_in=eul, euler_T=np.array([LC.xyzrpy_to_transform(list(e)) for e in eul]),
               euler_rot=np.array([LC.xyzrpy_to_rt(list(e))[0] for e in eul]),
               euler_back=np.array([LC.rt_to_xyzrpy(*LC.xyzrpy_to_rt(list(e))) for e in eul]))
    v = rng.normal(0, 1, (6, 2, 3))
    out.update(rot_in=v, rot_R=np.array([calib.calc_rot_from(p[0], p[1]) for p in v]))
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
