"""The detection boxes' rules restated in numpy f32, vectorised over pairs, and the seeded scenes of their tests.

box_overlap, box_union and iou_bev follow the reference's iou3d_cpu.cpp operation by operation (every product, sum and quotient is its own f32
numpy operation, so nothing is contracted); the polygon's ordering step is a stable sort on np.arctan2 in f32 (the reference's bubble sort
swaps on `>` alone, so it is stable).  The mask, the sweep, the AABB gate of nms_cpu, the filter, the stable score order and the GIoU3D formula
of iou3d_nms.py are restated beside them.  numpy's f32 cos / sin / arctan2 are neither glibc's nor the device's: results agree with either to
what last-bit differences of the three move (the spreads tools/record_boxes_golden.py measures and stores in tests/golden/boxes.npz).
"""
import os

import numpy as np

F = np.float32
EPS = F(1e-8)
MARGIN = F(1e-2)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boxes.npz")
ALLOWANCE_FACTOR = 8  # allowance = 8 x the recorded spread: device functions a few ULP off instead of half an ULP


# ---- per-box ---------------------------------------------------------------------------------------------------------------------------------
def corners(boxes):
    """(N, 4, 2): the corners rotated about the centre (rotate_around_center)"""
    b = np.asarray(boxes, F).reshape(-1, 7)
    x, y, dx, dy, h = b[:, 0], b[:, 1], b[:, 3], b[:, 4], b[:, 6]
    dxh, dyh = dx / F(2), dy / F(2)
    x1, y1, x2, y2 = x - dxh, y - dyh, x + dxh, y + dyh
    c, s = np.cos(h), np.sin(h)
    out = np.zeros((len(b), 4, 2), F)
    for k, (px, py) in enumerate(((x1, y1), (x2, y1), (x2, y2), (x1, y2))):
        out[:, k, 0] = (px - x) * c + (py - y) * (-s) + x
        out[:, k, 1] = (px - x) * s + (py - y) * c + y
    return out


def _cross3(p1, p2, p0):
    return (p1[..., 0] - p0[..., 0]) * (p2[..., 1] - p0[..., 1]) - (p2[..., 0] - p0[..., 0]) * (p1[..., 1] - p0[..., 1])


def _cross2(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def _min(a, b):
    return np.where(a > b, b, a)


def _max(a, b):
    return np.where(a > b, a, b)


def _intersection(p1, p0, q1, q0):
    """intersection(): (flag (P,), ans (P, 2))"""
    rc = ((_min(p0[:, 0], p1[:, 0]) <= _max(q0[:, 0], q1[:, 0])) & (_min(q0[:, 0], q1[:, 0]) <= _max(p0[:, 0], p1[:, 0])) &
          (_min(p0[:, 1], p1[:, 1]) <= _max(q0[:, 1], q1[:, 1])) & (_min(q0[:, 1], q1[:, 1]) <= _max(p0[:, 1], p1[:, 1])))
    s1, s2, s3, s4 = _cross3(q0, p1, p0), _cross3(p1, q1, p0), _cross3(p0, q1, q0), _cross3(q1, p1, q0)
    flag = rc & (s1 * s2 > 0) & (s3 * s4 > 0)
    s5 = _cross3(q1, p1, p0)
    with np.errstate(all="ignore"):
        ax = (s5 * q0[:, 0] - s1 * q1[:, 0]) / (s5 - s1)
        ay = (s5 * q0[:, 1] - s1 * q1[:, 1]) / (s5 - s1)
        a0, b0, c0 = p0[:, 1] - p1[:, 1], p1[:, 0] - p0[:, 0], p0[:, 0] * p1[:, 1] - p1[:, 0] * p0[:, 1]
        a1, b1, c1 = q0[:, 1] - q1[:, 1], q1[:, 0] - q0[:, 0], q0[:, 0] * q1[:, 1] - q1[:, 0] * q0[:, 1]
        D = a0 * b1 - a1 * b0
        bx, by = (b0 * c1 - b1 * c0) / D, (a1 * c0 - a0 * c1) / D
    first = np.abs(s5 - s1) > EPS
    return flag, np.stack([np.where(first, ax, bx), np.where(first, ay, by)], axis=1).astype(F)


def _in_box2d(box, p):
    """check_in_box2d(): box (P, 7), p (P, 2)"""
    cx, cy = box[:, 0], box[:, 1]
    c, s = np.cos(-box[:, 6]), np.sin(-box[:, 6])
    rx = (p[:, 0] - cx) * c + (p[:, 1] - cy) * (-s)
    ry = (p[:, 0] - cx) * s + (p[:, 1] - cy) * c
    return (np.abs(rx) < box[:, 3] / F(2) + MARGIN) & (np.abs(ry) < box[:, 4] / F(2) + MARGIN)


def _fan(pts, cnt):
    """the fan area from point 0 over the first cnt points of each row, summed in order"""
    area = np.zeros(len(pts), F)
    p0 = pts[:, 0]
    for k in range(pts.shape[1] - 1):
        term = _cross2(pts[:, k] - p0, pts[:, k + 1] - p0)
        area = np.where(k < cnt - 1, area + term, area).astype(F)
    return (np.abs(area) / F(2)).astype(F)


# ---- per-pair --------------------------------------------------------------------------------------------------------------------------------
def box_overlap(a, b):
    """box_overlap() over P pairs: a, b (P, 7) -> (P,) f32"""
    a, b = np.asarray(a, F).reshape(-1, 7), np.asarray(b, F).reshape(-1, 7)
    P = len(a)
    if P == 0:
        return np.zeros(0, F)
    A, B = corners(a), corners(b)
    A, B = np.concatenate([A, A[:, :1]], axis=1), np.concatenate([B, B[:, :1]], axis=1)
    pts, cnt, total = np.zeros((P, 16, 2), F), np.zeros(P, np.int64), np.zeros((P, 2), F)
    rows = np.arange(P)

    def push(flag, p):
        nonlocal total
        assert not (flag & (cnt >= 16)).any(), "more than 16 polygon points"
        idx = rows[flag]
        pts[idx, cnt[idx]] = p[idx]
        total = np.where(flag[:, None], total + p, total).astype(F)
        cnt[idx] += 1

    for i in range(4):
        for j in range(4):
            push(*_intersection(A[:, i + 1], A[:, i], B[:, j + 1], B[:, j]))
    for k in range(4):
        push(_in_box2d(a, B[:, k]), B[:, k])
        push(_in_box2d(b, A[:, k]), A[:, k])
    with np.errstate(all="ignore"):
        centre = (total / cnt.astype(F)[:, None]).astype(F)
        key = np.arctan2(pts[:, :, 1] - centre[:, 1:2], pts[:, :, 0] - centre[:, 0:1]).astype(F)
    key = np.where(np.arange(16)[None, :] < cnt[:, None], key, np.inf)
    order = np.argsort(key, axis=1, kind="stable")
    pts = np.take_along_axis(pts, order[:, :, None], axis=1)
    return np.where(cnt > 0, _fan(pts, cnt), F(0)).astype(F)


def _point_lt(a, b):
    return np.where(a[:, 0] == b[:, 0], a[:, 1] >= b[:, 1], a[:, 0] >= b[:, 0])


def box_union(a, b):
    """box_union() over P pairs: the area of the convex hull of the eight corners"""
    a, b = np.asarray(a, F).reshape(-1, 7), np.asarray(b, F).reshape(-1, 7)
    P = len(a)
    if P == 0:
        return np.zeros(0, F)
    T = np.concatenate([corners(a), corners(b)], axis=1)
    for k in range(8):
        for i in range(8 - k - 1):
            sw = _point_lt(T[:, i], T[:, i + 1])
            lo, hi = np.where(sw[:, None], T[:, i + 1], T[:, i]), np.where(sw[:, None], T[:, i], T[:, i + 1])
            T[:, i], T[:, i + 1] = lo, hi
    rows = np.arange(P)
    pos, hull, used = np.ones(P, np.int64), np.zeros((P, 9), np.int64), np.zeros((P, 8), bool)

    def pops(k, floor, active):
        while True:
            top, below = hull[rows, np.maximum(pos - 1, 0)], hull[rows, np.maximum(pos - 2, 0)]
            pop = active & (pos > floor) & (_cross3(T[rows, top], T[:, k], T[rows, below]) <= 0)
            if not pop.any():
                return
            used[rows[pop], top[pop]] = False
            pos[pop] -= 1

    def put(k, active):
        idx = rows[active]
        used[idx, k] = True
        hull[idx, pos[idx]] = k
        pos[idx] += 1

    everyone = np.ones(P, bool)
    for k in range(1, 8):
        pops(k, 1, everyone)
        put(k, everyone)
    m = pos.copy()
    for k in range(6, -1, -1):
        active = ~used[:, k]
        pops(k, m, active)
        put(k, active)
    pos -= 1
    pts = T[rows[:, None], hull[:, :8]]
    return _fan(pts, pos)


def iou_from_overlap(a, b, overlap):
    sa, sb = a[:, 3] * a[:, 4], b[:, 3] * b[:, 4]
    return (overlap / np.maximum(sa + sb - overlap, EPS)).astype(F)


def _pairs(a, b):
    a, b = np.asarray(a, F).reshape(-1, 7), np.asarray(b, F).reshape(-1, 7)
    return np.repeat(a, len(b), axis=0), np.tile(b, (len(a), 1)), (len(a), len(b))


def giou3d_from(a, b, overlaps_bev, convexhull_bev):
    """boxes_giou3d_gpu of iou3d_nms.py from the two BEV matrices, operation for operation in f32"""
    a, b = np.asarray(a, F).reshape(-1, 7), np.asarray(b, F).reshape(-1, 7)
    a_max, a_min = (a[:, 2] + a[:, 5] / 2).reshape(-1, 1), (a[:, 2] - a[:, 5] / 2).reshape(-1, 1)
    b_max, b_min = (b[:, 2] + b[:, 5] / 2).reshape(1, -1), (b[:, 2] - b[:, 5] / 2).reshape(1, -1)
    overlaps_h = np.clip(np.minimum(a_max, b_max) - np.maximum(a_min, b_min), 0, None)
    unions_h = np.clip(np.maximum(a_max, b_max) - np.minimum(a_min, b_min), 0, None)
    overlaps_3d = overlaps_bev * overlaps_h
    convexhull_3d = np.clip(convexhull_bev * unions_h, F(1e-6), None)
    vol_a, vol_b = (a[:, 3] * a[:, 4] * a[:, 5]).reshape(-1, 1), (b[:, 3] * b[:, 4] * b[:, 5]).reshape(1, -1)
    unions_3d = np.clip(vol_a + vol_b - overlaps_3d, F(1e-6), None)
    with np.errstate(all="ignore"):
        out = overlaps_3d / unions_3d - (convexhull_3d - unions_3d) / convexhull_3d
    assert out.dtype == F
    return out


def pairwise(a, b, what=("overlap", "hull", "iou_bev", "giou3d")):
    """dict of (N, M) f32 matrices"""
    pa, pb, shape = _pairs(a, b)
    out = {}
    need_ov = any(w in what for w in ("overlap", "iou_bev", "giou3d"))
    need_hull = any(w in what for w in ("hull", "giou3d"))
    ov = box_overlap(pa, pb) if need_ov else None
    hu = box_union(pa, pb) if need_hull else None
    if "overlap" in what:
        out["overlap"] = ov.reshape(shape)
    if "hull" in what:
        out["hull"] = hu.reshape(shape)
    if "iou_bev" in what:
        out["iou_bev"] = iou_from_overlap(pa, pb, ov).reshape(shape)
    if "giou3d" in what:
        out["giou3d"] = giou3d_from(a, b, ov.reshape(shape), hu.reshape(shape))
    return out


# ---- NMS -------------------------------------------------------------------------------------------------------------------------------------
def aabb_gate(boxes):
    """nms_cpu's gate as an (N, N) matrix: the axis-aligned extents overlap strictly in x, y and z"""
    b = np.asarray(boxes, F).reshape(-1, 7)
    ok = np.ones((len(b), len(b)), bool)
    for c in range(3):
        lo, hi = b[:, c] - b[:, c + 3] / F(2), b[:, c] + b[:, c + 3] / F(2)
        ok &= np.minimum(hi[:, None], hi[None, :]) > np.maximum(lo[:, None], lo[None, :])
    return ok


def sweep(mask, max_out=None):
    """the greedy sweep over mask[i, j] (kept i removes j > i): kept positions, at most max_out"""
    n = len(mask)
    removed, keep = np.zeros(n, bool), []
    for i in range(n):
        if max_out is not None and len(keep) >= max_out:
            break
        if not removed[i]:
            keep.append(i)
            removed[i + 1:] |= mask[i, i + 1:]
    return np.array(keep, np.int64)


def stable_order(scores):
    """descending score, ties to the smaller index, NaN last in index order"""
    return np.argsort(-np.asarray(scores, F), kind="stable")


def nms_from_iou(iou, thresh, gate=None, max_out=None):
    mask = iou > F(thresh)
    if gate is not None:
        mask &= gate
    return sweep(mask, max_out)


def nms(boxes, scores, thresh, mode=0, max_out=None):
    """indices into boxes of the kept ones, best first (scores None: boxes already in order)"""
    b = np.asarray(boxes, F).reshape(-1, 7)
    order = np.arange(len(b)) if scores is None else stable_order(scores)
    ob = b[order]
    iou = pairwise(ob, ob, ("iou_bev",))["iou_bev"]
    return order[nms_from_iou(iou, thresh, aabb_gate(ob) if mode else None, max_out)]


def passes(scores, labels, class_thresh):
    """class_agnostic_nms's mask: label c (1-based) has an entry (class_thresh[c - 1] >= 0) and score >= it"""
    scores, labels, ct = np.asarray(scores, F), np.asarray(labels, np.int64), np.asarray(class_thresh, F)
    ok = (labels >= 1) & (labels <= len(ct))
    t = np.where(ok, ct[np.clip(labels - 1, 0, len(ct) - 1)], F(-1))
    with np.errstate(invalid="ignore"):
        return ok & (t >= 0) & (scores >= t)


def postprocess(boxes, scores, labels, class_thresh, nms_thresh, post_max=None, mode=0):
    """(boxes, scores, labels, positions) of the fused post-process"""
    b, s, lab = np.asarray(boxes, F).reshape(-1, 7), np.asarray(scores, F), np.asarray(labels, np.int32)
    idx = np.flatnonzero(passes(s, lab, class_thresh))
    sel = idx[nms(b[idx], s[idx], nms_thresh, mode, post_max)] if len(idx) else idx
    return b[sel], s[sel], lab[sel], sel


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def clustered(seed, n=200, clusters=12, sigma=0.8, span=40.0):
    """n boxes around `clusters` centres: dx in [0.5, 5], dy in [0.5, 2.1], heading in [-2 pi, 2 pi]"""
    r = np.random.default_rng(seed)
    centres = r.uniform(-span, span, (clusters, 2))
    c = centres[r.integers(0, clusters, n)] + r.normal(0, sigma, (n, 2))
    b = np.zeros((n, 7))
    b[:, :2] = c
    b[:, 2] = r.uniform(-1.5, 0.5, n)
    b[:, 3], b[:, 4], b[:, 5] = r.uniform(0.5, 5, n), r.uniform(0.5, 2.1, n), r.uniform(1.2, 2.5, n)
    b[:, 6] = r.uniform(-2 * np.pi, 2 * np.pi, n)
    return b.astype(F)


def scored(seed, n, n_class=4):
    """distinct f32 scores in (0.02, 1) and labels 1 .. n_class"""
    r = np.random.default_rng(seed + 7919)
    s = np.unique(r.uniform(0.02, 1.0, 4 * n).astype(F))
    s = r.permutation(s)[:n]
    assert len(np.unique(s)) == n
    return s, r.integers(1, n_class + 1, n).astype(np.int32)


def handmade():
    """(a, b): pair k is a[k] against b[k]; the tests also take the full cross product"""
    q = np.pi / 4
    pairs = [
        ([0, 0, 0, 4, 2, 1.5, 0.3], [0, 0, 0, 4, 2, 1.5, 0.3]),              # identical
        ([0, 0, 0, 4, 2, 1.5, 0.3], [30, 30, 0, 4, 2, 1.5, 1.0]),            # disjoint
        ([0, 0, 0, 4, 2, 1.5, 0.0], [4, 0, 0, 4, 2, 1.5, 0.0]),              # touching along an edge
        ([0, 0, 0, 6, 4, 1.5, 0.2], [0.3, 0.2, 0, 1, 0.5, 1.0, 1.1]),        # one inside the other
        ([0, 0, 0, 2, 2, 1.5, 0.0], [0, 0, 0, 2, 2, 1.5, q]),                # a 45 degree cross: 8 intersections, an octagon
        ([1, 1, 0, 3, 1.5, 1.5, 5.9], [1.5, 0.5, 0, 2, 1, 1.5, -4.4]),       # headings beyond +-pi
        ([0, 0, 0, 0, 2, 1.5, 0.4], [0.1, 0, 0, 3, 1, 1.5, 0.0]),            # a zero-width box
        ([0, 0, 0, 4, 2, 1.5, 0.0], [4.005, 0, 0, 4, 2, 1.5, 0.0]),          # corners 5 mm outside the other box: the margin counts them
        ([0, 0, 0, 4, 2, 1.5, 0.0], [1, 0, 0, 2, 2, 1.5, 0.0]),              # collinear shared edges
        ([0, 0, 0, 2, 2, 1.5, 0.0], [2, 2, 0, 2, 2, 1.5, 0.0]),              # duplicated corner (1, 1) for the hull sort
        ([0, 0, 0, 2, 2, 1.5, 0.0], [0, 0, 3, 2, 2, 1.0, 0.0]),              # the same footprint, disjoint in height
    ]
    return np.array([p[0] for p in pairs], F), np.array([p[1] for p in pairs], F)


def chain_case():
    """130 boxes in order: A = row 0 removes B = row 63, and B would have removed C = row 64, which A does not touch; everything else is far
    away.  The sweep must keep C: the decision about B falls in block 0, its row must not reach block 1"""
    b = np.zeros((130, 7), F)
    b[:, 0] = 100.0 + 10.0 * np.arange(130)
    b[:, 3:6] = [4, 2, 1.5]
    b[0, :2] = [0, 0]
    b[63, :2] = [1.5, 0]   # IoU with A: 2.5 * 2 / (16 - 5) = 0.4545
    b[64, :2] = [3.0, 0]   # IoU with B 0.4545, with A: 1 * 2 / (16 - 2) = 0.1429
    return b


def z_gate_case():
    """two boxes with the same footprint, disjoint in z: mode 0 drops the second, the AABB gate keeps both"""
    return np.array([[0, 0, 0, 4, 2, 1.5, 0.1], [0.2, 0, 5, 4, 2, 1.5, 0.1], [20, 0, 0, 4, 2, 1.5, 0.1]], F), np.array([0.9, 0.8, 0.7], F)


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def allowances(g):
    """8 x the recorded spreads: overlap and IoU absolute, hull relative to the value"""
    return ALLOWANCE_FACTOR * float(g["spread_overlap"]), ALLOWANCE_FACTOR * float(g["spread_iou"]), ALLOWANCE_FACTOR * float(g["spread_hull_rel"])


def giou_allowance(a, b, ref, a_ov, a_hull_rel):
    """per-pair allowance of GIoU3D = o3 / u3 - 1 + u3 / c3 when the BEV overlap moves by a_ov and the hull by a_hull_rel of itself:
    o3 = o * h moves by a_ov * h, u3 = va + vb - o3 by as much, so o3 / u3 moves by at most a_ov * h * (1 + o3 / u3) / u3 <= 2 a_ov h / u3,
    and u3 / c3 by a_ov * h / c3 + (u3 / c3) * a_hull_rel; plus four f32 roundings of terms of size <= 1"""
    a, b = np.asarray(a, F).reshape(-1, 7).astype(np.float64), np.asarray(b, F).reshape(-1, 7).astype(np.float64)
    a_max, a_min = (a[:, 2] + a[:, 5] / 2)[:, None], (a[:, 2] - a[:, 5] / 2)[:, None]
    b_max, b_min = (b[:, 2] + b[:, 5] / 2)[None, :], (b[:, 2] - b[:, 5] / 2)[None, :]
    h = np.clip(np.minimum(a_max, b_max) - np.maximum(a_min, b_min), 0, None)
    uh = np.clip(np.maximum(a_max, b_max) - np.minimum(a_min, b_min), 0, None)
    o3 = ref["overlap"].astype(np.float64) * h
    c3 = np.clip(ref["hull"].astype(np.float64) * uh, 1e-6, None)
    u3 = np.clip((a[:, 3] * a[:, 4] * a[:, 5])[:, None] + (b[:, 3] * b[:, 4] * b[:, 5])[None, :] - o3, 1e-6, None)
    return 2 * a_ov * h / u3 + a_ov * h / c3 + (u3 / c3) * a_hull_rel + 4 * 2.0 ** -23
