"""Exact k nearest neighbours on the device (csrc/knn_index.hip, lio_knn_index_*) and texture_mesh over it (graph_utils.cpp:449-501).

The restatement lives here: candidates from scipy's cKDTree (f64, k + extra), re-ranked by the f32 distance ((dx*dx) + dy*dy) + dz*dz computed
with numpy float32 operations, then by index; a query whose candidates cannot prove the k-th place (the farthest candidate is not clearly beyond
it) is redone by brute force.  Only finite points are indexed; ties at equal f32 distance go to the smaller input index."""
import time

import numpy as np
import pytest
from scipy.spatial import cKDTree

pytestmark = pytest.mark.gpu


def _need_gpu():
    from lsd_amd import capi

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")


def _index(pts, rgb=None):
    from lsd_amd import lio

    _need_gpu()
    x = lio.KnnIndex()
    return x, x.build(pts, rgb)


def _d2(P, Q):
    """f32 sequential distance of P (.., 3) to Q broadcast against it"""
    dx, dy, dz = P[..., 0] - Q[..., 0], P[..., 1] - Q[..., 1], P[..., 2] - Q[..., 2]
    return dx * dx + dy * dy + dz * dz


def _brute(Pf, ids, Q, k):
    """the k smallest (d2, index) of every query over all of Pf"""
    ri, rd = np.empty((len(Q), k), np.int64), np.empty((len(Q), k), np.float32)
    for j, q in enumerate(Q):
        d = _d2(Pf, q[None, :])
        c = np.nonzero(d <= np.partition(d, k - 1)[k - 1])[0]
        o = np.lexsort((ids[c], d[c]))[:k]
        ri[j], rd[j] = ids[c][o], d[c][o]
    return ri, rd


def restated(P, Q, k, extra=8):
    P, Q = np.asarray(P, np.float32), np.asarray(Q, np.float32)
    fin = np.isfinite(P).all(1)
    ids = np.nonzero(fin)[0].astype(np.int64)
    Pf = P[fin]
    m, nf = len(Q), len(Pf)
    idx = np.full((m, k), -1, np.int64)
    d2 = np.full((m, k), np.inf, np.float32)
    qf = np.nonzero(np.isfinite(Q).all(1))[0]
    if nf == 0 or len(qf) == 0:
        return idx, d2
    kk, kt = min(k + extra, nf), min(k, nf)
    Qf = Q[qf]
    dist, cand = cKDTree(Pf.astype(np.float64)).query(Qf.astype(np.float64), k=kk, workers=16)
    cand = cand.reshape(len(qf), kk)
    dist = np.asarray(dist, np.float64).reshape(len(qf), kk)
    dc = _d2(Pf[cand], Qf[:, None, :])
    gi = ids[cand]
    order = np.lexsort((gi, dc), axis=-1)[:, :kt]
    ri, rd = np.take_along_axis(gi, order, 1), np.take_along_axis(dc, order, 1)
    if kk < nf:  # every point outside the candidates is at least dist[:, -1] away (f64): prove the k-th place or redo the query
        unsure = np.nonzero(~(rd[:, -1].astype(np.float64) < dist[:, -1] ** 2 * (1 - 1e-5)))[0]
        if len(unsure):
            ri[unsure], rd[unsure] = _brute(Pf, ids, Qf[unsure], kt)
    idx[qf, :kt] = ri
    d2[qf, :kt] = rd
    return idx, d2


def _check(x, P, Q, k, extra=8):
    gi, gd = x.query(Q, k)
    ri, rd = restated(P, Q, k, extra)
    assert np.array_equal(gi, ri), f"k={k}: {int((gi != ri).any(1).sum())} of {len(Q)} queries differ in their neighbours"
    assert np.array_equal(gd.view(np.uint32), rd.view(np.uint32)), f"k={k}: distances differ"


def _scene(n, seed):
    from lsd_amd import synth

    return synth.Scene(half=60.0, n_boxes=20, seed=3).sample_surface(n, seed=seed)[:, :3].copy()


def test_uniform_cloud_exact():
    rng = np.random.default_rng(1)
    P = rng.uniform(-20, 20, (100_000, 3)).astype(np.float32)
    Q = rng.uniform(-22, 22, (10_000, 3)).astype(np.float32)
    x, nf = _index(P)
    assert nf == len(P)
    for k in (1, 3, 8):
        _check(x, P, Q, k)


def test_surface_scene_near_off_and_far_queries():
    rng = np.random.default_rng(2)
    P = _scene(100_000, 4)
    on = _scene(4_000, 5)
    u = rng.normal(size=(4_000, 3))
    off = (on + u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    d = rng.normal(size=(2_000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = (P.mean(0) + d * (np.abs(P - P.mean(0)).max() + 1000.0)).astype(np.float32)  # 1 km outside the bounding box
    x, _ = _index(P)
    for k in (1, 3, 8):
        _check(x, P, on, k)
        _check(x, P, off, k)
        _check(x, P, far, k, extra=64)


def test_outliers_far_away_keep_the_tree_exact_and_fast():
    rng = np.random.default_rng(3)
    P = np.concatenate([_scene(100_000, 6), rng.normal(size=(5, 3)).astype(np.float32) * 10 + np.float32([5000, -5000, 5000])]).astype(np.float32)
    P = P[rng.permutation(len(P))]
    Q = np.concatenate([_scene(8_000, 7), P[np.linalg.norm(P, axis=1) > 4000] + 3.0]).astype(np.float32)
    x, _ = _index(P)
    t = time.time()
    for k in (1, 3, 8):
        _check(x, P, Q, k)
    assert time.time() - t < 30


def test_few_finite_points_among_non_finite_rows():
    rng = np.random.default_rng(4)
    for nfin in (1, 2, 3):
        P = np.full((40, 3), np.nan, np.float32)
        P[rng.choice(40, 12, replace=False), rng.integers(0, 3)] = np.inf
        keep = rng.choice(40, nfin, replace=False)
        P[keep] = rng.uniform(-1, 1, (nfin, 3))
        Q = rng.uniform(-2, 2, (100, 3)).astype(np.float32)
        Q[5] = [np.nan, 0, 0]
        Q[9] = [0, -np.inf, 0]
        x, nf = _index(P)
        assert nf == nfin
        for k in (1, 3, 8):
            gi, gd = x.query(Q, k)
            _check(x, P, Q, k)
            assert (gi[[5, 9]] == -1).all() and np.isinf(gd[[5, 9]]).all()
            if k > nfin:
                assert (gi[:, nfin:] == -1).all()


def test_all_non_finite_cloud():
    x, nf = _index(np.full((10, 3), np.nan, np.float32))
    assert nf == 0
    gi, gd = x.query(np.zeros((4, 3), np.float32), 3)
    assert (gi == -1).all() and np.isinf(gd).all()


def test_lattice_with_duplicates_smaller_index_wins():
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(*[np.arange(10, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    P = np.concatenate([g, g, g])[rng.permutation(3 * len(g))]  # every lattice point three times
    c = np.stack(np.meshgrid(*[np.arange(9, dtype=np.float32) + 0.5] * 3, indexing="ij"), -1).reshape(-1, 3)
    Q = np.concatenate([c, g[rng.choice(len(g), 200)]]).astype(np.float32)  # cell centres: 24 equally distant points; lattice points: 3 at 0
    x, _ = _index(P)
    ids = np.arange(len(P))
    for k in (1, 3, 8):
        gi, gd = x.query(Q, k)
        ri, rd = _brute(P, ids, Q, k)
        assert np.array_equal(gi, ri) and np.array_equal(gd, rd)


def test_kth_distance_equal_to_a_node_bound():
    """six arms along the axes, each arm's nearest point exactly at distance 1: a box of one arm has its bound exactly equal to the k-th
    distance once another arm's point is found, and must still be entered (a smaller index may sit in it)"""
    rng = np.random.default_rng(6)
    t = (1.0 + 0.25 * np.arange(40)).astype(np.float32)
    arms = []
    for ax in range(3):
        for s in (1, -1):
            a = np.zeros((40, 3), np.float32)
            a[:, ax] = s * t
            arms.append(a)
    off = np.float32([8, 16, -4])
    base = np.concatenate(arms) + off
    Q = np.stack([off, off + np.float32([0, 0, 0.5])]).astype(np.float32)
    for trial in range(12):
        P = base[rng.permutation(len(base))].astype(np.float32)
        x, _ = _index(P)
        ids = np.arange(len(P))
        for k in (1, 3, 6, 8):
            gi, gd = x.query(Q, k)
            ri, rd = _brute(P, ids, Q, k)
            assert np.array_equal(gi, ri) and np.array_equal(gd, rd), f"trial {trial} k={k}"


def test_colour_is_floor_mean_of_the_restated_neighbours():
    rng = np.random.default_rng(7)
    P = _scene(60_000, 8)
    P[rng.choice(len(P), 500, replace=False)] = np.nan
    rgb = rng.integers(0, 1 << 32, len(P), dtype=np.uint64).astype(np.uint32)
    Q = np.concatenate([_scene(5_000, 9), np.float32([[np.nan, 0, 0], [0, np.inf, 0]])]).astype(np.float32)
    x, _ = _index(P, rgb)
    chans = np.stack([(rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255], 1).astype(np.int64)
    for k in (1, 3, 8):
        got = x.colour(Q, k)
        ri, _ = restated(P, Q, k)
        ok = ri >= 0
        s = (chans[np.where(ok, ri, 0)] * ok[..., None]).sum(1)
        cnt = ok.sum(1)[:, None]
        want = np.where(cnt > 0, s // np.maximum(cnt, 1), 0).astype(np.uint8)
        assert np.array_equal(got, want), f"k={k}"
        assert (got[-2:] == 0).all()
    # fewer finite points than k: the mean over what there is
    x2, _ = _index(np.float32([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0]]), np.uint32([0x000A0B0C, 0xFFFFFFFF, 0x00140D0F]))
    assert x2.colour(np.float32([[0.2, 0, 0]]), 3).tolist() == [[15, 12, 13]]


def test_large_cloud_one_call():
    from lsd_amd import synth

    rng = np.random.default_rng(8)
    scene = synth.Scene(half=100.0, n_boxes=40, seed=1)
    P = scene.sample_surface(20_000_000, seed=10, sigma=0.02)[:, :3].copy()
    bad = rng.choice(len(P), 1000, replace=False)
    P[bad, rng.integers(0, 3, len(bad))] = np.nan
    Q = scene.sample_surface(1_000_000, seed=11, sigma=0.5)[:, :3].copy()
    x, nf = _index(P)
    assert nf == len(P) - len(bad)
    k = 3
    gi, gd = x.query(Q, k)
    assert (gi >= 0).all()
    assert ((gd[:, 1:] > gd[:, :-1]) | ((gd[:, 1:] == gd[:, :-1]) & (gi[:, 1:] > gi[:, :-1]))).all(), "not ascending in (d2, idx)"
    s = rng.choice(len(Q), 20_000, replace=False)
    ri, rd = restated(P, Q[s], k)
    assert np.array_equal(gi[s], ri) and np.array_equal(gd[s].view(np.uint32), rd.view(np.uint32))


def _write_pcd_rgb(path, xyz, rgb):
    with open(path, "wb") as f:
        f.write(("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
                 f"WIDTH {len(xyz)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(xyz)}\nDATA binary\n").encode())
        rec = np.zeros((len(xyz), 4), np.float32)
        rec[:, :3] = xyz
        rec[:, 3] = rgb.view(np.float32)
        f.write(rec.tobytes())


def test_texture_mesh_end_to_end(tmp_path):
    _need_gpu()
    import slam_wrapper

    rng = np.random.default_rng(9)
    P = _scene(150_000, 12)
    P[rng.choice(len(P), 100, replace=False)] = np.nan
    rgb = rng.integers(0, 1 << 24, len(P)).astype(np.uint32) | np.uint32(0x3F000000)
    _write_pcd_rgb(str(tmp_path / "c.pcd"), P, rgb)
    V = _scene(12_000, 13)
    V[:100] += rng.normal(size=(100, 3)).astype(np.float32) * 20  # vertices off the surface
    nv = len(V)
    lines = ["# mesh", "o m"] + ["v %r %r %r" % tuple(float(c) for c in v) for v in V] + ["vn 0 0 1", "vt 0 0"]
    faces = []
    for i in range(0, nv - 4, 4):
        if i % 8 == 0:
            faces.append([i, i + 1, i + 2, i + 3])
            lines.append("f %d/1 %d/1/1 %d//1 %d" % (i + 1, i + 2, i + 3, i + 4))
        else:  # relative indices: -1 is the last vertex, which every face follows
            faces.append([i + 2, i + 1, i])
            lines.append("f %d %d %d" % (i + 2 - nv, i + 1 - nv, i - nv))
    (tmp_path / "m.obj").write_text("\n".join(lines) + "\n")
    out = tmp_path / "out"
    out.mkdir()
    slam_wrapper.texture_mesh(str(tmp_path / "m.obj"), str(tmp_path / "c.pcd"), str(out))
    ply = out / "texture_mesh.ply"
    assert ply.exists()
    head, body = ply.read_bytes().split(b"end_header\n", 1)
    assert head.decode().startswith("ply\nformat binary_little_endian 1.0\n")
    vt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    vert = np.frombuffer(body[: nv * vt.itemsize], vt)
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1).view(np.uint32), V.view(np.uint32))
    got, o = [], nv * vt.itemsize
    for _ in range(len(faces)):
        c = body[o]
        got.append(np.frombuffer(body[o + 1: o + 1 + 4 * c], "<i4").tolist())
        o += 1 + 4 * c
    assert o == len(body) and got == faces
    ri, _ = restated(P, V, 3)
    assert (ri >= 0).all()
    want = np.stack([(rgb[ri] >> s) & 255 for s in (16, 8, 0)], -1).astype(np.int64).sum(1) // 3
    assert np.array_equal(np.stack([vert["r"], vert["g"], vert["b"]], 1), want.astype(np.uint8))
