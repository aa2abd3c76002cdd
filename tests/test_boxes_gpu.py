"""The detection boxes on the device (csrc/boxes.hip, lio.Boxes) against what the reference's iou3d_cpu.cpp recorded in tests/golden/boxes.npz
and against the numpy restatement of tests/boxes_cases.py.  Matrices agree within 8 x the recorded spread of the reference under last-bit
trigonometry differences (overlap and IoU absolute, the hull relative to its value); kept lists are equal (the recorder made sure no pair's
IoU lies within 1e-3 of the threshold); what does not pass through cosf / sinf / atan2f is compared bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import boxes_cases as bc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1), (17, 33), (65, 130)]


@pytest.fixture(scope="module")
def G():
    return bc.load_golden()


@pytest.fixture(scope="module")
def bx():
    from lsd_amd import capi, lio

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    b = lio.Boxes(256)
    yield b
    b.close()


@pytest.fixture(scope="module")
def restated():
    """the restatement at the odd shapes, computed once"""
    out = {}
    for na, nb in SHAPES:
        a, b = bc.clustered(300 + na, na, clusters=3), bc.clustered(400 + nb, nb, clusters=3)
        out[(na, nb)] = (a, b, bc.pairwise(a, b))
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_matrices(G, got, ref, a, b, what=""):
    a_ov, a_iou, a_hull = bc.allowances(G)
    d_ov = np.abs(got["overlap"] - ref["overlap"]).max()
    d_iou = np.abs(got["iou_bev"] - ref["iou_bev"]).max()
    d_hull = (np.abs(got["hull"] - ref["hull"]) / np.maximum(ref["hull"], 1e-6)).max()
    print(f"{what}: overlap {d_ov:.3g} (allowed {a_ov:.3g}), IoU {d_iou:.3g} ({a_iou:.3g}), hull rel {d_hull:.3g} ({a_hull:.3g})")
    assert d_ov <= a_ov and d_iou <= a_iou and d_hull <= a_hull
    for v in got.values():
        assert np.isfinite(v).all()
    # zero exactly where the reference is zero by a margin no rounding crosses: pairs whose centres are further apart than their diagonals
    far = np.linalg.norm(a[:, None, :2] - b[None, :, :2], axis=2) > (np.linalg.norm(a[:, 3:5], axis=1)[:, None] + np.linalg.norm(b[:, 3:5], axis=1)[None, :]) / 2 + 0.1
    assert (got["overlap"][far] == 0).all() and (got["iou_bev"][far] == 0).all()


@pytest.mark.parametrize("name", ["hand", "scene"])
def test_pairwise_against_the_reference(G, bx, name):
    b = G[name]
    got = bx.pairwise(b, b)
    ref = {k: G[f"{name}_{k}"] for k in ("overlap", "hull", "iou_bev")}
    check_matrices(G, got, ref, b, b, name)
    a_ov, _, a_hull = bc.allowances(G)
    want = bc.giou3d_from(b, b, ref["overlap"], ref["hull"])
    d = np.abs(got["giou3d"].astype(np.float64) - want)
    tol = bc.giou_allowance(b, b, ref, a_ov, a_hull)
    print(f"{name}: GIoU3D largest difference {d.max():.3g}, largest share of its allowance {(d / tol).max():.3g}")
    assert (d <= tol).all()
    # the formula itself over the device's own two matrices: bit for bit
    assert np.array_equal(bits(got["giou3d"]), bits(bc.giou3d_from(b, b, got["overlap"], got["hull"])))
    assert np.array_equal(bits(got["iou_bev"]), bits(bc.iou_from_overlap(*bc._pairs(b, b)[:2], got["overlap"].reshape(-1)).reshape(got["overlap"].shape)))


def test_handmade_pairs(G, bx):
    ha, hb = bc.handmade()
    got = bx.pairwise(ha, hb)
    n = np.arange(len(ha))
    ov, iou, gi = got["overlap"][n, n], got["iou_bev"][n, n], got["giou3d"][n, n]
    assert ov[1] == 0.0 and iou[1] == 0.0 and bits(ov[1:2])[0] == 0  # the disjoint pair: exactly +0
    assert ov[0] == 8.0 and iou[0] == 1.0 and ov[8] == 4.0
    assert ov[7] > 0.0  # the margin's sliver
    assert ov[10] == 4.0 and gi[10] < 0  # the same footprint, disjoint in height: no 3-D overlap, GIoU3D below zero
    for v in got.values():
        assert np.isfinite(v).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_pairwise_shapes(G, bx, restated, shape):
    a, b, ref = restated[shape]
    got = bx.pairwise(a, b)
    assert all(got[k].shape == shape for k in got)
    check_matrices(G, got, ref, a, b, str(shape))
    # all four at once equal each asked for alone
    for w in bx.WHAT:
        alone = bx.pairwise(a, b, what=(w,))
        assert list(alone) == [w] and np.array_equal(bits(alone[w]), bits(got[w])), w


def test_pairwise_empty_sides(bx):
    a = bc.clustered(1, 5)
    for na, nb in ((5, 0), (0, 5), (0, 0)):
        got = bx.pairwise(a[:na], a[:nb])
        assert all(got[k].shape == (na, nb) for k in bx.WHAT)


def test_oversize_and_bad_arguments(bx):
    from lsd_amd import capi

    big = bc.clustered(2, 257)
    with pytest.raises(capi.LioError, match="max_boxes"):
        bx.pairwise(big, big[:1])
    with pytest.raises(capi.LioError, match="max_boxes"):
        bx.nms(big, None, 0.25)
    with pytest.raises(capi.LioError):
        bx.nms(big[:4], None, 0.25, mode=7)
    with pytest.raises(capi.LioError, match="max_boxes"):
        bx.postprocess(big, np.ones(257), np.ones(257, np.int32), [0.1], 0.25)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 128, 129, 200])
def test_nms_sizes(G, bx, n):
    b, s, t = G["nms_boxes"][:n], G["nms_scores"][:n], float(G["nms_thresh"])
    keep = bx.nms(b, None, t)
    assert keep.dtype == np.int64 and np.array_equal(keep, G[f"nms_keep_{n}"])
    assert np.array_equal(bx.nms(b, None, t, mode=1), G[f"nms_keep_gate_{n}"])
    # out of order, with scores: the same boxes
    perm = np.random.default_rng(n).permutation(n)
    assert np.array_equal(bx.nms(b[perm], s[perm], t), np.argsort(perm)[G[f"nms_keep_{n}"]])


def test_nms_identical_and_disjoint(bx):
    same = np.tile(np.array([[1, 2, 0, 4, 2, 1.5, 0.7]], np.float32), (130, 1))
    assert list(bx.nms(same, None, 0.25)) == [0]
    apart = same.copy()
    apart[:, 0] = 10.0 * np.arange(130)
    assert np.array_equal(bx.nms(apart, None, 0.25), np.arange(130))


def test_nms_chain_across_a_block_edge(bx):
    keep = bx.nms(bc.chain_case(), None, 0.25)
    assert 63 not in keep and 64 in keep and len(keep) == 129  # A removes B (row 63); B would have removed C (row 64)


def test_nms_max_out(G, bx):
    b, t, full = G["nms_boxes"], float(G["nms_thresh"]), G["nms_keep_200"]
    assert np.array_equal(bx.nms(b, None, t, max_out=10), full[:10])
    assert np.array_equal(bx.nms(b, None, t, max_out=len(full)), full)
    assert np.array_equal(bx.nms(b, None, t, max_out=199), full)
    assert len(bx.nms(b, None, t, max_out=0)) == 0


def test_nms_aabb_gate_in_z(bx):
    b, s = bc.z_gate_case()
    assert list(bx.nms(b, s, 0.25)) == [0, 2] and list(bx.nms(b, s, 0.25, mode=1)) == [0, 1, 2]


def test_nms_ties_and_nan_follow_the_stable_rule(G, bx):
    b, t = G["nms_boxes"], float(G["nms_thresh"])
    s = (np.round(G["nms_scores"] * 20) / 20).astype(np.float32)[np.random.default_rng(5).permutation(200)]
    assert len(np.unique(s)) < 30
    assert np.array_equal(bx.nms(b, s, t), bc.nms(b, s, t))
    s[[3, 77]] = np.nan
    s[[5, 9]] = [0.0, -0.0]
    assert np.array_equal(bx.nms(b, s, t), bc.nms(b, s, t))


def test_postprocess_against_the_reference(G, bx):
    b, s, lab, ct = G["post_boxes"], G["post_scores"], G["post_labels"], G["post_class_thresh"]
    keep = G["post_keep"]
    ob, os_, ol = bx.postprocess(b, s, lab, ct, 0.25, 256)
    assert ob.shape == (len(keep), 7) and os_.shape == (len(keep),) and ol.shape == (len(keep),) and ol.dtype == np.int32
    assert np.array_equal(bits(ob), bits(b[keep])) and np.array_equal(bits(os_), bits(s[keep])) and np.array_equal(ol, lab[keep])
    assert np.array_equal(bx.last_indices(), keep)
    assert np.array_equal(bc.postprocess(b, s, lab, ct, 0.25, 256)[3], keep)
    assert not (ol == 3).any() and (lab == 3).any()  # the class without an entry
    # post_max below the kept count cuts the list
    ob5, os5, ol5 = bx.postprocess(b, s, lab, ct, 0.25, 5)
    assert np.array_equal(bits(ob5), bits(b[keep[:5]])) and np.array_equal(bx.last_indices(), keep[:5])
    order_us, mask_us, sweep_us, total_us = bx.last_times()
    assert order_us > 0 and mask_us > 0 and sweep_us > 0 and total_us >= order_us + mask_us + sweep_us - 1.0


def test_postprocess_score_equal_to_threshold_and_nan(bx):
    b = bc.clustered(9, 6, clusters=6, sigma=0.0, span=200.0)  # six boxes far apart: NMS removes none
    s = np.array([0.5, 0.1, np.float32(0.1) - np.float32(1e-7), np.nan, 0.9, 0.3], np.float32)
    lab = np.array([1, 1, 1, 1, 2, 7], np.int32)
    ob, os_, ol = bx.postprocess(b, s, lab, np.array([0.1, -1.0], np.float32), 0.25, 256)
    assert np.array_equal(bx.last_indices(), [0, 1])  # 0.1 >= 0.1 passes; just below, NaN, the class without an entry and the unknown label do not
    assert np.array_equal(bits(os_), bits(s[[0, 1]])) and list(ol) == [1, 1]


def test_postprocess_nothing_passes(G, bx):
    ob, os_, ol = bx.postprocess(G["post_boxes"], G["post_scores"], G["post_labels"], [2.0, 2.0, 2.0, 2.0], 0.25, 256)
    assert ob.shape == (0, 7) and os_.shape == (0,) and ol.shape == (0,) and len(bx.last_indices()) == 0
    ob, os_, ol = bx.postprocess(np.zeros((0, 7)), np.zeros(0), np.zeros(0, np.int32), [0.1], 0.25, 256)
    assert ob.shape == (0, 7) and os_.shape == (0,) and ol.shape == (0,)


def test_postprocess_ties(G, bx):
    b, lab, ct = G["post_boxes"], G["post_labels"], G["post_class_thresh"]
    s = (np.ceil(G["post_scores"] * 10) / 10).astype(np.float32)  # ten distinct scores, none below a threshold it was above
    want = bc.postprocess(b, s, lab, ct, 0.25, 256)
    ob, os_, ol = bx.postprocess(b, s, lab, ct, 0.25, 256)
    assert np.array_equal(bx.last_indices(), want[3]) and np.array_equal(bits(ob), bits(want[0]))
    # the gate as the post-process's mode
    want = bc.postprocess(b, s, lab, ct, 0.25, 256, mode=1)
    bx.postprocess(b, s, lab, ct, 0.25, 256, mode=1)
    assert np.array_equal(bx.last_indices(), want[3])


def test_postprocess_device_equals_postprocess():
    """over torch tensors' data_ptr(), in a process that imports torch before the library is loaded (tests/_boxes_torch_worker.py says why)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "_boxes_torch_worker.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "boxes torch worker ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_giou3d_against_the_restatement(G, bx, restated):
    a, b, ref = restated[(17, 33)]
    a, b = a.copy(), b.copy()
    a[::3, 2] += 6.0  # every third detection above every tracker: height-disjoint pairs
    got = bx.pairwise(a, b, what=("giou3d",))["giou3d"]
    want = bc.giou3d_from(a, b, ref["overlap"], ref["hull"])
    a_ov, _, a_hull = bc.allowances(G)
    assert (np.abs(got.astype(np.float64) - want) <= bc.giou_allowance(a, b, ref, a_ov, a_hull)).all()
    assert (got[::3] < 0).all() and (got >= -1).all() and (got <= 1 + 1e-6).all()
    assert bx.pairwise(a, b[:0], what=("giou3d",))["giou3d"].shape == (17, 0)  # no trackers yet
