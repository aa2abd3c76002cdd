"""The detection boxes without a GPU: the numpy restatement of tests/boxes_cases.py against what the reference's own iou3d_cpu.cpp recorded in
tests/golden/boxes.npz (matrices within 8 x the recorded spread of the reference under last-bit trigonometry differences, kept lists equal),
the contracts of lsd_amd.detect_post over a stub of the device call, and the error contract of the lio_boxes_* entries."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import boxes_cases as bc


@pytest.fixture(scope="module")
def G():
    return bc.load_golden()


@pytest.mark.parametrize("name", ["hand", "scene"])
def test_restatement_against_the_reference_matrices(G, name):
    b = G[name]
    a_ov, a_iou, a_hull = bc.allowances(G)
    r = bc.pairwise(b, b, ("overlap", "hull", "iou_bev"))
    d_ov = np.abs(r["overlap"] - G[name + "_overlap"]).max()
    d_iou = np.abs(r["iou_bev"] - G[name + "_iou_bev"]).max()
    d_hull = (np.abs(r["hull"] - G[name + "_hull"]) / np.maximum(G[name + "_hull"], 1e-6)).max()
    print(f"{name}: overlap {d_ov:.3g} (allowed {a_ov:.3g}), IoU {d_iou:.3g} ({a_iou:.3g}), hull rel {d_hull:.3g} ({a_hull:.3g})")
    assert d_ov <= a_ov and d_iou <= a_iou and d_hull <= a_hull
    for k in ("overlap", "hull", "iou_bev"):
        assert np.isfinite(G[f"{name}_{k}"]).all() and np.isfinite(r[k]).all()


def test_handmade_pairs_are_what_they_are_called(G):
    n = len(G["hand"]) // 2
    ov, hull = G["hand_overlap"][np.arange(n), np.arange(n) + n], G["hand_hull"][np.arange(n), np.arange(n) + n]
    assert ov[0] == 8.0 and hull[0] == 8.0          # identical
    assert ov[1] == 0.0                             # disjoint: exactly zero
    assert ov[2] == 0.0                             # touching along an edge: no strict crossing, corners outside the margin's reach in x
    assert abs(ov[3] - 0.5) < 1e-6                  # inside
    assert abs(ov[4] - 8 * (np.sqrt(2) - 1)) < 1e-5  # the cross of two 2 x 2 squares: the regular octagon
    assert ov[7] > 0.0                              # 5 mm apart: the margin counts the corners and makes a sliver
    assert ov[8] == 4.0 and ov[10] == 4.0


def test_spreads_are_recorded_and_small(G):
    assert 0 < float(G["spread_overlap"]) < 1e-3 and 0 < float(G["spread_iou"]) < 1e-3 and 0 < float(G["spread_hull_rel"]) < 1e-5
    assert int(G["spread_pairs"]) > 10000


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 128, 129, 200])
def test_restated_nms_keeps_what_the_reference_keeps(G, n):
    b = G["nms_boxes"][:n]
    assert np.array_equal(bc.nms(b, None, float(G["nms_thresh"])), G[f"nms_keep_{n}"])
    assert np.array_equal(bc.nms(b, None, float(G["nms_thresh"]), mode=1), G[f"nms_keep_gate_{n}"])


def test_gate_differs_from_plain_nms_somewhere(G):
    assert not np.array_equal(G["nms_keep_200"], G["nms_keep_gate_200"])
    b, s = bc.z_gate_case()
    assert list(bc.nms(b, s, 0.25)) == [0, 2] and list(bc.nms(b, s, 0.25, mode=1)) == [0, 1, 2]


def test_restated_chain_keeps_c():
    keep = bc.nms(bc.chain_case(), None, 0.25)
    assert 63 not in keep and 64 in keep and len(keep) == 129


def test_restated_post_process(G):
    b, s, lab, pos = bc.postprocess(G["post_boxes"], G["post_scores"], G["post_labels"], G["post_class_thresh"], 0.25, 256)
    assert np.array_equal(pos, G["post_keep"])
    assert int(G["post_equal_index"]) in np.flatnonzero(bc.passes(G["post_scores"], G["post_labels"], G["post_class_thresh"]))
    assert not (lab == 3).any() and (G["post_labels"] == 3).any()  # the class without an entry
    assert (np.diff(s) < 0).all()


def test_stable_order_rule():
    s = np.array([0.5, np.nan, 0.7, 0.5, -0.0, 0.0, np.nan, 0.7], np.float32)
    assert list(bc.stable_order(s)) == [2, 7, 0, 3, 4, 5, 1, 6]


class _StubExt:
    """the fused device call of iou3d_nms_ext, answered by the restatement"""

    def __init__(self):
        self.calls = 0

    def _postprocess(self, boxes, scores, labels, class_thresh, nms_thresh, post_max, mode=0):
        self.calls += 1
        b, s, lab, pos = bc.postprocess(boxes, scores, labels, class_thresh, nms_thresh, post_max or None, mode)
        return len(pos), b, s, lab, pos.astype(np.uint32)


def _cfg(nms_type="nms_gpu", post_max=256):
    nms = SimpleNamespace(NMS_TYPE=nms_type, NMS_THRESH=0.25, NMS_PRE_MAXSIZE=2048, NMS_POST_MAXSIZE=post_max)
    post = SimpleNamespace(SCORE_THRESH={"Vehicle": 0.10, "Pedestrian": 0.10, "Traffic_Cone": 0.10}, MAP_SCORE_THRESH={"Vehicle": 0.3}, NMS_CONFIG=nms)
    return SimpleNamespace(POST_PROCESSING=post)


def test_detect_post_contracts_over_a_stub(G, monkeypatch):
    from lsd_amd import detect_post, iou3d_nms

    stub = _StubExt()
    monkeypatch.setattr(iou3d_nms, "_ext_mod", stub)
    names = ["Vehicle", "Pedestrian", "Cyclist", "Traffic_Cone"]  # Cyclist (label 3) has no threshold
    pp = detect_post.PostProcesser(_cfg(), 4, names)
    assert pp.score_dict == {1: 0.10, 2: 0.10, 4: 0.10}
    boxes9 = np.concatenate([G["post_boxes"], np.arange(400, dtype=np.float32).reshape(200, 2)], axis=1)  # columns beyond the seventh travel along
    out = pp.forward(G["post_scores"], boxes9, G["post_labels"].astype(np.float32), None)
    keep = G["post_keep"]
    assert stub.calls == 1
    assert out["pred_boxes"].shape == (len(keep), 9) and out["pred_scores"].shape == (len(keep), 1) and out["pred_labels"].shape == (len(keep), 1)
    assert np.array_equal(out["pred_boxes"], boxes9[keep]) and np.array_equal(out["pred_scores"][:, 0], G["post_scores"][keep])
    assert out["pred_labels"].dtype == np.float32
    # post-max cuts the kept list
    s, b, lab = detect_post.class_agnostic_nms(G["post_scores"], G["post_boxes"], G["post_labels"], _cfg(post_max=5).POST_PROCESSING.NMS_CONFIG, {1: 0.1, 2: 0.1, 4: 0.1})
    assert np.array_equal(b, G["post_boxes"][keep[:5]]) and s.shape == (5,) and lab.shape == (5,)
    # nothing passes / nothing comes in: the empty case, without a device call
    calls = stub.calls
    s, b, lab = detect_post.class_agnostic_nms(G["post_scores"], G["post_boxes"], G["post_labels"], _cfg().POST_PROCESSING.NMS_CONFIG, {1: 2.0})
    assert s.shape == (0,) and b.shape == (0, 7) and lab.shape == (0,)
    out = pp.forward(np.zeros(0, np.float32), np.zeros((0, 7), np.float32), np.zeros(0, np.int32), None)
    assert out["pred_boxes"].shape == (0, 7) and out["pred_scores"].shape == (0, 1) and out["pred_labels"].shape == (0, 1)
    assert stub.calls == calls + 1  # the first reached the device call and came back empty, the second never called
    with pytest.raises(ValueError):
        detect_post.class_agnostic_nms(G["post_scores"], G["post_boxes"], G["post_labels"], _cfg("nms_fast").POST_PROCESSING.NMS_CONFIG, {1: 0.1})


def test_new_entries_reject_bad_arguments():
    from lsd_amd import capi

    L = capi.lib()
    assert L.lio_abi_version() >= 28
    for bad in (0, capi.BOXES_MAX + 1):
        assert not L.lio_boxes_create(0, bad)
        assert b"max_boxes" in L.lio_last_error()
    assert not L.lio_boxes_create(-1, 16)
    a = np.zeros((2, 7), np.float32)
    fp = a.ctypes.data_as(C.POINTER(C.c_float))
    keep = np.zeros(2, np.int64)
    assert L.lio_boxes_pairwise(None, fp, 2, fp, 2, None, None, None, None) == capi.LIO_E_INVALID
    assert L.lio_boxes_nms(None, fp, None, 2, 0.25, 0, 0, keep.ctypes.data_as(C.POINTER(C.c_int64))) == capi.LIO_E_INVALID
    assert L.lio_boxes_set_gate(None, 0) == capi.LIO_E_INVALID
    assert L.lio_boxes_postprocess(None, fp, fp, None, 2, fp, 1, 0.25, 0, None, None, None) == capi.LIO_E_INVALID
    assert L.lio_boxes_postprocess_device(None, None, None, None, 2, fp, 1, 0.25, 0, None, None, None) == capi.LIO_E_INVALID
    assert L.lio_boxes_last_indices(None, None, 0) == capi.LIO_E_INVALID
    assert L.lio_boxes_last_times(None, None, None, None, None) == capi.LIO_E_INVALID
    L.lio_boxes_destroy(None)


def test_boxes_fail_loudly_without_a_device():
    from lsd_amd import capi, lio

    if capi.lib().lio_device_count() > 0:
        lio.Boxes(16).close()
        return
    with pytest.raises(capi.LioError):
        lio.Boxes()
    import iou3d_nms_ext

    with pytest.raises(RuntimeError):
        iou3d_nms_ext.boxes_iou_bev_cpu(np.zeros((1, 7), np.float32), np.zeros((1, 7), np.float32), np.zeros((1, 1), np.float32))
