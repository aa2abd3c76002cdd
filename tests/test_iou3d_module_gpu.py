"""The reference's outer boundary of the detection boxes on the device: the pybind11 module `iou3d_nms_ext` under the reference's four names and
in-place outputs, lsd_amd/iou3d_nms.py over it with the reference module's argument orders and return shapes, and lsd_amd/detect_post.py over
the fused call."""
from types import SimpleNamespace

import numpy as np
import pytest

import boxes_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return bc.load_golden()


@pytest.fixture(scope="module")
def ext():
    from lsd_amd import capi

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    import iou3d_nms_ext

    return iou3d_nms_ext


def test_the_four_names_write_in_place(G, ext):
    b = G["hand"]
    a_ov, a_iou, a_hull = bc.allowances(G)
    ov, hull, iou = (np.zeros((len(b), len(b)), np.float32) for _ in range(3))
    assert ext.boxes_overlap_bev_gpu(b, b, ov) == 1 and ext.boxes_union_bev_gpu(b, b, hull) == 1 and ext.boxes_iou_bev_cpu(b, b, iou) == 1
    assert np.abs(ov - G["hand_overlap"]).max() <= a_ov and np.abs(iou - G["hand_iou_bev"]).max() <= a_iou
    assert (np.abs(hull - G["hand_hull"]) / np.maximum(G["hand_hull"], 1e-6)).max() <= a_hull
    n = 129
    keep = np.zeros(n, dtype=np.int_)
    num_out = ext.nms_gpu(G["nms_boxes"][:n], keep, float(G["nms_thresh"]))
    assert num_out == len(G[f"nms_keep_{n}"]) and np.array_equal(keep[:num_out], G[f"nms_keep_{n}"])
    with pytest.raises(ValueError):
        ext.boxes_overlap_bev_gpu(b, b, np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError):
        ext.boxes_overlap_bev_gpu(b[:, :6], b, ov)


def test_the_handle_grows(G, ext):
    big = bc.clustered(31, 2100, clusters=40, span=300.0)
    keep = np.zeros(len(big), dtype=np.int64)
    n = ext.nms_gpu(big, keep, 0.25)
    assert 0 < n < len(big)
    small = np.zeros((2, 2), np.float32)
    ext.boxes_iou_bev_cpu(big[:2], big[:2], small)
    assert small[0, 0] > 0.99 and small[1, 1] > 0.99


def test_reference_module_functions(G):
    from lsd_amd import iou3d_nms

    b, s, t = G["nms_boxes"], G["nms_scores"], float(G["nms_thresh"])
    perm = np.random.default_rng(3).permutation(len(b))
    inv = np.argsort(perm)  # where each box of the recorded order went
    keep = iou3d_nms.nms_gpu(b[perm], s[perm], t)
    assert keep.dtype == np.int64 and np.array_equal(keep, inv[G["nms_keep_200"]])
    assert np.array_equal(iou3d_nms.nms_cpu(b[perm], s[perm], t), inv[G["nms_keep_gate_200"]])
    # pre_maxsize: only the best enter
    assert np.array_equal(iou3d_nms.nms_gpu(b[perm], s[perm], t, pre_maxsize=128), inv[G["nms_keep_128"]])
    a_ov, a_iou, a_hull = bc.allowances(G)
    h = G["hand"]
    iou = iou3d_nms.boxes_bev_iou_cpu(h, h[:5])
    assert iou.shape == (len(h), 5) and iou.dtype == np.float32 and np.abs(iou - G["hand_iou_bev"][:, :5]).max() <= a_iou
    ref = {k: G[f"hand_{k}"] for k in ("overlap", "hull")}
    gi = iou3d_nms.boxes_giou3d_gpu(h, h)
    assert gi.shape == (len(h), len(h)) and gi.dtype == np.float32
    assert (np.abs(gi.astype(np.float64) - bc.giou3d_from(h, h, ref["overlap"], ref["hull"])) <= bc.giou_allowance(h, h, ref, a_ov, a_hull)).all()
    assert iou3d_nms.boxes_giou3d_gpu(h, np.zeros((0, 7), np.float32)).shape == (len(h), 0)  # the tracker's first frame: no tracks
    assert len(iou3d_nms.nms_gpu(np.zeros((0, 7), np.float32), np.zeros(0, np.float32), t)) == 0


def test_post_processer(G):
    from lsd_amd import detect_post

    def cfg(nms_type):
        nms = SimpleNamespace(NMS_TYPE=nms_type, NMS_THRESH=0.25, NMS_PRE_MAXSIZE=2048, NMS_POST_MAXSIZE=256)
        return SimpleNamespace(POST_PROCESSING=SimpleNamespace(SCORE_THRESH={"Vehicle": 0.10, "Pedestrian": 0.10, "Traffic_Cone": 0.10},
                                                               MAP_SCORE_THRESH={}, NMS_CONFIG=nms))

    names = ["Vehicle", "Pedestrian", "Cyclist", "Traffic_Cone"]
    b, s, lab, keep = G["post_boxes"], G["post_scores"], G["post_labels"], G["post_keep"]
    out = detect_post.PostProcesser(cfg("nms_gpu"), 4, names).forward(s, b, lab, None)
    assert out["pred_scores"].shape == (len(keep), 1) and out["pred_labels"].shape == (len(keep), 1)
    assert np.array_equal(out["pred_boxes"], b[keep]) and np.array_equal(out["pred_scores"][:, 0], s[keep]) and np.array_equal(out["pred_labels"][:, 0], lab[keep])
    want = bc.postprocess(b, s, lab, G["post_class_thresh"], 0.25, 256, mode=1)[3]
    out = detect_post.PostProcesser(cfg("nms_cpu"), 4, names).forward(s, b, lab, None)
    assert np.array_equal(out["pred_boxes"], b[want])
    out = detect_post.PostProcesser(cfg("nms_gpu"), 4, names).forward(s * 0, b, lab, None)
    assert out["pred_boxes"].shape == (0, 7) and out["pred_scores"].shape == (0, 1) and out["pred_labels"].shape == (0, 1)
