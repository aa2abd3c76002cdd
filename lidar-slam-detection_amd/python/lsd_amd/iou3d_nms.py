"""The reference's sensor_driver/inference/iou3d_nms.py under its four names, argument orders and return shapes, over this project's
`iou3d_nms_ext` (csrc/iou3d_nms_wrapper.cpp over lio_boxes_*, include/lio_hip.h).  Callers of the reference change one import line:
`import lsd_amd.iou3d_nms as iou3d_nms_utils`.  Everything runs on the device; without one the first call raises
RuntimeError (there is no CPU fallback).

Where this differs from the reference: the order of equal scores.  The reference's np.argsort(-scores) is numpy's unstable default and
leaves ties to the implementation; here the order is np.argsort(-scores, kind="stable"): descending score, ties to the smaller index."""
import importlib

import numpy as np

_ext_mod = None


def _ext():
    global _ext_mod
    if _ext_mod is None:
        _ext_mod = importlib.import_module("iou3d_nms_ext")
    return _ext_mod


def _rows(boxes):
    return np.ascontiguousarray(np.asarray(boxes)[:, :7], dtype=np.float32)


def boxes_bev_iou_cpu(boxes_a, boxes_b):
    """
    Args:
        boxes_a: (N, 7) [x, y, z, dx, dy, dz, heading]
        boxes_b: (M, 7) [x, y, z, dx, dy, dz, heading]

    Returns:
        ans_iou: (N, M) float32
    """
    boxes_a, boxes_b = _rows(boxes_a), _rows(boxes_b)
    ans_iou = np.zeros((boxes_a.shape[0], boxes_b.shape[0]), dtype=np.float32)
    _ext().boxes_iou_bev_cpu(boxes_a, boxes_b, ans_iou)
    return ans_iou


def boxes_giou3d_gpu(boxes_a, boxes_b):
    """
    Args:
        boxes_a: (N, 7) [x, y, z, dx, dy, dz, heading]
        boxes_b: (M, 7) [x, y, z, dx, dy, dz, heading]

    Returns:
        ans_iou: (N, M) float32, the reference's formula operation for operation in f32, in one pass over the pair on the device
    """
    boxes_a, boxes_b = _rows(boxes_a), _rows(boxes_b)
    giou3d = np.zeros((boxes_a.shape[0], boxes_b.shape[0]), dtype=np.float32)
    _ext()._giou3d(boxes_a, boxes_b, giou3d)
    return giou3d


def _nms(boxes, scores, thresh, mode, pre_maxsize=None):
    boxes = _rows(boxes)
    scores = np.ascontiguousarray(np.asarray(scores).reshape(-1), dtype=np.float32)
    if pre_maxsize is not None and pre_maxsize < len(scores):
        # only the pre_maxsize best enter, as the reference's callers cut them (torch.topk before the call)
        head = np.argsort(-scores, kind="stable")[:pre_maxsize]
        head.sort()
        keep = np.zeros(len(head), dtype=np.int64)
        num_out = _ext()._nms(boxes[head], scores[head], keep, thresh, mode, 0)
        return head[keep[:num_out]]
    keep = np.zeros(boxes.shape[0], dtype=np.int64)
    num_out = _ext()._nms(boxes, scores, keep, thresh, mode, 0)
    return keep[:num_out]


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """
    :param boxes: (N, 7) [x, y, z, dx, dy, dz, heading]
    :param scores: (N)
    :param thresh:
    :return: indices of the kept boxes (int64), best first
    """
    return _nms(boxes, scores, thresh, 0, pre_maxsize)


def nms_cpu(boxes, scores, thresh):
    """
    :param boxes: (N, 7) [x, y, z, dx, dy, dz, heading]
    :param scores: (N)
    :param thresh:
    :return: indices of the kept boxes (int64), best first; a pair suppresses only where the axis-aligned extents overlap in x, y and z
    """
    return _nms(boxes, scores, thresh, 1)
