"""The detector's post-process of the reference -- class_agnostic_nms of sensor_inference/utils/model_nms_utils.py and PostProcesser of
sensor_inference/utils/object_post_process.py -- with their contracts, over one fused device call (`iou3d_nms_ext._postprocess` over
lio_boxes_postprocess: filter, order, NMS, gather; one upload, one download of the kept rows).

The reference's file builds its mask with `np.bool`, which current numpy no longer has; nothing here needs it (where a mask is spoken of it
is `bool`).  Labels are compared as integers.  Equal scores are ordered by the smaller index (lsd_amd/iou3d_nms.py says why)."""
import numpy as np

from . import iou3d_nms

_MODES = {"nms_gpu": 0, "nms_cpu": 1}


def class_agnostic_nms(box_scores, box_preds, box_labels, nms_config, score_thresh=None):
    """(scores (K,), boxes (K, C), labels (K,)) of the boxes that pass their class's threshold (`score_thresh`: {1-based label: threshold},
    score >= threshold passes, a label without an entry never does) and survive `nms_config.NMS_TYPE` at `nms_config.NMS_THRESH`, best
    first, at most `nms_config.NMS_POST_MAXSIZE`.  The outputs keep the inputs' dtypes and box_preds' columns beyond the seventh."""
    box_scores, box_preds, box_labels = np.asarray(box_scores), np.asarray(box_preds), np.asarray(box_labels)
    if nms_config.NMS_TYPE not in _MODES:
        raise ValueError(f"NMS_TYPE {nms_config.NMS_TYPE!r}: nms_gpu or nms_cpu")
    selected = np.zeros(0, dtype=np.int64)
    n = box_scores.shape[0]
    if n > 0 and score_thresh:
        n_class = max(int(c) for c in score_thresh)
        thresh = np.full(max(n_class, 1), -1.0, dtype=np.float32)
        for cls_idx, score in score_thresh.items():
            if int(cls_idx) >= 1:
                thresh[int(cls_idx) - 1] = score
        labels = np.where(box_labels == np.round(box_labels), box_labels, 0).astype(np.int32).reshape(-1)
        # the fused call returns the kept rows and their positions; the positions select from the caller's own arrays, so the outputs keep
        # their dtypes and box_preds' columns beyond the seventh
        kept, _, _, _, pos = iou3d_nms._ext()._postprocess(iou3d_nms._rows(box_preds), np.ascontiguousarray(box_scores.reshape(-1), dtype=np.float32),
                                                           labels, thresh, float(nms_config.NMS_THRESH), int(nms_config.NMS_POST_MAXSIZE),
                                                           _MODES[nms_config.NMS_TYPE])
        selected = np.asarray(pos[:kept], dtype=np.int64)
    return box_scores[selected], box_preds[selected], box_labels[selected]


class PostProcesser():
    def __init__(self, model_cfg, num_class, class_names):
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.class_names = class_names
        self.score_dict = dict()
        for name, thresh in model_cfg.POST_PROCESSING.SCORE_THRESH.items():
            self.score_dict[self.class_names.index(name) + 1] = thresh

        self.map_score = model_cfg.POST_PROCESSING.MAP_SCORE_THRESH

    def forward(self, cls_preds, box_preds, label_preds, freespace):
        post_process_cfg = self.model_cfg.POST_PROCESSING

        final_scores, final_boxes, final_labels = class_agnostic_nms(
            box_scores=cls_preds, box_preds=box_preds, box_labels=label_preds,
            nms_config=post_process_cfg.NMS_CONFIG,
            score_thresh=self.score_dict
        )
        final_labels = final_labels.reshape(final_labels.shape[0], 1)
        final_scores = final_scores.reshape(final_scores.shape[0], 1)

        result_dict = {
            'pred_boxes': final_boxes,
            'pred_scores': final_scores,
            'pred_labels': final_labels,
        }

        return result_dict
