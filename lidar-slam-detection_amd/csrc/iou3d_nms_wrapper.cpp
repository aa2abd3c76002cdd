// iou3d_nms_wrapper.cpp -- the reference's outer boundary of the detection boxes: the pybind11 module `iou3d_nms_ext` with the four functions
// of sensor_driver/inference/iou3d_nms/iou3d_nms_api.cpp (names, in-place outputs, return values), over the C ABI's lio_boxes_*
// (include/lio_hip.h).
//
//   boxes_overlap_bev_gpu(boxes_a, boxes_b, ans_overlap)   (N, 7), (M, 7) -> ans_overlap (N, M) written in place; returns 1
//   boxes_union_bev_gpu(boxes_a, boxes_b, ans_union)       the area of the convex hull of the two boxes' corners; returns 1
//   boxes_iou_bev_cpu(boxes_a, boxes_b, ans_iou)           here on the device too; returns 1
//   nms_gpu(boxes, keep, nms_overlap_thresh)               boxes in order; keep (int64, N) receives the kept positions; returns how many
//
// One handle, created by the first call (without a device that call raises RuntimeError: no CPU fallback) and re-created larger when a call
// exceeds it.  `_giou3d`, `_nms` and `_postprocess` are this project's: the one-pass GIoU3D and the ordered, gated and fused forms that
// lsd_amd/iou3d_nms.py and detect_post.py use.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "../../include/lio_hip.h"

namespace py = pybind11;

namespace {

using farray = py::array_t<float, py::array::c_style | py::array::forcecast>;
using iarray = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;

lio_boxes* g_boxes = nullptr;
uint32_t g_cap = 0;

lio_boxes* handle(uint64_t need) {
    if (need > 16384) throw std::invalid_argument("iou3d_nms_ext: at most 16384 boxes a side");
    if (!g_boxes || need > g_cap) {
        uint32_t cap = std::max<uint32_t>(g_cap, 2048);
        while (cap < need) cap *= 2;
        if (g_boxes) lio_boxes_destroy(g_boxes);
        g_cap = 0;
        g_boxes = lio_boxes_create(0, cap);
        if (!g_boxes) throw std::runtime_error(std::string("iou3d_nms_ext: ") + lio_last_error());
        g_cap = cap;
    }
    return g_boxes;
}

void must(int64_t rc, const char* what) {
    if (rc < 0) throw std::runtime_error(std::string("iou3d_nms_ext: ") + what + ": " + lio_last_error());
}

uint32_t rows_of(const farray& boxes) {
    if (boxes.ndim() != 2 || boxes.shape(1) != 7) throw std::invalid_argument("iou3d_nms_ext: boxes must be (N, 7)");
    return (uint32_t)boxes.shape(0);
}

float* out_of(py::array_t<float>& ans, uint32_t na, uint32_t nb) {
    if (!(ans.flags() & py::array::c_style) || !ans.writeable() || (uint64_t)ans.size() != (uint64_t)na * nb)
        throw std::invalid_argument("iou3d_nms_ext: the output must be a writeable C-contiguous float32 (N, M)");
    return ans.mutable_data();
}

// which: 0 overlap, 1 hull, 2 IoU, 3 GIoU3D
int pairwise(const farray& a, const farray& b, py::array_t<float>& ans, int which) {
    const uint32_t na = rows_of(a), nb = rows_of(b);
    float* out[4] = {nullptr, nullptr, nullptr, nullptr};
    out[which] = out_of(ans, na, nb);
    if (na == 0 || nb == 0) return 1;
    must(lio_boxes_pairwise(handle(std::max(na, nb)), a.data(), na, b.data(), nb, out[0], out[1], out[2], out[3]), "pairwise");
    return 1;
}

int boxes_overlap_bev_gpu(farray boxes_a, farray boxes_b, py::array_t<float> ans_overlap) { return pairwise(boxes_a, boxes_b, ans_overlap, 0); }
int boxes_union_bev_gpu(farray boxes_a, farray boxes_b, py::array_t<float> ans_union) { return pairwise(boxes_a, boxes_b, ans_union, 1); }
int boxes_iou_bev_cpu(farray boxes_a, farray boxes_b, py::array_t<float> ans_iou) { return pairwise(boxes_a, boxes_b, ans_iou, 2); }
int boxes_giou3d(farray boxes_a, farray boxes_b, py::array_t<float> ans_giou) { return pairwise(boxes_a, boxes_b, ans_giou, 3); }

int64_t nms_into(const farray& boxes, const float* scores, py::array_t<int64_t>& keep, float thresh, int mode, uint32_t max_out) {
    const uint32_t n = rows_of(boxes);
    if (!(keep.flags() & py::array::c_style) || !keep.writeable() || (uint64_t)keep.size() < n)
        throw std::invalid_argument("iou3d_nms_ext: keep must be a writeable C-contiguous int64 array of N");
    if (n == 0) return 0;
    const int64_t kept = lio_boxes_nms(handle(n), boxes.data(), scores, n, thresh, mode, max_out, keep.mutable_data());
    must(kept, "nms");
    return kept;
}

int64_t nms_gpu(farray boxes, py::array_t<int64_t> keep, float nms_overlap_thresh) {
    return nms_into(boxes, nullptr, keep, nms_overlap_thresh, LIO_BOXES_NMS_ROTATED, 0);
}

int64_t nms_scored(farray boxes, farray scores, py::array_t<int64_t> keep, float thresh, int mode, uint32_t max_out) {
    if ((uint64_t)scores.size() != (uint64_t)rows_of(boxes)) throw std::invalid_argument("iou3d_nms_ext: one score per box");
    return nms_into(boxes, scores.data(), keep, thresh, mode, max_out);
}

py::tuple postprocess(farray boxes, farray scores, iarray labels, farray class_thresh, float nms_thresh, uint32_t post_max, int mode) {
    const uint32_t n = rows_of(boxes);
    if ((uint64_t)scores.size() != n || (uint64_t)labels.size() != n) throw std::invalid_argument("iou3d_nms_ext: one score and one label per box");
    const uint32_t room = (post_max == 0 || post_max > n) ? n : post_max;
    py::array_t<float> ob(py::array::ShapeContainer({(py::ssize_t)room, (py::ssize_t)7})), os(py::array::ShapeContainer({(py::ssize_t)room}));
    py::array_t<int32_t> ol(py::array::ShapeContainer({(py::ssize_t)room}));
    py::array_t<uint32_t> oi(py::array::ShapeContainer({(py::ssize_t)room}));
    int64_t kept = 0;
    if (n > 0) {
        lio_boxes* h = handle(n);
        must(lio_boxes_set_gate(h, mode), "set_gate");
        kept = lio_boxes_postprocess(h, boxes.data(), scores.data(), labels.data(), n, class_thresh.data(), (int)class_thresh.size(), nms_thresh, post_max,
                                     ob.mutable_data(), os.mutable_data(), ol.mutable_data());
        must(kept, "postprocess");
        must(lio_boxes_last_indices(h, oi.mutable_data(), room), "last_indices");
    }
    return py::make_tuple(kept, ob, os, ol, oi);
}

}  // namespace

PYBIND11_MODULE(iou3d_nms_ext, m) {
    m.doc() = "rotated box overlap, hull, IoU and NMS on the device";
    m.def("boxes_overlap_bev_gpu", &boxes_overlap_bev_gpu, "oriented boxes overlap");
    m.def("boxes_union_bev_gpu", &boxes_union_bev_gpu, "oriented boxes union");
    m.def("nms_gpu", &nms_gpu, "oriented nms gpu");
    m.def("boxes_iou_bev_cpu", &boxes_iou_bev_cpu, "oriented boxes iou");
    // this project's (leading underscore: not part of the reference's surface)
    m.def("_giou3d", &boxes_giou3d, "GIoU3D of iou3d_nms.py's boxes_giou3d_gpu, one pass over the pair");
    m.def("_nms", &nms_scored, py::arg("boxes"), py::arg("scores"), py::arg("keep"), py::arg("thresh"), py::arg("mode") = 0, py::arg("max_out") = 0);
    m.def("_postprocess", &postprocess, py::arg("boxes"), py::arg("scores"), py::arg("labels"), py::arg("class_thresh"), py::arg("nms_thresh"),
          py::arg("post_max"), py::arg("mode") = 0);
}
