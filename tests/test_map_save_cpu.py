"""A map's way to disk from mapping mode, the parts that need no device: the ABI of revision 21, the g2o writer against the reader, align_pose against
its numpy restatement (tests/map_save_cases.py), and dump_graph / del_graph_vertex without a pose graph."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lidar-slam-detection_amd", "python")
for p in (PKG, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import map_save_cases as MC  # noqa: E402
from lsd_amd import capi  # noqa: E402

HEADER = os.path.join(ROOT, "include", "lio_hip.h")
NEW = ["lio_graph_remove_node", "lio_graph_node_live", "lio_graph_edge_records", "lio_loop_retire"]


def _module():
    import slam_wrapper

    assert slam_wrapper.__file__.endswith(".so"), slam_wrapper.__file__
    return slam_wrapper


def test_header_and_abi():
    hdr = open(HEADER).read()
    rev = int(re.search(r"#define LIO_ABI_VERSION (\d+)", hdr).group(1))
    assert rev >= 21 and capi.lib().lio_abi_version() == rev
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in capi.SYMBOLS and getattr(capi.lib(), name) is not None
    # each declaration cites the reference lines it replaces
    assert "hdl_graph_slam_nodelet.cpp:868-891" in hdr and "graph_slam.cpp:154-156" in hdr and "hdl_graph_slam_nodelet.cpp:1088-1110" in hdr
    # a NULL handle is refused before anything is touched: no device needed
    L = capi.lib()
    assert L.lio_graph_remove_node(None, 0) == capi.LIO_E_INVALID and L.lio_graph_node_live(None, None, 0) == capi.LIO_E_INVALID
    assert L.lio_graph_edge_records(None, None, None, None, None, None, None, None, 0) == capi.LIO_E_INVALID and L.lio_loop_retire(None, 0) == capi.LIO_E_INVALID


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_write_g2o_read_g2o_round_trip(tmp_path):
    """8 vertices (2 fixed), 9 edges with random SPD information, 2 GNSS priors, 3 kernels: 17 significant digits give every double back bit for
    bit; the priors are still passed over by the reader's graph (the skipped count) and kept beside it under the new key"""
    sw = _module()
    rec = MC.g2o_record()
    assert len(rec["vertices"]) == 8 and len(rec["fixed"]) == 2 and len(rec["edges"]) == 9 and len(rec["priors"]) == 2
    path = str(tmp_path / "graph.g2o")
    sw._write_g2o(path, rec)
    got = sw._read_g2o(path)
    assert sorted(got["vertices"]) == sorted(rec["vertices"])
    for i, v in rec["vertices"].items():
        assert np.array_equal(_bits(got["vertices"][i]), _bits(v)), i
    assert len(got["edges"]) == len(rec["edges"])
    for (a, b, m, W), (a2, b2, m2, W2) in zip(rec["edges"], got["edges"]):
        assert (a, b) == (a2, b2) and np.array_equal(_bits(m), _bits(m2)) and np.array_equal(_bits(W), _bits(W2))
    assert sorted(got["fixed"]) == sorted(rec["fixed"])
    assert got["skipped"] == 2
    assert [(t, n) for t, n, _ in got["priors"]] == [(t, n) for t, n, _ in rec["priors"]]
    for (_, _, v), (_, _, v2) in zip(rec["priors"], got["priors"]):
        assert np.array_equal(_bits(v), _bits(v2))
    assert [(list(v), t, d) for v, t, d in got["kernels"]] == [(list(v), t, d) for v, t, d in rec["kernels"]]
    # the text: tags and field order of g2o's writer and of the reference's own edge classes; a FIX line behind its vertex
    lines = open(path).read().splitlines()
    tags = [ln.split()[0] for ln in lines]
    assert tags.count("VERTEX_SE3:QUAT") == 8 and tags.count("FIX") == 2 and tags.count("EDGE_SE3:QUAT") == 9
    assert tags.count("EDGE_SE3_PRIORXYZ") == 1 and tags.count("EDGE_SE3_PRIORQUAT") == 1
    assert lines[tags.index("FIX")] == "FIX 0" and lines[tags.index("FIX") - 1].startswith("VERTEX_SE3:QUAT 0 ")
    assert len(lines[tags.index("EDGE_SE3:QUAT")].split()) == 3 + 7 + 21 and len(lines[tags.index("EDGE_SE3_PRIORXYZ")].split()) == 2 + 3 + 6
    assert len(lines[tags.index("EDGE_SE3_PRIORQUAT")].split()) == 2 + 4 + 6
    assert open(path + ".kernels").read().splitlines()[0].split()[:4] == ["2", "21", "0", "Huber"]
    # written a second time from what was read: the same bytes
    sw._write_g2o(str(tmp_path / "again.g2o"), got)
    assert open(str(tmp_path / "again.g2o")).read() == open(path).read()


@pytest.mark.parametrize("name", sorted(MC.align_cases()))
def test_align_pose_against_the_restatement(name):
    """Both sides make the same dozen 4 x 4 f64 products and inverses (relative poses, the two deltas, pose * plus, estimate1 * pose).  One product
    of rigid matrices whose translations stay below L is wrong by at most 4 u (|A| |B|) <= 16 L u per entry (u = 2^-53), and a factor carrying such
    an error is multiplied by entries up to L again: 12 * 16 * L^2 * u in all, 1.9e-11 for L = 30.  The inverses differ in kind (cofactors here, LU
    in numpy) but not in that order.  The float the rotation vector's norm goes through is the same on both sides unless the two f64 norms fall on
    either side of a float's rounding boundary: 1e-15 against a spacing of 6e-8."""
    sw = _module()
    s1, s2, e1, e2, stamps, poses = MC.align_cases()[name]
    want = MC.align_pose(s1, s2, e1, e2, stamps, poses)
    got = sw.align_pose(s1, s2, e1, e2, stamps, [p.copy() for p in poses])
    assert len(got) == len(want) == len(poses)
    if not poses:
        return
    L = max(1.0, max(np.abs(np.asarray(T)[:3, 3]).max() for T in list(poses) + [e1, e2] + want))
    assert L <= 30.0
    tol = 12 * 16 * L * L * 2.0 ** -53
    err = max(np.abs(np.asarray(g) - w).max() for g, w in zip(got, want))
    moved = max(np.abs(np.asarray(g) - p).max() for g, p in zip(got, poses))
    print(name, "L", L, "tol", tol, "err", err, "moved from the input by", moved)
    assert err <= tol
    assert all(np.asarray(g).dtype == np.float64 and np.asarray(g).shape == (4, 4) for g in got)
    assert moved > 1e-3  # not the input handed back
    if name == "pure_translation":  # the norm < 1e-8 branch: no rotation is added
        assert all(np.array_equal(np.asarray(g)[:3, :3], np.eye(3)) for g in got)
    if name == "walk_with_rotation":  # the last pose lands on estimate2 when the duration is the list's span
        assert np.abs(np.asarray(got[-1]) - e2).max() < 1e-9
    if name == "duration_is_not_the_span":
        assert np.abs(np.asarray(got[-1]) - e2).max() > 1e-3


def test_dump_graph_and_del_vertex_without_a_graph(tmp_path):
    sw = _module()
    assert sw.init_slam("mapping", "", "FastLIO", ["0-lidar", "IMU"], 0.5, 0.2, 10.0, 60.0) == ["IMU", "0-lidar"]
    try:
        d = tmp_path / "out"
        d.mkdir()
        assert sw.dump_graph(str(d)) == [] and sw.del_graph_vertex(3) is None and sw.del_graph_vertex(-1) is None
        assert os.listdir(str(d)) == []
        assert sw.get_graph_map() == {"points": {}, "images": {}, "poses": {}, "stamps": {}} and sw.get_graph_meta() == {}
        sw.dump_odometry(str(d))  # an empty list still makes the file
        assert os.listdir(str(d)) == ["odometrys.txt"] and open(str(d / "odometrys.txt")).read() == ""
    finally:
        sw.deinit_slam()
    assert sw.dump_graph(str(tmp_path)) == [] and sw.del_graph_vertex(0) is None  # no session at all
