"""The colour map without a GPU: the numpy restatement (tests/render_cases.py) against hand-worked values, the ABI revision, the refusals
without a device, and the cases themselves -- every branch of the rules is taken by at least one of them, and none of them sits within 1e-6 of
a boundary where a last-bit difference could flip a decision.

One branch the issue lists cannot be taken by any input: "a colliding key from a different cell".  key = ox 100 + oy 10 + oz is not injective
over offsets 0 .. 10, but the offsets of ONE voxel are ten consecutive values per axis (0 .. 9 or 1 .. 10, by the sign of the coordinate and the
rounding of (box 0.2) 50): x * 5 and x * 50 are exact in f64 for an f32 x, so the cell can never leave the voxel's own ten.  Over ten
consecutive digits the key is injective.  test_key_collisions shows the collision on the formula, shows that it needs eleven values on one axis,
and checks the ten-value span over a few million points; the coverage test requires the duplicate branch and that the other one stays empty."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import render_cases as rc

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "lio_hip.h")


def test_header_and_library_are_at_revision_20_with_every_render_symbol():
    from lsd_amd import capi

    hdr = int(re.search(r"#define LIO_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    assert capi.lib().lio_abi_version() == hdr >= 20
    names = [s for s in capi.SYMBOLS if s.startswith("lio_render_")]
    assert len(names) == 12
    for n in names:
        assert hasattr(capi.lib(), n)
    assert (capi.RENDER_SKIPPED, capi.RENDER_NO_FLOOR, capi.RENDER_DONE) == (0, 1, 2)
    txt = open(HEADER).read()
    for word, value in (("LIO_RENDER_SKIPPED", 0), ("LIO_RENDER_NO_FLOOR", 1), ("LIO_RENDER_DONE", 2)):
        assert re.search(rf"#define {word} {value}\b", txt)


def test_image_struct_layout_matches_the_header(tmp_path):
    import subprocess

    from lsd_amd import capi

    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "lio_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(lio_render_image), '
           "offsetof(lio_render_image, rows), offsetof(lio_render_image, cols), offsetof(lio_render_image, bgr), offsetof(lio_render_image, pose)); return 0; }\n")
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.dirname(HEADER), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R = capi.RenderImage
    assert got == [C.sizeof(R), R.rows.offset, R.cols.offset, R.bgr.offset, R.pose.offset]


def test_null_handles_are_refused_and_nothing_is_thrown():
    from lsd_amd import capi

    L = capi.lib()
    assert L.lio_render_clear(None) == capi.LIO_E_INVALID
    assert L.lio_render_set_active(None, 1) == capi.LIO_E_INVALID
    assert L.lio_render_set_cameras(None, 0, None, None, None, None) == capi.LIO_E_INVALID
    assert L.lio_render_frame(None, None, 0, None, 0, 0, None, 0) == capi.LIO_E_INVALID
    assert L.lio_render_size(None, None, None) == capi.LIO_E_INVALID
    assert L.lio_render_download(None, None, 0) == capi.LIO_E_INVALID
    assert L.lio_render_download_voxels(None, None, None, None, 0) == capi.LIO_E_INVALID
    assert L.lio_render_download_points(None, None, None, None, None, None, 0) == capi.LIO_E_INVALID
    assert L.lio_render_download_last_image(None, None, None, None, 0, None, None) == capi.LIO_E_INVALID
    assert L.lio_render_last_times(None, None, None, None) == capi.LIO_E_INVALID
    L.lio_render_destroy(None)
    assert not L.lio_render_create(0, 0, 10) and b"max_voxels" in L.lio_last_error()
    assert not L.lio_render_create(0, 1 << 30, 1 << 30)  # 4 points + 8 voxels words would pass 2^32


def test_painter_without_a_device_raises():
    from lsd_amd import capi, lio

    if capi.lib().lio_device_count() > 0:
        pytest.skip("a HIP device is visible: covered by tests/test_render_gpu.py")
    with pytest.raises(capi.LioError, match="no HIP device"):
        lio.ColourMap(max_voxels=64, max_points=256)


def test_half_away_rounding():
    got = rc.round_half_away([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999999999999994, -0.49999999999999994, 2.4999999999999996, 0.0, -0.0, 7.0])
    assert got.tolist() == [1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 0.0, -0.0, 2.0, 0.0, -0.0, 7.0]


def test_voxel_centre_offsets_and_negative_coordinates():
    """by hand: f32 0.5 is exact, 0.5 * 5 = 2.5 rounds away to box 3, (3 * 0.2) * 50 = 30.000000000000004 truncates to 30, the cell is
    int(25.0) = 25, the offset 25 - 30 + 5 = 0.  -0.5 mirrors to box -3, centre -30, cell -25, offset 10: truncation toward zero moves the
    cells of negative coordinates up by one.  f32 0.1 is 0.100000001490116: * 5 = 0.50000000745 -> box 1, centre 10, cell 5, offset 0; f32
    0.3 is 0.300000011920929: box 2 (1.50000006), centre 20, cell 15, offset 0; 0.29 -> box 1 (1.45), cell 14, offset 9; -0.29 -> box -1, centre -10,
    cell -14, offset 1.  f32 -0.02 is -0.01999999955: * 50 = -0.99999998 truncates to cell 0, like 0.0 and 0.019 (0.95): offsets 5, 5, 5."""
    w = np.array([[0.5, -0.5, 0.1], [0.3, 0.29, -0.29], [0.0, -0.02, 0.019]], np.float32)
    ok, box, centre, cell, key = rc.voxel_of(w)
    assert ok.all()
    assert box.tolist() == [[3, -3, 1], [2, 1, -1], [0, 0, 0]]
    assert centre.tolist() == [[30, -30, 10], [20, 10, -10], [0, 0, 0]]
    assert cell.tolist() == [[25, -25, 5], [15, 14, -14], [0, 0, 0]]
    assert key.tolist() == [0 * 100 + 10 * 10 + 0, 0 * 100 + 9 * 10 + 1, 5 * 100 + 5 * 10 + 5]
    assert (3 * 0.2) * 50 == 30.000000000000004 and rc.INV_POINT_RES == 50.0 and rc.INV_VOXEL_RES == 5.0
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0.2 * (1 << 20)], [1, 1, 1]], np.float32)
    assert rc.voxel_of(bad)[0].tolist() == [False, False, False, True]


def test_key_collisions():
    """the formula collides: offsets (0, 10, 3) and (1, 0, 3) both give 103, (2, 3, 10) and (2, 4, 0) both 240 -- but only with 0 AND 10 on one
    axis.  The offsets of one voxel are ten consecutive values per axis, over which the key is injective."""
    def key(o):
        return o[0] * 100 + o[1] * 10 + o[2]

    assert key((0, 10, 3)) == key((1, 0, 3)) == 103 and key((2, 3, 10)) == key((2, 4, 0)) == 240
    for lo in ((0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 1)):  # every mix of the two ranges
        keys = {key((a, b, c)) for a in range(lo[0], lo[0] + 10) for b in range(lo[1], lo[1] + 10) for c in range(lo[2], lo[2] + 10)}
        assert len(keys) == 1000
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-60, 60, 1_000_000), rng.integers(-3000, 3000, 100_000) * 0.1, rng.integers(-3000, 3000, 100_000) * 0.02,
                        rng.integers(-600, 600, 50_000) * 0.5]).astype(np.float32)
    ok, box, centre, cell, _ = rc.voxel_of(np.stack([x, x, x], axis=1))
    o, b = (cell - centre + 5)[:, 0], box[:, 0]
    assert ok.all() and o.min() >= 0 and o.max() <= 10
    order = np.argsort(b, kind="stable")
    _, start = np.unique(b[order], return_index=True)
    span = np.maximum.reduceat(o[order], start) - np.minimum.reduceat(o[order], start)
    assert span.max() == 9
    # the same cell twice is the rejection the reference has: the second point of a cell is not stored, a neighbour cell's is
    p = rc.Painter({})
    p.insert(np.array([[0.501, 0.501, 0.501], [0.505, 0.505, 0.505], [0.521, 0.501, 0.501]], np.float32))
    assert len(p.pos) == 2 and p.stats["rejected_same_cell"] == 1 and p.stats["rejected_other_cell"] == 0 and p.hits == [1]


def test_u8_terms_round_half_to_even_and_add_with_saturation():
    assert [rc.u8_term(0.5, p) for p in (1, 3, 5, 7)] == [0, 2, 2, 4]
    assert rc.u8_term(0.25, 255) == 64 and rc.u8_term(1.0, 255) == 255 and rc.u8_term(0.0, 255) == 0
    img = np.full((2, 2, 3), 255, np.uint8)
    assert rc.sample_bgr(img, 0.5, 0.5) == [255, 255, 255]  # 4 x rint(63.75) = 256, saturated
    img[:] = 2
    assert rc.sample_bgr(img, 0.5, 0.5) == [0, 0, 0]  # 4 x rint(0.5) = 0: every term is rounded on its own
    img[:] = 6
    assert rc.sample_bgr(img, 0.5, 0.5) == [8, 8, 8]  # 4 x rint(1.5) = 8
    img = np.arange(12, dtype=np.uint8).reshape(2, 2, 3) * 20
    # weights (row 0.25, col 0.5): .375, .125, .375, .125 over pixels (0,0), (1,0), (0,1), (1,1); channel 0: 0, 120, 60, 180
    assert rc.sample_bgr(img, 0.25, 0.5)[0] == 0 + int(np.rint(15.0)) + int(np.rint(22.5)) + int(np.rint(22.5)) == 59
    one = np.zeros((1, 1, 3), np.uint8) + 9
    assert rc.sample_bgr(one, 0.0, 0.0) == [9, 9, 9]  # the three taps of weight zero lie outside a 1 x 1 image and are not read


def test_projection_and_availability_by_hand():
    cam = rc.Camera((256.0, 256.0, 80.0, 60.0), np.linalg.inv(rc.se3(np.diag([1.0, -1.0, -1.0]), (0.0, 0.0, 4.0))))
    cam.set_pose(rc.se3(None, (0.25, 0.0, 0.0)))
    assert cam.R.tolist() == [[1, 0, 0], [0, -1, 0], [0, 0, -1]] and cam.t.tolist() == [-0.25, 0.0, 4.0]
    ok, u, v, z = cam.project(np.array([[0.5, 0.25, 0.0], [0.0, 0.0, 3.9995], [0.0, 0.0, 4.5]]))
    assert ok.tolist() == [True, False, False] and (u[0], v[0], z[0]) == (96.0, 44.0, 4.0)
    # 160 x 120: u in [1.8, 159], v in [1.6, 119]
    a = rc.Camera.available(160, 120, np.array([1.8, 1.79, 159.0, 159.01, 80.0, 80.0, 80.0]), np.array([60.0, 60.0, 60.0, 60.0, 1.6, 119.0, 119.2]))
    assert a.tolist() == [True, False, True, False, True, True, False]
    k = rc.Camera((300.1, 1, 2, 3), np.eye(4))
    assert k.fx == float(np.float32(300.1)) != 300.1


def test_f32_depth_decides_the_pixel_and_ties_go_to_the_smaller_serial():
    """a camera 4 m above the plane z = 0, looking down with f = 256: u = 64 x + 80, v = 60 - 64 y.  Points 0 and 1 lie in neighbouring cells
    of one pixel; their f64 depths differ (4 and 4 - 1e-8), their f32 depths do not: the earlier serial owns the pixel although its f64 depth
    is the larger.  Point 5 (0.09 m up: depth 3.91, u = 80 + 0.335 * 256 / 3.91 = 101.93) is really nearer than point 4 in pixel (38, 102).
    The other points spread their voxels over more than 10 px, so that neither is masked; point 2 sits on a whole pixel."""
    E = np.linalg.inv(rc.se3(np.diag([1.0, -1.0, -1.0]), (0.0, 0.0, 4.0)))
    p = rc.Painter({"down": ((256.0, 256.0, 80.0, 60.0), E)})
    pts = np.array([[0.019, 0.0, 0.0, 0], [0.021, 0.0, 1e-8, 0], [-0.09375, -0.09375, 0.0, 0], [0.09, 0.09, 0.0, 0],
                    [0.35, 0.35, 0.0, 0], [0.335, 0.335, 0.09, 0], [0.31, 0.31, 0.0, 0], [0.49, 0.49, 0.0, 0]], np.float32)
    pts[:, 0] -= 0.5
    img = rc.image(120, 160, 1)
    assert p.frame(pts, rc.se3(None, (0.5, 0.0, 0.0)), {"down": (img, np.eye(4))}) == "rendered"
    assert len(p.pos) == 8 and p.hits == [1, 1]
    own, dep = p.last_image["owner"], p.last_image["depth"]
    assert own[60, 81] == 0 and own[38, 102] == 5 and own[66, 74] == 2
    assert p.stats["losers"] == 2 and p.stats["serial_ties"] == 1 and p.stats["masked"] == 0
    assert dep[60, 81] == np.float32(4.0) and dep[38, 102] == np.float32(4.0 - float(np.float32(0.09))) and dep[0, 0] == -1
    assert p.last_image["valid"].sum() == 6
    # the blend of a first sample on a whole pixel: rgb = the pixel, score = 1 - |74 - 80| / 80; a loser keeps its zeros
    assert p.score[2] == np.float32(0.925) and p.rgb[2].tolist() == [float(img[66, 74, 2]), float(img[66, 74, 1]), float(img[66, 74, 0])]
    assert p.score[1] == 0 and p.depth[1] == np.float32(100.0) and p.depth[0] == np.float32(4.0) and p.score[4] == 0


def test_blend_by_hand():
    """nine points of one voxel (spread over 11.5 px, so it is not masked) under the same camera.  The point (0.625, 0, 0) is seen at u = 120
    (score 0.5), then by a camera 0.3125 m back at u = 140 (score 0.25): rgb = (r1 * 0.5 + r2 * 0.25) / 0.75 and the score stays 0.5.  A camera
    6.5 m up (f = 512) is refused in between: 6.5 > 1.5 * 4."""
    E = np.linalg.inv(rc.se3(np.diag([1.0, -1.0, -1.0]), (0.0, 0.0, 4.0)))
    far = np.linalg.inv(rc.se3(np.diag([1.0, -1.0, -1.0]), (0.0, 0.0, 6.5)))
    p = rc.Painter({"a": ((256.0, 256.0, 80.0, 60.0), E), "b": ((512.0, 512.0, 80.0, 60.0), far)})
    cloud = np.array([[x, y, 0.0, 0] for x in (0.51, 0.625, 0.69) for y in (-0.09, 0.0, 0.09)], np.float32)
    s = 4  # the point (0.625, 0, 0)
    img1, img2 = rc.image(120, 160, 2), rc.image(120, 160, 3)
    cloud1 = cloud.copy()
    cloud1[:, 0] -= 1.0
    assert p.frame(cloud1, rc.se3(None, (1.0, 0.0, 0.0)), {"a": (img1, np.eye(4))}) == "rendered"
    assert p.pos[s].tolist() == [0.625, 0.0, 0.0] and p.score[s] == np.float32(0.5) and p.stats["masked"] == 0
    r1 = float(img1[60, 120, 2])
    assert p.rgb[s][0] == np.float32(r1)
    cloud2 = cloud.copy()
    cloud2[:, 0] = (cloud[:, 0].astype(np.float64) - 1.3).astype(np.float32)
    p.frame(cloud2, rc.se3(None, (1.3, 0.0, 0.0)), {"b": (img2, np.eye(4)), "a": (img2, rc.se3(None, (-0.3125, 0.0, 0.0)))})
    assert p.hits == [2] and len(p.pos) == len(cloud)  # the second frame's points fall into held cells
    r2 = float(img2[60, 140, 2])
    assert p.rgb[s][0] == np.float32((r1 * 0.5 + r2 * 0.25) / 0.75) and p.score[s] == np.float32(0.5)
    assert p.stats["too_deep"] == 9 and p.depth[s] == np.float32(4.0)
    assert len(p.colour_map()) == 0  # two hits only: getColorMap wants more than two


def test_gate_by_hand():
    p = rc.Painter({})
    pts = np.zeros((1, 4), np.float32)
    assert p.frame(pts, np.eye(4)) == "skipped"                       # last_pose starts as the identity
    assert p.frame(pts, rc.se3(None, (0.0999, 0, 0))) == "skipped"
    assert p.frame(pts, rc.se3(None, (0.06, 0.08, 0))) == "rendered"    # sqrt(0.0036 + 0.0064) = 0.1 is not < 0.1
    assert p.frame(pts, rc.se3(None, (0.06, 0.08, 0.05))) == "skipped"  # measured from the last RENDERED pose
    assert p.frame(pts, rc.se3(None, (0.3, 0, 0)), ground=lambda q: None) == "no_floor"
    assert p.frame(pts, rc.se3(None, (0.35, 0, 0))) == "skipped"        # last_pose moved before the ground test
    q = rc.Painter({}, active=False)
    assert q.frame(pts, rc.se3(None, (1, 0, 0))) == "skipped" and q.hits == []
    with pytest.raises(ValueError):
        rc.Painter({}).frame(pts, rc.se3(None, (1, 0, 0)), {"x": (np.zeros((180, 320), np.uint8), np.eye(4))})


def test_export_packs_truncated_channels():
    p = rc.Painter({})
    p.insert(np.array([[0.5, 0.5, 0.5]], np.float32))
    p.hits[0], p.score[0], p.rgb[0] = 3, np.float32(0.1), np.array([255.0, 12.999, 0.5], np.float32)
    out = p.colour_map()
    assert out.shape == (1, 4) and out[0, :3].tolist() == [0.5, 0.5, 0.5] and out[0, 3:].view(np.uint32)[0] == (255 << 16 | 12 << 8 | 0)
    p.score[0] = np.float32(0.0999)
    assert len(p.colour_map()) == 0
    p.score[0], p.hits[0] = np.float32(0.5), 2
    assert len(p.colour_map()) == 0


@pytest.mark.parametrize("name", rc.KERNEL_CASES)
def test_cases_keep_their_distance_from_every_boundary(name):
    """no projection within 1e-6 px of a rounding or availability boundary, no sample term within 1e-6 of a half"""
    p, _ = rc.reference(name)
    assert p.stats["min_boundary_margin"] > 1e-6, p.stats
    assert p.stats["min_term_margin"] > 1e-6, p.stats
    n = [len(f["points"]) for f in rc.case(name)["frames"]]
    if name != "integer_pixels":
        assert 2000 <= min(n) and max(n) <= 4000


def test_cases_take_every_branch():
    total = {}
    outcomes = {}
    for name in rc.KERNEL_CASES:
        p, out = rc.reference(name)
        outcomes[name] = out
        for k, v in p.stats.items():
            if not k.startswith("min_"):
                total[k] = total.get(k, 0) + v
        h = p.state()["hits"]
        total["hits_le_2"] = total.get("hits_le_2", 0) + int((h <= 2).sum())
        total["hits_gt_2"] = total.get("hits_gt_2", 0) + int((h > 2).sum())
        total["exported"] = total.get("exported", 0) + len(p.colour_map())
    for k in ("rejected_same_cell", "gated", "masked", "losers", "serial_ties", "discontinuous", "low_score", "too_deep", "two_cameras", "skipped", "rendered",
              "hits_le_2", "hits_gt_2", "exported", "blended"):
        assert total[k] > 0, (k, total)
    assert total["rejected_other_cell"] == 0  # (cannot happen: see the module's docstring and test_key_collisions)
    for name in ("one_camera", "two_cameras", "three_cameras_static"):
        o = outcomes[name]
        assert o[0] == "skipped" and o.count("skipped") == 2 and 4 <= o.count("rendered") <= 6  # the first frame at the identity, one 5 cm step
        assert len(rc.case(name)["cameras"]) == {"one_camera": 1, "two_cameras": 2, "three_cameras_static": 3}[name]
    assert rc.reference("two_cameras")[0].stats["too_deep"] > 0 and rc.reference("three_cameras_static")[0].stats["two_cameras"] > 0
    ip = rc.reference("integer_pixels")[0]
    assert ip.stats["serial_ties"] > 0
    c = rc.case("integer_pixels")
    assert c["frames"][0]["images"]["down"][0].shape == (120, 160, 3)
    g = rc.case("ground")
    assert g["ground"] and all(2500 <= len(f["points"]) for i, f in enumerate(g["frames"]) if i != 2)


def test_integer_pixels_really_are_integers():
    """the lattice of the 160 x 120 case projects onto whole pixels in every rendered frame, so three taps have weight zero"""
    c = rc.case("integer_pixels")
    cam = rc.Camera(*c["cameras"]["down"])
    f = c["frames"][1]
    cam.set_pose(f["pose"])
    w = rc.transform_f32(f["pose"], f["points"][: c["lattice"], :3])
    ok, u, v, z = cam.project(w.astype(np.float64))
    assert ok.all() and np.all(u == np.floor(u)) and np.all(v == np.floor(v)) and np.all(z == 4.0)
    e = rc.edge_tap_case()
    f = e["frames"][0]
    cam.set_pose(f["images"]["down"][1])
    ok, u, v, z = cam.project(rc.transform_f32(f["pose"], f["points"][:1, :3]).astype(np.float64))
    assert (u[0], v[0]) == (100.0, 119.0) and rc.Camera.available(160, 120, u, v)[0]
    p, out = rc.run(e)
    assert out == ["rendered"] and p.snapshots[0]["image"]["owner"][119, 100] == 0 and p.snapshots[0]["image"]["valid"][119, 100] == 1
    img = f["images"]["down"][0]
    assert p.rgb[0].tolist() == [float(img[119, 100, 2]), float(img[119, 100, 1]), float(img[119, 100, 0])]  # one tap, the others are not read


def test_module_stamp_pose_refusals_and_interpolation():
    """get_stamp_pose (graph_utils.cpp:514-544) is host code: no odometry, a stamp outside the odometry, no pair from the start index on --
    and a stamp that EQUALS the stamp at the start index finds no pair either (first == second), as in the reference"""
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(HEADER), "..", "lidar-slam-detection_amd", "python"))
    import slam_wrapper as sw

    sw.set_map_odometrys(np.zeros((0, 8)))
    assert sw._stamp_pose(5, 0)[0] is False
    od = np.array([[1_000_000 + 50_000 * i, 0.3 + 0.15 * i, 0.01 * i, 0.0, 0.0, 0.0, np.sin(0.002 * i), np.cos(0.002 * i)] for i in range(11)])
    sw.set_map_odometrys(od)
    assert [sw._stamp_pose(s, 0)[0] for s in (999_999, 1_500_001, 1_000_000)] == [False, False, False]
    assert sw._stamp_pose(1_025_000, 3)[0] is False and sw._stamp_pose(1_225_000, 3)[:2] == (True, 4) and sw._stamp_pose(1_500_000, 0)[:2] == (True, 9)
    ok, idx, T = sw._stamp_pose(1_025_000, 0)
    assert ok and idx == 0
    yaw = 0.5 * 0.004  # half way between yaw 0 and 2 * 0.002
    want = np.eye(4)
    want[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    want[:3, 3] = [0.375, 0.005, 0.0]
    assert np.allclose(T, want, atol=1e-12)
    # a general pair: the interpolated rotation is pre * exp(ratio * log(pre^-1 next)) and stays orthonormal
    q1 = np.array([0.1, -0.2, 0.3, 0.9]); q1 /= np.linalg.norm(q1)
    q2 = np.array([0.15, -0.1, 0.35, 0.88]); q2 /= np.linalg.norm(q2)
    sw.set_map_odometrys(np.array([[100, 1, 2, 3, *q1], [200, 2, 1, 3.5, *q2]]))
    ok, _, A = sw._stamp_pose(130, 0)
    _, _, B = sw._stamp_pose(200, 0)
    _, _, Z = sw._stamp_pose(100 + 1, 0)
    assert ok and np.allclose(A[:3, :3] @ A[:3, :3].T, np.eye(3), atol=1e-12)
    T1 = sw._tum_relative_poses(np.array([[100, 1, 2, 3, *q1], [200, 2, 1, 3.5, *q2]]))
    P, D = T1[0], T1[1][1]
    assert np.allclose(B, P @ D, atol=1e-12)
    ang = lambda R: np.arccos(np.clip((np.trace(R[:3, :3]) - 1) / 2, -1, 1))
    assert np.isclose(ang(np.linalg.inv(P) @ A), 0.3 * ang(D), atol=1e-12)
    assert np.allclose((np.linalg.inv(P) @ A)[:3, 3], 0.3 * D[:3, 3], atol=1e-12)
    sw.set_map_odometrys(np.zeros((0, 8)))
