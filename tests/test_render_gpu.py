"""The colour map on the device (csrc/render.hip through lio.ColourMap) against the numpy restatement of tests/render_cases.py: every case,
frame by frame.  Voxel keys, numbering, hits, stored points, z-buffer owners and valid flags are equal; stored rgb, score and depth are equal
bit for bit (the rules fix the order of every IEEE operation, so a difference is a bug, not a tolerance); the export is equal as bytes."""
import numpy as np
import pytest

import render_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lio():
    from lsd_amd import capi, lio

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    return lio


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make(lio, c, **over):
    cm = lio.ColourMap(max_voxels=over.get("max_voxels", c["max_voxels"]), max_points=over.get("max_points", c["max_points"]))
    cm.set_cameras(c["cameras"], c["lidar_static"])
    return cm


def same_image(cm, want, where):
    got = cm.last_image()
    assert got["owner"].shape == want["owner"].shape, where
    assert np.array_equal(got["owner"], want["owner"]), (where, "owners", int(np.sum(got["owner"] != want["owner"])))
    assert np.array_equal(got["valid"], want["valid"]), (where, "valid flags", int(np.sum(got["valid"] != want["valid"])))
    assert np.array_equal(bits(got["depth"]), bits(want["depth"])), (where, "depth buffer")


def same_map(cm, p, where):
    want = p.state()
    assert cm.size() == (len(want["hits"]), len(want["score"])), where
    v, q = cm.voxels(), cm.points()
    for k in ("box", "hits", "counts"):
        assert np.array_equal(v[k], want[k]), (where, k)
    assert np.array_equal(q["voxel"], want["voxel"]), (where, "voxel of point")
    for k in ("xyz", "rgb", "score", "depth"):
        d = bits(q[k]) != bits(want[k])
        assert not d.any(), (where, k, int(d.sum()), q[k][d][:4], want[k][d][:4])
    got, exp = cm.colour_map(), p.colour_map()
    assert got.shape == exp.shape and got.tobytes() == exp.tobytes(), (where, "export")


def drive(cm, c, p, outcomes):
    for i, f in enumerate(c["frames"]):
        out = cm.frame(f["points"], f["pose"], f["images"], use_ground=c["ground"], seed=f.get("seed", 0))
        assert out == outcomes[i], (i, out, outcomes[i])
        snap = p.snapshots[i]
        assert cm.size() == snap["size"], i
        if snap["image"] is not None:
            same_image(cm, snap["image"], f"frame {i}")


@pytest.mark.parametrize("name", rc.KERNEL_CASES)
def test_case_equals_the_restatement(lio, name):
    c = rc.case(name)
    p, outcomes = rc.reference(name)
    cm = make(lio, c)
    drive(cm, c, p, outcomes)
    same_map(cm, p, name)
    assert len(cm.colour_map()) > 100


def test_last_row_and_column_tap_is_not_read(lio):
    """u = 100, v = 119 in a 160 x 120 image: the taps at row 120 have weight zero and lie outside the image"""
    c = rc.edge_tap_case()
    p, outcomes = rc.run(c)
    assert outcomes == ["rendered"] and p.snapshots[0]["image"]["owner"][119, 100] == 0 and p.score[0] == np.float32(0.75)
    cm = make(lio, c)
    drive(cm, c, p, outcomes)
    same_map(cm, p, "edge tap")


def test_ground_test_on_renders_and_no_floor_does_not(lio):
    det = lio.GroundDetector()

    def ground(pts, seed):
        r = det.detect_host(pts, det.params(0, distance_threshold=rc.GROUND_THRESHOLD, seed=seed))
        return det.inliers() if r["found"] else None

    c = rc.case("ground")
    p, outcomes = rc.run("ground", ground)
    assert outcomes == ["rendered", "rendered", "no_floor", "rendered", "rendered"]
    assert all(s["size"][1] > 500 for s in p.snapshots) and p.snapshots[2]["size"] == p.snapshots[1]["size"]
    cm = make(lio, c)
    drive(cm, c, p, outcomes)
    same_map(cm, p, "ground")
    # last_pose moves before the ground test: 5 cm after a frame without a floor is "skipped", though 35 cm from the last rendered frame
    cm2 = make(lio, c)
    fr = c["frames"]
    assert cm2.frame(fr[0]["points"], fr[0]["pose"], {}, use_ground=True, seed=40) == "rendered"
    assert cm2.frame(fr[2]["points"], fr[1]["pose"], {}, use_ground=True, seed=41) == "no_floor"
    assert cm2.frame(fr[0]["points"], fr[1]["pose"] @ rc.se3(None, (0.05, 0, 0)), {}, use_ground=True, seed=42) == "skipped"
    assert cm2.size() == p.snapshots[0]["size"]


def test_capacity_overflow_leaves_the_map_unchanged_and_clear_empties_it(lio):
    from lsd_amd import capi

    c = rc.case("one_camera")
    ref, _ = rc.reference("one_camera")
    n_vox, n_pts = ref.snapshots[2]["size"]
    for over in (dict(max_points=n_pts + 10), dict(max_voxels=n_vox + 3)):
        cm = make(lio, c, **over)
        p = rc.Painter(c["cameras"], c["lidar_static"])
        for f in c["frames"][:3]:
            assert cm.frame(f["points"], f["pose"], f["images"], use_ground=False) == p.frame(f["points"], f["pose"], f["images"])
        same_map(cm, p, "before the overflow")
        f = c["frames"][4]
        with pytest.raises(capi.LioError, match="does not fit"):
            cm.frame(f["points"], f["pose"], f["images"], use_ground=False)
        same_map(cm, p, "after the overflow")
        p.last_pose = np.asarray(f["pose"], np.float64).copy()  # the gate had passed
        assert cm.frame(f["points"], f["pose"], f["images"], use_ground=False) == "skipped"
        # the tables took their tentative entries back: after clear (the map only) later frames land as in a fresh painter
        cm.clear()
        p.clear()
        assert cm.size() == (0, 0) and len(cm.colour_map()) == 0
        small = c["frames"][5]["points"][:400]
        for k in (5, 6):
            f = c["frames"][k]
            assert cm.frame(small, f["pose"], f["images"], use_ground=False) == p.frame(small, f["pose"], f["images"]) == "rendered"
        same_map(cm, p, "after clear")


def test_two_handles_do_not_share_state(lio):
    ca, cb = rc.case("integer_pixels"), rc.case("two_cameras")
    (pa, oa), (pb, ob) = rc.reference("integer_pixels"), rc.reference("two_cameras")
    a, b = make(lio, ca), make(lio, cb)
    for i in range(max(len(ca["frames"]), len(cb["frames"]))):
        for cm, c, o in ((a, ca, oa), (b, cb, ob)):
            if i < len(c["frames"]):
                f = c["frames"][i]
                assert cm.frame(f["points"], f["pose"], f["images"], use_ground=False) == o[i]
    same_map(a, pa, "first handle")
    same_map(b, pb, "second handle")


def test_inactive_painter_and_bad_arguments(lio):
    c = rc.case("integer_pixels")
    cm = make(lio, c)
    f = c["frames"][1]
    cm.set_active(False)
    assert cm.frame(f["points"], f["pose"], f["images"], use_ground=False) == "skipped" and cm.size() == (0, 0)
    cm.set_active(True)
    with pytest.raises(ValueError):
        cm.frame(f["points"], f["pose"], {"down": (np.zeros((180, 160), np.uint8), f["pose"])}, use_ground=False)  # a 2-D (I420) image
    with pytest.raises(ValueError):
        cm.frame(f["points"], f["pose"], {"nobody": (np.zeros((120, 160, 3), np.uint8), f["pose"])}, use_ground=False)
    assert cm.size() == (0, 0)
    # no images: the voxels are hit all the same
    assert cm.frame(f["points"], f["pose"], {}, use_ground=False) == "rendered"
    v = cm.voxels()
    assert len(v["hits"]) > 0 and np.all(v["hits"] == 1) and cm.last_image()["owner"].size == 0
    t = cm.last_times()
    assert t["insert_us"] > 0
