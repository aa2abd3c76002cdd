"""The bird's-eye image without a device: the numpy restatement of tests/bev_cases.py (what tests/test_bev_gpu.py holds the device to bit for
bit) against results recorded from the reference's convert_cloud_image.py on the base scene (tests/golden/bev.npz), and the files and
arguments of lsd_amd.bev.

The golden file was recorded by running the reference's own functions with stand-ins for the three modules that are not installed: cv2 (only
imwrite, unused), third_party.pypcd (the arrays handed over directly) and torch_scatter, whose scatter_mean became
torch.zeros(n).scatter_add_(0, index, src) divided by the counts -- the call torch_scatter itself makes.

Measured, restatement against golden, base scene (60 000 points, 35 529 occupied pixels, 203 of 204 nodes running): pixel coordinates, kept
set, pixel keys, intensity and z means and the grey table are identical; every node's step count equals the reference's (0 nodes within an f32
pairwise sum's rounding distance of 20480, so NEAR_NODES is empty); 23 pixels (0.065 %) differ by one grey level, none by more."""
import numpy as np
import pytest

import bev_cases as bc

F32 = np.float32
# nodes whose deciding mean lies within the rounding distance of numpy's f32 pairwise sum from 20480, by index: measured, none
NEAR_NODES = ()
# the share of occupied pixels that differ by one grey level was measured as 23 / 35 529; rounding flips are near-random, so twice that
ONE_LEVEL_SHARE_CAP = 2 * 23 / 35529


@pytest.fixture(scope="module")
def golden():
    return np.load(bc.GOLDEN)


@pytest.fixture(scope="module")
def restated(golden):
    pts = bc.golden_points(golden)
    res = bc.restate(pts, bc.BASE_WINDOW, bc.BASE_PPM)
    for a in res.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return pts, res


def test_base_scene_is_the_recorded_one_and_its_cuts_are_unique(golden):
    pts = bc.golden_points(golden)
    assert np.array_equal(bc.base_scene().view(np.uint32), pts.view(np.uint32))
    assert bc.cut_intensities_unique(pts)  # numpy's unstable argsort cannot matter for the comparison


def test_restated_pixels_kept_set_and_means_match_the_reference_bit_for_bit(golden, restated):
    pts, r = restated
    assert (r["w"], r["h"]) == tuple(golden["image_wh"]) == (301, 201)
    assert np.array_equal(r["xy"][:, 0], golden["xs"]) and np.array_equal(r["xy"][:, 1], golden["ys"])
    kept = np.zeros(len(pts), bool)
    kept[r["kept"]] = True
    assert np.array_equal(np.packbits(kept), golden["kept"])
    assert np.array_equal(r["pkey"], golden["pix_y"].astype(np.int64) * r["w"] + golden["pix_x"])
    assert np.array_equal(r["pI"].view(np.uint32), golden["pix_i"].view(np.uint32))
    assert np.array_equal(r["pz"].view(np.uint32), golden["pix_z"].view(np.uint32))


def test_grey_table_is_exact(golden):
    from lsd_amd import lio

    table = bc.grey_table()
    assert np.array_equal(table, golden["grey"])
    assert np.count_nonzero(table != np.arange(65536)) == 88
    assert np.array_equal(lio.bev_grey_table(), table)  # the library's host function: no device needed


def test_histogram_bins_are_numpys():
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.uniform(0, 65535, 200_000).astype(F32), bc.EDGES, np.nextafter(bc.EDGES, F32(0))[1:], np.nextafter(bc.EDGES, F32(1e9))[:-1]])
    hist, edges = np.histogram(v, bins=1024, range=[0.0, 65535.0])
    assert edges.dtype == F32 and np.array_equal(edges, bc.EDGES)
    assert np.array_equal(np.bincount(bc.bins_of(v), minlength=1024), hist)


def test_step_counts_equal_the_references(golden, restated):
    _, r = restated
    assert np.array_equal(r["count"], golden["node_count"])
    assert np.count_nonzero(golden["node_step"] >= 0) == 203
    differ = np.flatnonzero(r["step"] != golden["node_step"])
    assert set(differ) <= set(NEAR_NODES), (differ, r["step"][differ], golden["node_step"][differ])
    same = np.setdiff1d(np.flatnonzero(r["step"] >= 0), differ)
    # the clip limits start from means that differ in the last places (pairwise f32 there, exact integers here) and add up to 1 200 f32 steps
    # rounded alike: a few units in the last place of an f32
    assert np.max(np.abs(r["clip"][same] - golden["node_clip"][same]) / golden["node_clip"][same]) < 8 * 2.0**-23


def test_image_is_within_one_grey_level_of_the_references(golden, restated):
    _, r = restated
    P, hp, q, W, H, nx, ny = r["geometry"]
    assert r["image"].shape == golden["image"].shape == (220, 320)
    xs, ys = golden["pix_x"].astype(np.int64), golden["pix_y"].astype(np.int64)
    d = np.abs(r["image"][ys, xs].astype(np.int64) - golden["image"][ys, xs].astype(np.int64))
    # pixels whose deciding node has another step count than the reference's are left out (none: NEAR_NODES is empty)
    held = np.ones(len(xs), bool)
    for node in NEAR_NODES:
        xi, yi = (node // ny) * hp, (node % ny) * hp
        held &= ~((np.abs(xs - xi) <= q) & (np.abs(ys - yi) <= q))
    share = np.count_nonzero(d[held]) / np.count_nonzero(held)
    print(f"pixels that differ by one grey level: {np.count_nonzero(d[held])} of {np.count_nonzero(held)} ({share:.5f}); max {d[held].max()}")
    assert d[held].max() <= 1
    assert share <= ONE_LEVEL_SHARE_CAP
    empty = np.ones(golden["image"].shape, bool)
    empty[ys, xs] = False
    assert not r["image"][empty].any() and not golden["image"][empty].any()


def test_png_round_trip(tmp_path):
    from lsd_amd import bev

    rng = np.random.default_rng(1)
    for k, img in enumerate([rng.integers(0, 65536, (37, 53)).astype(np.uint16), np.array([[65535]], np.uint16), np.array([[0, 1, 256, 65535]], np.uint16)]):
        path = tmp_path / f"t{k}.png"
        bev.write_png16(path, img)
        back = bev.read_png16(path)
        assert back.dtype == np.uint16 and np.array_equal(back, img)
    raw = open(tmp_path / "t1.png", "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[12:16] == b"IHDR" and raw[24] == 16 and raw[25] == 0  # 16 bits, greyscale
    with pytest.raises(ValueError):
        bev.write_png16(tmp_path / "bad.png", np.zeros((2, 2), np.uint8))
    (tmp_path / "junk.png").write_bytes(b"not a png")
    with pytest.raises(ValueError):
        bev.read_png16(tmp_path / "junk.png")


def test_pcd_reader_field_orders_and_errors(tmp_path):
    from lsd_amd import bev

    pts = bc.base_scene(500)
    for k, (order, data, extra) in enumerate([(("x", "y", "z", "intensity"), "binary", None), (("intensity", "z", "y", "x"), "binary", "ring"),
                                              (("y", "x", "intensity", "z"), "ascii", "t"), (("x", "y", "z", "intensity"), "ascii", None)]):
        path = tmp_path / f"c{k}.pcd"
        bc.write_pcd(path, pts, order=order, data=data, extra=extra)
        assert np.array_equal(bev.read_pcd(path).view(np.uint32), pts.view(np.uint32)), (order, data)
    bc.write_pcd(tmp_path / "z.pcd", pts, data="binary_compressed")
    with pytest.raises(ValueError, match="binary_compressed"):
        bev.read_pcd(tmp_path / "z.pcd")
    bc.write_pcd(tmp_path / "m.pcd", pts, order=("x", "y", "z", "reflectivity"))
    with pytest.raises(ValueError, match="intensity"):
        bev.read_pcd(tmp_path / "m.pcd")
    raw = open(tmp_path / "c0.pcd", "rb").read()
    (tmp_path / "short.pcd").write_bytes(raw[:-100])
    with pytest.raises(ValueError):
        bev.read_pcd(tmp_path / "short.pcd")
    (tmp_path / "nohead.pcd").write_bytes(b"FIELDS x y z intensity\n")
    with pytest.raises(ValueError):
        bev.read_pcd(tmp_path / "nohead.pcd")


def test_cli_argument_errors_come_before_any_device_work(tmp_path, monkeypatch):
    from lsd_amd import bev, lio

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(lio, "BevImage", no_device)
    bc.write_pcd(tmp_path / "ok.pcd", bc.base_scene(200))
    good = ["-i", str(tmp_path / "ok.pcd"), "-o", str(tmp_path)]
    for argv in (["-o", str(tmp_path)], ["-i", str(tmp_path / "ok.pcd")], good + ["-r", "2.5"], good + ["-w", "abc"], good + ["-r", "0"], good + ["-w", "0.01"],
                 good + ["-w", "nan"], ["-i", str(tmp_path / "missing.pcd"), "-o", str(tmp_path)], ["-i", str(tmp_path / "ok.pcd"), "-o", str(tmp_path / "nodir")]):
        with pytest.raises(SystemExit) as e:
            bev.main(argv)
        assert e.value.code == 2, argv
    with pytest.raises(ValueError):
        bev.convert([0, 0], [0, 0], None, [0.1, 0.2], 4, 4, 8.0, 5)  # the same pixel twice
    with pytest.raises(ValueError):
        bev.convert([0, 9], [0, 0], None, [0.1, 0.2], 4, 4, 8.0, 5)  # outside the image
    with pytest.raises(ValueError):
        bev.from_cloud(np.zeros((4, 4), F32), window=0.0)
