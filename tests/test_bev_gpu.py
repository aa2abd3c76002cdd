"""The bird's-eye intensity image on the device (csrc/bev.hip, lio_bev_*; lsd_amd.bev) against the numpy restatement of tests/bev_cases.py:
every downloadable stage and the image bit for bit, on the base scene and on variants built to reach each rule's edge."""
import numpy as np
import pytest

import bev_cases as bc

pytestmark = pytest.mark.gpu
F32 = np.float32


def _need_gpu():
    from lsd_amd import capi

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")


@pytest.fixture(scope="module")
def handle():
    _need_gpu()
    from lsd_amd import lio

    h = lio.BevImage()
    yield h
    h.close()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _hold(h, pts, window, ppm, want=None):
    """run the device over pts and hold every stage to the restatement; returns (restatement, device image)"""
    want = want if want is not None else bc.restate(pts, window, ppm)
    info = h.preprocess_host(pts, ppm)
    image = h.convert(window, ppm)
    info = h.info()
    P, hp, q, W, H, nx, ny = want["geometry"]
    assert (info["n_in"], info["n_dropped"]) == (len(pts), int(np.count_nonzero(~want["fin"])))
    assert (info["image_w"], info["image_h"], info["padded_w"], info["padded_h"]) == (want["w"], want["h"], W, H)
    assert (info["patch"], info["half_patch"], info["quarter_patch"], info["nodes_x"], info["nodes_y"]) == (P, hp, q, nx, ny)
    assert (info["x_min"], info["x_max"], info["y_min"], info["y_max"]) == want["bounds"]
    assert np.array_equal(h.pixel_coords(), want["xy"])
    assert np.array_equal(h.kept(), want["kept"])
    assert info["n_kept"] == len(want["kept"])
    key, inten, z = h.pixels()
    assert np.array_equal(key, want["pkey"])
    assert np.array_equal(_bits(inten), _bits(want["pI"]))
    assert np.array_equal(_bits(z), _bits(want["pz"]))
    count, step, clip = h.nodes()
    assert np.array_equal(count, want["count"])
    assert np.array_equal(step, want["step"])
    assert np.array_equal(clip.view(np.uint64), want["clip"].view(np.uint64))
    assert np.array_equal(_bits(h.equalised()), _bits(want["eq"]))
    assert image.shape == (H, W) and image.dtype == np.uint16
    assert np.array_equal(image, want["image"])
    return want, image


def test_base_scene_every_stage_and_the_cli(handle, tmp_path):
    from lsd_amd import bev

    pts, want = bc.base_restated()
    assert bc.cut_intensities_unique(pts)
    _, image = _hold(handle, pts, bc.BASE_WINDOW, bc.BASE_PPM, want)
    assert (want["w"], want["h"]) == (301, 201) and image.shape == (220, 320)
    assert np.count_nonzero(want["step"] >= 0) == 203 and len(want["step"]) == 204
    # the scene has points exactly on half-pixel offsets (ties to even)
    fx = (pts[:, 0] - pts[:, 0].min()) * F32(bc.BASE_PPM)
    assert np.count_nonzero(fx - np.floor(fx) == 0.5) > 10
    # the command line: the reference's flags, <output>/bev.png
    bc.write_pcd(tmp_path / "map.pcd", pts, order=("intensity", "y", "x", "z"), extra="ring")
    assert bev.main(["-i", str(tmp_path / "map.pcd"), "-w", str(bc.BASE_WINDOW), "-r", str(bc.BASE_PPM), "-o", str(tmp_path)]) == 0
    assert np.array_equal(bev.read_png16(tmp_path / "bev.png"), image)
    # the reference-shaped functions: preprocess's pixel list through convert
    xs, ys, zs, inten, w, h, meta = bev.preprocess(str(tmp_path / "map.pcd"), bc.BASE_PPM)
    assert (w, h) == (301, 201) and np.array_equal(ys * w + xs, want["pkey"]) and meta["pixel_per_meter"] == bc.BASE_PPM
    perm = np.random.default_rng(0).permutation(len(xs))
    assert np.array_equal(bev.convert(xs[perm], ys[perm], zs[perm], inten[perm], w, h, bc.BASE_WINDOW, bc.BASE_PPM), image)


def _with_rows(pts, rows, at=None):
    at = len(pts) // 2 if at is None else at
    return np.concatenate([pts[:at], np.asarray(rows, F32).reshape(-1, 4), pts[at:]])


def _variant(name):
    """(points, window, ppm, check(restatement, image)) of one edge of the rules"""
    base, _ = bc.base_restated()
    pts = base.copy()
    rng = np.random.default_rng(11)
    window, ppm, check = bc.BASE_WINDOW, bc.BASE_PPM, None
    if name == "odd_patch":
        window = 8.2

        def check(w, img):
            assert w["geometry"][:3] == (41, 20, 10)
    elif name == "half_pixel_ties":
        # x = j + 0.1 at 5 px/m is (5 j + 0.5) pixels: rint goes to the even neighbour, both ways
        j = np.arange(0, 60, dtype=np.float64)
        rows = np.stack([j + 0.1, np.full(60, 20.1), np.zeros(60), np.full(60, 0.08)], 1)
        pts = _with_rows(pts, rows)

        def check(w, img):
            f = (np.float32(rows[:, 0].astype(F32)) - F32(0.0)) * F32(5)
            assert np.all(f - np.floor(f) == 0.5)
    elif name == "intensity_zero_one_above":
        idx = rng.permutation(len(pts))
        pts[idx[:900], 3] = 0.0
        pts[idx[900:1300], 3] = 1.0
        pts[idx[1300:1700], 3] = rng.uniform(1.0, 3.0, 400)

        def check(w, img):
            v = w["pI"] * F32(65535.0)
            assert np.any(v == 0) and np.any(v == F32(65535.0)) and np.any(v > F32(65535.0))
    elif name == "negative_zero":
        idx = rng.permutation(len(pts))[:900]  # the lower cut (rank 600) falls among them
        pts[idx[0::2], 3] = -0.0
        pts[idx[1::2], 3] = 0.0

        def check(w, img):
            dropped = np.setdiff1d(idx, w["kept"])
            assert 0 < len(dropped) < len(idx) and np.array_equal(np.sort(dropped), np.sort(idx)[:len(dropped)])  # ties go by input index
    elif name == "duplicates_at_the_cuts":
        s = np.sort(pts[:, 3])
        lo, hi = bc.cut_ranks(len(pts))
        idx = rng.permutation(len(pts))
        pts[idx[:40], 3] = s[lo - 20]  # 41 equal values over ranks lo - 20 .. lo + 20
        pts[idx[40:80], 3] = s[hi + 20]  # the 40 points leave the ranks below: 41 equal values over ranks hi - 20 .. hi + 20

        def check(w, img):
            for val in (s[lo - 20], s[hi + 20]):
                same = np.flatnonzero(pts[:, 3] == val)
                k = np.isin(same, w["kept"])
                assert k.any() and not k.all()
    elif name == "heavy_pixel":
        rows = np.stack([np.full(5000, 10.0), np.full(5000, 30.0), rng.normal(0, 0.1, 5000), rng.uniform(0.06, 0.09, 5000)], 1)
        pts = _with_rows(pts, rows)

        def check(w, img):
            assert w["pcount"].max() >= 4900
    elif name == "raw_patch_in_the_hole":
        # a few pixels around the node in the middle of the hole: it sees no more than 100, so its inner region keeps the raw means, while
        # the border it shares with its running neighbour is the neighbour's
        cx, cy = 40.0, 20.0
        ox, oy = np.meshgrid(np.arange(-10, 11, 5) / 5.0, np.arange(-10, 11, 5) / 5.0)
        rows = np.stack([cx + ox.ravel(), cy + oy.ravel(), np.zeros(ox.size), np.full(ox.size, 0.09)], 1)
        pts = _with_rows(pts, rows)

        def check(w, img):
            P, hp, q, W, H, nx, ny = w["geometry"]
            idle = np.flatnonzero(w["step"] < 0)
            assert len(idle) >= 1
            raw = _bits(w["eq"]) == _bits(w["pI"])
            assert np.count_nonzero(raw) == 9
            xs, ys = w["pkey"] % w["w"], w["pkey"] // w["w"]
            assert set(np.unique(img[ys[raw], xs[raw]])) <= {0, 1}
            inner = (np.abs(xs.astype(int) - 200) <= 10) & (np.abs(ys.astype(int) - 100) <= 10)
            assert np.count_nonzero(inner) == 25 and np.count_nonzero(inner & ~raw) == 16  # border pixels taken by a running neighbour
    elif name == "fewer_than_100_points":
        pts = base[:80].copy()

        def check(w, img):
            assert np.all(w["step"] < 0) and set(np.unique(img)) <= {0, 1}
    elif name == "nan_inf_rows":
        rows = [[np.nan, 1, 0, 0.1], [1, np.inf, 0, 0.1], [1, 1, 0, np.nan], [1, 1, 0, -np.inf], [1, 1, np.nan, 0.07]]
        pts = _with_rows(pts, rows)

        def check(w, img):
            assert np.count_nonzero(~w["fin"]) == 4
    else:
        raise KeyError(name)
    return pts, window, ppm, check


@pytest.mark.parametrize("name", ["odd_patch", "half_pixel_ties", "intensity_zero_one_above", "negative_zero", "duplicates_at_the_cuts", "heavy_pixel",
                                  "raw_patch_in_the_hole", "fewer_than_100_points", "nan_inf_rows"])
def test_variants_of_the_base_scene(handle, name):
    pts, window, ppm, check = _variant(name)
    want, image = _hold(handle, pts, window, ppm)
    check(want, image)


def test_node_window_with_exactly_100_and_101_pixels(handle):
    """two islands at 1 px/m under a window of 8 m: 10 x 10 pixels (the node over them sees exactly 100 and does not run) and 101 pixels"""
    ax, ay = np.meshgrid(np.arange(10.0), np.arange(10.0))
    a = np.stack([ax.ravel(), ay.ravel()], 1)
    b = np.concatenate([a + [40.0, 0.0], [[50.0, 0.0]]])
    xy = np.concatenate([a, b])
    rng = np.random.default_rng(3)
    inten = rng.uniform(0.05, 0.2, len(xy))
    extra = xy[rng.integers(0, len(xy), 46)]
    pts = np.concatenate([np.column_stack([xy, np.zeros(len(xy)), inten]), np.column_stack([extra, np.zeros(46), rng.uniform(0.05, 0.2, 46)]),
                          [[3.0, 3.0, 0.0, 0.001], [4.0, 4.0, 0.0, 0.002], [45.0, 5.0, 0.0, 0.9]]]).astype(F32)
    assert len(pts) == 250 and bc.cut_ranks(250) == (2, 249)
    want, _ = _hold(handle, pts[rng.permutation(250)], 8.0, 1)
    assert len(want["pkey"]) == 201
    assert np.all(want["step"][want["count"] == 100] < 0) and np.count_nonzero(want["count"] == 100) >= 1
    assert np.all(want["step"][want["count"] == 101] >= 0) and np.count_nonzero(want["count"] == 101) >= 1


def test_cloud_path_and_repeat_give_the_same_bits(handle):
    from lsd_amd import bev, lio

    pts, want = bc.base_restated()
    first = bev.from_cloud(pts, bc.BASE_WINDOW, bc.BASE_PPM, handle=handle)
    assert np.array_equal(first, want["image"])
    cloud = lio.Cloud()
    cloud.append_host(pts[:25_000])
    cloud.append_host(pts[25_000:])
    other = lio.BevImage()
    second = bev.from_cloud(cloud, bc.BASE_WINDOW, bc.BASE_PPM, handle=other)
    assert np.array_equal(second, first)
    assert np.array_equal(other.kept(), want["kept"]) and np.array_equal(_bits(other.equalised()), _bits(want["eq"]))
    again = bev.from_cloud(pts, bc.BASE_WINDOW, bc.BASE_PPM, handle=handle)
    assert np.array_equal(again, first) and np.array_equal(_bits(handle.equalised()), _bits(want["eq"]))
    other.close()
    cloud.close()


def test_invalid_input_is_an_error(handle):
    from lsd_amd import capi

    bad = np.full((10, 4), np.nan, F32)
    with pytest.raises(ValueError):
        handle.preprocess_host(bad, 5)
    with pytest.raises(ValueError):
        handle.preprocess_host(np.zeros((0, 4), F32), 5)
    pts, _ = bc.base_restated()
    handle.preprocess_host(pts, 5)
    with pytest.raises(ValueError):
        handle.convert(0.1, 5)  # a patch of 0 pixels
    huge = np.array([[0, 0, 0, 0.1], [1e6, 1e6, 0, 0.2], [5, 5, 0, 0.3]], F32)
    with pytest.raises(capi.LioError):
        handle.preprocess_host(huge, 25)  # 25 000 001 pixels a side: the key would not fit
