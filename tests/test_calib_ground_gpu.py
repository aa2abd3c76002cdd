"""The lidar ground calibration on the device (csrc/calib_ground.hip, lio.GroundCalib, lsd_amd.calib_lidar) against the numpy restatement of
tests/calib_ground_cases.py and what the reference recorded in tests/golden/calib_ground.npz: kept indices, every attempt's colinear flag,
count and plane, the winner and the coefficients, all bit for bit (counts are integers and every f32 operation is pinned: no tolerance)."""
import numpy as np
import pytest

import calib_ground_cases as CG

pytestmark = pytest.mark.gpu
BATCH = 128  # attempts the device scores per pass (csrc/calib_ground.hip: kBatch)


@pytest.fixture(scope="module")
def G():
    return CG.golden()


@pytest.fixture(scope="module")
def gc():
    from lsd_amd import capi, lio

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    g = lio.GroundCalib()
    yield g
    g.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_planes(a, b):
    """bit for bit where there is a plane, NaN rows at the same places"""
    na, nb = np.isnan(a).all(1), np.isnan(b).all(1)
    return np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def check_fit(gc, held, found, coef, **kw):
    """the last fit of the handle against the restatement over the points it holds; returns the restated run"""
    r = CG.fit(held, **kw)
    run = gc.last_run()
    assert run == {k: r[k] for k in ("iterations", "attempts", "skipped", "winner", "early_exit")}
    tri, col, cnt, pl = gc.draws()
    m = r["attempts"]
    assert len(cnt) >= m and (len(cnt) - m < BATCH or m == 0)
    assert np.array_equal(tri[:m], r["triples"]) and np.array_equal(col[:m], r["colinear"])
    assert np.array_equal(cnt[:m], r["counts"]) and same_planes(pl[:m], r["planes"])
    assert not cnt[col].any() and np.isnan(pl[col]).all()
    assert found == r["found"] and np.array_equal(bits(coef), bits(r["coef"]))
    return r


def floor_cloud(n_in, n_out=37, seed=0):
    """n_in points of a noisy tilted floor inside the square |x|, |y| < 5 and n_out outside it, interleaved; (points n x 4, polygon)"""
    rng = np.random.default_rng(seed)
    xy = np.concatenate([rng.uniform(-4.9, 4.9, (n_in, 2)), rng.uniform(5.5, 9.0, (n_out, 2)) * rng.choice([-1, 1], (n_out, 2))])
    z = -1.5 + 0.05 * xy[:, 0] + rng.normal(0, 0.03, len(xy))
    z[::5] += 0.4
    p = np.column_stack([xy, z, np.ones(len(xy))]).astype(np.float32)
    return p[rng.permutation(len(p))], np.array([[-5.0, -5.0], [5.0, -5.0], [5.0, 5.0], [-5.0, 5.0]])


@pytest.mark.parametrize("case", CG.FIT_CASES)
def test_golden_case_with_the_recorded_triples(G, gc, case):
    pts, poly, triples = G[case + "_points"], G[case + "_polygon"], G[case + "_triples"]
    n = gc.crop(pts, poly)
    keep = np.nonzero(G[case + "_mask"])[0]
    assert n == len(keep) and np.array_equal(gc.indices(), keep) and np.array_equal(keep, np.nonzero(CG.crop_mask(pts, poly))[0])
    held = gc.points()
    assert np.array_equal(bits(held), bits(pts[keep, :3]))
    found, coef = gc.fit(draws=triples)
    r = check_fit(gc, held, found, coef, draws=triples)
    assert r["attempts"] == len(triples) and same_planes(gc.draws()[3][:len(triples)], G[case + "_planes"])
    assert found and np.array_equal(coef.astype(np.float64), G[case + "_best_coef"])


def test_golden_crop_edges(G, gc):
    pts, poly = G["edges_points"], G["edges_polygon"]
    assert gc.crop(pts, poly) == G["edges_mask"].sum() and np.array_equal(gc.indices(), np.nonzero(G["edges_mask"])[0])
    assert gc.crop(pts[:, :3], poly) == G["edges_mask"].sum() and np.array_equal(gc.indices(), np.nonzero(G["edges_mask"])[0])  # stride 3


@pytest.mark.parametrize("case", CG.FIT_CASES)
def test_align_points_to_xyplane_is_the_references(G, case):
    """1e-12 absolute on the rotation (a few f64 operations on entries of magnitude <= 1); the translation must be equal"""
    from lsd_amd import calib_lidar as CL

    T = CL.align_points_to_xyplane(G[case + "_points"].reshape(-1), G[case + "_polygon"], draws=G[case + "_triples"])
    ref = G[case + "_T"]
    assert T.dtype == np.float64 and np.abs(T[:3, :3] - ref[:3, :3]).max() <= 1e-12
    assert np.array_equal(T[:, 3], ref[:, 3]) and np.array_equal(T[3], ref[3])
    crop = CL.crop_points(G[case + "_points"][:, :3], G[case + "_polygon"])
    assert np.array_equal(bits(crop), bits(G[case + "_points"][G[case + "_mask"], :3]))
    coef = CL.fit_plane(crop, sigma=0.05, num_iteration=100, draws=G[case + "_triples"])
    assert coef.dtype == np.float64 and np.array_equal(coef, G[case + "_best_coef"])


@pytest.mark.parametrize("seed", [0, 5])
def test_seeded_runs(G, gc, seed):
    from lsd_amd import calib_lidar as CL

    pts, poly = G["base_points"], G["base_polygon"]
    gc.crop(pts, poly)
    held = gc.points()
    found, coef = gc.fit(gc.params(seed=seed))
    r = check_fit(gc, held, found, coef, seed=seed)
    assert r["iterations"] == 100 and found
    found2, coef2 = gc.fit(gc.params(seed=seed))
    assert found2 and np.array_equal(bits(coef), bits(coef2))
    T = CL.align_points_to_xyplane(pts, poly, seed=seed)
    assert np.array_equal(T, CL.plane_to_transform(r["coef"])) and np.array_equal(T, CL.align_points_to_xyplane(pts, poly, seed=seed))
    coef = CL.fit_plane(held, seed=seed)  # fit_plane's own defaults: sigma 0.01, 1000 iterations (8 batches)
    assert np.array_equal(coef, CG.fit(held, sigma=1e-2, num_iteration=1000, seed=seed)["coef"].astype(np.float64))


@pytest.mark.parametrize("n_in", [3, 63, 64, 65, 255, 256, 257, 2049])
def test_cropped_counts_at_wave_workgroup_and_tile_edges(gc, n_in):
    pts, poly = floor_cloud(n_in, seed=n_in)
    assert gc.crop(pts, poly) == n_in
    keep = np.nonzero(CG.crop_mask(pts, poly))[0]
    assert len(keep) == n_in and np.array_equal(gc.indices(), keep)
    held = gc.points()
    assert np.array_equal(bits(held), bits(pts[keep, :3]))
    found, coef = gc.fit(gc.params(num_iteration=5, seed=n_in))
    check_fit(gc, held, found, coef, num_iteration=5, seed=n_in)


@pytest.mark.parametrize("num_iteration", [1, BATCH, BATCH + 1])
def test_num_iteration_at_the_batch_size(gc, num_iteration):
    """thresh = 2 switches the early exit off; a colinear attempt is the last of the first batch, so BATCH iterations take a second batch"""
    pts, _ = floor_cloud(300, n_out=0, seed=1)
    pts[1, :3] = pts[0, :3]  # (0, 1, k) is colinear
    gc.set_points(pts)
    held = gc.points()
    assert np.array_equal(gc.indices(), np.arange(300)) and np.array_equal(bits(held), bits(pts[:, :3]))
    draws = np.array([CG.draw(9, j, 300) for j in range(2 * BATCH + 8)])
    draws[BATCH - 1] = (0, 1, 17)
    found, coef = gc.fit(gc.params(num_iteration=num_iteration, thresh=2.0), draws=draws)
    r = check_fit(gc, held, found, coef, num_iteration=num_iteration, thresh=2.0, draws=draws)
    assert r["iterations"] == num_iteration and not r["early_exit"]
    if num_iteration >= BATCH:
        assert r["colinear"][BATCH - 1] and r["attempts"] == num_iteration + r["skipped"] > BATCH
    # the seeded draws through the same sizes
    found, coef = gc.fit(gc.params(num_iteration=num_iteration, thresh=2.0, seed=4))
    check_fit(gc, held, found, coef, num_iteration=num_iteration, thresh=2.0, seed=4)


def test_polygons_triangle_cap_nothing_everything(gc):
    from lsd_amd import capi, lio

    pts, square = floor_cloud(700, seed=2)
    tri = np.array([[-6.0, -4.0], [6.5, -3.0], [0.3, 7.0]])
    a = np.linspace(0, 2 * np.pi, lio.GroundCalib.MAX_VERTICES, endpoint=False)
    ring = np.column_stack([4.0 * np.cos(a), 3.0 * np.sin(a)])  # the vertex cap
    for poly in (tri, ring, ring[::-1], square * 100.0, square + 50.0):
        keep = np.nonzero(CG.crop_mask(pts, poly))[0]
        assert gc.crop(pts, poly) == len(keep) and np.array_equal(gc.indices(), keep)
        assert np.array_equal(bits(gc.points()), bits(pts[keep, :3]))
    assert len(np.nonzero(CG.crop_mask(pts, square * 100.0))[0]) == len(pts) and gc.crop(pts, square + 50.0) == 0
    assert len(gc.indices()) == 0 and gc.points().shape == (0, 3)
    with pytest.raises(capi.LioError):  # nothing is held: fewer than 3 points
        gc.fit()
    assert gc.crop(pts[:0], square) == 0


def test_nan_coordinates(gc):
    pts, poly = floor_cloud(200, seed=3)
    inside = np.nonzero(CG.crop_mask(pts, poly))[0]
    ix, iy, iz = inside[10], inside[20], inside[30]
    pts[ix, 0], pts[iy, 1], pts[iz, 2] = np.nan, np.nan, np.nan
    keep = np.nonzero(CG.crop_mask(pts, poly))[0]
    assert ix not in keep and iy not in keep and iz in keep and len(keep) == 198
    assert gc.crop(pts, poly) == 198 and np.array_equal(gc.indices(), keep)
    held = gc.points()
    k = int(np.nonzero(keep == iz)[0][0])
    assert np.isnan(held[k, 2]) and np.array_equal(bits(np.delete(held, k, 0)), bits(np.delete(pts[keep, :3], k, 0)))
    draws = np.array([[k, 3, 4], [5, k, 6], [7, 8, 9], [10, 11, k], [12, 13, 14]])  # a NaN plane is not colinear and counts nothing
    found, coef = gc.fit(gc.params(num_iteration=5), draws=draws)
    r = check_fit(gc, held, found, coef, num_iteration=5, draws=draws)
    assert not r["colinear"].any() and list(r["counts"][[0, 1, 3]]) == [0, 0, 0] and r["winner"] in (2, 4)


def test_a_cloud_that_is_one_point_stops_at_the_attempt_cap(gc):
    from lsd_amd import calib_lidar as CL

    pts = np.tile(np.array([1.0, 2.0, -1.5, 0.0], np.float32), (50, 1))
    gc.set_points(pts)
    found, coef = gc.fit(gc.params(num_iteration=13))
    r = check_fit(gc, gc.points(), found, coef, num_iteration=13)
    assert not found and r["attempts"] == r["skipped"] == 11 * 13 and not coef.any()
    assert not CL.fit_plane(pts[:, :3], num_iteration=2).any()
    with pytest.raises(ValueError, match="no plane found"):
        CL.align_points_to_xyplane(pts, [[0, 0], [3, 0], [3, 4], [0, 4]])
    with pytest.raises(ValueError, match="fewer than 3 points inside"):
        CL.align_points_to_xyplane(pts, [[10, 0], [13, 0], [13, 4], [10, 4]])
    with pytest.raises(ValueError, match="not three distinct"):
        CL.fit_plane(pts[:, :3], draws=[[0, 1, 1]])


def test_a_refused_call_leaves_the_handle_as_it_was(gc):
    from lsd_amd import capi

    pts, poly = floor_cloud(300, seed=4)
    gc.crop(pts, poly)
    keep, held = gc.indices(), gc.points()
    found, coef = gc.fit(gc.params(num_iteration=7, seed=2))
    run, log = gc.last_run(), gc.draws()
    refused = [lambda: gc.crop(pts, poly[:2]), lambda: gc.crop(pts, np.zeros((gc.MAX_VERTICES + 1, 2))), lambda: gc.fit(gc.params(num_iteration=0)),
               lambda: gc.fit(draws=[[0, 1, 300]]), lambda: gc.fit(draws=[[0, 1, 2], [5, 6, 5]])]
    for call in refused:
        with pytest.raises(capi.LioError, match="error -1"):
            call()
        assert np.array_equal(gc.indices(), keep) and np.array_equal(bits(gc.points()), bits(held))
        assert gc.last_run() == run and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(gc.draws(), log))
    found2, coef2 = gc.fit(gc.params(num_iteration=7, seed=2))
    assert found2 == found and np.array_equal(bits(coef), bits(coef2))
    found3, _ = gc.fit(draws=np.zeros((0, 3), np.uint32))  # an empty list: the loop ends at once with nothing
    assert not found3 and gc.last_run()["attempts"] == 0
    crop_us, fit_us, planes_us, score_us = gc.last_times()
    assert crop_us > 0 and fit_us >= 0 and planes_us + score_us == 0
