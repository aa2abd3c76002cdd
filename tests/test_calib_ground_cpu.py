"""The lidar ground calibration without a device: the ABI's new names, the numpy restatement (tests/calib_ground_cases.py) against what the
reference recorded (tests/golden/calib_ground.npz, tools/record_calib_ground_golden.py) bit for bit, the loop's replay on hand-made count
lists, and the host functions of lsd_amd.calib_lidar against the recorded values."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import calib_ground_cases as CG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["default_params", "create", "destroy", "crop_host", "set_points_host", "fit", "download_indices", "download_points", "download_draws",
         "last_run", "last_times"]


@pytest.fixture(scope="module")
def G():
    return CG.golden()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_abi_revision_and_symbols():
    from lsd_amd import capi

    hdr = open(os.path.join(ROOT, "include", "lio_hip.h")).read()
    rev = int(re.search(r"#define LIO_ABI_VERSION (\d+)", hdr).group(1))
    assert rev >= 26 and capi.lib().lio_abi_version() == rev
    for n in NAMES:
        assert "lio_calib_ground_" + n in capi.SYMBOLS and hasattr(capi.lib(), "lio_calib_ground_" + n)
    assert int(re.search(r"#define LIO_CALIB_GROUND_MAX_VERTICES (\d+)", hdr).group(1)) == capi.CALIB_GROUND_MAX_VERTICES >= 64
    src = open(os.path.join(ROOT, "lidar-slam-detection_amd", "csrc", "Makefile")).read()
    assert "calib_ground.hip" in src and "-ffp-contract=off" in src


def test_create_without_a_device_is_null_and_defaults():
    from lsd_amd import capi, lio

    assert not capi.lib().lio_calib_ground_create(-1)
    assert b"no HIP device" in capi.lib().lio_last_error()
    p = lio.GroundCalib.params()
    assert (p.sigma, p.num_iteration, p.thresh, p.seed) == (0.05, 100, 0.9, 0)
    with pytest.raises(ValueError):
        lio.GroundCalib.params(nothing=1)
    L = capi.lib()
    assert L.lio_calib_ground_fit(None, None, None, 0, None, None) == capi.LIO_E_INVALID
    assert L.lio_calib_ground_crop_host(None, None, 0, 3, None, 3, None) == capi.LIO_E_INVALID
    assert L.lio_calib_ground_download_indices(None, None, 0) == capi.LIO_E_INVALID
    L.lio_calib_ground_destroy(None)
    if L.lio_device_count() < 1:
        with pytest.raises(capi.LioError):
            lio.GroundCalib()


@pytest.mark.parametrize("case", CG.FIT_CASES + ("edges",))
def test_restated_crop_is_the_references(G, case):
    mask = CG.crop_mask(G[case + "_points"], G[case + "_polygon"])
    assert np.array_equal(mask, G[case + "_mask"])
    assert CG.crop_loop(G[case + "_points"][:200], G[case + "_polygon"]) == list(np.nonzero(mask[:200])[0])


def test_crop_edge_rules_by_hand(G):
    """y equal to a vertex's y never counts that vertex's edges; a point on a vertical edge is outside (xi > x is strict); a point on the
    horizontal edge y = 0 crosses nothing"""
    pts, mask = G["edges_points"], G["edges_mask"]
    at = {(float(p[0]), float(p[1])): bool(m) for p, m in zip(pts, mask)}
    assert at[(1.0, 1.0)] and at[(3.0, 1.0)] and at[(2.0, 1.0)]  # y = 1 is the notch vertex's y: its two edges do not count, the right edge does
    assert not at[(2.0, 2.0)]                                     # the notch above it is outside
    assert not at[(4.0, 1.5)] and at[(0.0, 1.5)]      # on the right vertical edge: outside; on the left one: the right edge alone crosses
    assert not at[(1.0, 0.0)] and not at[(1.0, 3.0)] and not at[(-0.5, 1.5)] and not at[(4.5, 0.5)]
    assert at[(0.25, 2.5)] and at[(3.75, 2.5)] and not at[(2.0, 2.5)]


@pytest.mark.parametrize("case", CG.FIT_CASES)
def test_restated_planes_and_best_coef_are_the_references(G, case):
    crop = G[case + "_points"][G[case + "_mask"]][:, :3]
    triples, ref = G[case + "_triples"], G[case + "_planes"]
    pl, col = CG.planes(crop, triples)
    assert np.array_equal(col, np.isnan(ref).all(1))
    assert np.array_equal(bits(pl[~col]), bits(ref[~col]))
    r = CG.fit(crop, draws=triples)
    assert r["attempts"] == len(triples) and r["found"]
    assert np.array_equal(r["coef"].astype(np.float64), G[case + "_best_coef"])
    assert np.array_equal(r["counts"], CG.counts(crop, r["planes"], CG.SIGMA)) and r["counts"].dtype == np.uint32
    acc = r["counts"][~r["colinear"]]
    if case == "base":
        assert not r["early_exit"] and r["iterations"] == 100 and acc.max() <= 0.9 * len(crop)
    if case == "early":
        assert r["early_exit"] and r["winner"] == len(triples) - 1 > 0
    if case == "skipped":
        assert r["skipped"] > 0 and r["iterations"] + r["skipped"] == r["attempts"]
    if case == "ties":
        assert np.count_nonzero(acc == acc.max()) > 1 and r["winner"] == int(np.nonzero(r["counts"] == acc.max())[0][0])


def test_restated_draws_are_three_distinct_indices():
    from lsd_amd import capi

    out = (C.c_uint32 * 3)()
    for seed, j, n in [(0, 0, 3), (0, 1, 3), (7, 5, 4), (1, 99, 1281), (0xFFFFFFFF, 123456, 2 ** 31 - 1)]:
        d = CG.draw(seed, j, n)
        assert len(set(d)) == 3 and max(d) < n
        capi.lib().lio_ground_draw(seed, j, n, out)  # the existing rule the restatement restates
        assert tuple(out) == d


def test_replay_on_hand_made_counts():
    n = 100
    no = [False] * 8
    # early exit at the first draw and at a later one: the count has to exceed 0.9 n strictly
    assert CG.replay(no, [91, 99, 5, 5, 5, 5, 5, 5], n, 5, 0.9) == dict(iterations=1, attempts=1, skipped=0, winner=0, early_exit=True)
    assert CG.replay(no, [90, 20, 95, 99, 5, 5, 5, 5], n, 5, 0.9) == dict(iterations=3, attempts=3, skipped=0, winner=2, early_exit=True)
    # the early exit wins even over a better earlier count when thresh is low
    assert CG.replay(no, [40, 50, 45, 5, 5, 5, 5, 5], n, 2, 0.49)["winner"] == 1
    # a tie: the first of equal counts stays; the loop ends after num_iteration iterations
    assert CG.replay(no, [30, 50, 50, 20, 60, 5, 5, 5], n, 4, 0.9) == dict(iterations=4, attempts=4, skipped=0, winner=1, early_exit=False)
    # colinear attempts are skipped and cost no iteration
    col = [True, False, True, True, False, False, False, False]
    assert CG.replay(col, [0, 10, 0, 0, 30, 30, 99, 5], n, 3, 0.9) == dict(iterations=3, attempts=6, skipped=3, winner=4, early_exit=False)
    # counts of 0 never become the best: nothing found
    assert CG.replay(no, [0] * 8, n, 8, 0.9) == dict(iterations=8, attempts=8, skipped=0, winner=-1, early_exit=False)
    # the attempt cap: 11 * num_iteration attempts, all colinear
    assert CG.replay([True] * 50, [0] * 50, n, 2, 0.9) == dict(iterations=0, attempts=22, skipped=22, winner=-1, early_exit=False)
    assert CG.replay([True] * 21 + [False], [0] * 21 + [7], n, 2, 0.9) == dict(iterations=1, attempts=22, skipped=21, winner=21, early_exit=False)
    # an explicit list running out ends the loop with what it has
    assert CG.replay([False, True, False], [10, 0, 20], n, 100, 0.9) == dict(iterations=2, attempts=3, skipped=1, winner=2, early_exit=False)
    assert CG.replay([], [], n, 100, 0.9) == dict(iterations=0, attempts=0, skipped=0, winner=-1, early_exit=False)


def test_fit_restatement_does_not_depend_on_its_chunks(G):
    crop = G["base_points"][G["base_mask"]][:, :3]
    a, b = CG.fit(crop, num_iteration=40, seed=3, chunk=64), CG.fit(crop, num_iteration=40, seed=3, chunk=7)
    assert a["winner"] == b["winner"] and np.array_equal(bits(a["planes"]), bits(b["planes"])) and np.array_equal(a["counts"], b["counts"])
    coef, winner = CG.fit_loop(crop[:150], 0.05, 6, 0.9, 3)
    c = CG.fit(crop[:150], num_iteration=6, seed=3)
    assert winner == c["winner"] and np.array_equal(bits(coef), bits(c["coef"]))


@pytest.mark.parametrize("case", CG.FIT_CASES)
def test_transform_of_the_recorded_plane(G, case):
    """1e-12 absolute: a few f64 operations on entries of magnitude <= 1; the translation (one f64 quotient) must be equal"""
    from lsd_amd import calib_lidar as CL

    coef, T = G[case + "_best_coef"], G[case + "_T"]
    mine = CL.plane_to_transform(coef)
    assert mine.dtype == np.float64 and mine.shape == (4, 4)
    assert np.abs(mine[:3, :3] - T[:3, :3]).max() <= 1e-12
    assert np.array_equal(mine[:, 3], T[:, 3]) and np.array_equal(mine[3], [0, 0, 0, 1])
    assert np.abs(CG.rot_to_z(coef) - T[:3, :3]).max() <= 1e-12


def test_calc_rot_from(G):
    from lsd_amd import calib_lidar as CL

    for v, R in zip(G["rot_in"], G["rot_R"]):
        mine = CL.calc_rot_from(v[0], v[1])
        assert np.abs(mine - R).max() <= 1e-12
        assert np.abs(mine @ (v[0] / np.linalg.norm(v[0])) - v[1] / np.linalg.norm(v[1])).max() <= 1e-12
    # deviation 2: parallel vectors give the identity (the reference: 0 / 0)
    assert np.array_equal(CL.calc_rot_from([0, 0, 1], [0, 0, 1]), np.eye(3))
    assert np.array_equal(CL.calc_rot_from(np.array([0, 0, 2.5]), np.array([0, 0, 1])), np.eye(3))
    with pytest.raises(ValueError):
        CL.calc_rot_from([0, 0, -1], [0, 0, 1])
    with pytest.raises(ValueError):
        CL.calc_rot_from([0, 0, 0], [0, 0, 1])


def test_planar_alignments(G):
    """1e-9 absolute: the same LAPACK inverse / pseudo-inverse and product as the recording; a different BLAS kernel can move the result by
    about cond(A) eps |x| (1e3 * 2e-16 * 20 = 4e-12 on these cases)"""
    from lsd_amd import calib_lidar as CL

    for c, R, t in zip(G["pq_in"], G["pq_R"], G["pq_t"]):
        r, tt = CL.align_pq_to_known(*c)
        assert r.shape == (3, 3) and tt.shape == (3,)
        assert np.abs(r - R).max() <= 1e-9 and np.abs(tt - t).max() <= 1e-9
        assert np.abs(r[:2, :2] @ c[0][:2] + tt[:2] - c[2][:2]).max() <= 1e-9 and np.abs(r[:2, :2] @ c[1][:2] + tt[:2] - c[3][:2]).max() <= 1e-9
    for i in range(3):
        T = CL.align_points(G[f"ap{i}_p0"], G[f"ap{i}_p1"])
        assert T.shape == (4, 4) and np.abs(T - G[f"ap{i}_T"]).max() <= 1e-9


def test_euler_helpers(G):
    """within 1e-9 degrees of scipy's intrinsic ZXY values, and the round trip holds"""
    from lsd_amd import calib_lidar as CL

    for e, T, R, back in zip(G["euler_in"], G["euler_T"], G["euler_rot"], G["euler_back"]):
        rot, t = CL.xyzrpy_to_rt(list(e))
        assert np.abs(rot - R).max() <= 1e-12 and np.array_equal(t, e[:3])
        assert np.abs(rot - CG.euler_zxy_matrix(*e[3:])).max() <= 1e-12
        TT = CL.xyzrpy_to_transform(list(e))
        assert np.abs(TT - T).max() <= 1e-12 and np.array_equal(TT[3], [0, 0, 0, 1])
        out = CL.rt_to_xyzrpy(R, e[:3])
        assert isinstance(out, list) and len(out) == 6
        assert np.abs(np.array(out) - back).max() <= 1e-9 and np.abs(np.array(out) - e).max() <= 1e-9
        assert np.abs(np.array(CL.rt_to_xyzrpy(*CL.xyzrpy_to_rt(out))) - e).max() <= 1e-9


def test_value_errors_that_need_no_device():
    from lsd_amd import calib_lidar as CL, lio

    pts = np.zeros((10, 4), np.float32)
    with pytest.raises(ValueError, match="fewer than 3 vertices"):
        CL.align_points_to_xyplane(pts, [[0, 0], [1, 1]])
    with pytest.raises(ValueError, match="fewer than 3 vertices"):
        CL.crop_points(pts[:, :3], [[0, 0], [1, 1]])
    ring = [[np.cos(a), np.sin(a)] for a in np.linspace(0, 6.2, lio.GroundCalib.MAX_VERTICES + 1)]
    with pytest.raises(ValueError, match="more than 256 vertices"):
        CL.crop_points(pts[:, :3], ring)
    with pytest.raises(ValueError, match="fewer than 3 points"):
        CL.fit_plane(pts[:2, :3])
    with pytest.raises(ValueError, match="c = 0"):
        CL.plane_to_transform([1.0, 0.0, 0.0, 2.0])
    with pytest.raises(ValueError, match="c = 0"):
        CL.plane_to_transform(np.zeros(4))


def test_nothing_new_in_the_calibration_module():
    """the reference binds none of this in calib_driver_ext; the package's surface is the reference's"""
    from lsd_amd import calib_lidar as CL

    for n in ("crop_points", "fit_plane", "calc_rot_from", "align_points_to_xyplane", "align_pq_to_known", "align_points", "xyzrpy_to_transform",
              "xyzrpy_to_rt", "rt_to_xyzrpy"):
        assert callable(getattr(CL, n))
    src = open(os.path.join(ROOT, "lidar-slam-detection_amd", "csrc", "calib_wrapper.cpp")).read()
    assert "calib_ground" not in src
