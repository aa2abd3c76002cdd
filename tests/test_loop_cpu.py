"""Loop detection, the parts that need no device: the ABI revision and symbols, lio_loop_find_candidates and lio_loop_information_matrix against
tests/loop_cases.py's restatement of loop_detector.hpp / information_matrix_calculator.cpp, the failure without a device, the wrapper's
surface, and the CONDITIONS the recorded vectors (tests/golden/loop.npz) must meet so that no decision of the GPU tests sits on a threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import loop_cases as LC
from lsd_amd import capi, lio

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "loop.npz")


def test_abi_revision_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "lio_hip.h")).read()
    rev = int(re.search(r"#define LIO_ABI_VERSION (\d+)", hdr).group(1))
    assert rev >= 12 and capi.lib().lio_abi_version() == rev
    for name in ("lio_loop_default_params", "lio_loop_find_candidates", "lio_loop_information_matrix", "lio_loop_create", "lio_loop_destroy", "lio_loop_reset",
                 "lio_loop_add_keyframe_host", "lio_loop_set_pose", "lio_loop_detect", "lio_loop_edges", "lio_loop_last_report", "lio_loop_last_times",
                 "lio_loop_align_candidates", "lio_loop_align_fine", "lio_loop_download_keyframe"):
        assert hasattr(capi.lib(), name) and name in hdr, name
    assert C.sizeof(capi.LoopEdge) == 8 + 64 + 8 + 288 and C.sizeof(capi.LoopReport) == 48


def test_default_params_are_the_constructor_s():
    p = lio.LoopDetector.default_params()
    got = {k: getattr(p, k) for k in LC.DEFAULTS}
    assert got == LC.DEFAULTS
    assert (p.voxel_resolution, p.coarse_translation_epsilon, p.coarse_rotation_epsilon_deg, p.max_iterations, p.k_correspondences) == (1.0, 0.1, 0.1, 64, 20)
    assert (p.fine_translation_epsilon, p.fine_rotation_epsilon_deg) == (0.01, 1e-2)


def _walk(seed, n=80):
    """a random walk that turns back on itself: accumulated distance and planar positions of n key frames"""
    rng = np.random.default_rng(seed)
    step = rng.uniform(0.5, 3.0, n)
    head = np.cumsum(rng.normal(0, 0.35, n)) + np.where(np.arange(n) > n // 2, np.pi, 0.0)
    xy = np.cumsum(np.stack([step * np.cos(head), step * np.sin(head)], 1), 0)
    return np.cumsum(step), xy


@pytest.mark.parametrize("seed", range(6))
def test_find_candidates_random_walks(seed):
    accum, xy = _walk(seed)
    hits = 0
    for i in range(5, len(accum)):
        for last_edge in (0.0, accum[i] - 20.0, accum[i] - 10.0):
            want = LC.find_candidates(accum[:i], xy[:i], accum[i], xy[i], last_edge)
            got = lio.LoopDetector.find_candidates(accum[:i], xy[:i], accum[i], xy[i], last_edge)
            assert list(got) == want
            hits += len(want)
    assert hits > 0


def test_find_candidates_edges():
    f = lio.LoopDetector.find_candidates
    # travelled difference exactly at the threshold stays (strict <), a micrometre short of it goes
    assert list(f([5.0], [[0, 0]], 30.0, [1, 0])) == [0]
    assert list(f([5.000001], [[0, 0]], 30.0, [1, 0])) == []
    # planar distance exactly 15 stays (strict >), z plays no part
    assert list(f([0.0], [[0, 0]], 40.0, [9, 12])) == [0]
    assert list(f([0.0], [[0, 0]], 40.0, [9, 12.0001])) == []
    # spacing from the last ACCEPTED frame, which starts at -100: frame 1 (1.5 m after frame 0) goes, frame 2 (2 m after frame 0) stays;
    # frame 3 is 1.9 m after frame 2 and goes, though it is 2.4 m after the rejected frame 1
    accum = [0.0, 1.5, 2.0, 3.9, 4.0]
    assert list(f(accum, [[0, 0]] * 5, 60.0, [0, 0])) == [0, 2, 4]
    # a frame rejected for its distance does not move the spacing
    assert list(f([0.0, 2.0, 2.5], [[0, 0], [100, 0], [0, 0]], 60.0, [0, 0])) == [0, 2]
    # the last-edge gate returns nothing, exactly at the threshold it lets through
    assert list(f([0.0], [[0, 0]], 40.0, [0, 0], last_edge_accum=25.5)) == []
    assert list(f([0.0], [[0, 0]], 40.0, [0, 0], last_edge_accum=25.0)) == [0]
    # an empty bank
    assert list(f([], np.zeros((0, 2)), 40.0, [0, 0])) == []
    # cap too small: -(count)
    out = np.zeros(1, np.int32)
    a, xy, nxy = np.array(accum), np.zeros((5, 2)), np.zeros(2)
    assert capi.lib().lio_loop_find_candidates(capi.ptr(a, C.c_double), capi.ptr(xy, C.c_double), 5, 60.0, capi.ptr(nxy, C.c_double), 0.0, None, capi.ptr(out, C.c_int32), 1) == -3


def test_information_matrix():
    I0 = lio.LoopDetector.information_matrix(0.0)
    # fitness 0: the minimum variances 0.1^2 and 0.05^2, rounded to f32 as the reference's float locals are
    assert I0[0, 0] == 1.0 / np.float64(np.float32(0.1 ** 2)) and I0[3, 3] == 1.0 / np.float64(np.float32(0.05 ** 2))
    assert I0[0, 0] != 1.0 / 0.1 ** 2  # the rounding is visible
    for s in (0.0, 1e-3, 0.1, 0.49, 0.5, 1.5, 1.4999, 3.0, 25.0):
        got, want = lio.LoopDetector.information_matrix(s), LC.information_matrix(s)
        assert np.array_equal(got, want), s
        assert np.count_nonzero(got - np.diag(np.diag(got))) == 0
    # at the calculator's own threshold (0.5) the weight is the maximum variance; above it the exponential saturates and it stays there
    assert lio.LoopDetector.information_matrix(0.5)[0, 0] == 1.0 / np.float64(np.float32(25.0))
    assert abs(lio.LoopDetector.information_matrix(1.5)[0, 0] - 1.0 / 25.0) < 1e-5


def test_create_fails_loudly_without_a_device():
    if capi.lib().lio_device_count() > 0:  # (with a device the same call must succeed)
        lio.LoopDetector(max_points=1024).close()
        return
    with pytest.raises(capi.LioError, match="no HIP device"):
        lio.LoopDetector()


def test_create_rejects_bad_params():
    with pytest.raises(capi.LioError, match="lio_loop"):
        lio.LoopDetector(k_correspondences=2)
    with pytest.raises(TypeError):
        lio.LoopDetector(no_such_field=1)


def test_wrapper_surface_and_defaults():
    import slam_wrapper as sw

    for name in ("set_loop_detection", "set_loop_config", "get_loop_edges"):
        assert hasattr(sw, name)
    assert sw.get_graph_status() == {"loop_detected": False}
    assert sw.get_loop_edges() == [] and sw.get_graph_edges() == {}


# ---- the recorded vectors: conditions, not measurements ----------------------------------------------------------------------------------------
def _matchings(G):
    """(coarse scores of the converged candidates, iterations, best score, fine score or None) of every recorded matching"""
    out = [(G["five/score"][G["five/converged"]], G["five/iterations"], float(G["five/score"][int(G["five/best"])]), float(G["five/fine_score"]),
            int(G["five/fine_iterations"]))]
    for m in range(len(G["drive/new_id"])):
        k = int(G["drive/n_candidates"][m])
        conv = G["drive/converged"][m, :k]
        out.append((G["drive/score"][m, :k][conv], G["drive/iterations"][m, :k], float(G["drive/best_score"][m]),
                    float(G["drive/fine_score"][m]) if G["drive/fine_ran"][m] else None, int(G["drive/fine_iterations"][m])))
    return out


def test_fixture_conditions():
    G = np.load(GOLD)
    assert len(G["five/converged"]) == 5 and len(G["drive/n_points"]) == LC.DRIVE_FRAMES and len(G["drive/edges"]) >= 1
    assert os.path.getsize(GOLD) < 256 * 1024
    for scores, its, best, fine, fine_it in _matchings(G):
        s = np.sort(scores)
        if len(s) >= 2:
            assert s[1] - s[0] > 0.01 * s[0], s  # the best and the runner-up are apart
        for v in s:
            assert abs(v - 3.0) > 0.03, v  # no coarse score near 2 x fitness_score_thresh
        if fine is not None:
            assert abs(fine - 1.5) > 0.015
            assert fine_it < 62
        for it in its:
            if it >= 0:
                assert it < 62, its  # no run stops at the iteration limit
    assert G["five/converged"].all()  # (no deliberately hopeless run is recorded: every run must stay clear of the iteration limit)
