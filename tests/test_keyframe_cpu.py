"""Key frames of the mapping mode, the parts that need no device: the ABI revision and symbols, lio_keyframe_decide against the numpy
restatement (tests/keyframe_cases.py) on and around its four thresholds, and the restatement's own radius / range rules on hand-made cases."""
import ctypes as C
import os
import re

import numpy as np

import keyframe_cases as kc
from lsd_amd import capi, lio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_revision_is_11_in_header_and_library():
    text = open(os.path.join(ROOT, "include", "lio_hip.h")).read()
    rev = int(re.search(r"#define LIO_ABI_VERSION (\d+)", text).group(1))
    assert rev >= 11 and capi.lib().lio_abi_version() == rev
    assert " 11 = lio_keyframe" in text


def test_new_symbols_resolve():
    L = capi.lib()
    for name in ("lio_keyframe_decide", "lio_keyframer_default_params", "lio_keyframer_create", "lio_keyframer_destroy", "lio_keyframer_reset",
                 "lio_keyframer_push_host", "lio_keyframer_pending", "lio_keyframer_pop", "lio_radius_outlier_host", "lio_keyframe_filter_host",
                 "lio_keyframer_fitness_host", "lio_keyframer_append_local_map_host", "lio_keyframer_download_local_map", "lio_keyframer_last_times"):
        assert getattr(L, name) is not None and name in capi.SYMBOLS
    p = lio.KeyFramer.default_params()
    assert (p.key_frame_distance, p.key_frame_degree, p.resolution, p.key_frame_range, p.scan_period) == (1.0, 10.0, 0.2, 50.0, 0.1)
    assert (p.radius, p.min_neighbours, p.local_map_cap, p.local_map_distance, p.fitness_range) == (1.0, 3, 100000, 2.0, 1.0)


def test_slam_wrapper_has_the_switch():
    import slam_wrapper

    assert callable(slam_wrapper.set_keyframe_output)


def _pose(t=(0, 0, 0), axis=(0, 0, 1), deg=0.0):
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    th = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def test_decide_on_and_around_the_thresholds():
    D, A = 2.0, 10.0
    prev = _pose((3.0, -2.0, 0.5), (0.2, -0.1, 1.0), 37.0)
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))    # noqa: E731  (the f32 neighbours: dx and da are stored as f32)
    down = lambda v: float(np.nextafter(np.float32(v), np.float32(-np.inf)))  # noqa: E731
    cases = []
    for d in (D / 2, 1.5 * D):
        for v in (d, up(d), down(d), d + 1e-3, d - 1e-3):
            cases.append(_pose((v, 0, 0)))
            cases.append(_pose((0, 0, v), (1, 0, 0), 1.0))
    for a in (A / 2, 1.5 * A):
        for v in (a, up(a), down(a), a + 1e-3, a - 1e-3):
            cases.append(_pose((0, 0, 0), (0, 0, 1), v))
            cases.append(_pose((0.1, 0.2, 0), (1, 2, 3), v))
    cases.append(_pose((0, 0, 0), (0, 0, 1), 180.0))     # a pure rotation of pi
    cases.append(_pose((0, 0, 0), (1, 1, 0), 180.0))
    cases.append(_pose())                                # no motion
    seen = set()
    for rel in cases:
        pose = prev @ rel
        need, must, dx, da = lio.keyframe_decide(prev, pose, D, A)
        rn, rm, rdx, rda, _ = kc.decide(prev, pose, D, A)
        assert (need, must) == (rn, rm), (rel, dx, da, rdx, rda)
        assert abs(dx - rdx) <= 1e-6 * max(1.0, rdx) and abs(da - rda) <= 1e-5 * max(1.0, rda)   # an f32 ulp: both are f32 values
        seen.add((need, must))
    assert seen == {(False, False), (True, False), (True, True)}
    # exactly on a threshold, from the identity (no rounding in prev^-1 * pose)
    I = np.eye(4)
    assert lio.keyframe_decide(I, _pose((1.0, 0, 0)), D, A)[:2] == (True, False)        # dx == D / 2: not below it
    assert lio.keyframe_decide(I, _pose((down(1.0), 0, 0)), D, A)[:2] == (False, False)
    assert lio.keyframe_decide(I, _pose((3.0, 0, 0)), D, A)[:2] == (True, True)         # dx == 1.5 D
    assert lio.keyframe_decide(I, _pose((down(3.0), 0, 0)), D, A)[:2] == (True, False)
    n, m, dx, da = lio.keyframe_decide(I, _pose((0, 0, 0), (0, 0, 1), 180.0), D, A)
    assert (n, m) == (True, True) and dx == 0.0 and da == float(np.float32(180.0))


def test_restatement_radius_rule_on_hand_made_cases():
    def cloud(*xyz):
        return np.array([[*p, 1.0] for p in xyz], np.float32)

    far = [(50.0, 50.0, 0.0), (50.1, 50.0, 0.0), (50.0, 50.1, 0.0), (50.1, 50.1, 0.0)]   # a cluster that always stays
    three = cloud((0, 0, 0), (0.1, 0, 0), (0, 0.1, 0), *far)
    assert kc.radius_keep(three)[0].tolist() == [3, 4, 5, 6]                  # exactly 3 points, themselves included: not MORE than 3
    four = cloud((0, 0, 0), (0.1, 0, 0), (0, 0.1, 0), (0, 0, 0.1), *far)
    assert kc.radius_keep(four)[0].tolist() == list(range(8))                 # exactly 4: kept
    assert kc.radius_keep(cloud(*[(1, 2, 3)] * 4))[0].tolist() == [0, 1, 2, 3]   # coincident points count
    assert kc.radius_keep(cloud(*[(1, 2, 3)] * 3))[0].tolist() == []
    one = np.float32(1.0)
    edge = cloud((0, 0, 0), (one, 0, 0), (0, one, 0), (0, 0, one))            # three neighbours at d2 == 1.0f exactly: the centre has 4
    assert kc.radius_keep(edge)[0].tolist() == [0]
    edge[1, 0] = np.nextafter(one, np.float32(2))                              # one of them an ulp farther: d2 > 1.0f
    assert kc.radius_keep(edge)[0].tolist() == []
    nan = cloud((0, 0, 0), (0.1, 0, 0), (np.nan, 0, 0), (0, 0.1, 0), (0, np.inf, 0), (0, 0, 0.1))
    idx, dropped = kc.radius_keep(nan)
    assert idx.tolist() == [0, 1, 3, 5] and dropped == 2
    assert kc.radius_keep(cloud((0, 0, 0), (9, 9, 9)), 1.0, 0)[0].tolist() == [0, 1]   # min_neighbours = 0: a point is its own neighbour
    r = cloud((0.0, 1, 0), (-0.0, 1, 0), (5.0, 1, 0), (1, np.nextafter(np.float32(5), np.float32(0)), 0), (1, -5.0, 0), (1e-30, -1e-30, 0))
    assert kc.range_keep(r, 5.0).tolist() == [False, False, False, True, False, True]


def test_gated_nearest_equals_brute_force():
    rng = np.random.default_rng(3)
    t = rng.uniform(-6, 6, (1500, 3)).astype(np.float32)
    s = rng.uniform(-8, 8, (700, 3)).astype(np.float32)
    s[:5] = t[:5] + np.array([1.0, 0, 0], np.float32)
    b, g = kc.nearest_d2_brute(s, t), kc.nearest_d2_gated(s, t, 1.0)
    inl = b <= np.float32(1.0)
    assert inl.sum() > 50 and (~inl).sum() > 50
    assert np.array_equal(inl, g <= np.float32(1.0)) and np.array_equal(b[inl].view(np.uint32), g[inl].view(np.uint32))
