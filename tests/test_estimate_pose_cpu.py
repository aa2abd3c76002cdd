"""The operator's pose hint without a device: the ABI revision and the new symbols, the numpy restatement of the nearest-key-frame rule against
cases worked by hand (lio_localmap_create needs a device, so the C entry itself is checked against the same cases in test_estimate_pose_gpu.py),
the chunked z sum, the hint matrix for arrows along +x, -x and +y, and the result logic."""
import ctypes as C
import os
import re

import numpy as np

import estimate_pose_cases as E
from lsd_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lio_hip.h")
NEW = ["lio_gicp_set_target_device", "lio_gicp_set_source_device", "lio_scan_ds_device", "lio_localmap_nearest", "lio_localmap_gather", "lio_localmap_z_mean",
       "lio_localmap_download_gather", "lio_localmap_gather_device", "lio_localmap_store_frame", "lio_localmap_frame", "lio_estimate_matcher_params",
       "lio_localmap_estimate_pose"]


def test_abi_19_and_the_new_symbols():
    hdr = open(HEADER).read()
    rev = int(re.search(r"#define LIO_ABI_VERSION (\d+)", hdr).group(1))
    assert rev >= 19 and capi.lib().lio_abi_version() == rev
    L = capi.lib()
    for name in NEW:
        assert name in capi.SYMBOLS and getattr(L, name).argtypes is not None, name
    assert int(re.search(r"#define LIO_ESTIMATE_K (\d+)", hdr).group(1)) == capi.ESTIMATE_K == E.ESTIMATE_K
    # the report's layout: six ints, two counts, four flags, then doubles
    assert C.sizeof(capi.EstimateReport) == 48 + 8 * (2 + 16 + 1 + 7) and capi.EstimateReport.z_mean_target.offset == 48
    # null handles are invalid arguments, nothing is launched
    assert L.lio_localmap_nearest(None, None, 5, None, None) == capi.LIO_E_INVALID
    assert L.lio_localmap_gather(None, None, 0, None, None) == capi.LIO_E_INVALID
    assert L.lio_localmap_estimate_pose(None, None, None, 0, None, None, None) == capi.LIO_E_INVALID
    assert L.lio_gicp_set_target_device(None, None, 0) == capi.LIO_E_INVALID and L.lio_gicp_set_source_device(None, None, 0) == capi.LIO_E_INVALID
    assert not L.lio_scan_ds_device(None, None) and not L.lio_localmap_frame(None, 0, None) and not L.lio_localmap_gather_device(None, None)
    p = capi.NdtParams()
    L.lio_estimate_matcher_params(C.byref(p))
    lp = capi.LoopParams()
    L.lio_loop_default_params(C.byref(lp))
    assert (p.rotation_epsilon_deg, p.transformation_epsilon, p.max_iterations, p.max_process_time_ms) == (
        lp.coarse_rotation_epsilon_deg, lp.coarse_translation_epsilon, lp.max_iterations, -1.0)


def test_nearest_restatement_against_hand_worked_cases():
    for name, pos, xy, k, want_ids, want_near in E.nearest_cases():
        ids, d2 = E.nearest(pos, xy, k)
        assert ids.tolist() == want_ids, name
        assert (np.diff(d2) >= 0).all() and d2.dtype == np.float32, name
        assert E.within_range(ids, d2) == want_near, name
    _, pos, xy, k, _, _ = [c for c in E.nearest_cases() if c[0] == "edge_of_20_m"][0]
    ids, d2 = E.nearest(pos, xy, k)
    assert d2[1] == np.float32(400.0) and d2[2] == np.nextafter(np.float32(400.0), np.float32(np.inf))  # exactly 20 m, and one ulp beyond
    _, pos, xy, k, _, _ = [c for c in E.nearest_cases() if c[0] == "equal_distance"][0]
    assert len(set(E.nearest(pos, xy, 4)[1][:3].tolist())) == 1


def test_chunked_z_sum():
    assert E.z_sum(np.zeros(0, np.float32)) == 0.0
    assert E.z_sum(np.float32([1.5])) == 1.5
    z = np.arange(1, 258, dtype=np.float32)  # two chunks: 1 .. 256 and 257
    assert E.chunk_sums(z).tolist() == [256 * 257 / 2, 257.0] and E.z_sum(z) == 257 * 258 / 2
    # the order is the rule: lane 0 of the tree meets lane 128 first, so 2^60 and -2^60 cancel before the 1 arrives; added in sequence the 1 is lost
    z = np.zeros(256, np.float32)
    z[0], z[1], z[128] = 2.0 ** 60, 1.0, -(2.0 ** 60)
    seq = np.float64(0.0)
    for v in z.astype(np.float64):
        seq = seq + v
    assert E.z_sum(z) == 1.0 and seq == 0.0
    cloud = np.zeros((3, 4), np.float32)
    cloud[:, 2] = [1, 2, 4]
    assert E.z_mean(cloud) == 7.0 / 3.0


def test_hint_matrix_for_arrows_along_the_axes():
    T = E.hint_matrix(-10.0, 0.2, -9.0, 0.2)  # +x: no rotation
    assert np.array_equal(T, np.array([[1, 0, 0, -10.0], [0, 1, 0, 0.2], [0, 0, 1, 0], [0, 0, 0, 1.0]]))
    T = E.hint_matrix(3.0, 4.0, 1.0, 4.0)  # -x: half a turn about z, where FromTwoVectors has no unique answer
    assert np.allclose(T[:3, :3], np.diag([-1.0, -1.0, 1.0]), atol=2e-16) and T[0, 0] == -1.0 and T[2, 2] == 1.0 and np.array_equal(T[:3, 3], [3.0, 4.0, 0.0])
    T = E.hint_matrix(0.0, 0.0, 0.0, 2.5)  # +y: a quarter turn
    assert np.allclose(T[:3, :3], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-16) and T[1, 0] == 1.0 and T[0, 1] == -1.0
    assert E.hint_matrix(1.0, 1.0, 1.0, 1.0) is None
    for T in (E.hint_matrix(0, 0, 1, 1), E.hint_matrix(0, 0, -1, 2)):
        assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-15 and np.array_equal(T[3], [0, 0, 0, 1]) and T[2, 3] == 0.0


def test_guess_and_result_logic():
    hint = E.hint_matrix(0.1, 0.2, 1.1, 0.7)
    T, g = E.guess_matrix(hint, 1.25, -0.55)
    assert T[2, 3] == 1.8 and np.array_equal(T[:2], hint[:2]) and np.array_equal(g, T.astype(np.float32).astype(np.float64)) and g[0, 3] == np.float64(np.float32(0.1))
    assert E.result_logic(False, 0.0) == (0, False)
    assert E.result_logic(True, 0.49) == (1, True) and E.result_logic(True, 0.5) == (0, True)
    assert E.result_logic(True, 4.99) == (0, True) and E.result_logic(True, 5.0) == (0, False)
    F = E.final_pose(np.full((4, 4), 0.1))
    assert F[0, 0] == np.float64(np.float32(0.1)) and np.array_equal(F[3], [0, 0, 0, 1])
