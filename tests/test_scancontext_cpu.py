"""Scan Context, the parts that need no device: the ABI revision and symbols, the refusal without a device, and the numpy restatement
(tests/sc_cases.py) against what the reference's own SCManager wrote for the scene (tests/golden/scancontext.npz, tools/record_sc_golden.py).

The rule of the comparison.  Descriptors are EQUAL: the inputs keep 1e-4 deg from every sector edge and 1e-4 m from every ring edge and from the
80 m limit (sc_cases.keep_margin asserts it), so atanf's last bit cannot move a point.  Ring keys agree within one f32 ulp, sector keys and
distances within 1e-12: Eigen's vectorised sums differ from sequential ones by a few ulp over 60 terms of size <= 10, ~1e-14, and this is a
hundred times that.  A choice (a candidate list, a shift, a globalSearch answer) is compared where the restatement shows a gap to the
runner-up larger than what those differences can move, and no more than 2 % of the comparisons may be skipped for lack of one."""
import os
import re

import numpy as np
import pytest

import sc_cases as S
from lsd_amd import capi, lio

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "lio_hip.h")
GOLD = np.load(os.path.join(HERE, "golden", "scancontext.npz"))
TOL = 1e-12


def test_abi_revision_and_symbols():
    hdr = open(HEADER).read()
    rev = int(re.search(r"#define LIO_ABI_VERSION (\d+)", hdr).group(1))
    assert rev >= 18 and capi.lib().lio_abi_version() == rev
    names = ["lio_sc_create", "lio_sc_destroy", "lio_sc_reset", "lio_sc_num_frames", "lio_sc_add_frames_host", "lio_sc_download_frame", "lio_sc_describe_host",
             "lio_sc_set_active", "lio_sc_distance", "lio_sc_search", "lio_sc_global_search_host", "lio_sc_shift_to_yaw", "lio_sc_last_dropped", "lio_sc_last_times",
             "lio_gicp_fitness_score"]
    for n in names:
        assert n in capi.SYMBOLS and re.search(r"\b%s\(" % n, hdr) and hasattr(capi.lib(), n), n
    for k, v in (("LIO_SC_RINGS", 20), ("LIO_SC_SECTORS", 60), ("LIO_SC_CANDIDATES", 10), ("LIO_SC_MAX_SHIFTS", 9)):
        assert int(re.search(r"#define %s (\d+)" % k, hdr).group(1)) == v
    assert (lio.ScanContext.RINGS, lio.ScanContext.SECTORS, lio.ScanContext.CANDIDATES) == (S.RINGS, S.SECTORS, S.CANDIDATES)
    assert lio.ScanContext.SEARCH_SHIFTS == S.SEARCH_SHIFTS


def test_host_only_entry_points():
    L = capi.lib()
    for s in range(60):  # the yaw of a shift needs no device
        assert np.float32(L.lio_sc_shift_to_yaw(s)).view(np.uint32) == S.shift_to_yaw(s).view(np.uint32)
    assert L.lio_sc_num_frames(None) == capi.LIO_E_INVALID and L.lio_sc_reset(None) == capi.LIO_E_INVALID
    assert L.lio_sc_set_active(None, None, 0) == capi.LIO_E_INVALID and L.lio_sc_last_times(None, None, None, None) == capi.LIO_E_INVALID
    assert L.lio_gicp_fitness_score(None, None, 1.0, None, None) == capi.LIO_E_INVALID
    L.lio_sc_destroy(None)
    assert not L.lio_sc_create(0, 0, 100) and not L.lio_sc_create(0, 100, 0)


def test_create_fails_loudly_without_a_device():
    if capi.lib().lio_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(capi.LioError, match="no HIP device"):
        lio.ScanContext()


def test_inputs_are_the_recorded_ones_and_keep_the_margin():
    scn = S.scene()
    assert [S.cloud_hash(c) for c in scn["frames"]] == list(GOLD["frame_hash"]) and [S.cloud_hash(c) for c in scn["queries"]] == list(GOLD["query_hash"])
    for c in scn["frames"][:3]:
        assert len(S.keep_margin(c)) == len(c)
    assert len(S.keep_margin(scn["queries"][1], S.SEARCH_SHIFTS)) == len(scn["queries"][1])
    # the margin filter does drop what lies on an edge
    edge = np.array([[4.0, 0.00001, 1, 0], [10.0, 10.0 * np.tan(np.radians(6.0)), 1, 0], [48.00003, 64.0, 1, 0], [10.3, 0.7, 1, 0]], np.float32)
    assert len(S.keep_margin(edge)) == 1


def test_descriptors_and_keys_against_the_reference():
    scn = S.scene()
    assert np.array_equal(scn["desc"], GOLD["frame_desc"].astype(np.float64))
    ulp = np.spacing(np.abs(GOLD["frame_ring"]))
    assert (np.abs(scn["ring"].astype(np.float64) - GOLD["frame_ring"].astype(np.float64)) <= ulp).all()
    assert np.abs(scn["sector"] - GOLD["frame_sector"]).max() <= TOL
    for q, c in enumerate(scn["queries"]):
        for k, (dx, dy) in enumerate(S.SEARCH_SHIFTS):
            d = S.describe(c, dx, dy)
            assert np.array_equal(d, GOLD["query_desc"][q, k].astype(np.float64)), (q, k)
            assert (np.abs(S.ring_key(d).astype(np.float64) - GOLD["query_ring"][q, k].astype(np.float64)) <= np.spacing(np.abs(GOLD["query_ring"][q, k]))).all()
            assert np.abs(S.sector_key(d) - GOLD["query_sector"][q, k]).max() <= TOL


def _ring_bound(d, keys):
    """what a one-ulp difference in every ring key can move a squared f32 ring-key distance d by: 2 * sum|a_i - b_i| * 2u <= 4u * sqrt(20 d), plus the
    f32 roundings of 40 operations on a sum of size d"""
    u = float(np.spacing(np.float32(np.abs(keys).max())))
    return 4.0 * u * np.sqrt(20.0 * d) + 40.0 * 2.0 ** -24 * d


def test_candidates_distances_and_answers_against_the_reference():
    scn = S.scene()
    n_cmp = n_skip = 0
    for q, res in enumerate(scn["search"]):
        for k, (ids, d, s, gap) in enumerate(res["per_shift"]):
            desc = S.describe(scn["queries"][q], *S.SEARCH_SHIFTS[k])
            # the candidate list: clear where every gap between neighbours of the first eleven ring-key distances is
            rd = np.sort(S.ring_distances(S.ring_key(desc), scn["ring"]).astype(np.float64))[:S.CANDIDATES + 1]
            n_cmp += 1
            if (np.diff(rd) <= 2.0 * _ring_bound(rd[1:], scn["ring"])).any():
                n_skip += 1
                continue
            assert np.array_equal(ids, GOLD["cand_ids"][q, k]), (q, k)
            assert np.abs(d - GOLD["cand_dist"][q, k]).max() <= TOL, (q, k)
            for c in range(len(ids)):
                n_cmp += 1
                if not gap[c] > TOL:
                    n_skip += 1
                    continue
                assert s[c] == GOLD["cand_shift"][q, k, c], (q, k, c)
        n_cmp += 1
        if not S.search_gap(res) > TOL:
            n_skip += 1
            continue
        assert res["match_id"] == GOLD["gs_id"][q] and abs(res["score"] - GOLD["gs_score"][q]) <= TOL
        assert res["yaw"].view(np.uint32) == GOLD["gs_yaw"][q].view(np.uint32)
    d, s, gaps = S.distance(GOLD["query_desc"][GOLD["pair_query"], 0].astype(np.float64), GOLD["frame_desc"][GOLD["pair_frame"]].astype(np.float64))
    assert np.abs(d - GOLD["pair_dist"]).max() <= TOL
    for c in range(len(d)):
        n_cmp += 1
        if not min(gaps["key_gap"][c], gaps["shift_gap"][c]) > TOL:
            n_skip += 1
            continue
        assert s[c] == GOLD["pair_shift"][c]
    print(f"{n_cmp} comparisons, {n_skip} skipped for lack of a gap")
    assert n_skip <= 0.02 * n_cmp
    # the first five are the positive cases of the relocalisation: the frame beside the scan, the heading as the column shift
    assert tuple(int(x) for x in GOLD["gs_id"][:5]) == S.POSITIVE_FRAMES
    assert tuple(r["shift"] for r in scn["search"][:5]) == S.POSITIVE_SHIFTS


def test_restatement_edges():
    """what the GPU test leans on, checked here against first principles"""
    one = S.describe(np.array([[3.0, 4.0, 1.0, 0.0]], np.float32))  # range 5 -> ring 2; atan(4/3) = 53.13 deg -> sector 9
    assert (one != 0).sum() == 1 and one[1, 8] == 1.5
    assert S.describe(np.array([[3.0, 4.0, -1000.5, 0.0]], np.float32)).max() == 0.0 and S.describe(np.array([[3.0, 4.0, -0.5, 0.0]], np.float32)).sum() == 0.0
    z, rng, theta, ring, sector, keep, bad = S.polar(np.array([[0, 0, 0, 0], [np.nan, 0, 0, 0], [80, 0, 0, 0], [np.nextafter(np.float32(80), np.float32(90)), 0, 0, 0]], np.float32))
    assert bad == 1 and list(ring) == [1, 20, 20] and list(sector) == [1, 1, 1] and list(keep) == [True, True, False]
    a = np.arange(20, dtype=np.float32)
    assert S.ring_distances(a, a[None] + 1)[0] == 20.0
    assert S.shift_to_yaw(30) == np.float32(np.pi)
