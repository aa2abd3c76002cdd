"""GNSS in localisation mode, the parts that need no device: lio_update_origin against the restatement of tests/gnss_loc_cases.py (built on
rtk_cases.UtmRef, which is pinned bit for bit to the reference's projector), the bracket rule of the localiser's INS list and the walk of the
INS-aided search in the restatement, case by case, and the ABI.

Bounds.  lio_update_origin against the restatement: 1e-6 m, the project's projection bound (tests/test_rtk_cpu.py: about 60 f64 operations on
values up to 1e7 m per projection, ulp 1.9e-9 m; an inverse and a forward here).  A map given under B and re-anchored to A against the same map
given under A: < 1e-4 m.  That number is the REFERENCE projector's own inverse error -- its FromLocalToGlobal is a truncated series -- measured
with the restatement alone, without the library: 4.8e-5 m for all three origin pairs (printed below)."""
import os
import re

import numpy as np
import pytest

import gnss_loc_cases as G
import rtk_cases as R
from lsd_amd import capi, lio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_revision_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "lio_hip.h")).read()
    rev = int(re.search(r"#define LIO_ABI_VERSION (\d+)", hdr).group(1))
    assert rev >= 23 and capi.lib().lio_abi_version() == rev >= capi.ABI_REQUIRED == 23
    for s in ("lio_sc_local_search", "lio_sc_set_positions", "lio_sc_last_local", "lio_update_origin"):
        assert s in capi.SYMBOLS and hasattr(capi.lib(), s) and s in hdr


def test_the_switch_is_off_by_default_in_localisation_mode(tmp_path, monkeypatch):
    import slam_wrapper as sw

    monkeypatch.delenv("LSD_AMD_GNSS", raising=False)
    assert sw.init_slam("offline", str(tmp_path), "Localization", ["0-lidar", "RTK", "IMU"], 0.2, 1.0, 10.0, 50.0) == ["0-lidar", "RTK", "IMU"]
    try:
        gs = sw._gnss_state()
        assert gs["enabled"] is False and gs["stamps"] == [] and gs["latest_held"] is False and gs["observation"]["used"] is False
        sw._push_gnss(dict(timestamp=1, latitude=31.2, longitude=121.5, altitude=4.0, heading=0.0, pitch=0.0, roll=0.0, Status=1))  # not looked at
        assert sw._gnss_state()["latest_held"] is False
        r = sw._last_relocalization()
        assert r["kind"] == "global" and r["n_examined"] == 0
        assert "Localisation mode" in sw.set_gnss.__doc__
    finally:
        sw.deinit_slam()


@pytest.mark.parametrize("pair", range(3))
def test_update_origin_against_the_restatement(pair):
    a, b = G.ORIGIN_PAIRS[pair]
    PA, PB = G.seeded_map(a, b)
    assert len(PA) == 200
    prior = PB[::7, :3, 3].copy()
    got_P, got_X = lio.update_origin(b, a, PB, prior)
    want_P, want_X = G.update_origin(b, a, PB, prior)
    err = max(np.abs(got_P - want_P).max(), np.abs(got_X - want_X).max())
    back = np.abs(got_P[:, :3, 3] - PA[:, :3, 3]).max()
    back_ref = np.abs(want_P[:, :3, 3] - PA[:, :3, 3]).max()
    moved = np.abs(PB[:, :3, 3] - PA[:, :3, 3]).max()
    print(f"pair {pair}: |library - restatement| {err:.3e} m; back under A within {back:.3e} m (restatement alone {back_ref:.3e} m); the origins move a pose by {moved:.3f} m")
    assert err <= 1e-6
    assert back < 1e-4 and back_ref < 1e-4
    assert moved > (1.0 if pair == 0 else 30.0)  # the case is not vacuous
    assert np.array_equal(got_P[:, :3, :3].view(np.uint64), PB[:, :3, :3].view(np.uint64)) and np.array_equal(got_P[:, 3], PB[:, 3])  # rotations bit-equal
    assert np.array_equal(got_X, got_P[::7, :3, 3])  # a prior's measurement moves as a pose's translation does
    assert np.array_equal(PB[::7, :3, 3], prior)     # the inputs are left alone


def test_update_origin_with_equal_origins_is_the_identity():
    a = G.ORIGIN_PAIRS[0][0]
    PA, _ = G.seeded_map(a, a)
    got_P, got_X = lio.update_origin(a, a, PA, PA[:5, :3, 3])
    want_P, _ = G.update_origin(a, a, PA)
    assert np.abs(got_P - want_P).max() <= 1e-6
    assert np.abs(got_P - PA).max() < 1e-4 and np.abs(got_X - PA[:5, :3, 3]).max() < 1e-4  # the inverse projection's own error, as above
    assert np.abs(got_P[:, 2, 3] - PA[:, 2, 3]).max() <= 2e-14  # (z + a) - a with |z| <= 5 and a = 14: two roundings at an ulp of 3.6e-15
    P0, X0 = lio.update_origin(a, G.ORIGIN_PAIRS[1][1])
    assert P0.shape == (0, 4, 4) and X0.shape == (0, 3)


# ---- the bracket rule ---------------------------------------------------------------------------------------------------------------------------
T0 = 1_700_000_000_000_000


def _entry(stamp, x=0.0, precision=1.0, dimension=6):
    T = R.transform_from_rpyt(x, 2.0 * x, 0.1 * x, 10.0 * x, 0.0, 0.0)
    return dict(stamp_us=int(stamp), T=T, precision=precision, dimension=dimension)


def _list(stamps, **kw):
    L = G.InsList()
    for k, s in enumerate(stamps):
        L.push(_entry(s, float(k), **kw))
    return L


def test_bracket_empty_list():
    L = G.InsList()
    assert L.observe(T0) is None and L.stamps() == []


def test_bracket_stamp_before_the_first_and_after_the_last():
    L = _list([T0, T0 + 50_000, T0 + 100_000])
    assert L.observe(T0 - 1) is None and len(L.stamps()) == 3  # below the first entry nothing happens
    assert L.observe(T0 + 100_001) is None and L.stamps() == []  # beyond the last the list is cleared
    L = _list([T0, T0 + 50_000])
    assert L.observe(T0 + 50_000) is not None and len(L.stamps()) == 2  # AT the last it is not


def test_bracket_gap_of_exactly_200_ms_and_just_under():
    L = _list([T0, T0 + 200_000])
    assert L.observe(T0 + 100_000) is None  # (dt2 - dt) < 0.2 is strict
    L = _list([T0, T0 + 199_999])
    o = L.observe(T0 + 100_000)
    assert o is not None and (o["first"], o["second"]) == (T0, T0 + 199_999)
    # a wide gap first, a narrow pair after it: the walk moves on to the pair that holds
    L = _list([T0, T0 + 300_000, T0 + 350_000])
    assert L.observe(T0 + 100_000) is None
    o = L.observe(T0 + 320_000)
    assert (o["first"], o["second"]) == (T0 + 300_000, T0 + 350_000)


def test_bracket_stamp_equal_to_an_entry():
    L = _list([T0, T0 + 50_000, T0 + 100_000])
    o = L.observe(T0)  # the walk starts with first == second: the pair (entry, itself), ratio 0 / 1
    assert (o["first"], o["second"], o["ratio"]) == (T0, T0, 0.0) and np.array_equal(o["T"][:3, 3], L.data[0]["T"][:3, 3])
    o = L.observe(T0 + 50_000)  # a later entry is first met as the SECOND of a pair
    assert (o["first"], o["second"]) == (T0, T0 + 50_000) and o["ratio"] == 50_000 / 50_001


def test_bracket_ratio_carries_plus_one():
    L = _list([T0, T0 + 50_000])
    o = L.observe(T0 + 25_000)
    assert o["ratio"] == 25_000 / 50_001 and o["ratio"] != 0.5
    want = R.interpolate_transform(L.data[0]["T"], L.data[1]["T"], 25_000 / 50_001)
    assert np.array_equal(o["T"], want)


def test_bracket_precision_and_dimension_from_the_first_entry():
    L = G.InsList()
    L.push(_entry(T0, 0.0, precision=0.5, dimension=6))
    L.push(_entry(T0 + 50_000, 1.0, precision=7.0, dimension=2))
    o = L.observe(T0 + 40_000)
    assert (o["precision"], o["dimension"]) == (0.5, 6)


def test_list_holds_ten_and_the_oldest_leaves_first():
    L = _list([T0 + 50_000 * k for k in range(13)])
    assert L.stamps() == [T0 + 50_000 * k for k in range(3, 13)]


# ---- the walk ------------------------------------------------------------------------------------------------------------------------------------
IDS = np.array([4, 9, 2, 7])


def test_walk_far_from_the_map():
    assert G.local_walk(IDS, [25.1, 30.0, 31.0, 40.0], [0.1, 0.1, 0.1, 0.1], [3, 4, 5, 6], 5.0) == (-1, 0, 1.0, 0)
    assert G.local_walk(IDS, [25.0, 30.0, 31.0, 40.0], [0.1, 0.2, 0.2, 0.2], [3, 4, 5, 6], 5.0) == (4, 3, 0.1, 1)  # > is strict: 25 is not far


def test_walk_stops_at_a_tenth_of_the_square_after_a_match():
    # precision 5: 25 before a match, 2.5 after one
    assert G.local_walk(IDS, [1.0, 2.5, 2.6, 2.7], [0.5, 0.4, 0.1, 0.1], [3, 4, 5, 6], 5.0) == (9, 4, 0.4, 2)
    # no match yet (nothing under 1.0): the wide gate goes on holding
    assert G.local_walk(IDS, [1.0, 2.6, 20.0, 26.0], [1.0, 1.5, 0.3, 0.1], [3, 4, 5, 6], 5.0) == (2, 5, 0.3, 3)


def test_walk_tie_in_descriptor_distance_keeps_the_earlier():
    assert G.local_walk(IDS, [1.0, 1.1, 1.2, 1.3], [0.3, 0.3, 0.3, 0.3], [3, 4, 5, 6], 5.0) == (4, 3, 0.3, 4)


def test_walk_no_frame_under_one():
    big = 10000000.0
    assert G.local_walk(IDS, [1.0, 1.1, 1.2, 1.3], [1.0, big, np.nan, 1.2], [3, 4, 5, 6], 5.0) == (-1, 0, 1.0, 4)


def test_walk_fewer_than_ten_frames():
    pos = np.array([[0, 0, 0], [3, 0, 0], [1, 0, 0]], np.float32)
    ids, d2 = G.nearest_ten(pos, (0.2, 0.0))
    assert ids.tolist() == [0, 2, 1] and len(d2) == 3
    assert G.local_walk(ids, d2, [0.9, 0.2, 0.1], [1, 2, 3], 5.0) == (2, 2, 0.2, 2)  # frame 1 lies beyond 2.5
    ids, d2 = G.nearest_ten(np.zeros((0, 3), np.float32), (0.0, 0.0))
    assert len(ids) == 0 and G.local_walk(ids, d2, [], [], 5.0) == (-1, 0, 1.0, 0)


def test_nearest_ten_orders_by_distance_then_id_and_ignores_the_query_height():
    pos = np.array([[5, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 9], [0, 1, 0]] + [[20 + k, 0, 0] for k in range(8)], np.float32)
    ids, d2 = G.nearest_ten(pos, (0.0, 0.0))
    assert ids.tolist() == [1, 2, 4, 0, 3, 5, 6, 7, 8, 9] and d2[:3].tolist() == [1.0, 1.0, 1.0] and d2[4] == 81.0
