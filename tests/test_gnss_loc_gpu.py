"""GNSS in localisation mode on the device: lio_sc_local_search (csrc/scancontext.hip) through the C ABI against the numpy restatement of
tests/gnss_loc_cases.py, to the last bit -- the matched frame, the column shift, the score as f64, the number of distances the walk read, and
the ten nearest frames with what the walk saw of each; the ten also against a brute-force ordering written here."""
import numpy as np
import pytest

import gnss_loc_cases as G
from lsd_amd import capi, lio

pytestmark = pytest.mark.gpu
SIZES = (1, 9, 10, 11, 64, 65, 2049)  # below / at / above the ten, one wave, one wave + 1, nine workgroups of the key kernel


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def sc():
    h = lio.ScanContext(max_frames=2100, max_points_per_call=1 << 19)
    yield h
    h.close()


_BANKS = {}


def _bank(sc, n, pos=None):
    """the bank of n frames on the device (positions: the case's own, or `pos`)"""
    if n not in _BANKS:
        _BANKS[n] = G.local_bank(n)
    clouds, p = _BANKS[n]
    sc.reset()
    assert sc.add_frames(clouds) == 0 and sc.num_frames() == n
    sc.set_positions(p if pos is None else pos)
    return clouds, (p if pos is None else pos)


def _check(got, want, what):
    print(f"{what}: match {got['match_id']} shift {got['shift']} score {got['score']!r} examined {got['n_examined']} ids {got['ids'].tolist()}")
    assert got["match_id"] == want["match_id"] and got["shift"] == want["shift"] and got["n_examined"] == want["n_examined"], (what, want)
    assert _same(np.float64(got["score"]).reshape(1), np.float64(want["score"]).reshape(1)), (what, got["score"], want["score"])
    assert _same(np.float32(got["yaw"]).reshape(1), np.float32(want["yaw"]).reshape(1)), what
    assert np.array_equal(got["ids"], want["ids"]) and _same(got["d2"], np.asarray(want["d2"], np.float32)), what
    assert _same(got["dist"], np.asarray(want["dist"], np.float64)) and np.array_equal(got["shifts"], want["shifts"]), what


def _brute(pos, xy):
    """the ten nearest by a plain sort over (d2, id), d2 from f32 scalars one frame at a time"""
    qx, qy = np.float32(xy[0]), np.float32(xy[1])
    rows = []
    for i, (x, y, z) in enumerate(np.asarray(pos, np.float32)):
        dx, dy = np.float32(x - qx), np.float32(y - qy)
        rows.append((float(np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(z * z))), i))
    return [i for _, i in sorted(rows)[:10]]


@pytest.mark.parametrize("n", SIZES)
def test_local_search_against_the_restatement(sc, n):
    clouds, pos = _bank(sc, n)
    rng = np.random.default_rng(n)
    for trial in range(4):
        k = int(rng.integers(n))
        xy = pos[k, :2].astype(np.float64) + rng.uniform(-1.0, 1.0, 2)
        precision = (5.0, 2.0, 50.0, 0.8)[trial]
        scan = G.query_of(clouds[k], seed=1000 * n + trial)
        got = sc.local_search(scan, [xy[0], xy[1], 123.0], precision)  # the INS height is not read
        want = G.local_search(scan, clouds, pos, xy, precision)
        _check(got, want, f"F={n} trial {trial} near {k} precision {precision}")
        assert got["ids"].tolist() == _brute(pos, xy) and len(got["ids"]) == min(10, n)
        if trial == 0 and n > 1:
            assert got["match_id"] == k and got["score"] < 0.5  # the frame the scan was made from, among its neighbours
        again = sc.local_search(scan, [xy[0], xy[1], -7.0], precision)
        _check(again, got, "two runs")


def test_equal_distances_go_to_the_smaller_id(sc):
    _, pos = _BANKS.setdefault(65, G.local_bank(65))
    pos = pos.copy()
    pos[40], pos[7] = pos[23], pos[23]  # three frames at one place
    clouds, pos = _bank(sc, 65, pos)
    xy = pos[23, :2].astype(np.float64) + 0.25
    got = sc.local_search(G.query_of(clouds[40], 5), [xy[0], xy[1], 0.0], 5.0)
    assert got["ids"][:3].tolist() == [7, 23, 40] and got["d2"][0] == got["d2"][1] == got["d2"][2]
    _check(got, G.local_search(G.query_of(clouds[40], 5), clouds, pos, xy, 5.0), "ties")


def test_a_frames_own_height_counts_and_the_query_has_none(sc):
    _, pos = _BANKS.setdefault(64, G.local_bank(64))
    pos = pos.copy()
    xy = pos[30, :2].astype(np.float64)
    pos[30, 2] = 50.0  # right under the INS position in x, y, and 50 m up: not among the ten, whatever height the INS reports
    clouds, pos = _bank(sc, 64, pos)
    scan = G.query_of(clouds[30], 6)
    got = sc.local_search(scan, [xy[0], xy[1], 50.0], 5.0)
    flat = np.lexsort((np.arange(64), ((pos[:, :2] - xy.astype(np.float32)) ** 2).sum(1)))[:10]
    assert flat[0] == 30 and 30 not in got["ids"].tolist()
    _check(got, G.local_search(scan, clouds, pos, xy, 5.0), "z quirk")


def test_the_precision_gates_on_both_sides(sc):
    clouds, pos = _bank(sc, 11)
    xy = pos[4, :2].astype(np.float64) + [0.4, -0.3]
    scan = G.query_of(clouds[4], 8)
    base = sc.local_search(scan, [xy[0], xy[1], 0.0], 100.0)
    assert base["ids"][0] == 4 and base["n_examined"] == 10 and base["match_id"] == 4
    d0, d1 = float(base["d2"][0]), float(base["d2"][1])
    # "far from the map": the nearest frame's d2 against precision^2
    lo, hi = np.sqrt(d0) * (1 - 1e-9), np.sqrt(d0) * (1 + 1e-9)
    assert d0 > lo * lo and not d0 > hi * hi
    far, near = sc.local_search(scan, [xy[0], xy[1], 0.0], lo), sc.local_search(scan, [xy[0], xy[1], 0.0], hi)
    assert far["match_id"] == -1 and far["n_examined"] == 0 and far["score"] == 1.0 and far["yaw"] == 0.0
    assert near["match_id"] == 4 and near["n_examined"] == 1  # the second frame lies beyond precision^2 / 10
    # after a match: the second frame's d2 against precision^2 / 10
    lo, hi = np.sqrt(10.0 * d1) * (1 - 1e-9), np.sqrt(10.0 * d1) * (1 + 1e-9)
    assert d1 > lo * lo / 10.0 and not d1 > hi * hi / 10.0
    stop, go = sc.local_search(scan, [xy[0], xy[1], 0.0], lo), sc.local_search(scan, [xy[0], xy[1], 0.0], hi)
    assert stop["n_examined"] == 1 and go["n_examined"] >= 2
    for got, p in ((far, np.sqrt(d0) * (1 - 1e-9)), (near, np.sqrt(d0) * (1 + 1e-9)), (stop, lo), (go, hi)):
        _check(got, G.local_search(scan, clouds, pos, xy, p), f"precision {p!r}")


def test_a_point_that_is_not_finite_is_dropped(sc):
    clouds, pos = _bank(sc, 10)
    xy = pos[2, :2].astype(np.float64)
    scan = G.query_of(clouds[2], 9)
    bad = np.concatenate([scan[:70], np.array([[np.nan, 1, 1, 0], [1, np.inf, 1, 0]], np.float32), scan[70:]])
    got = sc.local_search(bad, [xy[0], xy[1], 0.0], 5.0)
    assert sc.last_dropped() == 2
    _check(got, G.local_search(scan, clouds, pos, xy, 5.0), "non-finite")


def test_positions_must_cover_the_bank_and_an_empty_bank_answers_no(sc):
    sc.reset()
    got = sc.local_search(np.zeros((3, 4), np.float32), [0.0, 0.0, 0.0], 5.0)
    assert got["match_id"] == -1 and got["n_examined"] == 0 and len(got["ids"]) == 0 and got["score"] == 1.0
    sc.add_frames(G.local_bank(9)[0])
    with pytest.raises(capi.LioError):
        sc.local_search(np.zeros((3, 4), np.float32), [0.0, 0.0, 0.0], 5.0)


def test_an_ins_position_or_precision_that_is_not_finite_is_refused(sc):
    clouds, pos = _bank(sc, 9)
    for xyz, precision in (([np.nan, 0.0, 0.0], 5.0), ([0.0, np.inf, 0.0], 5.0), ([0.0, 0.0, 0.0], np.nan), ([0.0, 0.0, 0.0], np.inf)):
        with pytest.raises(capi.LioError):
            sc.local_search(clouds[0], xyz, precision)
    assert sc.local_search(clouds[0], [0.0, 0.0, np.nan], 5.0)["match_id"] >= 0  # the height is not read
