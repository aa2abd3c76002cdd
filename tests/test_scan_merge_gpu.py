"""lio_scan_merge (csrc/scanmerge.hip) against tests/rtk_cases.py's restatement of mergePoints + preprocessPoints: points and stamps bit for bit,
with the per-cloud kept / early / late counts.  The restatement itself is held to the reference's own mergePoints (tests/golden/rtk.npz)
on the CPU side of the comparison."""
import functools
import os

import numpy as np
import pytest

import rtk_cases as R
from lsd_amd import capi, lio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _merger():
    return lio.ScanMerge(max_clouds=16, max_points=1 << 16)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = R.merge_case(name)
    return c, R.merge_points(c["clouds"], c["stamps"], c["headers"], c["period"], c["T"])


def _run(c, m=None):
    m = m or _merger()
    m.set_transform(c["T"])
    n, kept, early, late = m.run(c["clouds"], c["stamps"], c["headers"], c["period"])
    pts, st = m.download()
    assert n == len(pts) == len(st)
    return pts, st, kept, early, late


def _same(got, want):
    pts, st, kept, early, late = got
    rp, rs, rk, re_, rl = want
    assert len(pts) == len(rp)
    assert np.array_equal(pts.view(np.uint32), rp.view(np.uint32)), int((pts.view(np.uint32) != rp.view(np.uint32)).any(axis=1).sum())
    assert np.array_equal(st, rs)
    assert np.array_equal(kept, rk) and np.array_equal(early, re_) and np.array_equal(late, rl)


@pytest.mark.parametrize("name", R.MERGE_CASES)
def test_merge_against_the_restatement(name):
    c, want = _case(name)
    _same(_run(c), want)


def test_the_cases_cover_what_they_claim():
    c, (_, _, kept, early, late) = _case("tiles")
    n = [len(p) for p in c["clouds"]]
    assert n == [300, 2047, 2048, 0, 2049, 4097, 1500] and max(c["headers"]) > 1 << 32
    assert kept[0] == 300 and kept[3] == 0 and kept[4] == 0 and late[4] == 2049 and kept[5] == 4097  # empty, wholly rejected, wholly kept
    assert early[2] > 0 and late[1] > 0 and 0 < kept[1] < 2047 and 0 < kept[2] < 2048  # a positive and a negative shift, both cutting
    c, (_, st, kept, early, late) = _case("edges")
    s1 = c["stamps"][1].astype(np.int64) - 5000
    s2 = c["stamps"][2].astype(np.int64) + 7000
    assert (s1 == 0).any() and (s1 == -1).any() and (s2 == c["period"]).any() and (s2 == c["period"] + 1).any()
    assert kept[1] == (s1 >= 0).sum() and early[1] == (s1 == -1).sum() + (s1 < -1).sum() and late[2] == (s2 > c["period"]).sum()
    assert (st[300:300 + kept[1]] == 0).sum() == (s1 == 0).sum() and (st[300 + kept[1]:] == c["period"]).sum() == (s2 == c["period"]).sum()
    c, (pts, st, kept, _, _) = _case("single")
    assert len(c["clouds"]) == 1 and kept[0] == len(pts) and (st > c["period"]).any()  # the base is ungated
    assert len(_case("sixteen")[0]["clouds"]) == 16
    assert np.abs(_case("tiles")[1][0][:, :2]).max() > 5e4 and abs(_case("tiles")[0]["T"][0, 3]) == 1e5  # the frame sits 1e5 m out
    c, (pts, _, _, _, _) = _case("nonfinite")
    raw = np.concatenate(c["clouds"])
    assert np.isnan(raw[:, :3]).any() and np.isinf(raw[:, :3]).any() and np.isnan(pts).any() and np.isinf(pts).any()


def test_two_runs_are_identical_and_the_handle_is_reusable():
    c, want = _case("tiles")
    a = _run(c)
    d, dwant = _case("sixteen")
    _same(_run(d), dwant)  # another shape in between
    b = _run(c)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    _same(b, want)
    up, merge = _merger().last_times()
    assert up >= 0 and merge > 0
    p, s, n = _merger().device_view()
    assert p and s and n == len(want[0])


def test_download_with_a_short_capacity_and_bad_arguments():
    c, want = _case("edges")
    m = _merger()
    _run(c, m)
    n = len(want[0])
    assert m.download(cap=n - 1) == -n and m.download(cap=0) == -n
    pts, st = m.download(cap=n + 5)
    assert len(pts) == n and np.array_equal(st, want[1])
    small = lio.ScanMerge(max_clouds=2, max_points=1000)
    with pytest.raises(capi.LioError):
        small.run(c["clouds"], c["stamps"], c["headers"], c["period"])          # three clouds
    with pytest.raises(capi.LioError):
        small.run(c["clouds"][1:], c["stamps"][1:], c["headers"][1:], c["period"])  # too many points
    with pytest.raises(capi.LioError):
        small.run(c["clouds"][:1], c["stamps"][:1], c["headers"][:1], 1 << 33)     # a period that does not fit a stamp
    n0, kept, _, _ = small.run([np.zeros((0, 4), np.float32)], [np.zeros(0, np.uint32)], [5], 100)  # an empty frame
    assert n0 == 0 and kept[0] == 0 and len(small.download()[0]) == 0
    with pytest.raises(capi.LioError):
        lio.ScanMerge(max_clouds=17)


@pytest.mark.parametrize("name", R.MERGE_CASES)
def test_the_restatement_against_the_reference(name):
    """the CPU side of the comparison: the restatement's mergePoints (before the transform) is the reference's own, bit for bit"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "rtk.npz"))
    c = R.merge_case(name, small=True)
    p, s, _, _, _ = R.merge_points(c["clouds"], c["stamps"], c["headers"], c["period"], transform=False)
    assert np.array_equal(p.view(np.uint32), g["merge_%s_points" % name].view(np.uint32)) and np.array_equal(s, g["merge_%s_stamps" % name])
    assert len(p) > 0
