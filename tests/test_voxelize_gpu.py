"""The detection front end on the device (csrc/voxelize.hip, lio.Voxelizer) against what the reference's own kernels recorded in
tests/golden/voxelize.npz and against the numpy restatement of tests/voxelize_cases.py.  Every comparison is an equality -- features as
uint16, indices, counts, the voxel number, the window's rows and counts: the device is pinned to the reference's kernels run one thread after
another in index order, and the arithmetic is IEEE f32 without contraction, so there is no tolerance to choose."""
import numpy as np
import pytest

import voxelize_cases as vc

pytestmark = pytest.mark.gpu
F = np.float32
ALL = dict(vc.CASES, **vc.DEVIATIONS)


@pytest.fixture(scope="module")
def G():
    return vc.load(vc.GOLDEN)


@pytest.fixture(scope="module")
def restated():
    """the restatement over every case, computed once and left alone"""
    return {name: vc.run_case(case) for name, case in ALL.items()}


@pytest.fixture(scope="module")
def lio_mod():
    from lsd_amd import capi, lio

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    return lio


def make(lio, p):
    return lio.Voxelizer(p["min"], p["max"], p["size"], p["max_voxels"], p["P"], p["max_points"], p["frames"], p["order"])


def snapshot(v):
    feat, idx, cnt = v.output()
    real, in_range, kept = v.last_counts()
    return dict(features=feat.view(np.uint16), indices=idx, counts=cnt, num=v.num_voxels, real=real, in_range=in_range, kept=kept, window=v.window(),
                window_counts=v.window_counts())


def run_device(lio, case, v=None):
    p, calls = case
    own = v is None
    v = make(lio, p) if own else v
    out = []
    for rows, motion, realtime in calls:
        v.forward(rows, motion, realtime)
        out.append(snapshot(v))
    if own:
        v.close()
    return out


EVERYTHING = vc.WHAT + ("window", "in_range", "kept")


@pytest.fixture(scope="module")
def device(lio_mod):
    """the device over every case, computed once"""
    return {name: run_device(lio_mod, case) for name, case in ALL.items()}


@pytest.mark.parametrize("name", sorted(ALL))
def test_device_equals_the_restatement(device, restated, name):
    for k, (got, want) in enumerate(zip(device[name], restated[name])):
        assert vc.check_call(got, want, EVERYTHING) == [], f"call {k}"


@pytest.mark.parametrize("name", sorted(vc.CASES))
def test_device_equals_the_recorded_reference(device, G, name):
    for k, got in enumerate(device[name]):
        what = vc.WHAT + (("window",) if f"{name}/{k}/window" in G else ())
        assert vc.check_call(got, {w: G[f"{name}/{k}/{w}"] for w in what}, what) == [], f"call {k}"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 4097])
def test_tile_edges_of_the_compaction(device, restated, n):
    got, want = device[f"tile_{n}"][0], restated[f"tile_{n}"][0]
    assert got["real"] == want["real"] and got["num"] == want["num"] and np.array_equal(got["indices"], want["indices"])
    assert got["in_range"] == want["in_range"] < n or n == 1


@pytest.mark.parametrize("name", ["slots_p", "slots_p1", "slots_4096"])
def test_a_voxel_keeps_its_first_points_in_window_order(device, name):
    """the mean of the crowded voxel is the mean of its first P rows in index order; the reversed rows keep the other end"""
    for case, rows in ((name, ALL[name][1][0][0]), (name + "_rev", ALL[name + "_rev"][1][0][0])):
        got = device[case][0]
        inside = np.flatnonzero((np.floor(rows[:, 0]) == 3) & (np.floor(rows[:, 1]) == 2) & (np.floor(rows[:, 2]) == 1))
        first = rows[inside[:5]]
        acc = first[0].copy()
        for r in first[1:]:
            acc = acc + r
        vox = int(np.flatnonzero((got["indices"] == (0, 1, 2, 3)).all(1))[0])
        assert got["counts"][vox] == 5
        assert np.array_equal(got["features"][vox], (acc / F(5)).astype(np.float16).view(np.uint16))
    assert not np.array_equal(device[name][0]["features"], device[name + "_rev"][0]["features"])


def test_ids_are_first_occurrence_ranks(device):
    for name in ("ids_a", "ids_b"):
        rows, got = ALL[name][1][0][0], device[name][0]
        assert got["num"] == 256 and (got["counts"] == 1).all()
        want = np.stack([np.zeros(256), np.floor(rows[:, 2]), np.floor(rows[:, 1]), np.floor(rows[:, 0])], 1).astype(np.int32)
        assert np.array_equal(got["indices"], want)  # voxel k is point k's
    assert not np.array_equal(device["ids_a"][0]["indices"], device["ids_b"][0]["indices"])


def test_cap_drops_whole_voxels_and_reports_the_real_number(device):
    eq, less, one = device["cap_eq"][0], device["cap_less"][0], device["cap_one"][0]
    assert (eq["num"], less["num"], one["num"]) == (12, 11, 1) and eq["real"] == less["real"] == one["real"] == 12
    assert np.array_equal(less["features"], eq["features"][:11]) and np.array_equal(less["indices"], eq["indices"][:11])
    assert np.array_equal(one["features"], eq["features"][:1]) and np.array_equal(one["counts"], eq["counts"][:1])
    assert less["kept"] == eq["kept"] - 3 and not (less["indices"] == (0, 3, 7, 7)).all(1).any()  # the dropped voxel's points appear nowhere
    assert eq["in_range"] == less["in_range"] == one["in_range"] == 90


def test_faces(device):
    got, rows = device["faces"][0], vc.face_rows()
    vox = {tuple(i[1:][::-1]) for i in got["indices"]}  # (x, y, z)
    assert (0, 0, 0) in vox and (7, 7, 3) in vox          # exactly at min; the largest floats below max
    assert (2, 1, 1) in vox and (3, 1, 1) in vox          # one ulp either side of an interior face
    assert (1, 4, 1) in vox and (1, 5, 1) in vox and (1, 1, 1) in vox and (1, 1, 2) in vox
    assert got["in_range"] == 13 and len(rows) == 26      # at max, outside on each of the six sides and far away: out
    nf = device["nonfinite"][0]
    assert nf["in_range"] == 4 and nf["num"] == 2         # NaN and +-inf in each coordinate are dropped


def test_yaml_geometry(device, restated):
    got = device["yaml"][0]
    assert got["indices"][:, 3].max() == 1279 and got["indices"][:, 2].max() == 1279 and got["indices"][:, 1].max() == 39
    assert got["indices"].min() == 0 and got["real"] == restated["yaml"][0]["real"] > 1500


def test_f16_rounding(device):
    f = device["f16"][0]["features"]
    h = f.view(np.float16)
    assert 0 < h[0, 3] < 6.2e-5 and f[0, 3] == np.float16(3e-6).view(np.uint16)  # subnormal kept
    assert h[1, 3] == 2048 and h[2, 3] == 2052                                   # halfway cases go to even
    assert np.isinf(h[3, 3]) and np.isinf(h[3, 4]) and h[4, 3] == 65504          # overflow to inf, and the last value that does not
    assert f[4, 4] == 0x8000 and f[5, 3] == 1 and f[5, 4] == 0                   # -0 kept; the smallest subnormal; below half of it


def test_orders(device):
    zyx, xyz = device["tile_65"][0], device["order_xyz"][0]
    assert np.array_equal(xyz["indices"], zyx["indices"][:, [0, 3, 2, 1]]) and np.array_equal(xyz["features"], zyx["features"])


def test_window_calls_clamp_pop_and_fill(device):
    assert [list(c["window_counts"]) for c in device["window_300"]] == [[300, 0, 0], [300, 300, 0]] + [[300, 300, 300]] * 3
    assert [list(c["window_counts"]) for c in device["window_400"]] == [[400, 0, 0], [400, 400, 0], [200, 400, 400], [400, 200, 400], [400, 400, 200]]
    assert [list(c["window_counts"]) for c in device["window_full"]][2] == [1, 500, 500]
    assert [len(c["window"]) for c in device["window_full"]] == [500, 1000, 1001, 801, 601]
    assert [list(c["window_counts"]) for c in device["window_mixed"]][:3] == [[200, 0, 0], [150, 0, 0], [120, 150, 0]]
    assert [list(c["window_counts"]) for c in device["stale_counts"]] == [[10, 0, 0], [10, 10, 0], [5, 0, 0], [4, 5, 0]]


def test_channel_4_after_k_sweeps_is_k_double_additions(device):
    calls, last = vc.CASES["window_identity"][1], device["window_identity"][3]["window"]
    for age, k in ((0, 3), (1, 2), (2, 1)):
        want = np.asarray(calls[k][0], F).copy()
        for _ in range(age):
            want[:, 4] = (want[:, 4].astype(np.float64) + 0.1).astype(F)
        assert np.array_equal(last[100 * age:100 * (age + 1)].view(np.uint32), want.view(np.uint32))  # identity motion: x y z bit for bit


def test_reset_and_repeated_calls_leave_no_state(lio_mod, device):
    case = vc.CASES["window_400"]
    v = make(lio_mod, case[0])
    first = run_device(lio_mod, case, v)
    v.reset()
    assert len(v.window()) == 0 and list(v.window_counts()) == [0, 0, 0] and v.num_voxels == 0
    second = run_device(lio_mod, case, v)
    for a, b, c in zip(first, second, device["window_400"]):
        assert vc.check_call(a, b, EVERYTHING) == [] and vc.check_call(a, c, EVERYTHING) == []
    # the same sweep, non-realtime, three times over whatever the tables held
    rows = vc.random_rows(700, 77)
    outs = []
    for _ in range(3):
        v.forward(rows, None, False)
        outs.append(snapshot(v))
    assert vc.check_call(outs[0], outs[1], EVERYTHING) == [] and vc.check_call(outs[0], outs[2], EVERYTHING) == []
    assert vc.check_call(outs[0], vc.run_case((case[0], [(rows, vc.EYE, False)]))[0], EVERYTHING) == []
    v.close()


def test_two_handles_with_different_params(lio_mod, device):
    a, b = make(lio_mod, vc.CASES["yaml"][0]), make(lio_mod, vc.CASES["p32"][0])
    ra, rb = vc.CASES["yaml"][1][0][0], vc.CASES["p32"][1][0][0]
    for _ in range(2):  # interleaved
        a.forward(ra, None, False)
        b.forward(rb, None, False)
        assert vc.check_call(snapshot(a), device["yaml"][0], EVERYTHING) == []
        assert vc.check_call(snapshot(b), device["p32"][0], EVERYTHING) == []
    a.close()
    b.close()


def test_forward_device_equals_forward(lio_mod, device):
    """the sweeps come from another handle's window in device memory: nothing is uploaded"""
    case = vc.CASES["window_300"]
    src = make(lio_mod, vc.params(max_points=1000))
    v = make(lio_mod, case[0])
    for k, (rows, motion, realtime) in enumerate(case[1]):
        src.forward(rows, None, False)
        addr, n = src.window_device()
        assert n == len(rows) and addr
        v.forward_device(addr, n, motion, realtime)
        assert vc.check_call(snapshot(v), device["window_300"][k], EVERYTHING) == [], f"call {k}"
    fa, ia, nv = v.output_device()
    assert fa and ia and nv == v.num_voxels
    src.close()
    v.close()


def test_forward_refuses_an_empty_sweep(lio_mod):
    from lsd_amd import capi

    v = make(lio_mod, vc.params(max_points=100))
    with pytest.raises(capi.LioError):
        v.forward(np.zeros((0, 5), F), None, True)
    v.forward(vc.random_rows(300, 5), None, True)  # the caller's n is clamped to max_points
    assert list(v.window_counts()) == [100] and len(v.window()) == 100
    v.close()


def test_last_times(lio_mod):
    v = make(lio_mod, vc.CASES["window_300"][0])
    for rows, motion, realtime in vc.CASES["window_300"][1][:2]:
        v.forward(rows, motion, realtime)
    t = v.last_times()
    assert len(t) == 6 and all(x > 0 for x in t) and sum(t[:5]) <= t[5] * 1.001 + 1.0 and t[5] < 1e6
    v.close()
