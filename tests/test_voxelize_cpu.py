"""The detection front end without a GPU: the numpy restatement of tests/voxelize_cases.py against what the reference's own
preprocess_kernel.cu and voxelization_kernel.cu recorded in tests/golden/voxelize.npz (every comparison an equality: the serial order is
deterministic and the arithmetic IEEE without contraction), the three stated deviations against voxelize_deviations.npz, the host-only grid
size, the error contract of the lio_voxelizer_* entries and lsd_amd.voxelize's argument handling over a stub of the device call."""
import ctypes as C

import numpy as np
import pytest

import voxelize_cases as vc

F = np.float32


@pytest.fixture(scope="module")
def G():
    return vc.load(vc.GOLDEN)


@pytest.fixture(scope="module")
def D():
    return vc.load(vc.GOLDEN_DEV)


def recorded(g, name, k):
    what = vc.WHAT + (("window",) if f"{name}/{k}/window" in g else ())
    return {w: g[f"{name}/{k}/{w}"] for w in what}


@pytest.mark.parametrize("name", sorted(vc.CASES))
def test_restatement_equals_the_recorded_reference(G, name):
    p, calls = vc.CASES[name]
    assert int(G[f"{name}/calls"]) == len(calls)
    assert np.array_equal(G[f"{name}/params_f"], np.concatenate([p["min"], p["max"], p["size"]]))
    assert list(G[f"{name}/params_i"]) == [p["max_voxels"], p["P"], p["max_points"], p["frames"], p["order"]]
    assert list(G[f"{name}/grid"]) == vc.grid_size(p["min"], p["max"], p["size"])
    for k, r in enumerate(vc.run_case(vc.CASES[name])):
        if f"{name}/{k}/in" in G:  # the builders still make what was recorded
            assert np.array_equal(G[f"{name}/{k}/in"].view(np.uint32), np.asarray(calls[k][0], F).view(np.uint32))
        want = recorded(G, name, k)
        assert vc.check_call(r, want, tuple(want)) == [], f"call {k}"
        assert (want["counts"] >= 1).all()  # no voxel without a point outside the deviation file


def test_the_golden_holds_every_case(G, D):
    assert {k.split("/")[0] for k in G} == set(vc.CASES) and {k.split("/")[0] for k in D} == set(vc.DEVIATIONS)


def test_cases_are_what_they_are_called(G):
    r = {name: vc.run_case(vc.CASES[name]) for name in ("slots_p", "slots_p1", "slots_4096", "slots_4096_rev", "ids_a", "ids_b", "cap_eq", "cap_less",
                                                         "cap_one", "f16", "window_300", "window_400", "window_full")}
    assert 5 in r["slots_p"][0]["counts"] and r["slots_p"][0]["kept"] == r["slots_p"][0]["in_range"]
    assert r["slots_p1"][0]["kept"] == r["slots_p1"][0]["in_range"] - 1  # exactly one point lost to a full voxel
    a, b = r["slots_4096"][0], r["slots_4096_rev"][0]
    assert list(a["slots"][0]) == [0, 1, 2, 3, 4] and list(b["slots"][0]) == [0, 1, 2, 3, 4] and a["real"] == 1
    assert not np.array_equal(a["features"], b["features"])  # the reversed rows keep the other end
    assert r["ids_a"][0]["real"] == 256 and (r["ids_a"][0]["counts"] == 1).all()
    assert not np.array_equal(r["ids_a"][0]["indices"], r["ids_b"][0]["indices"])
    assert sorted(map(tuple, r["ids_a"][0]["indices"])) == sorted(map(tuple, r["ids_b"][0]["indices"]))
    assert [r[k][0]["real"] for k in ("cap_eq", "cap_less", "cap_one")] == [12, 12, 12]
    assert [r[k][0]["num"] for k in ("cap_eq", "cap_less", "cap_one")] == [12, 11, 1]
    assert r["cap_less"][0]["kept"] == r["cap_eq"][0]["kept"] - 3  # the dropped voxel's three points appear nowhere
    f = r["f16"][0]["features"].view(np.float16)
    assert 0 < f[0, 3] < 6.2e-5 and f[1, 3] == 2048 and f[2, 3] == 2052 and np.isinf(f[3, 3]) and np.isinf(f[3, 4]) and f[4, 3] == 65504
    assert r["f16"][0]["features"][4, 4] == 0x8000 and r["f16"][0]["features"][5, 3] == 1 and r["f16"][0]["features"][5, 4] == 0
    assert [list(c["window_counts"]) for c in r["window_300"]] == [[300, 0, 0], [300, 300, 0]] + [[300, 300, 300]] * 3
    assert [list(c["window_counts"]) for c in r["window_400"]][2:4] == [[200, 400, 400], [400, 200, 400]]
    assert [list(c["window_counts"]) for c in r["window_full"]][2] == [1, 500, 500]  # a call into a full window stores one point
    assert [len(c["window"]) for c in r["window_full"]] == [500, 1000, 1001, 801, 601]


def test_channel_4_takes_the_double_rule_once_per_sweep(G):
    calls = vc.CASES["window_identity"][1]
    last = G["window_identity/3/window"]
    assert list(G["window_identity/3/window_counts"]) == [100, 100, 100]
    for age, k in ((1, 2), (2, 1)):
        t = np.asarray(calls[k][0], F)[:, 4]
        for _ in range(age):
            t = (t.astype(np.float64) + 0.1).astype(F)
        rows = last[100 * age:100 * (age + 1)]
        assert np.array_equal(rows[:, 4], t)
        assert np.array_equal(rows[:, :4].view(np.uint32), np.asarray(calls[k][0], F)[:, :4].view(np.uint32))  # identity: x y z bit for bit


def test_deviation_grid_only_voxel(D):
    """the reference creates a voxel for a point that passes the grid test alone: one voxel more, count 0; here it does not exist"""
    r = vc.run_case(vc.DEVIATIONS["grid_only"])[0]
    assert int(D["grid_only/0/num"]) == 3 and list(D["grid_only/0/counts"]) == [1, 0, 1]
    assert r["num"] == 2 and list(r["counts"]) == [1, 1]
    assert np.array_equal(r["features"], D["grid_only/0/features"][[0, 2]]) and np.array_equal(r["indices"], D["grid_only/0/indices"][[0, 2]])
    assert list(D["grid_only/grid"]) == [10, 2, 2]


def test_deviation_nonfinite_points(D):
    """undefined in the reference (its host build happened to drop them too); dropped here before both passes"""
    r = vc.run_case(vc.DEVIATIONS["nonfinite"])[0]
    assert r["num"] == 2 and r["in_range"] == 4 and list(r["counts"]) == [1, 3]
    assert vc.check_call(r, {w: D[f"nonfinite/0/{w}"] for w in vc.WHAT}, vc.WHAT) == []
    assert np.isnan(r["features"].view(np.float16)[0, 3])  # a NaN intensity of a good point is data


def test_deviation_stale_counts(D):
    """a non-realtime call keeps the older sweeps' counts in the reference; here they are zeroed"""
    r = vc.run_case(vc.DEVIATIONS["stale_counts"])
    assert list(D["stale_counts/2/window_counts"]) == [5, 10, 0] and list(r[2]["window_counts"]) == [5, 0, 0]
    assert list(D["stale_counts/3/window_counts"]) == [4, 5, 10] and list(r[3]["window_counts"]) == [4, 5, 0]
    for k in range(4):  # the rows and the voxels are the same up to here
        want = {w: D[f"stale_counts/{k}/{w}"] for w in ("features", "indices", "counts", "num", "real", "window")}
        assert vc.check_call(r[k], want, tuple(want)) == []


def _grid(L, mn, mx, sz):
    a = [np.asarray(v, F) for v in (mn, mx, sz)]
    out = np.zeros(3, np.int32)
    rc = L.lio_voxelize_grid_size(*[v.ctypes.data_as(C.POINTER(C.c_float)) for v in a], out.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, list(out)


def test_grid_size_equals_the_recorded_compute_grid_size(G):
    from lsd_amd import capi, lio

    L = capi.lib()
    assert L.lio_abi_version() >= 29
    for name, (p, _) in vc.CASES.items():
        assert _grid(L, p["min"], p["max"], p["size"]) == (0, list(G[f"{name}/grid"]))
    assert list(G["yaml/grid"]) == [1280, 1280, 40]  # (4 - (-2)) / 0.15 in f32
    assert lio.Voxelizer.grid_size((0, 0, -2), (1, 1, 4), (1, 1, 0.15)) == [1, 1, 40]
    assert _grid(L, (0, 0, 0), (2.5, 3.5, 0.96), (1, 1, 0.1)) == (0, [3, 4, 10])  # std::round: halves away from zero
    for mn, mx, sz in (((0, 0, 0), (1, 1, 1), (0, 1, 1)), ((0, 0, 0), (1, 1, 1), (1, -1, 1)), ((0, 0, 0), (1, 0, 1), (1, 1, 1)),
                       ((0, 0, 0), (1, 1, np.nan), (1, 1, 1)), ((0, 0, 0), (1, 1, 1), (1, 1, 1e-12))):
        assert _grid(L, mn, mx, sz)[0] == capi.LIO_E_INVALID


def test_params_layout_matches_the_header():
    from lsd_amd import capi

    assert C.sizeof(capi.VoxelizerParams) == 56
    assert [getattr(capi.VoxelizerParams, f).offset for f in ("min_range", "max_range", "voxel_size", "max_voxels", "max_points_per_voxel", "max_points",
                                                              "max_frame_num", "order")] == [0, 12, 24, 36, 40, 44, 48, 52]


def _params(**kw):
    from lsd_amd import capi

    d = dict(min_range=(0, 0, 0), max_range=(8, 8, 4), voxel_size=(1, 1, 1), max_voxels=300, max_points_per_voxel=5, max_points=1000, max_frame_num=1, order=2)
    d.update(kw)
    p = capi.VoxelizerParams()
    for k, v in d.items():
        setattr(p, k, (C.c_float * 3)(*v) if isinstance(v, tuple) else v)
    return p


@pytest.mark.parametrize("bad,word", [(dict(voxel_size=(0, 1, 1)), b"voxel size"), (dict(voxel_size=(1, -1, 1)), b"voxel size"),
                                      (dict(max_range=(8, 0, 4)), b"max > min"), (dict(max_range=(8, 8, 0)), b"max > min"),
                                      (dict(min_range=(-1e6, -1e6, -1e6), max_range=(1e6, 1e6, 1e6), voxel_size=(0.5, 0.5, 0.5)), b"32-bit key"),
                                      (dict(max_range=(65536, 65536, 1), max_voxels=10), b"32-bit key"),
                                      (dict(max_points_per_voxel=0), b"max_points_per_voxel"), (dict(max_points_per_voxel=33), b"max_points_per_voxel"),
                                      (dict(order=0), b"order"), (dict(order=3), b"order"), (dict(max_frame_num=0), b"max_frame_num"),
                                      (dict(max_points=0), b"max_points"), (dict(max_voxels=0), b"max_voxels")])
def test_create_refuses_bad_params(bad, word):
    from lsd_amd import capi

    L = capi.lib()
    assert not L.lio_voxelizer_create(0, C.byref(_params(**bad)))
    assert word in L.lio_last_error()


def test_null_handles_and_no_device():
    from lsd_amd import capi, lio

    L = capi.lib()
    assert not L.lio_voxelizer_create(0, None)
    assert not L.lio_voxelizer_create(-1, C.byref(_params()))
    assert b"no HIP device" in L.lio_last_error()
    a = np.zeros((2, 5), F)
    fp = a.ctypes.data_as(C.POINTER(C.c_float))
    assert L.lio_voxelizer_forward(None, fp, 2, fp, 1) == capi.LIO_E_INVALID
    assert L.lio_voxelizer_forward_device(None, None, 2, fp, 1) == capi.LIO_E_INVALID
    assert L.lio_voxelizer_reset(None) == capi.LIO_E_INVALID
    assert L.lio_voxelizer_output(None, None, None, None, 0) == capi.LIO_E_INVALID
    assert L.lio_voxelizer_output_device(None, None, None) == capi.LIO_E_INVALID
    assert L.lio_voxelizer_window(None, None, 0) == capi.LIO_E_INVALID
    assert L.lio_voxelizer_window_counts(None, None, 0) == capi.LIO_E_INVALID
    assert L.lio_voxelizer_window_device(None, None) == capi.LIO_E_INVALID
    assert L.lio_voxelizer_last_counts(None, None, None, None) == capi.LIO_E_INVALID
    assert L.lio_voxelizer_last_times(None, None, None, None, None, None, None) == capi.LIO_E_INVALID
    L.lio_voxelizer_destroy(None)
    if L.lio_device_count() > 0:
        lio.Voxelizer((0, 0, 0), (8, 8, 4), (1, 1, 1), 10, max_points=100).close()
        return
    with pytest.raises(capi.LioError, match="no HIP device"):  # there is no CPU fallback
        lio.Voxelizer((0, 0, 0), (8, 8, 4), (1, 1, 1), 10)


class _StubVoxelizer:
    """lio.Voxelizer answered by the restatement"""

    made = []

    def __init__(self, **kw):
        self.kw = kw
        self.p = vc.params(mn=kw["min_range"], mx=kw["max_range"], size=kw["voxel_size"], max_voxels=kw["max_voxels"], P=kw["max_points_per_voxel"],
                           max_points=kw["max_points"], frames=kw["max_frame_num"], order=kw["order"])
        self.w = vc.Window(kw["max_points"], kw["max_frame_num"])
        self.calls, self.closed = [], False
        _StubVoxelizer.made.append(self)

    def forward(self, points, motion=None, realtime=True):
        assert points.dtype == np.float32 and points.flags.c_contiguous and motion.dtype == np.float32 and motion.shape == (4, 4)
        self.calls.append((len(points), bool(realtime)))
        self.r = vc.voxelize(self.w.forward(points, motion, realtime), self.p)
        return len(self.r["counts"])

    def output(self):
        return self.r["features"].view(np.float16), self.r["indices"], self.r["counts"]

    def reset(self):
        self.w.reset()

    def close(self):
        self.closed = True


def test_voxelize_module_over_a_stub(monkeypatch):
    from lsd_amd import voxelize

    monkeypatch.setattr(voxelize, "_make", lambda **kw: _StubVoxelizer(**kw))
    monkeypatch.setattr(voxelize, "_engine", None)
    _StubVoxelizer.made.clear()
    assert voxelize.voxelize_reset() == -1
    with pytest.raises(RuntimeError):
        voxelize.voxelize_forward(np.zeros((1, 5)), np.eye(4), True)
    # inference_init's names: max_points is per voxel, max_points_use the window's
    voxelize.voxelize_init(voxel_size=[1, 1, 1], coors_range=np.array([0, 0, 0, 8, 8, 4], np.float32), max_points=5, max_voxels=300, max_points_use=1000,
                           frame_num=2)
    e = _StubVoxelizer.made[-1]
    assert e.kw["max_points_per_voxel"] == 5 and e.kw["max_points"] == 1000 and e.kw["max_frame_num"] == 2 and e.kw["order"] == vc.ZYX
    assert list(e.kw["min_range"]) == [0, 0, 0] and list(e.kw["max_range"]) == [8, 8, 4]
    # what ObjectInfer.process hands over: float64 rows (a concatenate with a float64 zero column), a float32 motion
    rows = vc.sweep(50, 1)
    pts64 = np.concatenate((rows[:, :4], np.zeros((50, 1))), axis=1)
    assert pts64.dtype == np.float64
    feat, idx = voxelize.voxelize_forward(pts64, np.eye(4), True)
    want = vc.voxelize(pts64.astype(F), e.p)
    assert feat.dtype == np.float16 and idx.dtype == np.int32 and feat.shape == (len(want["counts"]), 5)
    assert np.array_equal(feat.view(np.uint16), want["features"]) and np.array_equal(idx, want["indices"])
    voxelize.voxelize_forward(rows.tolist(), np.eye(4).tolist(), False)  # lists, and a non-realtime call
    assert e.calls == [(50, True), (50, False)]
    for bad in (np.zeros((3, 4)), np.zeros(5), np.zeros((0, 5))):
        with pytest.raises(ValueError):
            voxelize.voxelize_forward(bad, np.eye(4), True)
    with pytest.raises(ValueError):
        voxelize.voxelize_forward(rows, np.eye(3), True)
    assert voxelize.voxelize_reset() == 0 and len(e.w.rows) == 0
    with pytest.raises(ValueError):
        voxelize.voxelize_init([1, 1], [0, 0, 0, 8, 8, 4], 5, 300, 1000, 2)
    voxelize.voxelize_init([1, 1, 1], [0, 0, 0, 8, 8, 4], 5, 300, 1000, 1)  # a second init closes the first engine
    assert e.closed and _StubVoxelizer.made[-1] is not e
