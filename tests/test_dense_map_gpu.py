"""Dense-map export on the device (csrc/cloud.hip, lio_cloud_*; slam_wrapper's accumulate_cloud / save_accumulate_cloud /
save_undistortion_cloud / set_export_map_config / export_points / dump_map_points, graph_utils.cpp:160-200 and 384-446).

The whole-cloud VoxelGrid is held bit for bit to the CPU oracle (oracle.voxel_downsample) and to the per-scan chain; the append to a numpy
restatement of pcl::transformPointCloud(Matrix4d) + the intensity factor + the inclusive z band + the input order; the module's functions to
compositions of the pieces they are made of."""
import os

import numpy as np
import pytest

from voxelgrid_cases import cases

pytestmark = pytest.mark.gpu


def _need_gpu():
    from lsd_amd import capi

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")


def _module():
    import slam_wrapper

    assert slam_wrapper.__file__.endswith(".so")
    return slam_wrapper


def _same(a, b):
    """bit for bit, except that a NaN is a NaN whatever its payload (both sides' NaNs must sit in the same places)"""
    a, b = np.array(a, np.float32), np.array(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    a[np.isnan(a)] = 0
    b[np.isnan(b)] = 0
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _read_pcd(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"DATA binary\n", 1)
    h = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1] for ln in head.decode().splitlines() if ln and not ln.startswith("#")}
    assert h["FIELDS"] == "x y z intensity" and h["SIZE"] == "4 4 4 4" and h["TYPE"] == "F F F F"
    n = int(h["POINTS"])
    assert int(h["WIDTH"]) == n and len(body) == 16 * n
    return np.frombuffer(body, np.float32).reshape(n, 4).copy()


def _xform_restated(pts, T, scale=1.0, band=None):
    """pcl::transformPointCloud(in, out, Matrix4d) as PCL 1.9.1 evaluates it (f64, terms left to right, cast to f32), the intensity times the
    factor in f32 (when it is not 1), then the inclusive band on z compared in f64, in input order"""
    from lsd_amd import lio

    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    out = lio.transform_cloud_f64(p, T)
    if scale != 1.0:
        out[:, 3] = (p[:, 3] * np.float32(scale)).astype(np.float32)
    if band is not None:
        z = out[:, 2].astype(np.float64)
        out = out[(z >= band[0]) & (z <= band[1])]
    return out


def _pose(rng, yaw_deg, t):
    from lsd_amd import synth

    q = synth.quat_from_rotvec(np.deg2rad([rng.uniform(-2, 2), rng.uniform(-2, 2), yaw_deg]))  # (x, y, z, w)
    T = np.eye(4)
    x, y, z, w = q
    T[:3, :3] = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                          [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    T[:3, 3] = t
    return T, q


# ---- 1. the voxel grid --------------------------------------------------------------------------------------------------------------------
def test_cloud_voxel_grid_matches_the_oracle_and_the_scan_chain(oracle_mod):
    """every case of tests/voxelgrid_cases.py (NaN / inf skipped, the int32 guard returning the input): bit for bit the oracle, and the per-scan
    chain (lio_scan_voxel_downsample) on the same cloud"""
    _need_gpu()
    from lsd_amd import lio

    c = lio.Cloud()
    sc = lio.Scan(max_raw=1 << 18, max_ds=1 << 18)
    for name, (pts, leaf, _dense) in cases().items():
        c.clear()
        c.append_host(pts)
        assert c.size == len(pts)
        assert c.scratch_bytes() >= 32 * len(pts)  # keys, values (ping-pong) and the sorted copy
        n = c.voxel_downsample(leaf)
        got = c.download()
        ref = oracle_mod.voxel_downsample(pts, leaf)
        assert n == len(ref) and _same(got, ref), name
        sc.upload(pts)
        m = sc.voxel_downsample(leaf)
        assert m == n and _same(sc.get_ds(), got), name
    c.clear()
    assert c.voxel_downsample(0.5) == 0 and c.size == 0
    c.append_host(np.full((5, 4), np.nan, np.float32))
    assert c.voxel_downsample(0.5) == 0  # no finite point: nothing left, as the oracle
    c.close()
    sc.close()


def test_cloud_voxel_grid_four_radix_passes_on_2e7_points(oracle_mod):
    """2*10^7 points over 400 m x 400 m x 12 m at 0.1 m: 1.9*10^9 cells (keys of 31 bits, all four radix passes), appended in three pieces"""
    _need_gpu()
    from lsd_amd import lio

    rng = np.random.default_rng(7)
    n = 20_000_000
    p = np.empty((n, 4), np.float32)
    p[:, 0] = rng.uniform(-200, 200, n)
    p[:, 1] = rng.uniform(-200, 200, n)
    p[:, 2] = rng.uniform(-2, 10, n)
    p[:, 3] = rng.uniform(0, 255, n)
    p[: n // 2, :3] = np.round(p[: n // 2, :3] * 4) / 4  # half of the points on a coarse lattice: many shared voxels, runs of several points
    p[rng.integers(0, n, 1000), 2] = np.nan
    c = lio.Cloud(reserve=1 << 20)  # grows on the way
    for a, b in ((0, 5_000_000), (5_000_000, 12_000_000), (12_000_000, n)):
        c.append_host(p[a:b])
    assert c.size == n
    m = c.voxel_downsample(0.1)
    got = c.download()
    ref = oracle_mod.voxel_downsample(p, 0.1)
    assert m == len(ref) and _same(got, ref)
    c.close()


def test_cloud_voxel_grid_with_a_voxel_of_120000_points(oracle_mod):
    """a "monster" voxel (>= 10^5 points) beside long and short runs: the sequential f32 sum in ascending input index, bit for bit"""
    _need_gpu()
    from lsd_amd import lio

    rng = np.random.default_rng(11)
    big = np.concatenate([rng.uniform(0.0, 0.5, (120_000, 3)) + [10.0, 20.0, 1.0], rng.uniform(0, 255, (120_000, 1))], 1)
    mid = np.concatenate([rng.uniform(0.0, 0.5, (3_000, 3)) + [30.0, 20.0, 1.0], rng.uniform(0, 255, (3_000, 1))], 1)
    rest = np.concatenate([rng.uniform(-50, 50, (200_000, 3)), rng.uniform(0, 255, (200_000, 1))], 1)
    p = np.concatenate([big, rest, mid]).astype(np.float32)
    p = p[rng.permutation(len(p))]
    c = lio.Cloud()
    c.append_host(p)
    m = c.voxel_downsample(0.5)
    ref = oracle_mod.voxel_downsample(p, 0.5)
    assert m == len(ref) and _same(c.download(), ref)
    c.close()


# ---- 2. the append ------------------------------------------------------------------------------------------------------------------------
def test_append_matches_the_numpy_restatement():
    """host and scan inputs: f64 transform, x255, inclusive z band (points exactly on z_min / z_max kept, NaN z dropped), input order"""
    _need_gpu()
    from lsd_amd import lio

    rng = np.random.default_rng(3)
    T, _ = _pose(rng, 37.0, [12.5, -3.25, 0.7])
    band = (-0.5, 2.0)
    frames = []
    for k in range(3):
        p = np.concatenate([rng.normal(0, 20, (50_000 + 7 * k, 3)) * [1, 1, 0.2], rng.uniform(0, 1, (50_000 + 7 * k, 1))], 1).astype(np.float32)
        p[rng.integers(0, len(p), 50), 2] = np.nan
        frames.append(p)
    # points that land exactly on the band's ends after the transform: an identity transform keeps z as it is
    edge = np.array([[1, 2, -0.5, 3], [1, 2, 2.0, 3], [1, 2, np.nextafter(np.float32(2.0), np.float32(3)), 3], [1, 2, -0.5000001, 3]], np.float32)
    c = lio.Cloud()
    want = []
    for p in frames:
        c.append_host(p, T, 255.0, band)
        want.append(_xform_restated(p, T, 255.0, band))
    c.append_host(edge, np.eye(4), 255.0, band)
    want.append(_xform_restated(edge, np.eye(4), 255.0, band))
    assert len(want[-1]) == 2
    got = c.download()
    assert _same(got, np.concatenate(want))
    # no band, factor 1: every point (NaN ones too) transformed, intensity as given
    c.clear()
    c.append_host(frames[0], T)
    assert _same(c.download(), _xform_restated(frames[0], T))
    # a scan's raw cloud
    sc = lio.Scan(max_raw=1 << 17, max_ds=1 << 10)
    c.clear()
    for p in frames:
        sc.upload(p)
        c.append_scan(sc, T, 255.0, band)
    c.append_scan(sc, T)
    assert _same(c.download(), np.concatenate(want[:3] + [_xform_restated(frames[-1], T)]))
    sc.close()
    c.close()


# ---- 3. accumulate_cloud -> save_accumulate_cloud -----------------------------------------------------------------------------------------
def _drive(n_frames=4, seed=5):
    """frames of a synthetic drive: points, points_attr {points_attr: N x 2 (stamp us, id), timestamp}, TUM rows (5 poses per frame)"""
    from lsd_amd import synth

    rng = np.random.default_rng(seed)
    sc = synth.Scene(half=60.0, n_boxes=20, seed=seed)
    out = []
    for f in range(n_frames):
        raw, _ = synth.make_scan(sc, np.array([1.0 * f, 0.5, 1.8]), synth.quat_from_rotvec([0, 0, 0.05 * f]), seed=seed + f, n_az=300)
        pts = raw[:, :4].astype(np.float32)
        n = len(pts)
        stamps = np.sort(rng.integers(0, 100_000, n)).astype(np.float32)
        attr = np.stack([stamps, np.zeros(n, np.float32)], 1)
        header = 1_700_000_000_000_000 + 100_000 * f
        rows = []
        for k in range(5):
            T, q = _pose(rng, 3.0 * f + 0.4 * k, [1.0 * f + 0.025 * k, 0.5 + 0.01 * k, 0.02 * k])
            rows.append([header + 25_000 * k, T[0, 3], T[1, 3], T[2, 3], q[0], q[1], q[2], q[3]])
        out.append((pts, {"points_attr": attr, "timestamp": header}, np.array(rows, np.float64)))
    return out


def _composed(sw, frame, oracle_mod=None):
    """one frame as the test composes it: lio.Scan.undistort_poses with the module's relative poses, then T0 (f64 transform)"""
    from lsd_amd import lio

    pts, pa, rows = frame
    T0, rel = sw._tum_relative_poses(rows)
    st = pa["points_attr"][:, 0].astype(np.uint32)
    ps = rows[:, 0].astype(np.uint64)
    Ts = np.stack([np.asarray(r) for r in rel]).reshape(-1, 16)
    sc = lio.Scan(max_raw=1 << 18, max_ds=1 << 10)
    sc.upload(pts)
    sc.undistort_poses(st, pa["timestamp"], ps, Ts)
    und = sc.download_raw()
    sc.close()
    if oracle_mod is not None:  # the undistortion itself against the oracle, with test_hip_undistort_poses' tolerance
        ref = oracle_mod.undistort_poses(pts, st, pa["timestamp"], ps, Ts)
        d = np.abs(und[:, :3] - ref[:, :3])
        scale = np.maximum(np.abs(ref[:, :3]).max(axis=1, keepdims=True), 1e-3)
        assert (d / (scale * 2.0 ** -23)).max() <= 8.0 and (d > 0).mean() < 1e-2
        assert (np.abs(und[:, :3] - pts[:, :3]).max(1) > 0).mean() > 0.3  # the walk moved most points
    return und, np.asarray(T0)


def test_accumulate_then_save_equals_the_oracle_on_the_composition(oracle_mod, tmp_path):
    _need_gpu()
    sw = _module()
    drive = _drive()
    parts = []
    for fr in drive:
        sw.accumulate_cloud(fr[0], fr[1], fr[2], "TUM", False)
        und, T0 = _composed(sw, fr, oracle_mod)
        parts.append(_xform_restated(und, T0))
    whole = np.concatenate(parts)
    f1 = tmp_path / "dense_map_0.2.pcd"
    sw.save_accumulate_cloud(str(f1), 0.2)
    got = _read_pcd(f1)
    ref = oracle_mod.voxel_downsample(whole, 0.2)
    assert len(ref) > 1000 and _same(got, ref)
    # the cloud was cleared: a second save writes nothing
    f2 = tmp_path / "again.pcd"
    sw.save_accumulate_cloud(str(f2), 0.2)
    assert not f2.exists()
    # resolution 0: no filter, the accumulated cloud as it is
    for fr in drive[:2]:
        sw.accumulate_cloud(fr[0], fr[1], fr[2], "TUM", False)
    f3 = tmp_path / "raw.pcd"
    sw.save_accumulate_cloud(str(f3), 0.0)
    assert _same(_read_pcd(f3), np.concatenate(parts[:2]))


# ---- 4. the map-export sequence -----------------------------------------------------------------------------------------------------------
def test_export_points_then_dump_map_points(tmp_path):
    _need_gpu()
    sw = _module()
    rng = np.random.default_rng(9)
    frames = []
    for k in range(4):
        p = np.concatenate([rng.normal(0, 15, (20_000, 3)) * [1, 1, 0.3], rng.uniform(0, 1, (20_000, 1))], 1).astype(np.float32)
        T, _ = _pose(rng, 20.0 * k, [3.0 * k, -1.0, 0.5])
        frames.append((p, T.astype(np.float32)))
    band = (-1.0, 3.0)
    sw.set_export_map_config(band[0], band[1], "height")
    for p, T in frames:
        sw.export_points(p, T)
    f = tmp_path / "export_map.pcd"
    sw.dump_map_points(str(f))
    want = np.concatenate([_xform_restated(p, T.astype(np.float64), 255.0, band) for p, T in frames])
    assert len(want) > 10_000 and _same(_read_pcd(f), want)
    # set_export_map_config resets the key frames
    sw.set_export_map_config(0.0, 1.0, "height")
    sw.export_points(*frames[0])
    f.unlink()
    sw.dump_map_points(str(f))
    assert _same(_read_pcd(f), _xform_restated(frames[0][0], frames[0][1].astype(np.float64), 255.0, (0.0, 1.0)))
    # "rgb": the colour map is out of scope and empty -- no file
    sw.set_export_map_config(-1.0, 3.0, "rgb")
    sw.export_points(*frames[1])
    g = tmp_path / "rgb.pcd"
    sw.dump_map_points(str(g))
    assert not g.exists()
    # nothing exported: no file, as the reference
    sw.set_export_map_config(-1.0, 3.0, "height")
    sw.dump_map_points(str(g))
    assert not g.exists()


# ---- 5. save_undistortion_cloud -----------------------------------------------------------------------------------------------------------
def test_save_undistortion_cloud_equals_the_scan_undistortion(tmp_path):
    _need_gpu()
    sw = _module()
    fr = _drive(n_frames=1, seed=13)[0]
    f = tmp_path / "undistorted.pcd"
    sw.save_undistortion_cloud(str(f), fr[0], fr[1], fr[2])
    und, _ = _composed(sw, fr)
    assert _same(_read_pcd(f), und)


# ---- 6. refused inputs --------------------------------------------------------------------------------------------------------------------
def test_inputs_the_module_refuses_raise():
    _need_gpu()
    sw = _module()
    pts, pa, rows = _drive(n_frames=1, seed=17)[0]
    with pytest.raises(ValueError, match="extract_ground"):
        sw.accumulate_cloud(pts, pa, rows, "TUM", True)
    with pytest.raises(ValueError, match="KITTI"):
        sw.accumulate_cloud(pts, pa, rows, "KITTI", False)
    many = np.repeat(rows[:1], 65, 0)
    many[:, 0] += np.arange(65) * 1000
    with pytest.raises(ValueError, match="64 poses"):
        sw.accumulate_cloud(pts, pa, many, "TUM", False)
    with pytest.raises(ValueError, match="64 poses"):
        sw.save_undistortion_cloud(os.devnull, pts, pa, many)
    back = rows.copy()
    back[3, 0] = back[1, 0] - 1  # an interval that ends before its predecessor's
    with pytest.raises(ValueError, match="predecessors"):
        sw.accumulate_cloud(pts, pa, back, "TUM", False)
    with pytest.raises(ValueError, match="no poses"):
        sw.accumulate_cloud(pts, pa, rows[:0], "TUM", False)
