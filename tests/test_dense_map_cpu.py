"""Dense-map export, the parts that need no GPU: the module's TUM pose conversion and relative poses (numpy_to_odometry, py_utils.cpp:260-270;
undistortion_cloud, graph_utils.cpp:391-393), lio.Cloud's refusal without a device, export_points deferring its work to dump_map_points."""
import numpy as np
import pytest


def _module():
    import slam_wrapper

    assert slam_wrapper.__file__.endswith(".so")
    return slam_wrapper


def _rot(q):  # (x, y, z, w) -> R, as Eigen's Quaternion::toRotationMatrix writes it
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_tum_relative_poses_against_numpy():
    sw = _module()
    rng = np.random.default_rng(1)
    rows = []
    for k in range(6):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        rows.append([1_000_000 + 10_000 * k, *rng.uniform(-50, 50, 3), *q])  # stamp, x y z, qx qy qz qw
    rows = np.array(rows)
    T0, rel = sw._tum_relative_poses(rows)
    Ts = []
    for r in rows:
        T = np.eye(4)
        T[:3, :3] = _rot(r[4:8])  # columns 4, 5, 6 = x, y, z; column 7 = w
        T[:3, 3] = r[1:4]
        Ts.append(T)
    assert np.allclose(np.asarray(T0), Ts[0], rtol=0, atol=1e-15)
    assert len(rel) == len(rows)
    inv0 = np.linalg.inv(Ts[0])
    for R, T in zip(rel, Ts):
        assert np.allclose(np.asarray(R), inv0 @ T, rtol=0, atol=1e-12)
    E = np.asarray(rel[0]) - np.eye(4)  # T0^-1 * T0: identity to 1e-15 (the translation column relative to |t0|)
    assert np.abs(E[:, :3]).max() <= 1e-15 and np.abs(E[:, 3]).max() <= 1e-15 * np.abs(rows[0, 1:4]).max()
    # the column order matters: w taken from column 7, not column 4
    swapped = rows.copy()
    swapped[:, [4, 7]] = swapped[:, [7, 4]]
    assert not np.allclose(np.asarray(sw._tum_relative_poses(swapped)[0]), Ts[0])


def test_cloud_without_a_device_raises():
    from lsd_amd import capi, lio

    if capi.lib().lio_device_count() > 0:
        pytest.skip("a HIP device is visible: covered by tests/test_dense_map_gpu.py")
    with pytest.raises(capi.LioError):
        lio.Cloud()


def test_export_points_needs_no_device():
    sw = _module()
    rng = np.random.default_rng(2)
    sw.set_export_map_config(-1.0, 3.0, "height")
    for k in range(3):
        T = np.eye(4, dtype=np.float32)
        T[0, 3] = k
        sw.export_points(rng.normal(size=(100, 4)).astype(np.float32), T)
    sw.set_export_map_config(-1.0, 3.0, "height")  # (drop them again)


def test_refused_inputs_raise_before_any_device_work():
    sw = _module()
    pts = np.zeros((10, 4), np.float32)
    pa = {"points_attr": np.zeros((10, 2), np.float32), "timestamp": 0}
    rows = np.array([[0, 0, 0, 0, 0, 0, 0, 1.0], [1000, 0, 0, 0, 0, 0, 0, 1.0]])
    with pytest.raises(ValueError, match="extract_ground"):
        sw.accumulate_cloud(pts, pa, rows, "TUM", True)
    with pytest.raises(ValueError, match="KITTI"):
        sw.accumulate_cloud(pts, pa, rows, "KITTI", False)
