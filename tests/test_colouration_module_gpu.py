"""The colour map through the compiled module (csrc/slam_wrapper.cpp).  Offline: set_colouration_config, set_map_odometrys, colouration_frame
and save_render_cloud end to end into a PCD, read back and compared with the numpy restatement (tests/render_cases.py) fed the frames the module
undistorted and the poses its get_stamp_pose gave.  Live: the localisation drive of tests/test_outer_boundary.py with synthetic images --
get_color_map() is empty until the localisation is stable and N x 4 after, dump_map_points("rgb") writes the z-filtered cloud."""
import os
import sys

import numpy as np
import pytest

import render_cases as rc

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lidar-slam-detection_amd", "python")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

pytestmark = pytest.mark.gpu
# a camera 0.5 m ahead of and above the lidar, looking forward, pitched 20 degrees down: [x, y, z, roll, pitch, yaw] of camera_extrinsic, the
# inverse of the camera's pose in the lidar frame (getTransformFromRPYT(x, y, z, yaw, pitch, roll))
EXTRINSIC = [-0.0, 0.640856, -0.298836, -110.0, 0.0, 90.0]
INTRINSIC = [300.0, 300.0, 160.0, 120.0]
FOV = (-24.8, 2.0)


def _module():
    import slam_wrapper

    from lsd_amd import capi

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device")
    assert slam_wrapper.__file__.endswith(".so"), slam_wrapper.__file__
    return slam_wrapper


def _cameras(sw, names):
    cfg = [dict(name=n, intrinsic_parameters=INTRINSIC, extrinsic_parameters=EXTRINSIC) for n in names]
    E = sw._transform_from_rpyt(EXTRINSIC[0], EXTRINSIC[1], EXTRINSIC[2], EXTRINSIC[5], EXTRINSIC[4], EXTRINSIC[3])
    return cfg, {n: (INTRINSIC, E) for n in names}


def _ground(lio):
    det = lio.GroundDetector()

    def ground(pts, seed=0):
        r = det.detect_host(pts, det.params(0, distance_threshold=rc.GROUND_THRESHOLD, seed=seed))
        return det.inliers() if r["found"] else None

    return ground


def test_offline_path_into_a_pcd(tmp_path):
    from lsd_amd import lio

    sw = _module()
    cfg, cams = _cameras(sw, ["front", "side"])
    # odometry every 50 ms: 3 m/s along x with a slow yaw; frames every 100 ms, 20 ms off the odometry stamps
    od = np.array([[1_000_000 + 50_000 * i, 0.3 + 0.15 * i, 0.01 * i, 0.0, 0.0, 0.0, np.sin(0.002 * i), np.cos(0.002 * i)] for i in range(13)])
    sw.set_colouration_config(cfg)
    sw.set_map_odometrys(od)
    sw.set_colouration_seed(7)
    world = rc.world_scene(21, 6000, 300)
    p = rc.Painter(cams, None)
    ground = _ground(lio)
    outcomes = []
    for k in range(6):
        header = 1_020_000 + 100_000 * k
        ok, _, pose = sw._stamp_pose(header, 0)
        assert ok
        body = rc.body_frame(world, pose, (1.0, 5.5))
        stamps = np.linspace(0, 99_000, len(body)).astype(np.float32)
        attr = dict(timestamp=header, points_attr=np.stack([stamps, np.zeros(len(body), np.float32)], 1))
        images = {"front": rc.image(240, 320, 600 + k), "side": rc.image(240, 320, 700 + k)}
        # the side camera's image of frame 2 is stamped outside the odometry: it is dropped
        param = {"front": dict(timestamp=header + 10_000), "side": dict(timestamp=2_000_000 if k == 2 else header + 30_000)}
        sw.colouration_frame("0-lidar", {"0-lidar": body}, {"0-lidar": attr}, images, {}, param)
        rc_out, frame, start, iposes = sw._colouration_last()
        outcomes.append(rc_out)
        if rc_out < 0:
            continue
        assert set(iposes) == ({"front"} if k == 2 else {"front", "side"})
        assert np.array_equal(start, sw._stamp_pose(header, 0)[2]) and len(frame) == len(body)
        want = p.frame(frame, start, {n: (images[n], iposes[n]) for n in iposes}, lambda q: ground(q, seed=7))
        assert want == {0: "skipped", 1: "no_floor", 2: "rendered"}[rc_out], (k, want, rc_out)
    # the last frame ends 100 ms after 1.52 s, past the odometry's 1.6 s: get_stamp_pose refuses it and nothing happens
    assert outcomes == [2, 2, 2, 2, 2, -1]
    file = str(tmp_path / "render.pcd")
    sw.save_render_cloud(file)
    xyz, rgb = sw._read_rgb_pcd(file)
    want = p.colour_map()
    assert len(want) > 200 and xyz.shape == (len(want), 3)
    assert np.array_equal(xyz.view(np.uint32), want[:, :3].view(np.uint32))
    assert np.array_equal(rgb & 0xFFFFFF, np.ascontiguousarray(want[:, 3]).view(np.uint32))
    # the painter is released: nothing more is written, and a frame needs a new set_colouration_config
    os.remove(file)
    sw.save_render_cloud(file)
    assert not os.path.exists(file)
    with pytest.raises(RuntimeError, match="set_colouration_config"):
        sw.colouration_frame("0-lidar", {"0-lidar": body}, {"0-lidar": attr}, images, {}, param)
    # an empty map writes nothing either
    sw.set_colouration_config(cfg)
    sw.save_render_cloud(file)
    assert not os.path.exists(file)
    sw.set_colouration_config(cfg)
    with pytest.raises(ValueError):
        sw.colouration_frame("0-lidar", {"0-lidar": body}, {"0-lidar": attr}, {"front": np.zeros((360, 320), np.uint8)}, {}, param)
    sw.save_render_cloud(file)


def _write_map(sw, root, scene, n_frames=30, n_az=600):
    """tests/test_outer_boundary.py::_write_map: key frames every 2 m along x, clouds in the key frame's own frame"""
    from lsd_amd import synth

    os.makedirs(os.path.join(root, "graph"), exist_ok=True)
    for k in range(n_frames):
        pos = np.array([-20.0 + 2.0 * k, 0.3 * np.sin(0.5 * k), 1.8])
        q = synth.quat_from_rotvec([0, 0, 0.05 * np.cos(0.3 * k)])
        raw, _ = synth.make_scan(scene, pos, q, seed=400 + k, n_az=n_az, fov_deg=FOV)
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = synth.quat_to_R(q), pos
        d = os.path.join(root, "graph", "%06d" % k)
        os.makedirs(d, exist_ok=True)
        pts = raw.copy()
        pts[:, 3] /= 255.0
        sw.dump_keyframe(d, 1_000_000 + 100_000 * k, k, pts, T)


def test_live_path_over_the_localisation_drive(tmp_path):
    """the lidar sits 1.8 m above the ground; the INS frame is put 0.8 m above the lidar (set_ins_external_param), so that the floor lies 1 m
    below the INS origin, inside detect_ground's clip of +-1.5 m"""
    from lsd_amd import synth

    sw = _module()
    scene = synth.Scene(half=100.0, n_boxes=40, seed=1)
    root = str(tmp_path / "map")
    _write_map(sw, root, scene)
    cfg, _ = _cameras(sw, ["front"])
    assert sw.init_slam("offline", root, "Localization", ["0-lidar", "IMU"], 0.2, 1.0, 10.0, 50.0) == ["0-lidar", "IMU"]
    sw.set_ins_external_param(0, 0, 0.8, 0, 0, 0)
    sw.set_imu_external_param(0, 0, 0, 0, 0, 0)
    sw.set_camera_param(cfg)
    assert sw.setup_slam() is True
    try:
        sw.set_map_colouration(True)
        tr = synth.Trajectory(p0=(-10.0, 0.2, 1.8), t_static=0.2, speed=4.0, heading=0.0, sway=0.3, yaw_amp=0.1)
        imu = synth.imu_stream(tr, 0.0, 2.6, rate=100.0, seed=5, gyr_sigma=1e-3, acc_sigma=1e-2)
        p0, R0 = tr.pos(0.1), tr.R(0.1)
        sw.set_init_pose(p0[0] + 0.2, p0[1] - 0.15, p0[2] - 0.8, np.degrees(np.arctan2(R0[1, 0], R0[0, 0])) + 1.0, 0.0, 0.0)
        ii, states, sizes = 0, [], []
        for k in range(1, 25):
            tb = k * 0.1
            rows = []
            while ii < len(imu) and imu[ii][0] <= tb:
                t, g, a = imu[ii]
                rows.append([t * 1e6, *(g * 180.0 / np.pi), *(a / 9.81)])
                ii += 1
            pts, st = synth.make_sweep(scene, tr, tb, seed=500 + k, n_az=900, fov_deg=FOV)
            stamp = int(round(tb * 1e6))
            attr = dict(timestamp=stamp, points_attr=np.stack([st.astype(np.float32), np.zeros(len(st), np.float32)], 1))
            out = sw.process({"0-lidar": pts}, {"0-lidar": attr}, {"front": rc.image(240, 320, 900 + k)}, {}, {"front": dict(timestamp=stamp)}, {},
                             np.array(rows, np.float64).reshape(-1, 7), stamp)
            states.append(out["pose"]["state"])
            cm = sw.get_color_map()
            sizes.append(cm.shape)
            if states[-1] != "Localizing(L)":
                assert cm.shape == (0, 6), (k, cm.shape)  # before age 10 nothing is painted: what the module has always returned
        print("live colour map:", states.count("Localizing(L)"), "stable frames, sizes", sizes[-6:])
        assert states[0] == "Initializing" and states[-1] == "Localizing(L)"
        cm = sw.get_color_map()
        assert cm.ndim == 2 and cm.shape[1] == 4 and cm.dtype == np.float32 and len(cm) > 100
        word = np.ascontiguousarray(cm[:, 3]).view(np.uint32)
        assert np.all(word >> 24 == 0) and len(np.unique(word)) > 10
        assert np.all(np.abs(cm[:, 2]) < 0.5)  # the floor, z = 0 of the map, +- the localisation's error
        # dump_map_points("rgb"): the colour map between z_min and z_max
        z = np.sort(cm[:, 2])
        z_lo, z_hi = float(z[len(z) // 4]), float(z[3 * len(z) // 4])
        file = str(tmp_path / "colour.pcd")
        sw.set_export_map_config(z_lo, z_hi, "rgb")
        sw.export_points(np.zeros((5, 4), np.float32), np.eye(4, dtype=np.float32))  # (ignored for "rgb")
        sw.dump_map_points(file)
        xyz, rgb = sw._read_rgb_pcd(file)
        keep = (cm[:, 2].astype(np.float64) >= z_lo) & (cm[:, 2].astype(np.float64) <= z_hi)
        assert 0 < keep.sum() < len(cm) and np.array_equal(xyz, cm[keep, :3]) and np.array_equal(rgb & 0xFFFFFF, word[keep])
        # with colouration off the images are not looked at (a 2-D image would raise) and the map stays
        sw.set_map_colouration(False)
        out = sw.process({"0-lidar": pts}, {"0-lidar": attr}, {"front": np.zeros((10, 10), np.uint8)}, {}, {}, {}, np.zeros((0, 7)), stamp)
        assert np.array_equal(sw.get_color_map(), cm)
    finally:
        sw.deinit_slam()
