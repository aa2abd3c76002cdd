"""Global relocalisation through the compiled module (set_global_localization, csrc/slam_wrapper.cpp): in localisation mode the module finds its
own initial pose -- Scan Context search over the map's key frames, FAST_VGICP verification of the hit, the accept test of
GlobalLocalization::registrationAlign -- and then localises as it does after set_init_pose.  The map is the existing localisation test's
(tests/test_outer_boundary.py::_write_map, copied here), the bounds on the position error are that test's own."""
import os
import sys

import numpy as np
import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lidar-slam-detection_amd", "python")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

pytestmark = pytest.mark.gpu
FOV = (-24.8, 2.0)


def _module():
    import slam_wrapper  # the compiled module (lidar-slam-detection_amd/python/slam_wrapper.*.so)

    assert slam_wrapper.__file__.endswith(".so"), slam_wrapper.__file__
    return slam_wrapper


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


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from lsd_amd import capi, synth

    if capi.lib().lio_device_count() < 1:
        pytest.fail("no HIP device")
    sw = _module()
    scene = synth.Scene(half=100.0, n_boxes=40, seed=1)
    root = str(tmp_path_factory.mktemp("reloc") / "map")
    _write_map(sw, root, scene)
    return sw, scene, root


def _start(sw, root, reloc):
    assert sw.init_slam("offline", root, "Localization", ["0-lidar", "IMU"], 0.2, 1.0, 10.0, 50.0) == ["0-lidar", "IMU"]
    sw.set_ins_external_param(0, 0, 0, 0, 0, 0)
    sw.set_imu_external_param(0, 0, 0, 0, 0, 0)
    if reloc:
        sw.set_global_localization(True)
    assert sw.setup_slam() is True


def _frame(sw, scene, tr, imu, state, k, seed0, empty=False):
    tb = k * 0.1
    rows = []
    while state["ii"] < len(imu) and imu[state["ii"]][0] <= tb:
        t, g, a = imu[state["ii"]]
        rows.append([t * 1e6, *(g * 180.0 / np.pi), *(a / 9.81)])
        state["ii"] += 1
    from lsd_amd import synth

    pts, st = synth.make_sweep(scene, tr, tb, seed=seed0 + k, n_az=900, fov_deg=FOV)
    if empty:
        pts, st = pts[:0], st[:0]
    attr = dict(timestamp=int(round(tb * 1e6)), points_attr=np.stack([st.astype(np.float32), np.zeros(len(st), np.float32)], 1))
    return sw.process({"0-lidar": pts}, {"0-lidar": attr}, {}, {}, {}, {}, np.array(rows, np.float64).reshape(-1, 7), int(round(tb * 1e6)))


def _drive(sw, scene, p0, heading, want_frame, want_shift):
    from lsd_amd import synth

    tr = synth.Trajectory(p0=p0, t_static=0.2, speed=4.0, heading=heading, sway=0.3, yaw_amp=0.1)
    imu = synth.imu_stream(tr, 0.0, 4.3, rate=100.0, seed=5, gyr_sigma=1e-3, acc_sigma=1e-2)
    state, errs, states = dict(ii=0), [], []
    for k in range(1, 41):
        out = _frame(sw, scene, tr, imu, state, k, 500)
        M = out["pose"]["odom_matrix"]
        if k == 1:
            r = sw._last_relocalization()
            print("first frame:", r)
            assert r["searched"] and r["match_id"] == want_frame and r["accepted"] and r["converged"] and r["fitness"] < 1.5 and r["score"] < 0.30
            assert int(round(np.degrees(r["yaw"]) / 6.0)) % 60 == want_shift
            assert np.linalg.norm(M[:3, 3] - tr.pos(0.1)) < 0.15
        errs.append(float(np.linalg.norm(M[:3, 3] - tr.pos(k * 0.1))))
        states.append(out["pose"]["state"])
    print("relocalised drive: position error median %.3f m, max after the first second %.3f m" % (np.median(errs), max(errs[10:])))
    assert max(errs[10:]) < 0.15 and np.median(errs) < 0.08
    assert states[-1] == "Localizing(L)"
    return tr, imu, state


def test_switch_off_waits_for_an_initial_pose(world):
    from lsd_amd import synth

    sw, scene, root = world
    _start(sw, root, False)
    try:
        tr = synth.Trajectory(p0=(-10.0, 0.2, 1.8), t_static=0.2, speed=4.0, heading=0.0, sway=0.3, yaw_amp=0.1)
        out = _frame(sw, scene, tr, [], dict(ii=0), 1, 500)
        assert out["pose"]["state"] == "Initializing" and np.array_equal(out["pose"]["odom_matrix"], np.eye(4, dtype=np.float32))
        assert sw._last_relocalization()["searched"] is False
    finally:
        sw.deinit_slam()


def test_forward_drive(world):
    sw, scene, root = world
    _start(sw, root, True)
    try:
        _drive(sw, scene, (-10.0, 0.2, 1.8), 0.0, 5, 0)
        assert sw._last_relocalization()["searches"] == 1  # one search started the filter; none since
    finally:
        sw.deinit_slam()


def test_fallback_leads_back_into_the_search(world):
    """five empty clouds after the initialisation bring back "Initializing"; the next real frame searches and initialises again.  The frames lie in
    the first 0.8 s of the drive, within half a metre of key frame 5 (the trajectory rests for 0.2 s and has moved 0.42 m by 0.8 s): a scan taken
    a metre or more beside the nearest key frame is no positive case, for the reference either"""
    from lsd_amd import synth

    sw, scene, root = world
    _start(sw, root, True)
    try:
        tr = synth.Trajectory(p0=(-10.0, 0.2, 1.8), t_static=0.2, speed=4.0, heading=0.0, sway=0.3, yaw_amp=0.1)
        imu = synth.imu_stream(tr, 0.0, 1.0, rate=100.0, seed=5, gyr_sigma=1e-3, acc_sigma=1e-2)
        assert np.linalg.norm(tr.pos(0.8) - tr.pos(0.0)) < 0.5
        state = dict(ii=0)
        for k in (1, 2):
            out = _frame(sw, scene, tr, imu, state, k, 500)
        r = sw._last_relocalization()
        assert r["accepted"] and r["searches"] == 1 and np.linalg.norm(out["pose"]["odom_matrix"][:3, 3] - tr.pos(0.2)) < 0.15
        for k in range(3, 8):
            out = _frame(sw, scene, tr, imu, state, k, 500, empty=True)
        assert out["pose"]["state"] == "Initializing" and sw._last_relocalization()["searches"] == 1
        out = _frame(sw, scene, tr, imu, state, 8, 500)
        r = sw._last_relocalization()
        print("after the fallback:", r)
        assert r["searches"] == 2 and r["match_id"] == 5 and r["accepted"]
        assert np.linalg.norm(out["pose"]["odom_matrix"][:3, 3] - tr.pos(0.8)) < 0.15
    finally:
        sw.deinit_slam()


def test_reverse_drive(world):
    sw, scene, root = world
    _start(sw, root, True)
    try:
        _drive(sw, scene, (20.0, 0.2, 1.8), np.pi, 20, 30)
    finally:
        sw.deinit_slam()


def test_a_scan_of_another_place_is_refused(world):
    from lsd_amd import synth

    sw, scene, root = world
    other = synth.Scene(half=100.0, n_boxes=40, seed=99)  # the same generator, another town
    _start(sw, root, True)
    try:
        tr = synth.Trajectory(p0=(-10.0, 0.2, 1.8), t_static=0.2, speed=4.0, heading=0.0, sway=0.3, yaw_amp=0.1)
        out = _frame(sw, other, tr, [], dict(ii=0), 1, 500)
        r = sw._last_relocalization()
        print("another place:", r)
        assert out["pose"]["state"] == "Initializing" and np.array_equal(out["pose"]["odom_matrix"], np.eye(4, dtype=np.float32))
        assert r["searched"] and not r["accepted"]
        assert r["match_id"] < 0 or not r["converged"] or not (r["fitness"] < 1.5 and r["dx"] < 10.0 and r["da"] < 30.0)
    finally:
        sw.deinit_slam()
