"""get_estimate_pose through the compiled module (csrc/slam_wrapper.cpp): the operator draws an arrow on the map, the module matches the latest
scan against the key frames near it (FAST_VGICP on the device), answers with the refined pose and, when the match is good, starts the localiser
from it -- handing over through the next frame (pose * delta).  The map and the frames are tests/test_relocalization_gpu.py's (helpers copied),
relocalisation off; the bounds on the position error are the localisation test's own."""
import os
import sys

import numpy as np
import pytest

import estimate_pose_cases as E

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lidar-slam-detection_amd", "python")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

pytestmark = pytest.mark.gpu
FOV = (-24.8, 2.0)
P0 = (-10.0, 0.2, 1.8)  # key frame 5 of the map


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
    root = str(tmp_path_factory.mktemp("estimate") / "map")
    _write_map(sw, root, scene)
    return sw, scene, root


def _start(sw, root):
    assert sw.init_slam("offline", root, "Localization", ["0-lidar", "IMU"], 0.2, 1.0, 10.0, 50.0) == ["0-lidar", "IMU"]
    sw.set_ins_external_param(0, 0, 0, 0, 0, 0)
    sw.set_imu_external_param(0, 0, 0, 0, 0, 0)
    assert sw.setup_slam() is True


def _frame(sw, scene, tr, imu, state, k, seed0):
    from lsd_amd import synth

    tb = k * 0.1
    rows = []
    while state["ii"] < len(imu) and imu[state["ii"]][0] <= tb:
        t, g, a = imu[state["ii"]]
        rows.append([t * 1e6, *(g * 180.0 / np.pi), *(a / 9.81)])
        state["ii"] += 1
    pts, st = synth.make_sweep(scene, tr, tb, seed=seed0 + k, n_az=900, fov_deg=FOV)
    attr = dict(timestamp=int(round(tb * 1e6)), points_attr=np.stack([st.astype(np.float32), np.zeros(len(st), np.float32)], 1))
    return sw.process({"0-lidar": pts}, {"0-lidar": attr}, {}, {}, {}, {}, np.array(rows, np.float64).reshape(-1, 7), int(round(tb * 1e6)))


def _traj(t_end, p0=P0, t_static=0.2, sway=0.3, yaw_amp=0.1):
    from lsd_amd import synth

    tr = synth.Trajectory(p0=p0, t_static=t_static, speed=4.0, heading=0.0, sway=sway, yaw_amp=yaw_amp)
    return tr, synth.imu_stream(tr, 0.0, t_end, rate=100.0, seed=5, gyr_sigma=1e-3, acc_sigma=1e-2)


def _frame_beside_a_key_frame(tr, lo, hi):
    """the frame in [lo, hi) taken nearest to a key frame of the map.  The fitness score is a mean squared nearest-neighbour distance between
    two samplings of the scene, and it grows with the distance between the viewpoints (tests/test_relocalization_gpu.py: a scan taken a metre
    beside the nearest key frame is no positive case, for the reference either); the positive cases hint where the map can confirm them"""
    kf = np.array([[-20.0 + 2.0 * j, 0.3 * np.sin(0.5 * j)] for j in range(30)])
    d = [np.min(np.linalg.norm(kf - tr.pos(k * 0.1)[:2], axis=1)) for k in range(lo, hi)]
    return lo + int(np.argmin(d)), float(np.min(d))


def _arrow(tr, t, off=(0.25, -0.166), ddeg=3.0):
    """an arrow 0.3 m beside and 3 degrees off the true pose at time t"""
    p, R = tr.pos(t), tr.R(t)
    a = np.arctan2(R[1, 0], R[0, 0]) + np.radians(ddeg)
    x0, y0 = p[0] + off[0], p[1] + off[1]
    return x0, y0, x0 + np.cos(a), y0 + np.sin(a)


def _rule(sw, pose, arrow):
    """what every answer must satisfy: result 1 iff converged and score < 0.5; the pose replaced iff converged and score < 5"""
    r = sw._last_estimate_pose()
    hint = E.hint_matrix(*arrow)
    print("get_estimate_pose:", [round(float(v), 4) for v in pose], {k: r[k] for k in ("rc", "result", "converged", "iterations", "score", "ids", "n_target", "n_source")},
          {k: round(v) for k, v in r["times"].items()})
    assert r["called"] and r["rc"] == 0 and np.array_equal(r["hint"], hint)
    want_result, want_replaced = E.result_logic(r["converged"], r["score"])
    assert r["result"] == want_result == int(pose[6]) and r["pose_replaced"] == want_replaced
    assert np.allclose(pose[:3], r["out_T"][:3, 3], atol=1e-12)
    if not want_replaced:  # the hint, with the height the two clouds give when the matcher ran
        assert np.array_equal(r["out_T"][:3, :3], hint[:3, :3]) and np.array_equal(r["out_T"][:2, 3], hint[:2, 3])
        if r["n_target"] and r["n_source"]:
            assert r["out_T"][2, 3] == r["z_mean_target"] - r["z_mean_source"]
        else:
            assert r["out_T"][2, 3] == 0.0
    return r


def _bounds(errs, states, whole_median=True):
    print("after the hint: position error median %.3f m, max after the first second %.3f m" % (np.median(errs), max(errs[10:])))
    assert max(errs[10:]) < 0.15 and np.median(errs if whole_median else errs[10:]) < 0.08
    assert states[-1] == "Localizing(L)"


def test_a_before_any_frame_the_hint_comes_back(world):
    sw, scene, root = world
    _start(sw, root)
    try:
        pose = sw.get_estimate_pose(-10.0, 0.2, -9.0, 0.2)
        assert len(pose) == 7 and np.allclose(pose, [-10.0, 0.2, 0, 0, 0, 0, 0], atol=1e-9)
        r = sw._last_estimate_pose()
        assert r["called"] and r["result"] == 0 and r["n_source"] == 0 and r["handover"] is False
    finally:
        sw.deinit_slam()


def test_b_hint_at_rest_starts_the_localiser(world):
    sw, scene, root = world
    _start(sw, root)
    try:
        tr, imu = _traj(4.4)
        state = dict(ii=0)
        out = _frame(sw, scene, tr, imu, state, 1, 500)
        assert out["pose"]["state"] == "Initializing"
        arrow = _arrow(tr, 0.1)
        pose = sw.get_estimate_pose(*arrow)
        r = _rule(sw, pose, arrow)
        assert r["result"] == 1 and r["ids"][0] == 5 and len(r["ids"]) == 5
        assert np.linalg.norm(np.array(pose[:3]) - tr.pos(0.1)) < 0.15
        errs, states = [], []
        for k in range(2, 42):
            out = _frame(sw, scene, tr, imu, state, k, 500)
            errs.append(float(np.linalg.norm(out["pose"]["odom_matrix"][:3, 3] - tr.pos(k * 0.1))))
            states.append(out["pose"]["state"])
            if k == 2:
                h = sw._last_estimate_pose()
                print("hand-over: ran %s converged %s |t| %.4f" % (h["delta_ran"], h["delta_converged"], np.linalg.norm(h["delta"][:3, 3])))
                assert h["handover"] and h["delta_ran"] and np.linalg.norm(h["delta"][:3, 3]) < 0.1  # the vehicle has hardly moved yet
        _bounds(errs, states)
    finally:
        sw.deinit_slam()


def test_c_hint_while_moving_is_handed_over_by_the_delta(world):
    sw, scene, root = world
    _start(sw, root)
    try:
        # a straight drive that passes over key frame 8 (x = -4, y = 0.3 sin 4): the hinted frame is taken there, at speed
        tr, imu = _traj(6.8, p0=(-10.0, 0.3 * np.sin(4.0), 1.8), sway=0.0, yaw_amp=0.0)
        state = dict(ii=0)
        k0, beside = _frame_beside_a_key_frame(tr, 25, 35)  # up to speed (the trajectory approaches 4 m/s: 0.3 - 0.4 m a frame)
        print("hint on frame %d, %.3f m beside a key frame, %.3f m before the next frame" % (k0, beside, np.linalg.norm(tr.pos((k0 + 1) * 0.1) - tr.pos(k0 * 0.1))))
        assert np.linalg.norm(tr.pos((k0 + 1) * 0.1) - tr.pos(k0 * 0.1)) > 0.3
        for k in range(k0 - 1, k0 + 1):
            out = _frame(sw, scene, tr, imu, state, k, 500)
            assert out["pose"]["state"] == "Initializing"
        arrow = _arrow(tr, k0 * 0.1)
        pose = sw.get_estimate_pose(*arrow)
        r = _rule(sw, pose, arrow)
        assert r["result"] == 1
        errs, states = [], []
        for k in range(k0 + 1, k0 + 32):
            out = _frame(sw, scene, tr, imu, state, k, 500)
            p = out["pose"]["odom_matrix"][:3, 3]
            errs.append(float(np.linalg.norm(p - tr.pos(k * 0.1))))
            states.append(out["pose"]["state"])
            if k == k0 + 1:  # the first localised pose belongs to its own stamp, not to the hinted frame's: the delta was applied
                h = sw._last_estimate_pose()
                print("hand-over: ran %s converged %s |t| %.4f; to the truth now %.3f m, to the truth at the hint %.3f m"
                      % (h["delta_ran"], h["delta_converged"], np.linalg.norm(h["delta"][:3, 3]), errs[0], np.linalg.norm(p - tr.pos(k0 * 0.1))))
                assert h["handover"] and h["delta_ran"]
                assert errs[0] < np.linalg.norm(p - tr.pos(k0 * 0.1))
        _bounds(errs, states, whole_median=False)
    finally:
        sw.deinit_slam()


def test_d_hint_far_from_the_map_changes_nothing(world):
    sw, scene, root = world
    _start(sw, root)
    try:
        tr, imu = _traj(1.0)
        state = dict(ii=0)
        _frame(sw, scene, tr, imu, state, 1, 500)
        arrow = (-50.0, 0.2, -49.0, 0.2)  # the first key frame is at x = -20
        pose = sw.get_estimate_pose(*arrow)
        r = _rule(sw, pose, arrow)
        assert r["result"] == 0 and r["ids"] == [] and np.allclose(pose, [-50.0, 0.2, 0, 0, 0, 0, 0], atol=1e-9)
        out = _frame(sw, scene, tr, imu, state, 2, 500)
        assert out["pose"]["state"] == "Initializing" and sw._last_estimate_pose()["handover"] is False
    finally:
        sw.deinit_slam()


def test_e_hint_at_the_far_end_of_the_map_follows_the_rule(world):
    """which way this goes is not asserted (a scan of one place against key frames of another): only the rule, and the score is printed"""
    sw, scene, root = world
    _start(sw, root)
    try:
        tr, imu = _traj(1.0)
        state = dict(ii=0)
        _frame(sw, scene, tr, imu, state, 1, 500)
        arrow = (36.0, 0.2, 37.0, 0.2)
        pose = sw.get_estimate_pose(*arrow)
        r = _rule(sw, pose, arrow)
        print("far end of the map: converged %s score %.4f result %d" % (r["converged"], r["score"], r["result"]))
        assert len(r["ids"]) == 5 and r["ids"][0] == 28
        if r["result"] == 0:
            out = _frame(sw, scene, tr, imu, state, 2, 500)
            assert out["pose"]["state"] == "Initializing"
    finally:
        sw.deinit_slam()


def test_f_correct_hint_while_localising_drops_and_resumes(world):
    sw, scene, root = world
    _start(sw, root)
    try:
        tr, imu = _traj(5.0, t_static=2.0)  # two seconds at rest at key frame 5: localising, then hinted where the map can confirm it, then off
        state = dict(ii=0)
        p0, R0 = tr.pos(0.1), tr.R(0.1)
        sw.set_init_pose(p0[0] + 0.2, p0[1] - 0.15, p0[2], np.degrees(np.arctan2(R0[1, 0], R0[0, 0])) + 1.0, 0.0, 0.0)
        k0, beside = _frame_beside_a_key_frame(tr, 13, 19)  # localising since frame 1: stable from frame 10 on; at rest until frame 20
        print("hint on frame %d, %.3f m beside a key frame" % (k0, beside))
        assert beside < 0.05
        for k in range(1, k0 + 1):
            out = _frame(sw, scene, tr, imu, state, k, 500)
        assert out["pose"]["state"] == "Localizing(L)"
        arrow = _arrow(tr, k0 * 0.1, off=(0.0, 0.0), ddeg=0.0)
        pose = sw.get_estimate_pose(*arrow)
        r = _rule(sw, pose, arrow)
        assert r["result"] == 1
        errs, states = [], []
        for k in range(k0 + 1, k0 + 32):
            out = _frame(sw, scene, tr, imu, state, k, 500)
            errs.append(float(np.linalg.norm(out["pose"]["odom_matrix"][:3, 3] - tr.pos(k * 0.1))))
            states.append(out["pose"]["state"])
        assert states[0] == "Initializing"  # the localisation dropped ...
        _bounds(errs, states, whole_median=False)  # ... and resumed
    finally:
        sw.deinit_slam()


def test_g_mapping_mode_and_a_zero_length_arrow_answer_zeros(world):
    sw, scene, root = world
    sw.init_slam("mapping", "", "FastLIO", ["0-lidar", "IMU"], 0.2, 1.0, 10.0, 50.0)
    try:
        assert list(sw.get_estimate_pose(0.0, 0.0, 1.0, 0.0)) == [0.0] * 7
    finally:
        sw.deinit_slam()
    assert list(sw.get_estimate_pose(0.0, 0.0, 1.0, 0.0)) == [0.0] * 7  # no session at all
    _start(sw, root)
    try:
        tr, imu = _traj(1.0)
        _frame(sw, scene, tr, imu, dict(ii=0), 1, 500)
        assert list(sw.get_estimate_pose(-10.0, 0.2, -10.0, 0.2)) == [0.0] * 7
        assert sw._last_estimate_pose()["called"] is False  # nothing ran
        assert list(sw.get_estimate_pose(float("nan"), 0.2, -9.0, 0.2)) == [0.0] * 7
    finally:
        sw.deinit_slam()
    assert sw.init_slam("offline", root, "Localization", ["0-lidar", "IMU"], 0.2, 1.0, 10.0, 50.0) == ["0-lidar", "IMU"]
    try:
        assert list(sw.get_estimate_pose(-10.0, 0.2, -9.0, 0.2)) == [0.0] * 7  # before setup_slam
    finally:
        sw.deinit_slam()
