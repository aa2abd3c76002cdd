"""The GNSS side of mapping mode through slam_wrapper: init_slam(method="RTKM") on lsd_amd.synth scenes, the FastLIO side (set_gnss, the GNSS
queue into the pose graph's priors) without running the engine, and the localisation mode's latitude / longitude from the map's origin --
against tests/rtk_cases.py's restatement."""
import functools
import os
import shutil

import numpy as np
import pytest

import keyframe_cases as kc
import map_save_cases as MC
import rtk_cases as R
from lsd_amd import capi, lio, synth

pytestmark = pytest.mark.gpu

POS_TOL, ROT_TOL = 1e-4, 1e-5  # the project's parity tolerance (metres, radians)
N_FRAMES, T0, PERIOD = 30, 1_700_000_000_000_000, 100_000
INS_EXT = (1.0, 0.5, 1.2, 3.0, 1.0, -2.0)
LAT0, LON0, ALT0 = 31.2, 121.5, 4.0


def _rot_angle(A, B):
    M = A[:3, :3].T @ B[:3, :3]
    return float(np.arctan2(np.linalg.norm(M - M.T) / (2.0 * np.sqrt(2.0)), (np.trace(M) - 1.0) / 2.0))


def _rtk(f, status=1):
    """the dict slam.py hands to process() for a fix"""
    return dict(timestamp=int(f["stamp_us"]), latitude=f["latitude"], longitude=f["longitude"], altitude=f["altitude"], heading=f["heading"], pitch=f["pitch"],
                roll=f["roll"], gyro_x=0.0, gyro_y=0.0, gyro_z=0.0, acc_x=0.0, acc_y=0.0, acc_z=0.0, Ve=0.0, Vn=0.0, Vu=0.0, Status=status, Sensor="GNSS")


@functools.lru_cache(maxsize=None)
def _drive():
    """30 frames at 1 m per frame heading north-east, three lidars of 2 000 points each (the base is the second by name), fixes at 20 Hz built with the restated projector from the
    trajectory: fix j at T0 + 50 000 j + 7 000 us (no frame stamp falls on a fix)"""
    scene = synth.Scene(half=60.0, n_boxes=20, seed=3)
    proj = R.UtmRef()
    x0, y0 = proj.forward(LAT0, LON0)
    yaw = np.radians(40.0)
    fixes = []
    for j in range(2 * N_FRAMES + 2):
        d = 0.5 * j + 0.07  # metres along the track at the fix's stamp
        lat, lon = proj.inverse(x0 + d * np.sin(yaw), y0 + d * np.cos(yaw))
        fixes.append(R.fix(T0 + 50_000 * j + 7_000, lat, lon, ALT0 + 0.01 * j, 40.0 + 0.2 * j, 0.5 * np.sin(0.2 * j), 0.3 * np.cos(0.3 * j)))
    frames = []
    for k in range(N_FRAMES):
        pos = np.array([-20.0 + 1.0 * k * np.sin(yaw), -15.0 + 1.0 * k * np.cos(yaw), 1.8])
        clouds = {}
        for name, seed, shift in (("0-front", 100 + k, 0), ("1-rear", 200 + k, 3_000), ("2-side", 300 + k, -2_500)):
            raw, _ = synth.make_scan(scene, pos, synth.quat_from_rotvec([0, 0, 0.5]), seed=seed, n_beams=16, n_az=200)
            rng = np.random.default_rng(seed)
            raw = raw[np.sort(rng.choice(len(raw), min(2000, len(raw)), replace=False))]
            st = np.sort(rng.integers(0, PERIOD + 1, len(raw))).astype(np.float32)
            clouds[name] = (raw, dict(timestamp=T0 + PERIOD * k + shift, points_attr=np.stack([st, np.arange(len(raw), dtype=np.float32)], 1)))
        frames.append(clouds)
    return fixes, frames


def _start_rtkm(sw, sensors=("1-rear", "RTK", "0-front", "2-side")):
    # the first "n-" name in the list is the base lidar: 1-rear, which is not the first in name order
    assert sw.init_slam("mapping", "", "RTKM", list(sensors), 0.5, 0.2, 10.0, 60.0) == ["RTK", "1-rear", "0-front", "2-side"]
    sw.set_ins_external_param(*INS_EXT)
    assert sw.setup_slam() is True


def test_rtkm_drive_against_the_restatement():
    import slam_wrapper as sw

    fixes, frames = _drive()
    _start_rtkm(sw)
    track = R.TrackRef()
    T_static = np.array(sw._transform_from_rpyt(*INS_EXT))
    twin = lio.KeyFramer(key_frame_distance=float(np.float32(0.2)), key_frame_degree=10.0, resolution=0.5, key_frame_range=60.0)
    try:
        sw.set_keyframe_output(True)
        assert np.array_equal(sw.get_map_origin(), np.zeros((1, 7)))
        last, n_interp, worst_p, worst_r = np.eye(4), 0, 0.0, 0.0
        for k, clouds in enumerate(frames):
            mine = [fixes[2 * k - 1], fixes[2 * k]] if k else [fixes[0]]
            for f in mine[:-1]:
                sw._push_gnss(_rtk(f))
            if k == 0:
                took, last = track.set_origin(fixes[0])
                assert took
            for f in mine:
                track.feed(f)
            pts = {n: c[0] for n, c in clouds.items()}
            attr = {n: c[1] for n, c in clouds.items()}
            out = sw.process(pts, attr, {}, {}, {}, _rtk(mine[-1]), np.zeros((0, 7)), T0 + PERIOD * k)
            p = out["pose"]
            # the merged frame: base 1-rear, then 0-front and 2-side in name order
            order = ["1-rear", "0-front", "2-side"]
            want_p, want_s, kept, early, late = R.merge_points([clouds[n][0] for n in order], [clouds[n][1]["points_attr"][:, 0].astype(np.uint32) for n in order],
                                                               [clouds[n][1]["timestamp"] for n in order], PERIOD, T_static)
            got_p, got_s = sw._last_merged()
            assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32)) and np.array_equal(got_s, want_s)
            assert kept[0] == len(clouds["1-rear"][0]) and early[1] + late[1] > 0 and early[2] + late[2] > 0  # both other lidars lose points to the gate
            header = clouds["1-rear"][1]["timestamp"]
            assert p["timestamp"] == header and p["state"] == "Mapping" and p["Status"] == 1 and out["frame_start_timestamp"] == T0 + PERIOD * k
            assert (p["latitude"], p["longitude"], p["altitude"]) == (mine[-1]["latitude"], mine[-1]["longitude"], mine[-1]["altitude"])  # the frame's fix
            code, odom = track.interpolate(header)
            if odom is None:
                assert k == 0 and code == R.TOO_FEW  # the frames before the second fix keep mLastOdom (the origin's pose)
                odom = last
            else:
                assert code == R.INTERPOLATED
                n_interp += 1
            M = p["odom_matrix"]
            assert M.dtype == np.float32 and M.shape == (4, 4)
            worst_p, worst_r = max(worst_p, np.abs(M[:3, 3] - odom[:3, 3]).max()), max(worst_r, _rot_angle(M.astype(np.float64), odom))
            start, end = sw._last_odometry()
            assert np.abs(start - last).max() < 1e-9 and np.abs(end - odom).max() < 1e-9
            twin.push(got_p, got_s, header, end, delta=kc.rigid_inverse(start) @ end)
            last = odom
            if k == 0:
                o = sw.get_map_origin()
                assert np.array_equal(o, [[fixes[0][n] for n in ("latitude", "longitude", "altitude", "heading", "pitch", "roll")] + [0.0]])
                sw.set_map_origin(10.0, 20.0, 30.0, 0.0, 0.0, 0.0)  # a later origin does not move it
                assert np.array_equal(sw.get_map_origin(), o)
        print("RTKM: %d interpolated frames, worst |dp| %.2e m, worst rotation %.2e rad" % (n_interp, worst_p, worst_r))
        assert n_interp == N_FRAMES - 1 and worst_p <= POS_TOL and worst_r <= ROT_TOL
        assert 25.0 < np.linalg.norm(last[:3, 3]) < 300.0  # about 29 m from the origin
        assert sw._gnss_state()["tracked"] == 2 * N_FRAMES - 1 and sw._gnss_state()["queued"] == 0  # RTKM pushes nothing into the graph's queue
        d = sw.update_odom()
        assert d["odoms"] == {} and len(d["keyframes"]) >= 2 and twin.pending() == len(d["keyframes"])
        for f in d["keyframes"]:
            want = twin.pop()
            # (the twin's delta is the same product of f64 matrices summed in numpy's order: its last bits may differ, the frame's points with them)
            assert f["stamp"] == want["stamp"] and f["points"].shape == want["points"].shape and np.abs(f["points"] - want["points"]).max() <= POS_TOL
            assert np.array_equal(f["pose"], want["pose"].astype(np.float32))
    finally:
        twin.close()
        sw.deinit_slam()


def test_rtkm_without_the_base_lidar_or_a_fix():
    import slam_wrapper as sw

    fixes, frames = _drive()
    _start_rtkm(sw)
    try:
        clouds = frames[0]
        pts = {n: c[0] for n, c in clouds.items() if n != "1-rear"}
        attr = {n: c[1] for n, c in clouds.items() if n != "1-rear"}
        out = sw.process(pts, attr, {}, {}, {}, {}, np.zeros((0, 7)), T0)  # no base lidar: an empty frame; no fix: no origin, the identity
        assert len(sw._last_merged()[0]) == 0 and np.array_equal(out["pose"]["odom_matrix"], np.eye(4, dtype=np.float32))
        invalid = _rtk(R.fix(T0, 0.0, 0.0, 0.0), status=0)  # the validity filter's zero fix
        sw._push_gnss(invalid)
        assert sw._gnss_state()["origin_set"] is False and sw._gnss_state()["tracked"] == 0
    finally:
        sw.deinit_slam()


# ---- FastLIO mapping with the switch on: the GNSS queue into the pose graph's priors, without running the engine ---------------------------------
def _gnss_session(sw, gnss_on, via_queue=True, matches=None):
    """MC's 8 key frames (2 m apart, 0.1 s apart) with fixes at 20 Hz over the same stretch; update_odom() after every key frame.  via_queue False:
    the twin session, fed `matches` [(key frame, xyz, precision, dimension, quat)] through add_graph_gnss at the pass the queue matched them"""
    scene = MC.scene()
    frames = MC.keyframes(scene)
    proj = R.UtmRef()
    x0, y0 = proj.forward(LAT0, LON0)
    fixes = []
    for j in range(-1, 19):  # from before the first key frame (stamp 1 000 000) to after the last (1 700 000)
        t = 1_000_000 + 50_000 * j + 3_000
        d = 2.0 * (t - 1_000_000) / 100_000
        lat, lon = proj.inverse(x0 + 6.0 * d, y0 + 0.5 * d)  # 12 m between key frames: outside the 10 m gate of this precision
        fixes.append(R.fix(t, lat, lon, ALT0 + 0.02 * j, 85.0 + 0.3 * j, 0.2, -0.1))
    assert sw.init_slam("mapping", "", "FastLIO", ["RTK", "IMU", "0-lidar"], 0.5, 0.2, 10.0, 60.0) == ["RTK", "IMU", "0-lidar"]
    log = []
    try:
        sw.set_ins_config(dict(ins_type="6D", ins_normal=dict(use=True, status=1, stable_time=0.0, precision=0.05), ins_float=dict(use=False, status=2, stable_time=0.0, precision=1.0),
                               ins_fix=dict(use=False, status=4, stable_time=0.0, precision=0.01)))
        sw.set_gnss(gnss_on)
        sw.set_pose_graph(True)
        fed = 0
        for k, (pts, T, stamp, accum) in enumerate(frames):
            while via_queue and fed < len(fixes) and fixes[fed]["stamp_us"] <= stamp + 60_000:
                sw._push_gnss(_rtk(fixes[fed]))
                fed += 1
            sw._push_keyframe(pts, T, stamp, accum)
            before = {p["id"] for p in sw._graph_priors()}
            assert len(sw.update_odom()["keyframes"]) == 1
            if not via_queue:
                for m in [m for m in matches if m[0] == k]:
                    for (kf, xyz, prec, dim, quat) in m[1]:
                        assert len(sw.add_graph_gnss(kf, xyz, prec, dim, quat)) == 2
            log.append(sorted({p["id"] for p in sw._graph_priors()} - before))
        return fixes, frames, sw._graph_priors(), sw.get_graph_meta()["vertex"]["0"]["fix"], np.array(sw.get_map_origin()), sw._gnss_state(), log
    finally:
        sw.deinit_slam()


def _restated_matches(fixes, frames):
    """the restated queue through the same passes: at the pass of key frame k the flush sees key frames 0 .. k - 1"""
    q = R.GnssQueueRef()
    valid = [dict(f, precision=0.05, dimension=6) for f in fixes]  # what the validity filter leaves: the configured dimension and precision
    q.set_origin(valid[0], None)  # the first valid fix; no key frame is in the graph yet
    stamps = np.array([f[2] for f in frames], np.uint64)
    has = np.zeros(len(frames), np.uint8)
    fed, per_pass = 0, []
    for k in range(len(frames)):
        while fed < len(valid) and valid[fed]["stamp_us"] <= int(stamps[k]) + 60_000:
            q.push(valid[fed])
            fed += 1
        sub = has[:k].copy()
        found = q.flush(stamps[:k], sub) if k else []
        has[:k] = sub
        per_pass.append(found)
    return per_pass


def test_fastlio_gnss_priors_against_the_restatement():
    import slam_wrapper as sw

    fixes, frames, priors, meta, origin, state, log = _gnss_session(sw, True)
    per_pass = _restated_matches(fixes, frames)
    want = [m for found in per_pass for m in found]
    assert len(want) >= 2 and {m["dimension"] for m in want} == {6}
    f0 = fixes[0]
    assert np.array_equal(origin, [[f0["latitude"], f0["longitude"], f0["altitude"], f0["heading"], f0["pitch"], f0["roll"], 0.0]]) and state["origin_set"]
    xyz = [p for p in priors if p["type"] == 0]
    quat = [p for p in priors if p["type"] == 1]
    assert [p["node"] for p in xyz] == [m["keyframe"] for m in want] == [p["node"] for p in quat] and len(priors) == 2 * len(want)
    for p, r, m in zip(xyz, quat, want):
        info, rot = R.gnss_information(m)
        assert np.abs(p["measurement"][:3] - m["xyz"]).max() <= 1e-6
        assert np.abs(p["information"] - info).max() <= 1e-12 * np.abs(info).max() and np.abs(r["information"] - rot).max() <= 1e-12 * np.abs(rot).max()
        assert min(np.abs(r["measurement"] - m["quat"]).max(), np.abs(r["measurement"] + m["quat"]).max()) <= 1e-9
        assert p["kernel"] == 1 and r["kernel"] == 1 and p["delta"] == 1.0 and r["delta"] == 1.0  # Huber 1.0
    # a key frame added in a pass is matched at the next one at the earliest
    assert all(m["keyframe"] < k for k, found in enumerate(per_pass) for m in found) and [len(x) for x in log] == [2 * len(found) for found in per_pass]
    assert meta is False  # node 0 is released
    # a twin session fed the same matches through add_graph_gnss holds the same priors
    matches = [(k, [(m["keyframe"], m["xyz"], m["precision"], m["dimension"], m["quat"]) for m in found]) for k, found in enumerate(per_pass)]
    _, _, twin, twin_meta, twin_origin, _, _ = _gnss_session(sw, False, via_queue=False, matches=matches)
    assert len(twin) == len(priors) and np.array_equal(twin_origin, np.zeros((1, 7))) and twin_meta is False
    for a, b in zip(priors, twin):
        assert (a["node"], a["type"], a["kernel"], a["delta"]) == (b["node"], b["type"], b["kernel"], b["delta"])
        assert np.abs(a["measurement"] - b["measurement"]).max() <= 1e-6 and np.array_equal(a["information"], b["information"])


def test_fastlio_gnss_switch_off_leaves_no_origin_and_no_prior():
    import slam_wrapper as sw

    _, _, priors, meta, origin, state, _ = _gnss_session(sw, False)
    assert priors == [] and np.array_equal(origin, np.zeros((1, 7))) and state["queued"] == 0 and not state["origin_set"] and meta is True


# ---- localisation: latitude / longitude from the loaded map's origin ---------------------------------------------------------------------------------
def _localise(sw, root, scene, n=16):
    assert sw.init_slam("offline", root, "Localization", ["0-lidar", "IMU"], 0.2, 1.0, 10.0, 50.0) == ["0-lidar", "IMU"]
    sw.set_ins_external_param(0, 0, 0, 0, 0, 0)
    sw.set_imu_external_param(0, 0, 0, 0, 0, 0)
    assert sw.setup_slam() is True
    try:
        pos, q, T4 = MC.keyframe_pose(4)
        yaw = float(np.arctan2(T4[1, 0], T4[0, 0]))
        tr = synth.Trajectory(p0=tuple(pos), t_static=100.0, heading=yaw, sway=0.0, yaw_amp=0.0, pitch_amp=0.0, roll_amp=0.0)
        imu = synth.imu_stream(tr, 0.0, 0.1 * n + 0.2, rate=100.0, seed=5, gyr_sigma=1e-3, acc_sigma=1e-2)
        ii, poses = 0, []
        for k in range(n):
            tb = k * 0.1
            rows = []
            while ii < len(imu) and imu[ii][0] <= tb:
                t, gy, ac = imu[ii]
                rows.append([t * 1e6, *(gy * 180.0 / np.pi), *(ac / 9.81)])
                ii += 1
            pts, st = synth.make_sweep(scene, tr, tb, seed=500 + k, n_az=900, fov_deg=(-24.8, 2.0))
            attr = dict(timestamp=int(round(tb * 1e6)), points_attr=np.stack([st.astype(np.float32), np.zeros(len(st), np.float32)], 1))
            out = sw.process({"0-lidar": pts}, {"0-lidar": attr}, {}, {}, {}, {}, np.array(rows, np.float64).reshape(-1, 7), int(round(tb * 1e6)))
            if k == 0:
                sw.set_init_pose(pos[0] + 0.2, pos[1] - 0.15, pos[2], np.degrees(yaw) + 1.0, 0.0, 0.0)
            poses.append(out["pose"])
        return poses
    finally:
        sw.deinit_slam()


def test_localisation_reports_the_inverse_projection_of_its_pose(tmp_path):
    import slam_wrapper as sw

    scene = MC.scene()
    root, bare = str(tmp_path / "map"), str(tmp_path / "bare")
    MC.start_mapping(sw)  # (sets MC.ORIGIN)
    try:
        held = dict(points={}, poses={}, stamps={})
        MC.push(sw, MC.keyframes(scene), held)
        MC.save_map(sw, root, held)
    finally:
        sw.deinit_slam()
    shutil.copytree(root, bare)
    np.savetxt(os.path.join(bare, "graph", "map_info.txt"), np.zeros((1, 7)), fmt="%1.10f")  # the same map without an origin
    poses = _localise(sw, root, scene)
    assert poses[0]["state"] == "Initializing" and poses[-1]["state"] == "Localizing(L)"
    proj = R.UtmRef()
    origin = np.loadtxt(os.path.join(root, "graph", "map_info.txt")).reshape(-1)
    zx, zy = proj.forward(origin[0], origin[1])
    n_checked = 0
    for p in poses:
        if p["state"] != "Localizing(L)":  # not inited: zeros, origin or not
            assert (p["latitude"], p["longitude"], p["altitude"]) == (0.0, 0.0, 0.0)
            continue
        M = p["odom_matrix"].astype(np.float64)  # (the f32 the pose goes out in: 1e-6 m of 10 m, 1e-11 degrees)
        lat, lon = proj.inverse(zx + M[0, 3], zy + M[1, 3])
        assert abs(p["latitude"] - lat) <= 1e-9 and abs(p["longitude"] - lon) <= 1e-9 and abs(p["altitude"] - (origin[2] + M[2, 3])) <= 1e-5
        assert abs(p["latitude"] - MC.ORIGIN[0]) < 1e-3 and abs(p["longitude"] - MC.ORIGIN[1]) < 1e-3
        n_checked += 1
    assert n_checked >= 1
    poses = _localise(sw, bare, scene)
    assert poses[-1]["state"] == "Localizing(L)" and all((p["latitude"], p["longitude"], p["altitude"]) == (0.0, 0.0, 0.0) for p in poses)
