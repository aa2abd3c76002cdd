"""GNSS in localisation mode through the compiled module (set_gnss in localisation mode, csrc/slam_wrapper.cpp); the C entry points alone are
in tests/test_gnss_loc_gpu.py, which needs neither the module nor a map on disk.  Further down: merge_map across origins.  First the INS-aided
start and the fused fixes, on the 30-frame map and the forward drive of tests/test_relocalization_gpu.py (its helpers and its own bounds: 0.08 m median,
0.15 m maximum after the first second), the map given an origin.  Fixes come from the truth poses through rtk_cases.UtmRef's inverse, at
20 Hz: fix j at 50 000 j + 7 000 us, so frame k (stamp 100 000 k us) lies between fixes 2k - 1 and 2k.  The observation of every located frame
is compared with the restated bracket + interpolation (gnss_loc_cases.InsList) under tests/test_rtkm_module_gpu.py's tolerances for the same
interpolation, 1e-4 m and 1e-5 rad; measured maxima: printed by the test (both sides are f64 from the same statements)."""
import os

import numpy as np
import pytest

import gnss_loc_cases as G
import rtk_cases as R
import test_relocalization_gpu as TR

pytestmark = pytest.mark.gpu
LAT0, LON0, ALT0 = 31.2, 121.5, 4.0
POS_TOL, ROT_TOL = 1e-4, 1e-5
P0 = (-10.0, 0.2, 1.8)  # the forward drive of the relocalisation test: key frame 5 lies under it


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from lsd_amd import synth

    sw = TR._module()
    scene = synth.Scene(half=100.0, n_boxes=40, seed=1)
    root = str(tmp_path_factory.mktemp("gnss_loc") / "map")
    TR._write_map(sw, root, scene)
    with open(os.path.join(root, "graph", "map_info.txt"), "w") as f:
        f.write(f"{LAT0!r} {LON0!r} {ALT0!r} 0.0 0.0 0.0 0\n")
    kf_pos = np.array([[-20.0 + 2.0 * k, 0.3 * np.sin(0.5 * k), 1.8] for k in range(30)], np.float32)
    return sw, scene, root, kf_pos


def _projector():
    proj = R.UtmRef()
    x0, y0 = proj.forward(LAT0, LON0)
    return proj, (x0, y0, ALT0)


def _fix_at(tr, j, proj, zero, offset=(0.0, 0.0)):
    """fix j from the truth pose at its stamp: the place through the inverse projection, the heading from the pose's yaw"""
    stamp = 50_000 * j + 7_000
    p, Rm = tr.pos(stamp * 1e-6), tr.R(stamp * 1e-6)
    lat, lon = proj.inverse(zero[0] + p[0] + offset[0], zero[1] + p[1] + offset[1])
    yaw = np.degrees(np.arctan2(Rm[1, 0], Rm[0, 0]))
    heading = R.grid_convergence(proj.longitude0(), lat, lon) - yaw
    return R.fix(stamp, lat, lon, ALT0 + p[2], heading, 0.0, 0.0)


def _rtk(f, status=1):
    return dict(timestamp=int(f["stamp_us"]), latitude=f["latitude"], longitude=f["longitude"], altitude=f["altitude"], heading=f["heading"], pitch=f["pitch"],
                roll=f["roll"], gyro_x=0.0, gyro_y=0.0, gyro_z=0.0, acc_x=0.0, acc_y=0.0, acc_z=0.0, Ve=0.0, Vn=0.0, Vu=0.0, Status=status, Sensor="GNSS")


def _start(sw, root, gnss, sensors=("0-lidar", "RTK", "IMU"), ins_type="6D", precision=5.0):
    assert sw.init_slam("offline", root, "Localization", list(sensors), 0.2, 1.0, 10.0, 50.0) == list(sensors)
    sw.set_ins_external_param(0, 0, 0, 0, 0, 0)
    sw.set_imu_external_param(0, 0, 0, 0, 0, 0)
    sw.set_ins_config(dict(ins_type=ins_type, ins_normal=dict(use=True, status=1, stable_time=0.0, precision=precision),
                           ins_float=dict(use=False, status=2, stable_time=0.0, precision=1.0), ins_fix=dict(use=False, status=4, stable_time=0.0, precision=0.01)))
    sw.set_global_localization(True)
    assert sw._gnss_state()["enabled"] is False  # off by default in localisation mode
    sw.set_gnss(gnss)
    assert sw.setup_slam() is True


def _frame(sw, scene, tr, imu, state, k, rtk):
    from lsd_amd import synth

    tb = k * 0.1
    rows = []
    while state["ii"] < len(imu) and imu[state["ii"]][0] <= tb:
        t, g, a = imu[state["ii"]]
        rows.append([t * 1e6, *(g * 180.0 / np.pi), *(a / 9.81)])
        state["ii"] += 1
    pts, st = synth.make_sweep(scene, tr, tb, seed=500 + k, n_az=900, fov_deg=TR.FOV)
    attr = dict(timestamp=int(round(tb * 1e6)), points_attr=np.stack([st.astype(np.float32), np.zeros(len(st), np.float32)], 1))
    return sw.process({"0-lidar": pts}, {"0-lidar": attr}, {}, {}, {}, rtk, np.array(rows, np.float64).reshape(-1, 7), int(round(tb * 1e6)))


def _traj(n_frames):
    from lsd_amd import synth

    tr = synth.Trajectory(p0=P0, t_static=0.2, speed=4.0, heading=0.0, sway=0.3, yaw_amp=0.1)
    return tr, synth.imu_stream(tr, 0.0, 0.1 * n_frames + 0.3, rate=100.0, seed=5, gyr_sigma=1e-3, acc_sigma=1e-2)


def _rot_angle(A, B):
    M = A[:3, :3].T @ B[:3, :3]
    return float(np.arctan2(np.linalg.norm(M - M.T) / (2.0 * np.sqrt(2.0)), (np.trace(M) - 1.0) / 2.0))


def test_ins_aided_start_and_fused_drive(world):
    sw, scene, root, kf_pos = world
    proj, zero = _projector()
    tr, imu = _traj(31)
    _start(sw, root, True)
    invalid = {12, 20}  # frames whose call carries a fix that is not valid
    try:
        twin, state, errs, worst_p, worst_r, n_obs = G.InsList(), dict(ii=0), [], 0.0, 0.0, 0
        for k in range(1, 31):
            a, b = _fix_at(tr, 2 * k - 1, proj, zero), _fix_at(tr, 2 * k, proj, zero)
            sw._push_gnss(_rtk(a))
            rtk = _rtk(b) if k not in invalid else dict(timestamp=int(b["stamp_us"]), latitude=0.0, longitude=0.0, altitude=0.0, heading=0.0, pitch=0.0, roll=0.0, Status=0)
            fed = [a] if k in invalid else [a, b]
            if k > 1:  # frame 1 finds the localiser not initialised: its fixes go to the search, not to the list
                for f in fed:
                    twin.push(dict(stamp_us=f["stamp_us"], T=R.rtk_transform_utm(proj, f, zero), precision=5.0, dimension=6))
            out = _frame(sw, scene, tr, imu, state, k, rtk)
            M = out["pose"]["odom_matrix"]
            errs.append(float(np.linalg.norm(M[:3, 3] - tr.pos(k * 0.1))))
            gs = sw._gnss_state()
            if k == 1:
                r = sw._last_relocalization()
                print("first frame:", {n: v for n, v in r.items() if n != "guess"})
                ids, _ = G.nearest_ten(kf_pos, R.rtk_transform_utm(proj, b, zero)[:2, 3])
                assert r["kind"] == "local" and r["searched"] and r["accepted"] and r["match_id"] in ids.tolist() and 1 <= r["n_examined"] <= 10
                # dimension 6: the guess is the INS pose seen from the matched key frame, on the ground
                kf = np.eye(4, dtype=np.float32)
                from lsd_amd import synth
                kf[:3, :3] = synth.quat_to_R(synth.quat_from_rotvec([0, 0, 0.05 * np.cos(0.3 * r["match_id"])]))
                kf[:3, 3] = kf_pos[r["match_id"]]
                want = np.linalg.inv(kf.astype(np.float64)) @ R.rtk_transform_utm(proj, b, zero).astype(np.float32).astype(np.float64)
                want[2, 3] = 0.0
                assert np.abs(r["guess"] - want).max() < POS_TOL, np.abs(r["guess"] - want).max()
                assert gs["latest_held"] is False and gs["stamps"] == [] and not gs["observation"]["used"]  # the search consumed the fix
                assert np.linalg.norm(M[:3, 3] - tr.pos(0.1)) < 0.15
                continue
            want = twin.observe(100_000 * k)
            assert gs["stamps"] == twin.stamps(), k
            got = gs["observation"]
            assert got["used"] == (want is not None), k
            if want is not None:
                n_obs += 1
                assert (want["first"], want["second"]) == (a["stamp_us"], b["stamp_us"]) and k not in invalid  # (a frame beyond the last fix clears the list)
                assert got["precision"] == want["precision"] and got["dimension"] == want["dimension"] and got["ratio"] == want["ratio"]
                worst_p, worst_r = max(worst_p, np.abs(got["T"][:3, 3] - want["T"][:3, 3]).max()), max(worst_r, _rot_angle(got["T"], want["T"]))
            inited = out["pose"]["state"] != "Initializing"
            assert out["pose"]["state"] == ("Initializing" if not inited else "Localizing(L)" if k in invalid else "Localizing(L+G)"), (k, out["pose"]["state"])
            assert inited or k < 12, k  # ten located frames make the localisation stable
        print(f"{n_obs} observations against the restatement: worst {worst_p:.3e} m, {worst_r:.3e} rad; position error median {np.median(errs):.3f} m, "
              f"max after the first second {max(errs[10:]):.3f} m")
        assert n_obs == 27 and worst_p <= POS_TOL and worst_r <= ROT_TOL  # frames 2 .. 30 but the two whose second fix was not valid
        assert max(errs[10:]) < 0.15 and np.median(errs) < 0.08
        assert sw._last_relocalization()["searches"] == 1
    finally:
        sw.deinit_slam()


def test_a_fix_far_from_the_map_is_refused_without_a_global_search(world):
    sw, scene, root, _ = world
    proj, zero = _projector()
    tr, imu = _traj(2)
    _start(sw, root, True)
    try:
        out = _frame(sw, scene, tr, imu, dict(ii=0), 1, _rtk(_fix_at(tr, 2, proj, zero, offset=(10_000.0, 0.0))))
        r = sw._last_relocalization()
        assert out["pose"]["state"] == "Initializing" and np.array_equal(out["pose"]["odom_matrix"], np.eye(4, dtype=np.float32))
        assert r["kind"] == "local" and r["searched"] and r["match_id"] == -1 and r["n_examined"] == 0 and not r["accepted"] and r["searches"] == 1
    finally:
        sw.deinit_slam()


def test_a_two_dimensional_fix_starts_from_the_yaw_alone(world):
    sw, scene, root, kf_pos = world
    proj, zero = _projector()
    tr, imu = _traj(2)
    _start(sw, root, True, ins_type="2D")
    try:
        _frame(sw, scene, tr, imu, dict(ii=0), 1, _rtk(_fix_at(tr, 2, proj, zero)))
        r = sw._last_relocalization()
        c, s = np.cos(np.float32(-r["yaw"])), np.sin(np.float32(-r["yaw"]))
        assert r["kind"] == "local" and r["accepted"]
        assert np.array_equal(r["guess"], np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64))
    finally:
        sw.deinit_slam()


def _short_drive(sw, scene, with_fix, n=13):
    proj, zero = _projector()
    tr, imu = _traj(n + 1)
    state, poses, states = dict(ii=0), [], []
    for k in range(1, n + 1):
        out = _frame(sw, scene, tr, imu, state, k, _rtk(_fix_at(tr, 2 * k, proj, zero)) if with_fix else {})
        poses.append(out["pose"]["odom_matrix"].copy())
        states.append(out["pose"]["state"])
    return np.array(poses), states


def test_switch_off_and_rtk_not_a_sensor(world):
    sw, scene, root, _ = world
    runs = {}
    for name, gnss, sensors, with_fix in (("off_fix", False, ("0-lidar", "RTK", "IMU"), True), ("off_none", False, ("0-lidar", "RTK", "IMU"), False),
                                          ("on_no_rtk", True, ("0-lidar", "IMU"), True)):
        _start(sw, root, gnss, sensors)
        try:
            runs[name] = _short_drive(sw, scene, with_fix)
            r, gs = sw._last_relocalization(), sw._gnss_state()
            assert r["kind"] == "global" and r["searches"] == 1 and gs["stamps"] == [] and not gs["observation"]["used"], name
        finally:
            sw.deinit_slam()
    assert np.array_equal(runs["off_fix"][0].view(np.uint32), runs["off_none"][0].view(np.uint32))  # switch off: the fix is not looked at
    for name in runs:
        assert runs[name][1][-1] == "Localizing(L)" and "Localizing(L+G)" not in runs[name][1], name


# ---- merge_map across origins ---------------------------------------------------------------------------------------------------------------------
# tests/overlap_cases.py's scene_merge(): its new map written under origin B = A + (3e-4 deg, 4e-4 deg, 2 m), poses and a handful of XYZ priors
# expressed under B by the restatement.  A prior's measurement is the restated merge's own optimum for its vertex, so the priors pull nowhere and
# the final graph is want's up to the projector's inverse error (4.8e-5 m, tests/test_gnss_loc_cpu.py): the existing merge test's 1e-3 holds
PRIOR_INFO = (1.0, 0.0, 0.0, 1.0, 0.0, 1.0)


def _merge_world(root, under_b):
    import overlap_cases as OC

    sc, want = OC.scene_merge()
    ref, new, own = OC.scene_graphs(sc)
    A = OC.ORIGIN[:3]
    B = (A[0] + 3e-4, A[1] + 4e-4, A[2] + 2.0)
    file_ids = sorted(new[0])
    merged_of = dict(zip(file_ids, want["new_ids"]))
    prior_ids = file_ids[::3]
    prior_a = np.array([want["poses"][merged_of[f]][:3, 3] for f in prior_ids])
    poses = np.array([new[0][f] for f in file_ids])
    if under_b:
        poses, prior_xyz = G.update_origin(A, B, poses, prior_a)
    else:
        prior_xyz = prior_a
    r = lambda v: " ".join(repr(float(x)) for x in v)
    lines = [f"EDGE_SE3_PRIORXYZ {f} {r(prior_xyz[j])} {r(PRIOR_INFO)}" for j, f in enumerate(prior_ids)]
    OC.write_map(os.path.join(root, "ref"), {k: sc["clouds"][k] for k in sc["ref_ids"]}, *ref)
    new_path = os.path.join(root, "new")
    OC.write_map(new_path, {own[k]: sc["clouds"][k] for k in sc["new_ids"]}, dict(zip(file_ids, poses)), new[1], new[2],
                 origin=(B if under_b else A) + OC.ORIGIN[3:], extra_lines=lines)
    with open(os.path.join(new_path, "graph", "graph.g2o.kernels"), "w") as f:
        for p in prior_ids:
            f.write(f"1 {p} Huber 1.0\n")
    return dict(sc=sc, want=want, ref=os.path.join(root, "ref"), new=new_path, A=A, B=B, prior_ids=prior_ids, prior_xyz=prior_xyz, merged_of=merged_of)


def _loc(sw, ref_path, gnss):
    assert sw.init_slam("offline", ref_path, "Localization", ["0-lidar", "IMU"], 0.2, 1.0, 10.0, 50.0) == ["0-lidar", "IMU"]
    sw.set_ins_external_param(0, 0, 0, 0, 0, 0)
    sw.set_imu_external_param(0, 0, 0, 0, 0, 0)
    sw.set_gnss(gnss)
    assert sw.setup_slam() is True


def _check_merge(sw, w, got, rep):
    from lsd_amd import lio

    want, sc = w["want"], w["sc"]
    print(rep, "want", want["overlaps"])
    assert sorted(got["points"], key=int) == [str(k) for k in want["new_ids"]]
    assert [(a, b) for a, b, _ in rep["overlaps"]] == want["overlaps"] and rep["fragments"] == 2
    reasons = dict(rep["reasons"])
    assert [lio.OverlapDetector.REASONS[reasons[r["new_id"]]] for r in want["records"]] == [r["reason"] for r in want["records"]]
    worst = max(np.abs(got["poses"][str(k)].astype(np.float64) - want["poses"][k]).max() for k in want["new_ids"])
    print(f"merged poses against the restated merge: worst {worst:.3e}")
    assert worst < 1e-3


def test_merge_map_under_another_origin(tmp_path):
    sw = TR._module()
    w = _merge_world(str(tmp_path / "maps"), under_b=True)
    n = len(w["prior_ids"])
    assert n >= 3
    _loc(sw, w["ref"], False)
    try:
        assert sw.merge_map(w["new"]) == {}  # switch off: origins that differ are refused, as always
    finally:
        sw.deinit_slam()
    _loc(sw, w["ref"], True)
    try:
        origin = sw.get_map_origin().copy()
        got = sw.merge_map(w["new"])
        rep = sw._last_merge()
        _check_merge(sw, w, got, rep)
        assert rep["origin_updated"] is True and rep["priors"] == n and rep["skipped_tags"] == 0
        assert np.array_equal(sw.get_map_origin(), origin)  # the merged map keeps the loaded map's origin
        out = str(tmp_path / "dump")
        os.makedirs(out)
        sw.dump_graph(out)
        rec = sw._read_g2o(os.path.join(out, "graph.g2o"))
        _, back = G.update_origin(w["B"], w["A"], xyz=w["prior_xyz"])
        assert [(t, v) for t, v, _ in rec["priors"]] == [("EDGE_SE3_PRIORXYZ", w["merged_of"][f]) for f in w["prior_ids"]]
        err = max(np.abs(np.asarray(vals)[:3] - back[j]).max() for j, (_, _, vals) in enumerate(rec["priors"]))
        print(f"dumped prior measurements against the restated re-anchoring: worst {err:.3e} m")
        assert err <= 1e-6
        assert all(np.array_equal(np.asarray(vals)[3:], PRIOR_INFO) for _, _, vals in rec["priors"])
        single = [(v, t, d) for v, t, d in rec["kernels"] if len(v) == 1]
        assert single == [([w["merged_of"][f]], "Huber", 1.0) for f in w["prior_ids"]]
    finally:
        sw.deinit_slam()


def test_an_equal_origin_merge_carries_the_priors_under_the_switch_only(tmp_path):
    sw = TR._module()
    w = _merge_world(str(tmp_path / "maps"), under_b=False)
    n = len(w["prior_ids"])
    for gnss in (True, False):
        _loc(sw, w["ref"], gnss)
        try:
            got = sw.merge_map(w["new"])
            rep = sw._last_merge()
            _check_merge(sw, w, got, rep)
            assert rep["origin_updated"] is False
            assert (rep["priors"], rep["skipped_tags"]) == ((n, 0) if gnss else (0, n))  # off: passed over and counted, as before
            out = str(tmp_path / f"dump_{gnss}")
            os.makedirs(out)
            sw.dump_graph(out)
            assert len(sw._read_g2o(os.path.join(out, "graph.g2o"))["priors"]) == (n if gnss else 0)
        finally:
            sw.deinit_slam()
