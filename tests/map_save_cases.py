"""Cases shared by tests/test_map_save_cpu.py and tests/test_map_save_gpu.py: the reference's align_pose restated in numpy, a seeded g2o record,
the seeded key frames of a short mapping session, and the calls map_manager.py's saving thread makes."""
import os

import numpy as np


# ---- align_pose (slam/src/graph_utils.cpp:230-282), statement for statement in f64 ------------------------------------------------------------
def _quat_of(R):
    """Eigen's Quaterniond(Matrix3d) -> (w, x, y, z)"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        r = np.sqrt(t + 1.0)
        k = 0.5 / r
        q[:] = [0.5 * r, (R[2, 1] - R[1, 2]) * k, (R[0, 2] - R[2, 0]) * k, (R[1, 0] - R[0, 1]) * k]
        return q
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    r = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    kk = 0.5 / r
    q[1 + i] = 0.5 * r
    q[0] = (R[k, j] - R[j, k]) * kk
    q[1 + j] = (R[j, i] + R[i, j]) * kk
    q[1 + k] = (R[k, i] + R[i, k]) * kk
    return q


def _R_of(w, x, y, z):
    """Eigen's Quaternion::toRotationMatrix"""
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def align_pose(stamp1, stamp2, estimate1, estimate2, poses_stamp, poses):
    poses = [np.array(p, np.float64).reshape(4, 4) for p in poses]
    if not poses:
        return []  # (the reference would read poses.back())
    stamps = np.asarray(poses_stamp, np.float64)
    for i in range(len(poses) - 1, -1, -1):  # from the back forward: poses[0] is the original until its own turn
        poses[i] = np.linalg.inv(poses[0]) @ poses[i]
    e1, e2 = np.array(estimate1, np.float64).reshape(4, 4), np.array(estimate2, np.float64).reshape(4, 4)
    dd = np.linalg.inv(poses[-1]) @ (np.linalg.inv(e1) @ e2)
    q = _quat_of(dd[:3, :3])
    # Eigen::AngleAxisd(q)
    n = np.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    angle, axis = 0.0, np.array([1.0, 0.0, 0.0])
    if n != 0.0:
        angle = 2.0 * np.arctan2(n, abs(q[0]))
        if q[0] < 0:
            n = -n
        axis = q[1:] / n
    duration = stamp2 - stamp1
    out = []
    for i, P in enumerate(poses):
        ratio = (stamps[i] - stamps[0]) / duration
        lt = ratio * dd[:3, 3]
        lr = ratio * (angle * axis)
        norm = np.float32(np.sqrt(lr[0] * lr[0] + lr[1] * lr[1] + lr[2] * lr[2]))  # `const float norm`
        plus = np.eye(4)
        if not (norm < 1e-8):
            a = float(norm)
            sh, w = np.sin(0.5 * a), np.cos(0.5 * a)
            plus[:3, :3] = _R_of(w, sh * (lr[0] / a), sh * (lr[1] / a), sh * (lr[2] / a))
        plus[:3, 3] = lt
        out.append(e1 @ (P @ plus))
    return out


def pose(x, y, z, rotvec=(0.0, 0.0, 0.0)):
    v = np.asarray(rotvec, np.float64)
    a = np.linalg.norm(v)
    T = np.eye(4)
    if a > 0:
        k = v / a
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    T[:3, 3] = [x, y, z]
    return T


def align_cases():
    """name -> (stamp1, stamp2, estimate1, estimate2, stamps, poses): translations stay below 30 m (the bound of the test is worked out for that)"""
    rng = np.random.default_rng(23)
    walk = [pose(10 + 2.0 * k + rng.normal(0, 0.1), -5 + 0.3 * k, 1.0 + 0.02 * k, [0.01 * k, -0.02 * k, 0.05 * k]) for k in range(5)]
    st = np.array([100.0, 100.1, 100.2, 100.3, 100.4])
    e1 = pose(3.0, 4.0, 0.5, [0.02, 0.01, 0.4])
    e2 = e1 @ np.linalg.inv(walk[0]) @ walk[-1] @ pose(0.3, -0.2, 0.05, [0.01, -0.02, 0.03])
    slide = [pose(1.0 + k, 2.0, 0.0) for k in range(4)]
    return {
        "walk_with_rotation": (100.0, 100.4, e1, e2, st, walk),
        "pure_translation": (0.0, 0.3, pose(5, 5, 0), pose(5, 5, 0) @ pose(3.4, 0.2, -0.1), np.array([0.0, 0.1, 0.2, 0.3]), slide),  # norm < 1e-8
        "one_pose": (7.0, 8.0, e1, e2, np.array([7.0]), [walk[2]]),
        "empty": (0.0, 1.0, e1, e2, np.zeros(0), []),
        "duration_is_not_the_span": (100.0, 100.9, e1, e2, st, walk),  # stamp2 - stamp1 = 0.9, the list spans 0.4
    }


# ---- a g2o record in the shape _read_g2o returns ------------------------------------------------------------------------------------------------
def g2o_record(seed=5):
    rng = np.random.default_rng(seed)

    def tq():
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        return np.concatenate([rng.uniform(-50, 50, 3), q])

    def spd(n):
        A = rng.normal(size=(n, n))
        W = A @ A.T + n * np.eye(n)
        return (W + W.T) / 2

    ids = [0, 1, 2, 3, 5, 8, 13, 21]
    vertices = {i: tq() for i in ids}
    pairs = [(1, 0), (2, 1), (3, 2), (5, 3), (8, 5), (13, 8), (21, 13), (21, 0), (13, 2)]
    edges = [(a, b, tq(), spd(6)) for a, b in pairs]

    def tri(W):
        return [W[r, c] for r in range(3) for c in range(r, 3)]

    priors = [("EDGE_SE3_PRIORXYZ", 3, np.array(list(rng.uniform(-50, 50, 3)) + tri(spd(3)))),
              ("EDGE_SE3_PRIORQUAT", 8, np.array(list(tq()[3:]) + tri(spd(3))))]
    kernels = [([21, 0], "Huber", 1.0), ([13, 2], "Huber", 1.0), ([3], "DCS2", 0.37)]
    return dict(vertices=vertices, edges=edges, fixed=[0, 13], priors=priors, kernels=kernels)


# ---- a short mapping session --------------------------------------------------------------------------------------------------------------------
N_KEYFRAMES = 8


def scene():
    """The seeded scene of the mapping session: a 30 m yard (ground, four 8 m walls, a few boxes outside the 20 m square the drive stays in).
    Its size follows from what the saved map has to be good for.  The localiser matches against NDT voxels of 1 m that need 7 points, and the
    session is 8 key frames of 2 200 points: 17 600 points fill 1 m voxels with 7 each on at most 2 500 m^2 of surface.  The yard has 900 m^2 of
    ground and 960 m^2 of wall.  In the 200 m scene of the other localisation tests (40 000 m^2 of ground alone) the same 17 600 points leave 8
    voxels above the ground with 7 points, so x and y are held by nothing; here 198 (filled_voxels below; asserted by the test that localises)."""
    from lsd_amd import synth

    return synth.Scene(half=15.0, n_boxes=8, seed=1, box_size=(1.5, 5.0), box_h=(2.0, 6.0), keep_clear=10.0)


def filled_voxels(frames, min_points=7):
    """the 1 m voxels of the frames' clouds in the map frame that hold min_points -> (all of them, those at z >= 1 m: walls and boxes)"""
    W = np.concatenate([pts[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3] for pts, T, _, _ in frames])
    v, c = np.unique(np.floor(W).astype(int), axis=0, return_counts=True)
    good = c >= min_points
    return int(good.sum()), int((good & (v[:, 2] >= 1)).sum())


def keyframe_pose(k):
    from lsd_amd import synth

    pos = np.array([-8.0 + 2.0 * k, 0.3 * np.sin(0.5 * k), 1.8])
    q = synth.quat_from_rotvec([0, 0, 0.05 * np.cos(0.3 * k)])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = synth.quat_to_R(q), pos
    return pos, q, T


def keyframes(scene, n=N_KEYFRAMES, seed0=400):
    """[(points N x 4 f32 with the intensity in [0, 1], pose 4 x 4 f64, stamp us, accumulated distance)]: 2 200 points each, every 2 m along x.
    A frame is a seeded uniform subsample (in scan order) of a 64 x 600 scan, not a coarser scan pattern: a pattern of 2 200 rays has its azimuth
    columns 5 degrees apart and samples a wall at 50 m every 4 m; the subsample keeps the scan's angular coverage."""
    from lsd_amd import synth

    out = []
    for k in range(n):
        pos, q, T = keyframe_pose(k)
        raw, _ = synth.make_scan(scene, pos, q, seed=seed0 + k, n_beams=64, n_az=600, fov_deg=(-24.8, 2.0))
        raw = raw[np.sort(np.random.default_rng(seed0 + k).choice(len(raw), 2200, replace=False))]
        pts = raw.copy()
        pts[:, 3] /= np.float32(255.0)
        out.append((pts, T, 1_000_000 + 100_000 * k, 2.0 * k))
    return out


ORIGIN = (31.2, 121.5, 4.0, 10.0, 0.0, 0.0)


def start_mapping(sw):
    assert sw.init_slam("mapping", "", "FastLIO", ["0-lidar", "IMU"], 0.5, 0.2, 10.0, 60.0) == ["IMU", "0-lidar"]
    sw.set_keyframe_output(True)
    sw.set_loop_detection(True)
    sw.set_pose_graph(True)
    sw.set_map_origin(*ORIGIN)


def push(sw, frames, held):
    """the key frames through _push_keyframe / update_odom; `held` collects what map_manager.py keeps (points, poses f32, stamps by str(id))"""
    for pts, T, stamp, accum in frames:
        sw._push_keyframe(pts, T, stamp, accum)
        d = sw.update_odom()
        assert len(d["keyframes"]) == 1
        kf = d["keyframes"][0]
        idx = str(len(held["stamps"]))
        held["points"][idx], held["poses"][idx], held["stamps"][idx] = kf["points"], kf["pose"], kf["stamp"]
        for i, P in d["odoms"].items():
            held["poses"][i] = np.asarray(P, np.float32)


def save_map(sw, root, held):
    """what MapManager.start_save_mapping and saving_thread_loop do (slam/map_manager.py:235-299) -> the ids dump_graph returned"""
    g = os.path.join(root, "graph")
    os.makedirs(g, exist_ok=True)
    np.savetxt(os.path.join(g, "map_info.txt"), sw.get_map_origin(), fmt="%1.10f")
    sw.dump_odometry(g)
    vertexes = sw.dump_graph(g)
    for idx, stamp in held["stamps"].items():
        if idx not in vertexes:
            continue
        d = os.path.join(g, "{0:06d}".format(int(idx)))
        os.makedirs(d, exist_ok=True)
        sw.dump_keyframe(d, stamp, int(idx), held["points"][idx], held["poses"][idx])
    return vertexes
