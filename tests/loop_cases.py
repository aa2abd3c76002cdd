"""The numpy restatement behind tests/test_loop_*.py and tools/record_loop_golden.py: hdl_graph_slam::LoopDetector
(slam/backend/hdl_graph_slam/include/hdl_graph_slam/loop_detector.hpp, "LD") by the rules include/lio_hip.h states -- find_candidates
(LD:106-140), detect's gate (LD:69-93), matching's guess, selection and thresholds (LD:148-219), pcl::Registration::getFitnessScore under the
project's f32 distance rule, InformationMatrixCalculator::weight.  The alignments themselves come from a pluggable matcher pair: oracle/gicp.py's
Vgicp / Gicp by default (pinned to the reference), the reference's own RefVgicp / RefGicp in the recorder.  Seeded scenes at the size of
gicp_cases.  Nothing here calls the library under test."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

import gicp_cases  # noqa: E402
import keyframe_cases as KC  # noqa: E402

DBL_MAX = np.finfo(np.float64).max
F32 = np.float32

DEFAULTS = dict(distance_thresh=15.0, accum_distance_thresh=25.0, distance_from_last_edge_thresh=15.0, distance_new_keyframe_thresh=2.0,
                distance_keyframe_thresh=2.0, fitness_score_max_range=25.0, fitness_score_thresh=1.5, fine_max_corr_dist=0.5)


# ---- find_candidates (LD:106-140) ----------------------------------------------------------------------------------------------------------
def find_candidates(accum, pos_xy, new_accum, new_xy, last_edge_accum, p=DEFAULTS):
    if new_accum - last_edge_accum < p["distance_from_last_edge_thresh"]:
        return []
    out, last = [], -100.0
    for i in range(len(accum)):
        if new_accum - accum[i] < p["accum_distance_thresh"]:
            continue
        if (accum[i] - last) < p["distance_keyframe_thresh"]:
            continue
        d = np.asarray(pos_xy[i], np.float64) - np.asarray(new_xy, np.float64)
        if np.sqrt(d[0] * d[0] + d[1] * d[1]) > p["distance_thresh"]:
            continue
        last = accum[i]
        out.append(i)
    return out


# ---- information_matrix_calculator.{hpp,cpp} -------------------------------------------------------------------------------------------------
def weight(a, max_x, min_y, max_y, x):
    y = (1.0 - np.exp(-a * x)) / (1.0 - np.exp(-a * max_x))
    return min_y + (max_y - min_y) * y


def information_matrix(fitness):
    w_x = F32(weight(20.0, 0.5, 0.1 ** 2, 5.0 ** 2, fitness))  # the reference's float locals
    w_q = F32(weight(20.0, 0.5, 0.05 ** 2, 0.2 ** 2, fitness))
    inf = np.zeros((6, 6))
    inf[:3, :3] = np.eye(3) / np.float64(w_x)
    inf[3:, 3:] = np.eye(3) / np.float64(w_q)
    return inf


# ---- matching's guess (LD:168-173) ---------------------------------------------------------------------------------------------------------
def _renormalise(R):
    """Eigen::Quaterniond(R).normalized().toRotationMatrix()"""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(3)
    if tr > 0:
        t = np.sqrt(tr + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        q[:] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        w = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    n = np.sqrt(q @ q + w * w)
    w, (x, y, z) = w / n, q / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_guess(new_pose, cand_pose):
    """(new^-1 * candidate).cast<float>(), guess(2, 3) = 0; returned as the f64 matrix align() casts it to"""
    pn, pc = np.asarray(new_pose, np.float64).reshape(4, 4), np.asarray(cand_pose, np.float64).reshape(4, 4)
    Rn, Rc = _renormalise(pn[:3, :3]), _renormalise(pc[:3, :3])
    g = np.eye(4)
    g[:3, :3] = Rn.T @ Rc
    g[:3, 3] = Rn.T @ pc[:3, 3] - Rn.T @ pn[:3, 3]
    g = g.astype(F32)
    g[2, 3] = 0.0
    return g.astype(np.float64)


# ---- getFitnessScore (PCL 1.9.1 registration.hpp) under the project's f32 rule ---------------------------------------------------------------
def fitness(target, source, T, max_range=25.0):
    """(score, nr): source moved by T.cast<float>() (terms left to right), exact nearest target point by the f32 d2, d2 <= max_range"""
    return KC.fitness(np.ascontiguousarray(target, F32), np.ascontiguousarray(source, F32), np.asarray(T, np.float64), max_range, gated=False)


# ---- the matchers ----------------------------------------------------------------------------------------------------------------------------
class OracleMatchers:
    """coarse(target, source, guess) / fine(target, source, guess) -> (T f32 4 x 4, iterations, converged) with oracle/gicp.py"""

    def coarse(self, target, source, guess):
        import gicp as OG

        m = OG.Vgicp(k=20, resolution=1.0, search_method=1, transformation_epsilon=0.1, rotation_epsilon=0.1, max_iterations=64)
        m.set_target(target)
        m.set_source(source)
        return m.align(guess)

    def fine(self, target, source, guess, max_corr_dist=0.5):
        import gicp as OG

        m = OG.Gicp(k=20, max_corr_dist=max_corr_dist, transformation_epsilon=0.01, rotation_epsilon=1e-2, max_iterations=64)
        m.set_target(target)
        m.set_source(source)
        return m.align(guess)


# ---- matching (LD:148-219) and detect (LD:69-93) -------------------------------------------------------------------------------------------
def select(converged, scores):
    """(best index or -1, best_score): a candidate that did not converge is skipped; a candidate replaces the best unless score > best_score"""
    best, best_score = -1, DBL_MAX
    for k in range(len(scores)):
        if not converged[k]:
            continue
        if scores[k] > best_score:
            continue
        best, best_score = k, scores[k]
    return best, best_score


def matching(clouds, poses, new_id, cand, matchers, p=DEFAULTS):
    """-> dict: per candidate T / iterations / converged / score / nr, best, best_score, fine (T, iterations, converged, score, nr) or None, edge or None"""
    rec = dict(new_id=new_id, candidates=list(cand), T=[], iterations=[], converged=[], score=[], nr=[], best=-1, best_score=DBL_MAX, fine=None, edge=None)
    if not cand:
        return rec
    tgt = clouds[new_id]
    for c in cand:
        T, it, conv = matchers.coarse(tgt, clouds[c], make_guess(poses[new_id], poses[c]).astype(F32))
        s, nr = fitness(tgt, clouds[c], T, p["fitness_score_max_range"]) if conv else (DBL_MAX, 0)
        rec["T"].append(np.asarray(T, F32)); rec["iterations"].append(int(it)); rec["converged"].append(bool(conv)); rec["score"].append(s); rec["nr"].append(nr)
    best, best_score = select(rec["converged"], rec["score"])
    rec["best"], rec["best_score"] = best, best_score
    if best_score > 2.0 * p["fitness_score_thresh"]:
        return rec
    T, it, conv = matchers.fine(tgt, clouds[cand[best]], rec["T"][best], p["fine_max_corr_dist"])
    s, nr = fitness(tgt, clouds[cand[best]], T, p["fitness_score_max_range"])
    rec["fine"] = (np.asarray(T, F32), int(it), bool(conv), s, nr)
    if conv and not s > p["fitness_score_thresh"]:
        rec["edge"] = dict(key1=new_id, key2=cand[best], relative_pose=np.asarray(T, F32), score=s, information=information_matrix(s))
    return rec


class RefLoopDetector:
    """detect() over a queue of new frames, then the new frames join the key frames (hdl_graph_slam_nodelet.cpp:623)"""

    def __init__(self, matchers=None, **over):
        self.p = dict(DEFAULTS)
        self.p.update(over)
        self.m = matchers or OracleMatchers()
        self.reset()

    def reset(self):
        self.clouds, self.poses, self.accum = [], [], []
        self.n_keyframes, self.last_edge_accum = 0, 0.0
        self.edges, self.matchings = [], []

    def add_keyframe(self, cloud, pose, accum):
        self.clouds.append(np.ascontiguousarray(cloud, F32).reshape(-1, 4))
        self.poses.append(np.asarray(pose, np.float64).reshape(4, 4).copy())
        self.accum.append(float(accum))
        return len(self.clouds) - 1

    def detect(self):
        out, running = [], 0.0
        nk = self.n_keyframes
        for i in range(nk, len(self.clouds)):
            if (self.accum[i] - running) < self.p["distance_new_keyframe_thresh"]:
                continue
            running = self.accum[i]
            cand = find_candidates(self.accum[:nk], [q[:2, 3] for q in self.poses[:nk]], self.accum[i], self.poses[i][:2, 3], self.last_edge_accum, self.p)
            rec = matching(self.clouds, self.poses, i, cand, self.m, self.p)
            self.matchings.append(rec)
            if rec["edge"] is not None:
                self.last_edge_accum = self.accum[i]
                out.append(rec["edge"])
        self.n_keyframes = len(self.clouds)
        self.edges += out
        return out


# ---- seeded scenes ---------------------------------------------------------------------------------------------------------------------------
def _scan(scene, T, seed):
    from lsd_amd import synth

    R = T[:3, :3]
    # quaternion (x, y, z, w) of R through the rotation vector
    ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    rv = ax / (np.linalg.norm(ax) + 1e-300) * ang
    raw, _ = synth.make_scan(scene, T[:3, 3], synth.quat_from_rotvec(rv), seed=seed, n_az=300, n_beams=16, max_range=40.0)
    return gicp_cases._thin(raw[:, :4].astype(F32), 0.5)


def _pose(x, y, yaw, z=1.8):
    from lsd_amd import synth

    return gicp_cases._pose([x, y, z], synth.quat_from_rotvec([0, 0, yaw]))


FIVE_SEED = 11


def five_candidates(seed=FIVE_SEED):
    """one target and five candidates around it: (target cloud, [candidate clouds], [guesses f64 of f32])"""
    from lsd_amd import synth

    sc = synth.Scene(half=25.0, n_boxes=12, seed=seed)
    Tt = _pose(0.5, -1.0, 0.2)
    tgt = _scan(sc, Tt, seed + 10)
    offs = [(1.1, 0.6, 0.15), (-0.8, 0.9, -0.1), (0.4, -1.2, 0.25), (2.0, 1.5, 0.3), (-1.5, -0.5, -0.2)]
    rng = np.random.default_rng(seed + 20)
    cands, guesses = [], []
    for k, (dx, dy, dyaw) in enumerate(offs):
        Tc = _pose(0.5 + dx, -1.0 + dy, 0.2 + dyaw)
        cands.append(_scan(sc, Tc, seed + 30 + k))
        drift = _pose(*(rng.normal(size=2) * 0.15), rng.normal() * 0.02, z=0.0)
        guesses.append(make_guess(Tt, Tc @ drift))
    return tgt, cands, guesses


DRIVE_SEED = 21
DRIVE_FRAMES = 60


def drive(seed=DRIVE_SEED, n=DRIVE_FRAMES, radius=9.0, step=1.25):
    """a closed drive: n key frames `step` m apart on a circle of `radius` m (one lap = 2 pi radius), so that the start is revisited after about
    45 frames.  -> [(cloud, estimated pose, accumulated distance)]; the estimate is the true pose plus a drift that grows with the distance"""
    from lsd_amd import synth

    sc = synth.Scene(half=25.0, n_boxes=12, seed=seed)
    out = []
    for k in range(n):
        s = k * step
        a = s / radius
        T = _pose(radius * np.cos(a) - 2.0, radius * np.sin(a) + 1.0, a + np.pi / 2)
        drift = _pose(0.004 * s, -0.003 * s, 0.0004 * s, z=0.0)
        out.append((_scan(sc, T, seed + 100 + k), T @ drift, s))
    return out
