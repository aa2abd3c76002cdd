"""The numpy restatement behind tests/test_overlap_*.py: OverlapDetector of the reference's map merge (slam/localization/include/overlap_merge.hpp,
"OM") by the rules include/lio_hip.h states -- get_connection_count (OM:265-296), find_candidates (OM:113-145), the range-gated
calc_fitness_score (OM:225-263), matching (OM:147-211) and detect (OM:63-110) over a fragment.  The alignments come from oracle/gicp.py's
Vgicp / Gicp (pinned to the reference) with their brute-force neighbour searches replaced by a k-d tree that only SELECTS what the f32 rule
then ranks.  A seeded two-map scene at the size of gicp_cases, and a writer of map directories.  Nothing here calls the library under test."""
import os
import sys
from collections import deque

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

import keyframe_cases as KC  # noqa: E402
import loop_cases as LC  # noqa: E402

DBL_MAX = LC.DBL_MAX
F32 = np.float32

DEFAULTS = dict(distance_thresh=30.0, candidate_link_dist=10, max_candidate_num=3, knn=10, fitness_score_max_range=25.0, fitness_score_thresh=1.5,
                fitness_inlier_thresh=0.2, gate_max_range=1.0, xy_range=100.0, min_z=0.5, fine_max_corr_dist=0.5, fine_translation_epsilon=0.001)


# ---- get_connection_count (OM:265-296) ------------------------------------------------------------------------------------------------------
def connection_map(edges):
    m = {}
    for a, b in edges:
        m.setdefault(int(a), set()).add(int(b))
        m.setdefault(int(b), set()).add(int(a))
    return m


def connection_count(conn, source, target, max_count):
    """levels of the breadth-first walk from source until target is popped; visited is set at the pop, so a node can be queued twice"""
    count = 0
    visited = set()
    q = deque([source])
    while q:
        for _ in range(len(q)):
            curr = q.popleft()
            if curr == target:
                return count
            visited.add(curr)
            for adj in sorted(conn.get(curr, ())):
                if adj not in visited:
                    q.append(adj)
        count += 1
        if max_count > 0 and count >= max_count:
            break
    return count


# ---- find_candidates (OM:113-145) -----------------------------------------------------------------------------------------------------------
def find_candidates(pos_xyz, ids, conn, new_id, new_xyz, p=DEFAULTS, distances=None):
    """indices into the key frames in the order they are accepted; `distances` (a list) receives the f32 d2 of every accepted one"""
    pos = np.asarray(pos_xyz, np.float64).reshape(-1, 3).astype(F32)
    if len(pos) == 0:
        return []
    d2 = KC.d2_f32(np.asarray(new_xyz, np.float64).astype(F32), pos)
    order = np.lexsort((np.arange(len(pos)), d2))[:p["knn"]]  # rising distance, equal distances to the smaller index
    out = []
    for i in order:
        if int(ids[i]) == new_id:
            continue
        if int(ids[i]) in conn.get(new_id, ()):
            continue
        if np.float64(d2[i]) < p["distance_thresh"] * p["distance_thresh"]:
            if connection_count(conn, new_id, int(ids[i]), p["candidate_link_dist"]) >= p["candidate_link_dist"]:
                out.append(int(i))
                if distances is not None:
                    distances.append(float(d2[i]))
        if len(out) >= p["max_candidate_num"]:
            break
    return out


# ---- calc_fitness_score (OM:225-263) --------------------------------------------------------------------------------------------------------
def range_filter(xyzi, xy_range=100.0, min_z=0.5):
    """filter() (OM:213-217): f32 sqrt((x*x) + (y*y)) < f32(xy_range) and z > f32(min_z), both strict; rows that are not finite do not pass"""
    p = np.ascontiguousarray(xyzi, F32).reshape(-1, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        dist = np.sqrt((p[:, 0] * p[:, 0]) + (p[:, 1] * p[:, 1]))
        return np.isfinite(p[:, :3]).all(1) & (dist < F32(xy_range)) & (p[:, 2] > F32(min_z))


def gated_fitness(target, source, T, max_range, p=DEFAULTS):
    """(score, nr, n_in): both clouds range-filtered, the source after T.cast<float>(); exact nearest by the f32 d2, d2 <= max_range"""
    tgt = np.ascontiguousarray(target, F32).reshape(-1, 4)
    tgt = tgt[range_filter(tgt, p["xy_range"], p["min_z"])]
    moved = KC.transform_f32(source, T)
    moved = moved[range_filter(moved, p["xy_range"], p["min_z"])]
    n_in = len(moved)
    if n_in == 0 or len(tgt) == 0:
        return DBL_MAX, 0, n_in
    d2 = KC.nearest_d2_gated(moved, tgt, max_range)
    inl = d2 <= F32(max_range) if max_range < 3e38 else np.isfinite(d2)
    nr = int(inl.sum())
    return (float(d2[inl].astype(np.float64).sum() / nr), nr, n_in) if nr else (DBL_MAX, 0, n_in)


# ---- poses ----------------------------------------------------------------------------------------------------------------------------------
def rel_pose(a, b):
    """a^-1 * b of two rigid transforms in f64: the inverse is R^T, -(R^T t); every sum of three products left to right"""
    a, b = np.asarray(a, np.float64).reshape(4, 4), np.asarray(b, np.float64).reshape(4, 4)
    out = np.eye(4)
    for i in range(3):
        ti = -((a[0, i] * a[0, 3] + a[1, i] * a[1, 3]) + a[2, i] * a[2, 3])
        for j in range(3):
            out[i, j] = (a[0, i] * b[0, j] + a[1, i] * b[1, j]) + a[2, i] * b[2, j]
        out[i, 3] = ((a[0, i] * b[0, 3] + a[1, i] * b[1, 3]) + a[2, i] * b[2, 3]) + ti
    return out


def make_guess(new_pose, cand_pose):
    """(new^-1 * candidate).cast<float>() as the f64 matrix align() casts it to; no renormalisation, no guess(2, 3) = 0"""
    return rel_pose(new_pose, cand_pose).astype(F32).astype(np.float64)


def inverse_f32(T):
    """Isometry3f(T).inverse(): R^T, -(R^T t) in f32"""
    M = np.asarray(T, F32).reshape(4, 4)
    out = np.eye(4, dtype=F32)
    for r in range(3):
        for c in range(3):
            out[r, c] = M[c, r]
        out[r, 3] = -((M[0, r] * M[0, 3] + M[1, r] * M[1, 3]) + M[2, r] * M[2, 3])
    return out


def accumulate(clouds, poses, best, neighbours):
    """OM:186-194: best's cloud, then every neighbour's moved by best^-1 * neighbour (Matrix4d rule), in the order given"""
    parts = [np.ascontiguousarray(clouds[best], F32).reshape(-1, 4)]
    for c in neighbours:
        parts.append(KC.transform_f64(clouds[c], rel_pose(poses[best], poses[c])))
    return np.ascontiguousarray(np.concatenate(parts), F32)


# ---- the matchers: oracle/gicp.py with a tree that selects and the f32 rule that ranks -----------------------------------------------------------
def _knn_tree(cloud, k):
    """oracle/gicp.py's knn(): the k nearest within the cloud by ascending (f32 d2, index); the tree hands over 2 k + 8 candidates"""
    from scipy.spatial import cKDTree

    c = np.asarray(cloud, F32)[:, :3]
    m = min(len(c), 2 * k + 8)
    _, cand = cKDTree(c.astype(np.float64)).query(c.astype(np.float64), m)
    cand = np.sort(cand.reshape(len(c), m), axis=1)
    e = c[cand] - c[:, None, :]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]  # candidates are in index order: stable = ties to the smaller index
    return np.take_along_axis(cand, order, axis=1)


def covariances(cloud, k=20):
    """oracle/gicp.py's covariances() over _knn_tree"""
    cloud = np.asarray(cloud, F32).reshape(-1, 4)
    nb = cloud[_knn_tree(cloud, k)][..., :3].astype(np.float64)
    nb = nb - nb.mean(axis=1, keepdims=True)
    cov = np.einsum("nka,nkb->nab", nb, nb) / k
    U, _, Vt = np.linalg.svd(cov)
    return U @ np.diag([1.0, 1.0, 1e-3]) @ Vt


def _matchers():
    import gicp as OG
    from scipy.spatial import cKDTree

    class FastCov:
        def set_target(self, xyzi):
            self.tgt = np.asarray(xyzi, F32).reshape(-1, 4)
            self.cov_tgt = covariances(self.tgt, self.k)
            self.voxels = None
            self._tree = None
            return self.cov_tgt

        def set_source(self, xyzi):
            self.src = np.asarray(xyzi, F32).reshape(-1, 4)
            self.cov_src = covariances(self.src, self.k)
            return self.cov_src

    class Vgicp(FastCov, OG.Vgicp):
        pass

    class Gicp(FastCov, OG.Gicp):
        def linearize(self, T):  # update_correspondences with the tree selecting inside max_corr_dist + 1 %
            T = np.asarray(T, np.float64)
            if getattr(self, "_tree", None) is None:
                self._tree = cKDTree(self.tgt[:, :3].astype(np.float64))
            q = OG.transform_f(T, self.src)
            thr = F32(self.maxd) * F32(self.maxd)
            near = self._tree.query_ball_point(q.astype(np.float64), self.maxd * 1.01)
            corr = np.full(len(q), -1, np.int32)
            sq = np.full(len(q), np.inf, F32)
            for i, c in enumerate(near):
                if c:
                    c = np.sort(np.asarray(c))
                    e = self.tgt[c, :3] - q[i]
                    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
                    j = int(np.argmin(d2))  # the first minimum: ties to the smaller index
                    sq[i] = d2[j]
                    if d2[j] < thr:
                        corr[i] = c[j]
            maha = np.zeros((len(q), 3, 3))
            R = T[:3, :3]
            on = np.nonzero(corr >= 0)[0]
            if len(on):
                maha[on] = np.linalg.inv(self.cov_tgt[corr[on]] + R @ self.cov_src[on] @ R.T)
            self.corr, self.sq, self.maha = corr, sq, maha
            return OG.cost(self.src, self.tgt, corr, maha, T, True)

    return Vgicp, Gicp


class OracleMatchers:
    """coarse(target, source, guess) / fine(target, source, guess) -> (T f32 4 x 4, iterations, converged)"""

    def __init__(self, p=DEFAULTS):
        self.p = p
        self.Vgicp, self.Gicp = _matchers()
        self.memo = {}  # the scene's restatements ask for the same alignments more than once

    def _memo(self, kind, target, source, guess, run):
        key = (kind, hash(np.ascontiguousarray(target, F32).tobytes()), hash(np.ascontiguousarray(source, F32).tobytes()), np.asarray(guess, F32).tobytes())
        if key not in self.memo:
            self.memo[key] = run(target, source, guess)
        T, it, conv = self.memo[key]
        return np.array(T), it, conv

    def coarse(self, target, source, guess):
        return self._memo("coarse", target, source, guess, self._coarse)

    def fine(self, target, source, guess):
        return self._memo("fine", target, source, guess, self._fine)

    def _coarse(self, target, source, guess):
        m = self.Vgicp(k=20, resolution=1.0, search_method=1, transformation_epsilon=0.1, rotation_epsilon=0.1, max_iterations=64)
        m.set_target(target)
        m.set_source(source)
        try:
            return m.align(guess)
        except np.linalg.LinAlgError:  # H = 0: the device's ldlt_solve6 ends not converged (include/lio_hip.h)
            return np.asarray(guess, F32), 0, False

    def _fine(self, target, source, guess):
        m = self.Gicp(k=20, max_corr_dist=self.p["fine_max_corr_dist"], transformation_epsilon=self.p["fine_translation_epsilon"], rotation_epsilon=1e-2, max_iterations=64)
        m.set_target(target)
        m.set_source(source)
        return m.align(guess)


_shared = {}


def shared_matchers(p=DEFAULTS):
    key = tuple(sorted(p.items()))
    if key not in _shared:
        _shared[key] = OracleMatchers(p)
    return _shared[key]


# ---- matching (OM:147-211) and detect (OM:63-110) --------------------------------------------------------------------------------------------
REASONS = ("found", "no_candidate", "gate", "coarse", "fine_not_converged", "fine_score")


def matching(clouds, poses, ref_ids, conn, cand, new, matchers, p=DEFAULTS):
    """clouds / poses by key-frame id; cand: key-frame ids -> the record of one new frame"""
    rec = dict(new_id=new, candidates=list(cand), gate=[], ratio=[], T=[], iterations=[], converged=[], score=[], best=-1, best_score=DBL_MAX, neighbours=[],
               skipped=0, fine=None, fine_score=DBL_MAX, edge=None, reason="no_candidate")
    if not cand:
        return rec
    rec["reason"] = "gate"
    best, best_score, best_T = -1, DBL_MAX, None
    for k, c in enumerate(cand):
        guess = make_guess(poses[new], poses[c])
        s, nr, n_in = gated_fitness(clouds[new], clouds[c], guess, p["gate_max_range"], p)
        ratio = nr / n_in if nr else 0.0
        rec["gate"].append((s, nr, n_in)); rec["ratio"].append(ratio)
        rec["T"].append(None); rec["iterations"].append(0); rec["converged"].append(False); rec["score"].append(DBL_MAX)
        if ratio < p["fitness_inlier_thresh"]:
            continue
        if rec["reason"] == "gate":
            rec["reason"] = "coarse"
        T, it, conv = matchers.coarse(clouds[new], clouds[c], guess.astype(F32))
        rec["T"][k], rec["iterations"][k], rec["converged"][k] = np.asarray(T, F32), int(it), bool(conv)
        if not conv:
            continue
        score, _ = LC.fitness(clouds[new], clouds[c], T, p["fitness_score_max_range"])
        rec["score"][k] = score
        if score > best_score:
            continue
        best, best_score, best_T = k, score, np.asarray(T, F32)
    rec["best"], rec["best_score"] = best, best_score
    if best < 0:
        return rec
    ref = set(ref_ids)
    for c in sorted(conn.get(cand[best], ())):  # std::set order
        if c in ref:
            rec["neighbours"].append(c)
        else:
            rec["skipped"] += 1  # OM:189 would take frame 0 (the deviation include/lio_hip.h states)
    acc = accumulate(clouds, poses, cand[best], rec["neighbours"])
    T, it, conv = matchers.fine(acc, clouds[new], inverse_f32(best_T))
    rec["fine"] = (np.asarray(T, F32), int(it), bool(conv))
    if not conv:
        rec["reason"] = "fine_not_converged"
        return rec
    s, _, _ = gated_fitness(acc, clouds[new], T, p["fitness_score_max_range"], p)
    rec["fine_score"] = s
    if s > p["fitness_score_thresh"]:
        rec["reason"] = "fine_score"
        return rec
    rec["reason"] = "found"
    rec["edge"] = dict(key1=cand[best], key2=new, relative_pose=np.asarray(T, F32), score=s, information=LC.information_matrix(s))
    return rec


def detect(clouds, poses, ref_ids, new_ids, edges, matchers=None, p=DEFAULTS):
    """one detect() call: -> (overlap edges, the record of every new frame); the distances of the accepted candidates ride in rec["cand_d2"]"""
    matchers = matchers or shared_matchers(p)
    conn = connection_map(edges)
    pos = [np.asarray(poses[k], np.float64)[:3, 3] for k in ref_ids]
    out, recs = [], []
    for new in new_ids:
        d2 = []
        idx = find_candidates(pos, ref_ids, conn, new, np.asarray(poses[new], np.float64)[:3, 3], p, d2)
        rec = matching(clouds, poses, ref_ids, conn, [ref_ids[i] for i in idx], new, matchers, p)
        rec["cand_d2"] = d2
        recs.append(rec)
        if rec["edge"] is not None:
            out.append(rec["edge"])
    return out, recs


# ---- the two-map scene ------------------------------------------------------------------------------------------------------------------------
SCENE_SEED = 31
N_REF, N_NEW = 14, 12


def two_maps(seed=SCENE_SEED):
    """A reference map of N_REF key frames (ids 0 ..) driven along x, and a new map of N_NEW key frames (ids 100 ..) over the same scene that runs
    beside it for about half its length and then turns away.  -> dict: clouds / poses (estimates) / truth by key-frame id, ref_ids, new_ids,
    edges (both chains).  The reference map's estimates are the truth; the new map's are the truth perturbed by up to 0.3 m / 1 degree.
    In a 12-chain only frames 0-2 and 9-11 are 10 levels deep (connection_count), so only they can have candidates."""
    from lsd_amd import synth

    sc = synth.Scene(half=25.0, n_boxes=12, seed=seed)
    rng = np.random.default_rng(seed + 1)
    clouds, poses, truth = {}, {}, {}
    ref_ids, new_ids = list(range(N_REF)), list(range(100, 100 + N_NEW))
    for k in ref_ids:
        T = LC._pose(-9.0 + 1.4 * k, -2.0 + 0.1 * k, 0.05 * np.sin(0.5 * k))
        clouds[k], poses[k], truth[k] = LC._scan(sc, T, seed + 100 + k), T, T
    for j, k in enumerate(new_ids):
        # frames 0-2 run beside the reference drive; the chain then leaves it in y and comes back for frames 9 and 10; the last frame looks at the
        # scene from a far corner, where the gate refuses every candidate
        y = 0.8 + (0.0 if j < 3 else 2.5 * min(j - 2, 3) if j < 9 else 2.5 - 1.3 * (j - 9))
        T = LC._pose(-7.5 + 1.5 * j, y, 0.1 + 0.03 * j) if j < 11 else LC._pose(23.0, 20.0, 3.0)
        d = rng.uniform(-1, 1, 3)
        drift = LC._pose(0.3 * d[0] * 0.7, 0.3 * d[1] * 0.7, np.radians(1.0) * d[2], z=0.0)
        clouds[k], truth[k], poses[k] = LC._scan(sc, T, seed + 300 + j), T, T @ drift
    edges = [(a, a + 1) for a in ref_ids[:-1]] + [(a, a + 1) for a in new_ids[:-1]]
    return dict(clouds=clouds, poses=poses, truth=truth, ref_ids=ref_ids, new_ids=new_ids, edges=edges)


def fixture_conditions(recs, p=DEFAULTS, content=True):
    """what the scene must keep clear of so that no rounding on the device can flip a decision, and (content) what it must contain; returns the
    list of violations"""
    bad = []
    kinds = set()
    for r in recs:
        kinds.add(r["reason"])
        for ratio in r["ratio"]:
            if abs(ratio - p["fitness_inlier_thresh"]) < 0.02:
                bad.append(f"frame {r['new_id']}: gate ratio {ratio} within 0.02 of the threshold")
        if r["fine_score"] != DBL_MAX and abs(r["fine_score"] - p["fitness_score_thresh"]) < 0.05 * p["fitness_score_thresh"]:
            bad.append(f"frame {r['new_id']}: final score {r['fine_score']} within 5 % of the threshold")
        d = np.sqrt(np.asarray(r["cand_d2"], np.float64))
        if len(d) and (np.abs(d - p["distance_thresh"]) < 1e-3).any():
            bad.append(f"frame {r['new_id']}: a candidate within 1e-3 m of distance_thresh")
        if len(d) > 1 and (np.diff(np.sort(d)) < 1e-3).any():
            bad.append(f"frame {r['new_id']}: two candidates within 1e-3 m of each other")
        s = sorted(x for x in r["score"] if x != DBL_MAX)
        if any(b - a <= 1e-6 * b for a, b in zip(s, s[1:])):
            bad.append(f"frame {r['new_id']}: two coarse scores within 1e-6 relative")
    if not content:
        return bad
    if "no_candidate" not in kinds or not any(len(r["candidates"]) for r in recs):
        bad.append("the scene needs frames with and without candidates")
    if not any(ratio < p["fitness_inlier_thresh"] for r in recs for ratio in r["ratio"]):
        bad.append("the scene needs a pair the gate refuses")
    if "found" not in kinds:
        bad.append("the scene needs a found overlap")
    return bad


_scene_cache = {}


def scene_restatement(seed=SCENE_SEED):
    """(scene, edges, records) of the restatement on the two-map scene, computed once per process"""
    if seed not in _scene_cache:
        sc = two_maps(seed)
        out, recs = detect(sc["clouds"], sc["poses"], sc["ref_ids"], sc["new_ids"], sc["edges"])
        _scene_cache[seed] = (sc, out, recs)
    return _scene_cache[seed]


# ---- maps on disk, and the merge (MapLoader::mergeMapSLAM, map_loader.cpp:82-169) ------------------------------------------------------------
ORIGIN = (31.2, 121.5, 4.0, 10.0, 0.0, 0.0)
ODOM_INFO = np.diag([400.0, 400.0, 400.0, 2500.0, 2500.0, 2500.0])  # the odometry edges of the written graphs: 5 cm, about 1 degree


def scene_graphs(sc):
    """the two graphs of the scene as they go to disk: (vertices {id: pose}, edges [(a, b, M, info)], fixed ids) per map, in each map's own
    ids (the new map counts from 0).  The reference map is consistent and its frame 0 fixed; the new map's vertices (and key frames) carry the
    perturbed estimates while its odometry edges measured the true motion, as a map does that was never optimised"""
    import graph_cases as GC

    ref = ({k: sc["poses"][k] for k in sc["ref_ids"]},
           [(a, a + 1, GC.inv_T(sc["truth"][a]) @ sc["truth"][a + 1], ODOM_INFO) for a in sc["ref_ids"][:-1]], [sc["ref_ids"][0]])
    own = {k: j for j, k in enumerate(sc["new_ids"])}
    new = ({own[k]: sc["poses"][k] for k in sc["new_ids"]},
           [(own[a], own[a] + 1, GC.inv_T(sc["truth"][a]) @ sc["truth"][a + 1], ODOM_INFO) for a in sc["new_ids"][:-1]], [])
    return ref, new, own


def write_map(path, clouds, vertices, edges, fixed, origin=ORIGIN, coordinate=0, extra_lines=(), stamp0=1_700_000_000):
    """a map directory as the reference saves it: graph/map_info.txt, graph/graph.g2o, graph/<id>/{data, cloud.pcd}; clouds / vertices by id"""
    import graph_cases as GC

    g = os.path.join(path, "graph")
    os.makedirs(g, exist_ok=True)
    if origin is not None:
        with open(os.path.join(g, "map_info.txt"), "w") as f:
            f.write(" ".join(repr(float(v)) for v in origin) + f" {int(coordinate)}\n")
    r = lambda v: " ".join(repr(float(x)) for x in v)
    with open(os.path.join(g, "graph.g2o"), "w") as f:
        for k in sorted(vertices):
            t, q = GC.T_to_tq(vertices[k])
            f.write(f"VERTEX_SE3:QUAT {k} {r(t)} {r(q)}\n")
        for k in fixed:
            f.write(f"FIX {k}\n")
        for line in extra_lines:
            f.write(line + "\n")
        for a, b, M, info in edges:
            t, q = GC.T_to_tq(M)
            f.write(f"EDGE_SE3:QUAT {a} {b} {r(t)} {r(q)} {r([info[i, j] for i in range(6) for j in range(i, 6)])}\n")
    for k in sorted(clouds):
        d = os.path.join(g, f"{k:06d}")
        os.makedirs(d, exist_ok=True)
        T = np.asarray(vertices[k], np.float64)
        rows = "\n".join(r(T[i]) for i in range(4))
        with open(os.path.join(d, "data"), "w") as f:
            f.write(f"stamp {stamp0 + k} 0\nestimate\n{rows}\nodom \n{rows}\nid {k}\n")
        pts = np.ascontiguousarray(clouds[k], F32).reshape(-1, 4)
        with open(os.path.join(d, "cloud.pcd"), "wb") as f:
            f.write((f"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH {len(pts)}\n"
                     f"HEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(pts)}\nDATA binary\n").encode())
            f.write(pts.tobytes())


def write_scene(root, sc, **over):
    """the scene's two maps under root/ref and root/new (keyword arguments reach the NEW map's write_map) -> (ref path, new path)"""
    ref, new, own = scene_graphs(sc)
    write_map(os.path.join(root, "ref"), {k: sc["clouds"][k] for k in sc["ref_ids"]}, *ref)
    write_map(os.path.join(root, "new"), {own[k]: sc["clouds"][k] for k in sc["new_ids"]}, *new, **over)
    return os.path.join(root, "ref"), os.path.join(root, "new")


def merge(sc, matchers=None, p=DEFAULTS, fragment=10):
    """mergeMapSLAM over the scene: graph_merge (new ids max + 1 ... in key-frame order), then per fragment of 10 new frames detect, the overlaps
    as edges key1 -> key2 with information(score) and Huber 1.0, graph_optimize(1024), the poses back; a last optimise.
    -> dict: new_ids (in the merged map), overlaps [(key1, key2)], records, poses {merged id: pose} after the merge"""
    import graph_cases as GC

    matchers = matchers or shared_matchers(p)
    ref, new, own = scene_graphs(sc)
    G, node = GC.Graph(), {}
    poses, clouds = {}, {}
    for k in sc["ref_ids"]:
        node[k] = G.add_node(ref[0][k], fixed=k in ref[2])
        poses[k], clouds[k] = np.array(ref[0][k], np.float64), sc["clouds"][k]
    edges = []
    for a, b, M, info in ref[1]:
        G.add_edge(node[a], node[b], M, info)
        edges.append((a, b))
    top = max(sc["ref_ids"])
    ids = {own[k]: top + 1 + j for j, k in enumerate(sc["new_ids"])}  # file id -> merged id, in key-frame order
    scene_of = {ids[own[k]]: k for k in sc["new_ids"]}
    for f in sorted(ids):
        node[ids[f]] = G.add_node(new[0][f], fixed=f in new[2])
        poses[ids[f]], clouds[ids[f]] = np.array(new[0][f], np.float64), sc["clouds"][scene_of[ids[f]]]
    for a, b, M, info in new[1]:
        G.add_edge(node[ids[a]], node[ids[b]], M, info)
        edges.append((ids[a], ids[b]))
    new_ids = [ids[f] for f in sorted(ids)]
    overlaps, records = [], []

    def sync():
        G.optimize(1024)
        est = G.estimates()
        for k in poses:
            poses[k] = est[node[k]]

    for i in range(len(new_ids) // fragment + 1):
        out, recs = detect(clouds, poses, sc["ref_ids"], new_ids[i * fragment:(i + 1) * fragment], edges, matchers, p)
        records += recs
        for e in out:
            G.add_edge(node[e["key1"]], node[e["key2"]], e["relative_pose"].astype(np.float64), e["information"], GC.HUBER, 1.0)
            edges.append((e["key1"], e["key2"]))
            overlaps.append((e["key1"], e["key2"]))
        sync()
    sync()
    return dict(new_ids=new_ids, overlaps=overlaps, records=records, poses=poses, scene_of=scene_of)


def scene_merge(seed=SCENE_SEED):
    """(scene, merge()) computed once per process"""
    key = ("merge", seed)
    if key not in _scene_cache:
        sc = scene_restatement(seed)[0]
        _scene_cache[key] = (sc, merge(sc))
    return _scene_cache[key]
