"""The pose graph's rules (include/lio_hip.h, "The pose graph on the device") restated in f64 numpy, and the seeded graphs of the tests.

g2o is not in the reference tree, so the rules are restated from g2o's published source: toVectorMQT / fromVectorMQT
(types/slam3d/isometry3d_mappings), EdgeSE3's error, RobustKernelHuber, OptimizationAlgorithmLevenberg::solve.  The Jacobians are analytic
(checked here against central differences by tests/test_graph_cpu.py); the linear solve is numpy.linalg.solve on the dense damped system, or
-- to measure what an inexact solve costs -- the same block-Jacobi conjugate gradients the device runs.  Quaternions are (x, y, z, w)."""
import numpy as np

NONE, HUBER = 0, 1
MAX_TRIALS = 10


def q_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                     a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def q_conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def q_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def R_to_q(R):
    """Eigen's Quaternion(Matrix3), normalised"""
    q = np.zeros(4)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0)
        q[3] = 0.5 * s
        s = 0.5 / s
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * s, (R[0, 2] - R[2, 0]) * s, (R[1, 0] - R[0, 1]) * s
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * s
        s = 0.5 / s
        q[3] = (R[k, j] - R[j, k]) * s
        q[j] = (R[j, i] + R[i, j]) * s
        q[k] = (R[k, i] + R[i, k]) * s
    return q / np.linalg.norm(q)


def tq_to_T(t, q):
    T = np.eye(4)
    T[:3, :3] = q_to_R(q)
    T[:3, 3] = t
    return T


def T_to_tq(T):
    T = np.asarray(T, np.float64)
    return T[:3, 3].copy(), R_to_q(T[:3, :3])


def inv_T(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def from_mqt(v):
    """g2o's fromVectorMQT: w = sqrt(1 - |q|^2), the identity rotation when 1 - |q|^2 < 0"""
    v = np.asarray(v, np.float64)
    w2 = 1.0 - ((v[3] * v[3] + v[4] * v[4]) + v[5] * v[5])  # (this order: near a half turn w^2 is the difference's last bits)
    q = np.array([0.0, 0.0, 0.0, 1.0]) if w2 < 0 else np.array([v[3], v[4], v[5], np.sqrt(w2)])
    return tq_to_T(v[:3], q)


def to_mqt(T):
    t, q = T_to_tq(T)
    if q[3] < 0:
        q = -q
    return np.concatenate([t, q[:3]])


def edge_error_T(Xi, Xj, M):
    """the error through 4 x 4 matrices: toVectorMQT(M^-1 Xi^-1 Xj)"""
    return to_mqt(inv_T(M) @ inv_T(Xi) @ Xj)


def edge_eval(ti, qi, tj, qj, mt, mq):
    """the error through translation + quaternion (the state the graph keeps); also tb, qb of Xi^-1 Xj and the error quaternion (w >= 0)"""
    tb = q_to_R(qi).T @ (tj - ti)
    qb = q_mul(q_conj(qi), qj)
    te = q_to_R(mq).T @ (tb - mt)
    qe = q_mul(q_conj(mq), qb)
    qe = qe / np.linalg.norm(qe)
    if qe[3] < 0:
        qe = -qe
    return np.concatenate([te, qe[:3]]), tb, qb, qe


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def jacobians(ti, qi, tj, qj, mt, mq):
    """d e / d delta_i and d e / d delta_j at 0, X <- X fromVectorMQT(delta)"""
    _, tb, qb, qe = edge_eval(ti, qi, tj, qj, mt, mq)
    Ra = q_to_R(mq).T
    a = q_conj(mq)
    sgn = -1.0 if q_mul(a, qb) @ qe < 0 else 1.0
    L = (qb[3] * np.eye(3) - skew(qb[:3])) @ (a[3] * np.eye(3) + skew(a[:3])) - np.outer(qb[:3], a[:3])
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    Ji[:3, :3] = -Ra
    Ji[:3, 3:] = 2.0 * Ra @ skew(tb)
    Ji[3:, 3:] = -sgn * L
    Jj[:3, :3] = q_to_R(qe)
    Jj[3:, 3:] = qe[3] * np.eye(3) + skew(qe[:3])
    return Ji, Jj


def apply_delta(t, q, d):
    """X <- X fromVectorMQT(d); the quaternion renormalised (the project's rule)"""
    t = t + q_to_R(q) @ d[:3]
    w2 = 1.0 - ((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5])
    if w2 < 0:
        return t, q
    q = q_mul(q, np.array([d[3], d[4], d[5], np.sqrt(w2)]))
    return t, q / np.linalg.norm(q)


def robustify(chi2, kernel, delta):
    if kernel == HUBER:
        s = np.sqrt(chi2)
        if not s <= delta:
            return 2.0 * delta * s - delta * delta, delta / s
    return chi2, 1.0


class Graph:
    def __init__(self):
        self.t, self.q, self.fixed, self.edges = [], [], [], []

    def add_node(self, T, fixed=False):
        t, q = T_to_tq(T)
        self.t.append(t)
        self.q.append(q)
        self.fixed.append(bool(fixed))
        return len(self.t) - 1

    def set_estimate(self, n, T):
        self.t[n], self.q[n] = T_to_tq(T)

    def add_edge(self, i, j, M, info, kernel=NONE, delta=1.0):
        mt, mq = T_to_tq(M)
        self.edges.append(dict(i=i, j=j, M=np.asarray(M, np.float64), mt=mt, mq=mq, info=np.asarray(info, np.float64), kernel=kernel, delta=delta, live=True))
        return len(self.edges) - 1

    def remove_edge(self, e):
        self.edges[e]["live"] = False

    def estimates(self):
        return np.array([tq_to_T(t, q) for t, q in zip(self.t, self.q)])

    def n_live(self):
        return sum(e["live"] for e in self.edges)

    def active(self):
        deg = np.zeros(len(self.t), int)
        for e in self.edges:
            if e["live"]:
                deg[e["i"]] += 1
                deg[e["j"]] += 1
        return [n for n in range(len(self.t)) if not self.fixed[n] and deg[n]]

    def edge_rho(self, e):
        err = edge_eval(self.t[e["i"]], self.q[e["i"]], self.t[e["j"]], self.q[e["j"]], e["mt"], e["mq"])[0]
        return robustify(err @ e["info"] @ err, e["kernel"], e["delta"])

    def chi2(self):
        return sum(self.edge_rho(e)[0] for e in self.edges if e["live"])

    def linearize(self):
        """-> errors (E, 6), chi2 (E,), rho' (E,), b (N, 6), Hdiag (N, 6, 6), and the dense system (H, b, active nodes)"""
        N, E = len(self.t), len(self.edges)
        act = self.active()
        idx = {n: k for k, n in enumerate(act)}
        H, b = np.zeros((6 * len(act), 6 * len(act))), np.zeros(6 * len(act))
        errs, c2, r1 = np.zeros((E, 6)), np.zeros(E), np.zeros(E)
        for k, e in enumerate(self.edges):
            if not e["live"]:
                continue
            i, j = e["i"], e["j"]
            args = (self.t[i], self.q[i], self.t[j], self.q[j], e["mt"], e["mq"])
            err = edge_eval(*args)[0]
            Ji, Jj = jacobians(*args)
            chi2 = err @ e["info"] @ err
            _, rho1 = robustify(chi2, e["kernel"], e["delta"])
            errs[k], c2[k], r1[k] = err, chi2, rho1
            W = rho1 * e["info"]
            for (n, Jn) in ((i, Ji), (j, Jj)):
                if n in idx:
                    s = slice(6 * idx[n], 6 * idx[n] + 6)
                    b[s] -= Jn.T @ W @ err
                    H[s, s] += Jn.T @ W @ Jn
            if i in idx and j in idx:
                si, sj = slice(6 * idx[i], 6 * idx[i] + 6), slice(6 * idx[j], 6 * idx[j] + 6)
                H[si, sj] += Ji.T @ W @ Jj
                H[sj, si] += Jj.T @ W @ Ji
        bn, Hd = np.zeros((N, 6)), np.zeros((N, 6, 6))
        for n, k in idx.items():
            bn[n] = b[6 * k:6 * k + 6]
            Hd[n] = H[6 * k:6 * k + 6, 6 * k:6 * k + 6]
        return errs, c2, r1, bn, Hd, (H, b, act)

    @staticmethod
    def _pcg(H, b, lam, eps, max_it):
        """the device's solve: conjugate gradients preconditioned by the inverse of every damped 6 x 6 diagonal block"""
        n = len(b) // 6
        A = H + lam * np.eye(len(b))
        Minv = np.zeros_like(A)
        for k in range(n):
            s = slice(6 * k, 6 * k + 6)
            Minv[s, s] = np.linalg.inv(A[s, s])
        x, r = np.zeros_like(b), b.copy()
        z = Minv @ r
        p, rz, bb = z.copy(), r @ z, b @ b
        it = 0
        while it < max_it and r @ r > eps * eps * bb:
            Ap = A @ p
            pAp = p @ Ap
            if not pAp > 0:
                break
            alpha = rz / pAp
            x += alpha * p
            r -= alpha * Ap
            it += 1
            if not r @ r > eps * eps * bb:
                break
            z = Minv @ r
            rz2 = r @ z
            p = z + (rz2 / rz) * p
            rz = rz2
        return x

    def optimize(self, max_iterations, min_edges=10, solver="exact", cg_epsilon=1e-10, chi2_rel_stop=0.0):
        """OptimizationAlgorithmLevenberg::solve, iteration after iteration -> (iterations run or -1, report)"""
        if self.n_live() < min_edges:
            return -1, {}
        chi2 = self.chi2()
        rep = dict(chi2_initial=chi2, trials=0, accepted=0, stop="none")
        lam, nu, it = 0.0, 2.0, 0
        if not self.active():
            max_iterations = 0
        while it < max_iterations:
            H, b, act = self.linearize()[5]
            if it == 0:
                lam = 1e-5 * np.max(np.abs(np.diag(H)))
            trials, stop = 0, None
            while True:
                if solver == "exact":
                    d = np.linalg.solve(H + lam * np.eye(len(b)), b)
                else:
                    d = self._pcg(H, b, lam, cg_epsilon, 12 * len(act))
                bak = ([x.copy() for x in self.t], [x.copy() for x in self.q])
                for k, n in enumerate(act):
                    self.t[n], self.q[n] = apply_delta(self.t[n], self.q[n], d[6 * k:6 * k + 6])
                new = self.chi2()
                rho = (chi2 - new) / (d @ (lam * d + b) + 1e-3)
                accept = rho > 0 and np.isfinite(new)
                rel = False
                if accept:
                    lam *= max(1.0 / 3.0, min(2.0 / 3.0, 1.0 - (2.0 * rho - 1.0) * (2.0 * rho - 1.0) * (2.0 * rho - 1.0)))
                    nu = 2.0
                    rel = chi2_rel_stop > 0 and (chi2 - new) <= chi2_rel_stop * chi2
                    chi2 = new
                    rep["accepted"] += 1
                else:
                    self.t, self.q = bak
                    lam *= nu
                    nu *= 2.0
                trials += 1
                rep["trials"] += 1
                if not (rho < 0 and trials < MAX_TRIALS and np.isfinite(lam)):
                    break
            it += 1
            if not np.isfinite(lam):
                stop = "lambda"
            elif trials == MAX_TRIALS:
                stop = "trials"
            elif rho == 0:
                stop = "rho_zero"
            elif rel:
                stop = "chi2_rel"
            elif it >= max_iterations:
                stop = "max_iterations"
            if stop:
                rep["stop"] = stop
                break
        rep.update(iterations=it, chi2_final=chi2, **{"lambda": lam})
        return it, rep


# ---- seeded poses and graphs ---------------------------------------------------------------------------------------------------------------

def rotvec_q(v):
    v = np.asarray(v, np.float64)
    a = np.linalg.norm(v)
    if a < 1e-300:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(a / 2) * v / a, [np.cos(a / 2)]])


def random_pose(rng, t_scale=1.0, angle=None):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(0, np.pi) if angle is None else angle
    return tq_to_T(rng.uniform(-t_scale, t_scale, 3), rotvec_q(a * axis))


def random_info(rng):
    """a symmetric positive definite 6 x 6 with off-diagonal entries"""
    A = rng.normal(size=(6, 6))
    W = A @ A.T + 6.0 * np.eye(6)
    W[:3] *= 2.0
    W[:, :3] *= 2.0
    return 0.5 * (W + W.T)


def drive(n, seed, step=1.0, turn=0.08):
    """n true poses along a gently turning path"""
    rng = np.random.default_rng(seed)
    X = [np.eye(4)]
    for _ in range(n - 1):
        X.append(X[-1] @ tq_to_T([step, 0.0, 0.0] + rng.normal(0, 0.02, 3), rotvec_q([rng.normal(0, 0.01), rng.normal(0, 0.01), turn + rng.normal(0, 0.02)])))
    return X


def perturbed(X, rng, dt, da):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    return X @ tq_to_T(rng.uniform(-1, 1, 3) * dt / np.sqrt(3.0), rotvec_q(da * axis))


def spec_chain(n, seed, loops=(), noise=(0.0, 0.0), start_noise=(0.05, 0.01), fix_first=True, loop_kernel=NONE, loop_offset=None, extra_random_edges=0, odom_scale=1.0):
    """a specification {nodes: [(T, fixed)], edges: [(i, j, M, info, kernel, delta)], truth} of a drive: edge k -> k - 1 as the wrapper adds
    them (measurement X_k^-1 X_{k-1} of the truth, noise on top), the loop edges, extra random edges between true poses"""
    rng = np.random.default_rng(seed + 1000)
    X = drive(n, seed)
    nodes = [(X[0] if k == 0 else perturbed(X[k], rng, *start_noise), fix_first and k == 0) for k in range(n)]
    edges = []
    for k in range(1, n):
        M = perturbed(inv_T(X[k]) @ X[k - 1], rng, *noise) if noise[0] or noise[1] else inv_T(X[k]) @ X[k - 1]
        edges.append((k, k - 1, M, odom_scale * random_info(rng), NONE, 1.0))
    for (i, j) in loops:
        M = inv_T(X[i]) @ X[j]
        if loop_offset is not None:
            M = M @ loop_offset
        edges.append((i, j, M, random_info(rng), loop_kernel, 1.0))
    for _ in range(extra_random_edges):
        i, j = rng.choice(n, 2, replace=False)
        edges.append((int(i), int(j), inv_T(X[i]) @ X[j], random_info(rng), HUBER if rng.random() < 0.3 else NONE, float(rng.uniform(0.5, 3.0))))
    return dict(nodes=nodes, edges=edges, truth=X)


def spec_ring(n=12, seed=5):
    """a consistent ring: n poses on a circle, edge k -> k + 1 and the closing one; estimates perturbed by 0.3 m / 0.1 rad"""
    rng = np.random.default_rng(seed)
    X = [tq_to_T([5 * np.cos(2 * np.pi * k / n), 5 * np.sin(2 * np.pi * k / n), 0.1 * k], rotvec_q([0, 0, 2 * np.pi * k / n + np.pi / 2])) for k in range(n)]
    nodes = [(X[0], True)] + [(perturbed(X[k], rng, 0.3, 0.1), False) for k in range(1, n)]
    edges = [(k, (k + 1) % n, inv_T(X[k]) @ X[(k + 1) % n], random_info(rng), NONE, 1.0) for k in range(n)]
    return dict(nodes=nodes, edges=edges, truth=X)


def spec_hub(degree=40, seed=6):
    rng = np.random.default_rng(seed)
    X = [random_pose(rng, 3.0) for _ in range(degree + 1)]
    nodes = [(perturbed(x, rng, 0.1, 0.05), False) for x in X]
    edges = [((0, k) if k % 2 else (k, 0)) for k in range(1, degree + 1)]
    edges = [(i, j, perturbed(inv_T(X[i]) @ X[j], rng, 0.05, 0.02), random_info(rng), HUBER if i else NONE, 0.7) for (i, j) in edges]
    return dict(nodes=nodes, edges=edges, truth=X)


def spec_parallel(seed=7):
    rng = np.random.default_rng(seed)
    X = [random_pose(rng, 2.0), random_pose(rng, 2.0)]
    nodes = [(perturbed(x, rng, 0.2, 0.1), False) for x in X]
    edges = [(0, 1, perturbed(inv_T(X[0]) @ X[1], rng, 0.05, 0.02), random_info(rng), NONE, 1.0),
             (1, 0, perturbed(inv_T(X[1]) @ X[0], rng, 0.05, 0.02), random_info(rng), HUBER, 0.5),
             (0, 1, perturbed(inv_T(X[0]) @ X[1], rng, 0.05, 0.02), random_info(rng), HUBER, 5.0)]
    return dict(nodes=nodes, edges=edges, truth=X)


def build(spec, graph, remove=()):
    """a specification into a Graph (this file's) or a lsd_amd.lio.PoseGraph: both take add_node / add_edge / remove_edge"""
    for T, fixed in spec["nodes"]:
        graph.add_node(T, fixed)
    for (i, j, M, info, kernel, delta) in spec["edges"]:
        graph.add_edge(i, j, M, info, kernel, delta)
    for e in remove:
        graph.remove_edge(e)
    return graph


def pose_diff(A, B):
    """(metres, radians) between two 4 x 4 poses"""
    D = inv_T(A) @ B
    return float(np.linalg.norm(D[:3, 3])), float(2.0 * np.arcsin(min(1.0, np.linalg.norm(to_mqt(D)[3:]))))


def spec_huber():
    """60 nodes, noisy odometry of high information, two loop edges that contradict it (about 0.9 m / 0.16 rad and 1.5 m / 0.1 rad off), Huber 1.0
    on both: the optimum leaves both in Huber's linear branch"""
    off = tq_to_T([0.8, -0.3, 0.2], rotvec_q([0.02, -0.05, 0.15]))
    s = spec_chain(60, 21, loops=((59, 3),), noise=(0.03, 0.005), loop_kernel=HUBER, loop_offset=off, odom_scale=1.0e4)
    rng = np.random.default_rng(22)
    X = s["truth"]
    s["edges"].append((45, 10, inv_T(X[45]) @ X[10] @ tq_to_T([-1.2, 0.9, 0.1], rotvec_q([0.0, 0.03, -0.1])), random_info(rng), HUBER, 1.0))
    return s
