"""The pose graph's unary edges (include/lio_hip.h, "priors", "DCS2", "outliers") restated in f64 numpy on top of tests/graph_cases.py, and the
seeded scenes of the prior tests.

g2o and hdl_graph_slam's edge types are restated from their published source: EdgeSE3PriorXYZ, EdgeSE3PriorQuat, EdgeSE3Plane (whose plane vertex
the reference always fixes, so the edge carries its world plane), g2o's Plane3D (azimuth / elevation / distance), RobustKernelDCS2.  The Jacobians
are analytic (checked against central differences by tests/test_graph_priors_cpu.py).  A prior is an entry of Graph.edges like any other -- the
shared list is the shared id counter -- with j = None."""
import numpy as np

import graph_cases as GC

NONE, HUBER, DCS2 = 0, 1, 2
XYZ, QUAT, PLANE = 0, 1, 2


def robustify(chi2, kernel, delta):
    """-> (rho, rho')"""
    if kernel == DCS2:
        p = delta + chi2
        s = (2.0 * delta) / p
        if not s >= 1.0:
            return s * chi2 * s, (4.0 * delta * delta * (delta - chi2)) / (p * p * p)
        return chi2, 1.0
    return GC.robustify(chi2, kernel, delta)


def dcs_scale(chi2, delta):
    return (2.0 * delta) / (delta + chi2)


def az(x):
    return np.arctan2(x[1], x[0])


def el(x):
    return np.arctan2(x[2], np.hypot(x[0], x[1]))


def Rz(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def Ry(a):
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def normalise_prior(kind, m, plane):
    """the measurement and the world plane as the graph keeps them"""
    m = np.asarray(m, np.float64).copy()
    if kind == XYZ:
        return np.concatenate([m[:3], [0.0]]), np.zeros(4)
    if kind == QUAT:
        m = m / np.linalg.norm(m)
        return (-m if m[3] < 0 else m), np.zeros(4)
    plane = np.asarray(plane, np.float64).copy()
    return m / np.linalg.norm(m[:3]), plane / np.linalg.norm(plane[:3])


def prior_error(kind, t, q, m, plane):
    """m and plane normalised (normalise_prior)"""
    if kind == XYZ:
        return t - m[:3]
    if kind == QUAT:
        s = -1.0 if m @ q < 0 else 1.0
        return s * q[:3] - m[:3]
    nl = GC.q_to_R(q).T @ plane[:3]
    dl = plane[3] + t @ plane[:3]
    A = Rz(az(m[:3])) @ Ry(-el(m[:3]))
    u = A.T @ nl
    return np.array([az(u), el(u), m[3] - dl])


def prior_jacobian(kind, t, q, m, plane):
    """d e / d delta at 0, X <- X fromVectorMQT(delta): 3 x 6"""
    J = np.zeros((3, 6))
    if kind == XYZ:
        J[:, :3] = GC.q_to_R(q)
    elif kind == QUAT:
        s = -1.0 if m @ q < 0 else 1.0
        J[:, 3:] = s * (q[3] * np.eye(3) + GC.skew(q[:3]))
    else:
        nl = GC.q_to_R(q).T @ plane[:3]
        A = Rz(az(m[:3])) @ Ry(-el(m[:3]))
        u = A.T @ nl
        D = 2.0 * A.T @ GC.skew(nl)
        r2 = u[0] * u[0] + u[1] * u[1]
        if r2 > 0:
            r = np.sqrt(r2)
            J[0, 3:] = (np.array([-u[1], u[0], 0.0]) / r2) @ D
            J[1, 3:] = np.array([-u[0] * u[2] / r, -u[1] * u[2] / r, r]) @ D
        J[2, :3] = -nl
    return J


class Graph(GC.Graph):
    """graph_cases.Graph with priors: entries of self.edges with j = None"""

    def add_prior(self, node, kind, measurement, information, kernel=NONE, delta=1.0, plane=None):
        m, pl = normalise_prior(kind, measurement, plane)
        self.edges.append(dict(i=node, j=None, type=kind, m=m, plane=pl, info=np.asarray(information, np.float64).reshape(3, 3), kernel=kernel, delta=delta, live=True))
        return len(self.edges) - 1

    def set_kernel(self, e, kernel, delta=1.0):
        self.edges[e]["kernel"], self.edges[e]["delta"] = kernel, delta

    def priors(self):
        return [dict(id=k, node=e["i"], type=e["type"], measurement=e["m"], plane=e["plane"], information=e["info"], kernel=e["kernel"], delta=e["delta"])
                for k, e in enumerate(self.edges) if e["j"] is None and e["live"]]

    def active(self):
        deg = np.zeros(len(self.t), int)
        for e in self.edges:
            if e["live"]:
                deg[e["i"]] += 1
                if e["j"] is not None:
                    deg[e["j"]] += 1
        return [n for n in range(len(self.t)) if not self.fixed[n] and deg[n]]

    def edge_chi2(self, e):
        if e["j"] is None:
            err = prior_error(e["type"], self.t[e["i"]], self.q[e["i"]], e["m"], e["plane"])
        else:
            err = GC.edge_eval(self.t[e["i"]], self.q[e["i"]], self.t[e["j"]], self.q[e["j"]], e["mt"], e["mq"])[0]
        return err @ e["info"] @ err

    def edge_rho(self, e):
        return robustify(self.edge_chi2(e), e["kernel"], e["delta"])

    def linearize(self):
        """as graph_cases.Graph.linearize; a prior's error fills the first three of its six slots"""
        N, E = len(self.t), len(self.edges)
        act = self.active()
        idx = {n: k for k, n in enumerate(act)}
        H, b = np.zeros((6 * len(act), 6 * len(act))), np.zeros(6 * len(act))
        errs, c2, r1 = np.zeros((E, 6)), np.zeros(E), np.zeros(E)
        for k, e in enumerate(self.edges):
            if not e["live"]:
                continue
            i, j = e["i"], e["j"]
            if j is None:
                err = prior_error(e["type"], self.t[i], self.q[i], e["m"], e["plane"])
                blocks = ((i, prior_jacobian(e["type"], self.t[i], self.q[i], e["m"], e["plane"])),)
            else:
                args = (self.t[i], self.q[i], self.t[j], self.q[j], e["mt"], e["mq"])
                err = GC.edge_eval(*args)[0]
                blocks = tuple(zip((i, j), GC.jacobians(*args)))
            chi2 = err @ e["info"] @ err
            rho1 = robustify(chi2, e["kernel"], e["delta"])[1]
            errs[k, :len(err)], c2[k], r1[k] = err, chi2, rho1
            W = rho1 * e["info"]
            for (n, Jn) in blocks:
                if n in idx:
                    s = slice(6 * idx[n], 6 * idx[n] + 6)
                    b[s] -= Jn.T @ W @ err
                    H[s, s] += Jn.T @ W @ Jn
            if j is not None and i in idx and j in idx:
                si, sj = slice(6 * idx[i], 6 * idx[i] + 6), slice(6 * idx[j], 6 * idx[j] + 6)
                H[si, sj] += blocks[0][1].T @ W @ blocks[1][1]
                H[sj, si] += blocks[1][1].T @ W @ blocks[0][1]
        bn, Hd = np.zeros((N, 6)), np.zeros((N, 6, 6))
        for n, k in idx.items():
            bn[n] = b[6 * k:6 * k + 6]
            Hd[n] = H[6 * k:6 * k + 6, 6 * k:6 * k + 6]
        return errs, c2, r1, bn, Hd, (H, b, act)

    def remove_gnss_outliers(self, max_distance_error=1.0, max_iterations=1024, **kw):
        """the first stage of robust_graph_optimize -> (ids removed or None below min_edges, the second optimisation's report, the scales seen)"""
        if self.n_live() < kw.get("min_edges", 10):
            return None, {}, {}
        gnss = [k for k, e in enumerate(self.edges) if e["live"] and e["j"] is None and e["type"] == XYZ]
        for k in gnss:
            self.set_kernel(k, DCS2, max_distance_error * max_distance_error * self.edges[k]["info"][0, 0])
        self.optimize(max_iterations, **kw)
        scales = {k: dcs_scale(self.edge_chi2(self.edges[k]), self.edges[k]["delta"]) for k in gnss}
        removed = [k for k in gnss if scales[k] < 0.1]
        for k in removed:
            self.remove_edge(k)
        return removed, self.optimize(max_iterations, **kw)[1], scales


# ---- seeded scenes -------------------------------------------------------------------------------------------------------------------------
# a specification is graph_cases' {nodes, edges, truth}; an entry of edges is graph_cases' 6-tuple or ("prior", node, type, measurement,
# information, kernel, delta, plane)

def prior(node, kind, m, info, kernel=NONE, delta=1.0, plane=None):
    return ("prior", node, kind, np.asarray(m, np.float64), np.asarray(info, np.float64), kernel, delta, plane)


def build(spec, graph, remove=()):
    """a specification into a Graph (this file's) or a lsd_amd.lio.PoseGraph"""
    for T, fixed in spec["nodes"]:
        graph.add_node(T, fixed)
    for e in spec["edges"]:
        if e[0] == "prior":
            graph.add_prior(e[1], e[2], e[3], e[4], e[5], e[6], plane=e[7])
        else:
            graph.add_edge(*e)
    for e in remove:
        graph.remove_edge(e)
    return graph


def random_info3(rng):
    A = rng.normal(size=(3, 3))
    W = A @ A.T + 3.0 * np.eye(3)
    return 0.5 * (W + W.T)


def random_prior(rng, node, X, kind, err=0.1, kernel=NONE, delta=1.0, tilt=None):
    """a prior of the given type on a node whose pose is about X: the measurement is the pose's own, off by about err (m, or rad / 2)"""
    t, q = GC.T_to_tq(X)
    if kind == XYZ:
        return prior(node, XYZ, t + rng.normal(0, err, 3), random_info3(rng), kernel, delta)
    if kind == QUAT:
        return prior(node, QUAT, GC.q_mul(q, GC.rotvec_q(rng.normal(0, err, 3))) * rng.uniform(0.5, 2.0), random_info3(rng), kernel, delta)
    n = rng.normal(size=3)
    world = np.concatenate([n, [rng.uniform(-2, 2)]]) * rng.uniform(0.5, 2.0)
    Y = X @ GC.tq_to_T(rng.normal(0, err, 3), GC.rotvec_q(rng.normal(0, err, 3) if tilt is None else tilt))
    wn = world / np.linalg.norm(world[:3])
    local = np.concatenate([Y[:3, :3].T @ wn[:3], [wn[3] + Y[:3, 3] @ wn[:3]]])
    return prior(node, PLANE, local * rng.uniform(0.5, 2.0), random_info3(rng), kernel, delta, plane=world)


def spec_interleaved(n_priors, seed):
    """a chain whose binary edges and priors of all three types alternate by id; every third prior under Huber, every fifth of the rest under DCS2"""
    rng = np.random.default_rng(seed)
    n = n_priors + 1
    base = GC.spec_chain(n, seed, noise=(0.05, 0.02))
    X = [T for T, _ in base["nodes"]]
    edges = []
    for k in range(n_priors):
        edges.append(base["edges"][k])
        kernel = HUBER if k % 3 == 0 else (DCS2 if k % 5 == 0 else NONE)
        node = k if k % 2 else int(rng.integers(0, n))  # every other prior sits on a node far from its measurement: the kernels' outer branches
        edges.append(random_prior(rng, node, X[k], k % 3, kernel=kernel, delta=float(rng.uniform(0.5, 3.0))))
    return dict(nodes=base["nodes"], edges=edges, truth=base["truth"])


def spec_gnss(n=60, seed=41, outliers=(12, 39), every=3, sigma=0.05, jump=15.0):
    """a chain with nothing fixed, noisy odometry, XYZ priors (Omega = I / 0.05, Huber 1.0 as the wrapper adds them) on every third node, the
    priors of the nodes in `outliers` displaced by 15 m"""
    rng = np.random.default_rng(seed + 500)
    s = GC.spec_chain(n, seed, noise=(0.03, 0.005), fix_first=False)
    planted = []
    for k in range(0, n, every):
        m = s["truth"][k][:3, 3] + rng.normal(0, 0.05, 3)
        if k in outliers:
            d = rng.normal(size=3)
            m = m + jump * d / np.linalg.norm(d)
            planted.append(len(s["edges"]))
        s["edges"].append(prior(k, XYZ, m, np.eye(3) / sigma, HUBER, 1.0))
    s["planted"] = planted
    return s


def spec_floor(n=60, seed=43, bias=0.004, every=5, with_priors=True):
    """the same kind of chain, every odometry edge pitched by 0.004 rad, the estimates integrated from that odometry, nothing fixed; PLANE priors
    (information I / 10, Huber 1.0 as the wrapper adds them) of the floor z = 0 seen from the true pose on every fifth node"""
    rng = np.random.default_rng(seed + 500)
    X = GC.drive(n, seed)
    pitch = GC.tq_to_T([0, 0, 0], GC.rotvec_q([0.0, bias, 0.0]))
    est, edges = [X[0]], []
    for k in range(1, n):
        rel = GC.inv_T(X[k - 1]) @ X[k] @ pitch
        est.append(est[-1] @ rel)
        edges.append((k, k - 1, GC.inv_T(rel), GC.random_info(rng), NONE, 1.0))
    world = np.array([0.0, 0.0, 1.0, 0.0])
    if with_priors:
        for k in range(0, n, every):
            local = np.concatenate([X[k][:3, :3].T @ world[:3], [world[3] + X[k][:3, 3] @ world[:3]]])
            edges.append(prior(k, PLANE, local, np.eye(3) / 10.0, HUBER, 1.0, plane=world))
    return dict(nodes=[(T, False) for T in est], edges=edges, truth=X)
