"""The GNSS moment stage of the pose graph (include/lio_hip.h, "moment") restated in f64 numpy on top of tests/graph_prior_cases.py, and the
seeded scenes of the moment tests.

hdl_graph_slam's EdgeSE3GNSS and the stage of robust_graph_optimize's mode `mapping` are restated from their published source; the Jacobians are
analytic (checked against central differences by tests/test_graph_moment_cpu.py).  While the stage is open (Graph.moment is not None) every live
XYZ prior is a moment edge e = t - (z + R m) on its node and the one shared moment m, the system has 6 Na + 3 unknowns -- the moment's three last --
and the linear solve is numpy.linalg.solve on the dense damped system or the device's block-Jacobi conjugate gradients with the damped 3 x 3 as
one more block.  SIGN: fixes z = t + R l give m = -l."""
import numpy as np

import graph_cases as GC
import graph_prior_cases as GP

NONE, HUBER, DCS2 = GP.NONE, GP.HUBER, GP.DCS2
XYZ, QUAT, PLANE = GP.XYZ, GP.QUAT, GP.PLANE
REF_PRIOR_INFO = np.diag([1.0 / 2000.0, 1.0 / 2000.0, 1.0 / 200.0])


def moment_error(t, q, z, m):
    return t - (z + GC.q_to_R(q) @ m)


def moment_jacobians(t, q, z, m):
    """d e / d delta (3 x 6, X <- X fromVectorMQT(delta)) and d e / d m (3 x 3, m <- m + d_m)"""
    R = GC.q_to_R(q)
    return np.hstack([R, 2.0 * R @ GC.skew(m)]), -R


class Graph(GP.Graph):
    """graph_prior_cases.Graph with the moment stage: between moment_begin and moment_end every live XYZ prior is a moment edge"""

    def __init__(self):
        super().__init__()
        self.moment, self.moment_info = None, None

    def moment_begin(self, m0=None, prior_information=None):
        assert self.moment is None
        self.moment = np.zeros(3) if m0 is None else np.asarray(m0, np.float64).copy()
        self.moment_info = REF_PRIOR_INFO.copy() if prior_information is None else np.asarray(prior_information, np.float64).reshape(3, 3)

    def moment_end(self, apply=True):
        n = 0
        if apply:
            for e in self.edges:
                if self.is_moment_edge(e):
                    e["m"] = np.concatenate([e["m"][:3] + GC.q_to_R(self.q[e["i"]]) @ self.moment, [0.0]])
                    n += 1
        self.moment, self.moment_info = None, None
        return n

    def is_moment_edge(self, e):
        return self.moment is not None and e["live"] and e["j"] is None and e["type"] == XYZ

    def n_live(self):
        return super().n_live() + (1 if self.moment is not None else 0)  # the moment's own prior

    def edge_chi2(self, e):
        if self.is_moment_edge(e):
            err = moment_error(self.t[e["i"]], self.q[e["i"]], e["m"][:3], self.moment)
            return err @ e["info"] @ err
        return super().edge_chi2(e)

    def chi2(self):
        c = sum(self.edge_rho(e)[0] for e in self.edges if e["live"])
        if self.moment is not None:
            c += self.moment @ self.moment_info @ self.moment
        return c

    def linearize(self):
        """as graph_prior_cases.Graph.linearize; with the stage open the dense system is the bordered one (the moment's three unknowns last) and
        self.border = (b_m (3,), H_mm (3, 3), H_pm (N, 6, 3))"""
        if self.moment is None:
            return super().linearize()
        N, E = len(self.t), len(self.edges)
        act = self.active()
        idx = {n: k for k, n in enumerate(act)}
        n6 = 6 * len(act)
        H, b = np.zeros((n6 + 3, n6 + 3)), np.zeros(n6 + 3)
        sm = slice(n6, n6 + 3)
        errs, c2, r1 = np.zeros((E, 6)), np.zeros(E), np.zeros(E)
        Hpm = np.zeros((N, 6, 3))
        for k, e in enumerate(self.edges):
            if not e["live"]:
                continue
            i, j = e["i"], e["j"]
            Jm = None
            if self.is_moment_edge(e):
                err = moment_error(self.t[i], self.q[i], e["m"][:3], self.moment)
                Ji, Jm = moment_jacobians(self.t[i], self.q[i], e["m"][:3], self.moment)
                blocks = ((i, Ji),)
            elif j is None:
                err = GP.prior_error(e["type"], self.t[i], self.q[i], e["m"], e["plane"])
                blocks = ((i, GP.prior_jacobian(e["type"], self.t[i], self.q[i], e["m"], e["plane"])),)
            else:
                args = (self.t[i], self.q[i], self.t[j], self.q[j], e["mt"], e["mq"])
                err = GC.edge_eval(*args)[0]
                blocks = tuple(zip((i, j), GC.jacobians(*args)))
            chi2 = err @ e["info"] @ err
            rho1 = GP.robustify(chi2, e["kernel"], e["delta"])[1]
            errs[k, :len(err)], c2[k], r1[k] = err, chi2, rho1
            W = rho1 * e["info"]
            for (n, Jn) in blocks:
                if n in idx:
                    s = slice(6 * idx[n], 6 * idx[n] + 6)
                    b[s] -= Jn.T @ W @ err
                    H[s, s] += Jn.T @ W @ Jn
            if Jm is not None:
                b[sm] -= Jm.T @ W @ err
                H[sm, sm] += Jm.T @ W @ Jm
                if i in idx:
                    s = slice(6 * idx[i], 6 * idx[i] + 6)
                    C = blocks[0][1].T @ W @ Jm
                    H[s, sm] += C
                    H[sm, s] += C.T
                    Hpm[i] += C
            elif j is not None and i in idx and j in idx:
                si, sj = slice(6 * idx[i], 6 * idx[i] + 6), slice(6 * idx[j], 6 * idx[j] + 6)
                H[si, sj] += blocks[0][1].T @ W @ blocks[1][1]
                H[sj, si] += blocks[1][1].T @ W @ blocks[0][1]
        H[sm, sm] += self.moment_info  # the moment's own prior: e_m = m
        b[sm] -= self.moment_info @ self.moment
        bn, Hd = np.zeros((N, 6)), np.zeros((N, 6, 6))
        for n, k in idx.items():
            bn[n] = b[6 * k:6 * k + 6]
            Hd[n] = H[6 * k:6 * k + 6, 6 * k:6 * k + 6]
        self.border = (b[sm].copy(), H[sm, sm].copy(), Hpm)
        return errs, c2, r1, bn, Hd, (H, b, act)

    @staticmethod
    def _pcg_border(H, b, lam, eps, max_it):
        """graph_cases.Graph._pcg with the damped trailing 3 x 3 as one more block of the preconditioner -> (x, iterations)"""
        n6 = len(b) - 3
        A = H + lam * np.eye(len(b))
        Minv = np.zeros_like(A)
        for k in range(n6 // 6):
            s = slice(6 * k, 6 * k + 6)
            Minv[s, s] = np.linalg.inv(A[s, s])
        Minv[n6:, n6:] = np.linalg.inv(A[n6:, n6:])
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
        return x, it

    def optimize(self, max_iterations, min_edges=10, solver="exact", cg_epsilon=1e-10, chi2_rel_stop=0.0):
        """graph_cases.Graph.optimize over the bordered system while the stage is open: lambda_0 and the scale cover the border's three entries,
        a rejected trial restores m with the poses.  The report also has history (chi2 after every iteration) and cg_max (the largest
        iteration count of one solve)"""
        if self.moment is None:
            return super().optimize(max_iterations, min_edges=min_edges, solver=solver, cg_epsilon=cg_epsilon, chi2_rel_stop=chi2_rel_stop)
        if self.n_live() < min_edges:
            return -1, {}
        chi2 = self.chi2()
        rep = dict(chi2_initial=chi2, trials=0, accepted=0, stop="none", history=[], cg_max=0)
        lam, nu, it = 0.0, 2.0, 0
        while it < max_iterations:
            H, b, act = self.linearize()[5]
            n6 = 6 * len(act)
            if it == 0:
                lam = 1e-5 * np.max(np.abs(np.diag(H)))
            trials, stop = 0, None
            while True:
                if solver == "exact":
                    d = np.linalg.solve(H + lam * np.eye(len(b)), b)
                else:
                    d, cg = self._pcg_border(H, b, lam, cg_epsilon, 12 * len(act) if act else 3)
                    rep["cg_max"] = max(rep["cg_max"], cg)
                bak = ([x.copy() for x in self.t], [x.copy() for x in self.q], self.moment.copy())
                for k, n in enumerate(act):
                    self.t[n], self.q[n] = GC.apply_delta(self.t[n], self.q[n], d[6 * k:6 * k + 6])
                self.moment = self.moment + d[n6:]
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
                    self.t, self.q, self.moment = bak
                    lam *= nu
                    nu *= 2.0
                trials += 1
                rep["trials"] += 1
                if not (rho < 0 and trials < GC.MAX_TRIALS and np.isfinite(lam)):
                    break
            it += 1
            rep["history"].append(chi2)
            if not np.isfinite(lam):
                stop = "lambda"
            elif trials == GC.MAX_TRIALS:
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

    def estimate_gnss_moment(self, max_distance_error=1.0, max_iterations=1024, prior_information=None, **kw):
        """the stage -> (priors re-anchored, or None below min_edges; the moment; the report)"""
        gnss = [k for k, e in enumerate(self.edges) if e["live"] and e["j"] is None and e["type"] == XYZ]
        if not gnss:
            return 0, np.zeros(3), {}
        if super().n_live() + 1 < kw.get("min_edges", 10):
            return None, np.zeros(3), {}
        for k in gnss:
            self.set_kernel(k, DCS2, max_distance_error * max_distance_error * self.edges[k]["info"][0, 0])
        self.moment_begin(None, prior_information)
        rep = self.optimize(max_iterations, **kw)[1]
        m = self.moment.copy()
        return self.moment_end(True), m, rep


# ---- seeded scenes -------------------------------------------------------------------------------------------------------------------------

def weave(n, seed, step=1.0, tilt=0.06):
    """n true poses of a drive that can tell the moment apart: the yaw rate changes sign every 15 steps and its size from step to step (on a
    circle the forward component of m is a rotation of the whole drive), roll and pitch swing by +-tilt (with a level drive and nothing fixed in
    height m_z is a free shift of all heights)"""
    rng = np.random.default_rng(seed)
    X = [np.eye(4)]
    for k in range(n - 1):
        sign = 1.0 if (k // 15) % 2 == 0 else -1.0
        yaw = sign * rng.uniform(0.04, 0.16)
        roll, pitch = tilt * np.sin(0.9 * k + 0.3), tilt * np.cos(0.7 * k)
        Xk = X[-1] @ GC.tq_to_T([step, 0.0, 0.0] + rng.normal(0, 0.02, 3), GC.rotvec_q([0.0, 0.0, yaw]))
        R = GC.q_to_R(GC.rotvec_q([0.0, 0.0, np.arctan2(Xk[1, 0], Xk[0, 0])])) @ GC.q_to_R(GC.rotvec_q([0.0, pitch, 0.0])) @ GC.q_to_R(GC.rotvec_q([roll, 0.0, 0.0]))
        Xk[:3, :3] = R
        X.append(Xk)
    return X


def spec_moment(n=60, seed=41, lever=(0.6, -0.3, 0.4), outliers=(12, 39), every=3, sigma=0.05, jump=15.0, fix_first=True):
    """the weave with noisy odometry (0.03 m, 0.005 rad), the first node fixed at the truth, XYZ priors (Omega = I / 0.05, Huber 1.0 as the wrapper
    adds them) on every third node at z = t + R lever + N(0, 0.05), those of the nodes in `outliers` displaced by 15 m"""
    rng = np.random.default_rng(seed + 500)
    X = weave(n, seed)
    lever = np.asarray(lever, np.float64)
    nodes = [(X[0] if k == 0 else GC.perturbed(X[k], rng, 0.05, 0.01), fix_first and k == 0) for k in range(n)]
    edges = []
    for k in range(1, n):
        edges.append((k, k - 1, GC.perturbed(GC.inv_T(X[k]) @ X[k - 1], rng, 0.03, 0.005), GC.random_info(rng), NONE, 1.0))
    planted = []
    for k in range(0, n, every):
        z = X[k][:3, 3] + X[k][:3, :3] @ lever + rng.normal(0, 0.05, 3)
        if k in outliers:
            d = rng.normal(size=3)
            z = z + jump * d / np.linalg.norm(d)
            planted.append(len(edges))
        edges.append(GP.prior(k, XYZ, z, np.eye(3) / sigma, HUBER, 1.0))
    return dict(nodes=nodes, edges=edges, truth=X, planted=planted, lever=lever)


def spec_long(n=300, seed=7, lever=(0.5, 0.2, -0.3), every=4):
    """a 300-node weave (6 Na > 1024 rows, more than 256 edge ids), XYZ priors under DCS2 on every fourth node, the first node fixed"""
    s = spec_moment(n, seed, lever, outliers=(), every=every)
    s["edges"] = [(e[:5] + (DCS2, 1.0 / 0.05) + e[7:]) if e[0] == "prior" else e for e in s["edges"]]
    return s


build = GP.build

# the scenes of the accuracy tests.  The seeds were chosen on the CPU with the restatement alone: |m + l| < 0.15 m, at least one rejected trial,
# and an LM iteration count that moves as little as a seed's can.  Every run ends in a tail of steps at rounding level -- chi2 falls by parts in
# 1e15, a trial is accepted or not by the last bits -- so the count is not a property of the scene: over seeds 41 .. 57 the exact solve and the
# restated conjugate gradients, whose moments agree to 1e-9 m, take the same number of iterations on a third of the scenes (11 to 26 iterations),
# and of seeds 44 .. 70 none keeps its count in all of six runs whose initial estimates are moved by 1e-9 m and 1e-9 rad.  Seed 47 keeps it in five
# of the six (12 iterations; the sixth takes 15) and is the steadiest of them; seed 45 without a lever arm gives 16 iterations and 27 trials
# under both restated solvers, their moments 7e-17 m apart
SCENES = {
    "lever": dict(seed=47, lever=(0.6, -0.3, 0.4)),
    "no_lever": dict(seed=45, lever=(0.0, 0.0, 0.0)),
}
_REFERENCE = {}


def reference(name):
    """the restatement (exact solve) through the outlier stage and the moment stage of a scene, computed once: removed ids, priors moved, moment,
    report, estimates, the moved measurements"""
    if name not in _REFERENCE:
        g = build(spec_moment(**SCENES[name]), Graph())
        removed = g.remove_gnss_outliers(1.0, 1024)[0]
        n, m, rep = g.estimate_gnss_moment(1.0, 1024)
        _REFERENCE[name] = dict(removed=removed, priors=n, moment=m, report=rep, estimates=g.estimates(), measurements=[p["measurement"][:3].copy() for p in g.priors()])
    return _REFERENCE[name]


def _lin_cases():
    """name -> (specification, ids removed) of the linearisation shapes"""
    rng = np.random.default_rng(91)
    chain = lambda n, seed, fix_first=False: GC.spec_chain(n, seed, noise=(0.05, 0.02), fix_first=fix_first)
    fix = lambda s, node, off=0.1, **kw: GP.random_prior(rng, node, s["nodes"][node][0], XYZ, err=off, **kw)
    out = {}
    X = GC.random_pose(rng, 2.0)
    s = dict(nodes=[(X, False)], edges=[], truth=[X])
    s["edges"].append(fix(s, 0))
    out["one"] = (s, ())
    s = chain(4, 92)
    s["edges"] += [fix(s, 2), fix(s, 3, kernel=HUBER, delta=0.2), fix(s, 2, kernel=DCS2, delta=50.0)]  # two on node 2, another id between them
    out["two_on_one"] = (s, ())
    s = chain(4, 93, fix_first=True)
    s["edges"] += [fix(s, 0), fix(s, 2)]
    out["fixed_node"] = (s, ())
    s = chain(5, 94)
    s["edges"] += [fix(s, k) for k in (1, 2, 3, 4)]
    out["dead"] = (s, (5,))  # the fix on node 2
    out["mixed"] = (GP.spec_interleaved(12, 95), ())
    s = chain(4, 96)
    s["edges"] += [fix(s, 1), GP.prior(2, XYZ, s["nodes"][2][0][:3, 3] + [3.0, -2.0, 1.0], np.eye(3), DCS2, 2.0)]  # chi2 about 14 > phi: rho' < 0
    out["dcs_out"] = (s, ())
    s = chain(3, 97)
    s["nodes"] = [(T, True) for T, _ in s["nodes"]]
    s["edges"] += [fix(s, k) for k in range(3)]
    out["all_fixed"] = (s, ())
    return out


LIN_CASES = _lin_cases()
