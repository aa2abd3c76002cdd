"""Times one lio.PoseGraph.optimize(1024) on a seeded 5 000-node drive with 50 loop edges (Huber 1.0 on the loops, noisy odometry, the first
node fixed): the stage times from lio_graph_last_times (HIP events: linearise, assemble, solve, update) and the wall clock around the
synchronous call.  A warm-up, then the median of 3; the graph is rebuilt before every run so that each starts from the same estimates.

Baseline beside it, A STAND-IN: tests/graph_cases.py's restatement of the same LM schedule with the damped system assembled as a scipy sparse
matrix and solved by scipy.sparse.linalg.spsolve on the CPU.  It stands in for g2o's lm_var + CHOLMOD, which cannot be built here; it is not g2o.

Writes profiles/graph_bench.json.  No threshold: the record is the result."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-slam-detection_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graph_cases as GC  # noqa: E402
from lsd_amd import lio  # noqa: E402

N_NODES, N_LOOPS, SEED = 5000, 50, 41


def spec():
    rng = np.random.default_rng(SEED)
    loops = []
    while len(loops) < N_LOOPS:
        i = int(rng.integers(200, N_NODES))
        loops.append((i, int(rng.integers(0, i - 100))))
    return GC.spec_chain(N_NODES, SEED, loops=tuple(loops), noise=(0.02, 0.002), start_noise=(0.0, 0.0), loop_kernel=GC.HUBER)


def spsolve_lm(g, max_iterations):
    """Graph.optimize with the dense solve replaced by a sparse one (the same schedule, the same stop rules)"""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve

    def linearize():
        act = g.active()
        idx = {n: k for k, n in enumerate(act)}
        rows, cols, vals, b = [], [], [], np.zeros(6 * len(act))
        r6, c6 = np.repeat(np.arange(6), 6), np.tile(np.arange(6), 6)
        for e in g.edges:
            if not e["live"]:
                continue
            i, j = e["i"], e["j"]
            args = (g.t[i], g.q[i], g.t[j], g.q[j], e["mt"], e["mq"])
            err = GC.edge_eval(*args)[0]
            Ji, Jj = GC.jacobians(*args)
            W = GC.robustify(err @ e["info"] @ err, e["kernel"], e["delta"])[1] * e["info"]
            for (n, Jn) in ((i, Ji), (j, Jj)):
                if n in idx:
                    b[6 * idx[n]:6 * idx[n] + 6] -= Jn.T @ W @ err
                    for (m, Jm) in ((i, Ji), (j, Jj)):
                        if m in idx:
                            rows.append(6 * idx[n] + r6); cols.append(6 * idx[m] + c6); vals.append((Jn.T @ W @ Jm).ravel())
        H = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(b), len(b))).tocsc()
        return H, b, act

    chi2 = g.chi2()
    lam, nu, it, trials_all = 0.0, 2.0, 0, 0
    while it < max_iterations:
        H, b, act = linearize()
        if it == 0:
            lam = 1e-5 * np.abs(H.diagonal()).max()
        trials = 0
        while True:
            d = spsolve(H + lam * sp.identity(len(b), format="csc"), b)
            bak = ([x.copy() for x in g.t], [x.copy() for x in g.q])
            for k, n in enumerate(act):
                g.t[n], g.q[n] = GC.apply_delta(g.t[n], g.q[n], d[6 * k:6 * k + 6])
            new = g.chi2()
            rho = (chi2 - new) / (d @ (lam * d + b) + 1e-3)
            if rho > 0 and np.isfinite(new):
                lam *= max(1.0 / 3.0, min(2.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
                nu, chi2 = 2.0, new
            else:
                g.t, g.q = bak
                lam *= nu
                nu *= 2.0
            trials += 1
            trials_all += 1
            if not (rho < 0 and trials < GC.MAX_TRIALS and np.isfinite(lam)):
                break
        it += 1
        if trials == GC.MAX_TRIALS or rho == 0 or not np.isfinite(lam):
            break
    return it, trials_all, chi2


def main():
    s = spec()
    g = lio.PoseGraph()

    def run():
        g.reset()
        GC.build(s, g)
        g.chi2()  # (uploads the graph and builds the topology outside the timed call)
        t0 = time.perf_counter()
        n, rep = g.optimize(1024)
        wall = (time.perf_counter() - t0) * 1e3
        out = dict(wall_ms=wall, iterations=n, trials=rep["trials"], cg_iterations_total=rep["cg_iterations_total"], chi2_initial=rep["chi2_initial"],
                   chi2_final=rep["chi2_final"])
        out.update(g.last_times())
        return out

    print("warm-up", json.dumps(run()), flush=True)
    runs = []
    for _ in range(3):
        runs.append(run())
        print("run", json.dumps(runs[-1]), flush=True)
    dev = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    rec = dict(bench="graph_bench", nodes=N_NODES, edges=len(s["edges"]), loops=N_LOOPS, device=dev)
    print("device", json.dumps(rec), flush=True)
    r = GC.build(s, GC.Graph())
    t0 = time.perf_counter()
    it, trials, chi2 = spsolve_lm(r, 1024)
    base = dict(wall_ms=(time.perf_counter() - t0) * 1e3, iterations=it, trials=trials, chi2_final=float(chi2),
                what="STAND-IN for g2o (which cannot be built here): the numpy restatement's LM with scipy.sparse.linalg.spsolve on the CPU, one run")
    rec = dict(bench="graph_bench", nodes=N_NODES, edges=len(s["edges"]), loops=N_LOOPS, device=dev, baseline_spsolve_cpu=base)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "graph_bench.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
