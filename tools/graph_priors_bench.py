"""Times lio.PoseGraph.optimize(1024) on a seeded 2 000-node drive with 20 loop edges (Huber 1.0 on the loops, noisy odometry, nothing fixed
by hand: the first node is fixed), once as it is and once with 700 priors (500 XYZ, 100 QUAT, 100 PLANE, Huber 1.0) spread over the nodes:
the stage times from lio_graph_last_times (HIP events) and the wall clock around the synchronous call.  A warm-up, then 5 repetitions of each;
the graph is rebuilt before every run.  The record holds the median, the spread (max - min) over the five and every run.

    python tools/graph_priors_bench.py [--package DIR] [--no-priors] [--out FILE]

--package DIR imports lsd_amd from DIR (a build of another commit, to time its prior-free graph in the same session); --no-priors skips the graph
with priors (a commit that has none).  Writes profiles/graph_priors_bench.json unless --out names another file.  No threshold: the record is the
result."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NODES, N_LOOPS, N_PRIORS, SEED, REPS = 2000, 20, 700, 43, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=os.path.join(ROOT, "lidar-slam-detection_amd", "python"))
    ap.add_argument("--no-priors", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_priors_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, a.package)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import graph_cases as GC
    import graph_prior_cases as PC
    from lsd_amd import lio

    rng = np.random.default_rng(SEED)
    loops = []
    while len(loops) < N_LOOPS:
        i = int(rng.integers(200, N_NODES))
        loops.append((i, int(rng.integers(0, i - 100))))
    bare = GC.spec_chain(N_NODES, SEED, loops=tuple(loops), noise=(0.02, 0.002), start_noise=(0.0, 0.0), loop_kernel=GC.HUBER)
    with_priors = dict(bare, edges=list(bare["edges"]))
    nodes = rng.choice(np.arange(1, N_NODES), N_PRIORS, replace=False)
    for k, n in enumerate(nodes):
        kind = PC.XYZ if k < 500 else (PC.QUAT if k < 600 else PC.PLANE)
        with_priors["edges"].append(PC.random_prior(rng, int(n), bare["truth"][int(n)], kind, err=0.02, kernel=PC.HUBER, delta=1.0))
    g = lio.PoseGraph()

    def run(spec):
        g.reset()
        PC.build(spec, g)
        g.chi2()  # (uploads the graph and builds the topology outside the timed call)
        t0 = time.perf_counter()
        n, rep = g.optimize(1024)
        out = dict(wall_ms=(time.perf_counter() - t0) * 1e3, iterations=n, trials=rep["trials"], cg_iterations_total=rep["cg_iterations_total"],
                   chi2_initial=rep["chi2_initial"], chi2_final=rep["chi2_final"])
        out.update(g.last_times())
        out["device_us"] = sum(g.last_times().values())
        return out

    def series(name, spec):
        print(name, "warm-up", json.dumps(run(spec)), flush=True)
        runs = [run(spec) for _ in range(REPS)]
        for r in runs:
            print(name, "run", json.dumps(r), flush=True)
        return dict(median={k: float(np.median([r[k] for r in runs])) for k in runs[0]},
                    spread={k: float(max(r[k] for r in runs) - min(r[k] for r in runs)) for k in ("wall_ms", "device_us", "linearize_us")}, runs=runs)

    rec = dict(bench="graph_priors_bench", package=os.path.relpath(a.package, ROOT), nodes=N_NODES, edges=len(bare["edges"]), loops=N_LOOPS, repetitions=REPS,
               no_priors=series("no priors", bare))
    if not a.no_priors:
        rec["priors"] = N_PRIORS
        rec["with_priors"] = series("with priors", with_priors)
        # graph_linearize_prior runs between the same two events as graph_linearize: its share of the device time is what linearize_us grew by
        # per iteration (the two graphs need not take the same number of iterations)
        w, b = rec["with_priors"]["median"], rec["no_priors"]["median"]
        grew = w["linearize_us"] / w["iterations"] - b["linearize_us"] / b["iterations"]
        rec["prior_kernel_us_per_iteration"] = grew
        rec["prior_kernel_share_of_device_time"] = grew * w["iterations"] / w["device_us"]
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k not in ("no_priors", "with_priors")}))


if __name__ == "__main__":
    main()
