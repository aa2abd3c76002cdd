"""Times the GNSS moment stage (lio.PoseGraph.estimate_gnss_moment) on a seeded 2 000-key-frame weave (tests/graph_moment_cases.spec_moment:
noisy odometry, the first node fixed, an XYZ fix on every fifth key frame taken 0.7 m from the lidar frame) and, beside it, the plain
lio_graph_optimize of the same graph with the same DCS2 kernels on its fixes: wall clock around the synchronous call, device time from
lio_graph_last_times (HIP events: linearise, assemble, solve, update), LM and conjugate-gradient iteration counts.  A warm-up, then 3 repetitions
of each; the graph is rebuilt before every run.  (About 3.4 s per optimisation on an MI355X; --repetitions 1 --no-warm-up is the short
form.)

    python tools/graph_moment_bench.py [--nodes N] [--max-iterations K] [--repetitions R] [--no-warm-up] [--out FILE]

Writes profiles/graph_moment_bench.json unless --out names another file.  No threshold: the record is the result."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-slam-detection_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graph_moment_cases as MC  # noqa: E402
from lsd_amd import lio  # noqa: E402

SEED, EVERY, LEVER = 47, 5, (0.6, -0.3, 0.2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=2000)
    ap.add_argument("--max-iterations", type=int, default=1024)
    ap.add_argument("--repetitions", type=int, default=3)
    ap.add_argument("--no-warm-up", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_moment_bench.json"))
    a = ap.parse_args()
    spec = MC.spec_moment(n=a.nodes, seed=SEED, lever=LEVER, outliers=(), every=EVERY)
    # the fixes under the kernel the stage gives them, so that the plain optimisation beside it minimises the same cost but for the moment
    spec["edges"] = [(e[:5] + (MC.DCS2, 1.0 / 0.05) + e[7:]) if e[0] == "prior" else e for e in spec["edges"]]
    g = lio.PoseGraph()

    def run(stage):
        g.reset()
        MC.build(spec, g)
        g.chi2()  # (uploads the graph and builds the topology outside the timed call)
        t0 = time.perf_counter()
        if stage:
            n, m, rep = g.estimate_gnss_moment(1.0, a.max_iterations)
        else:
            n, rep = g.optimize(a.max_iterations)
        out = dict(wall_ms=(time.perf_counter() - t0) * 1e3, iterations=rep["iterations"], trials=rep["trials"], accepted=rep["accepted"],
                   cg_iterations_total=rep["cg_iterations_total"], chi2_initial=rep["chi2_initial"], chi2_final=rep["chi2_final"], stop=rep["stop"])
        out.update(g.last_times())
        out["device_us"] = sum(g.last_times().values())
        if stage:
            out.update(priors=n, moment=[float(x) for x in m], moment_miss_m=float(np.linalg.norm(m + spec["lever"])))
        return out

    def series(name, stage):
        if not a.no_warm_up:
            print(name, "warm-up", json.dumps(run(stage)), flush=True)
        runs = [run(stage) for _ in range(a.repetitions)]
        for r in runs:
            print(name, "run", json.dumps(r), flush=True)
        keys = [k for k, v in runs[0].items() if isinstance(v, (int, float))]
        return dict(median={k: float(np.median([r[k] for r in runs])) for k in keys},
                    spread={k: float(max(r[k] for r in runs) - min(r[k] for r in runs)) for k in ("wall_ms", "device_us", "solve_us")}, runs=runs)

    rec = dict(bench="graph_moment_bench", nodes=a.nodes, edges=len(spec["edges"]), fixes=len([e for e in spec["edges"] if e[0] == "prior"]), lever=list(LEVER),
               max_iterations=a.max_iterations, repetitions=a.repetitions, warm_up=not a.no_warm_up, moment_stage=series("moment stage", True), plain_optimize=series("plain optimize", False))
    s, p = rec["moment_stage"]["median"], rec["plain_optimize"]["median"]
    rec["solve_us_per_cg_iteration"] = dict(moment_stage=s["solve_us"] / max(s["cg_iterations_total"], 1), plain_optimize=p["solve_us"] / max(p["cg_iterations_total"], 1))
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k not in ("moment_stage", "plain_optimize")}))


if __name__ == "__main__":
    main()
