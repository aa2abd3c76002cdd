"""bench.py (default configuration): the headline measurement and everything reported beside it."""
from .common import *  # noqa: F401,F403  (argparse, json, os, sys, time, np, ROOT, BENCH_PY, the roofline constants, emit, usable_cpus ...)
from .common import dump_outputs
from .rccl import rccl_probe


def bench_metric(args, torch, dist, world, rank, local_rank, dev):
    """the metric configuration: 120 000-point scans against the 1e7-point map, the batched engine timed on exactly --steps scans.  --full: beside it the
    pose check, the latencies, the upload-included leg, the roofline, the CPU baselines, the parity legs and (--secondary) the other BASELINE
    configurations as child processes"""
    from lsd_amd import lio, synth

    # ---- synthetic workload (SURVEY.md section 8d, config 2 scaled to the metric's 1e7-point map) -------------
    # map and scans are generated ON the GPU (lsd_amd/synth_gpu.py: the same scene and ray model as synth.py, torch's random streams) and copied
    # to the host for the CPU baselines: numpy needs 27 s for the 1e7 surface samples and 0.7 s per scan, i.e. minutes for a pool of 128
    from lsd_amd import synth_gpu

    scene = synth.Scene(half=100.0, n_boxes=40, seed=1)
    d_map = synth_gpu.sample_surface(scene, args.map_points, dev, seed=2, sigma=0.01)
    if args.frame_z:
        d_map[:, 2] -= float(np.float32(args.frame_z))
    scanner = synth_gpu.StaticScanner(scene, dev, n_az=args.n_az, fov_deg=(-24.8, 2.0), max_range=150.0)

    def make_pool(n_scans, spread, seed0):
        """n_scans scans with their true poses and priors.  spread: sensor positions uniform over [-spread, spread]^2 (outside the boxes, 1.5 m
        clear), any yaw -- SURVEY 8d config 2: distinct seeds seed0 .. seed0 + n_scans - 1; the prior is within --prior-t / --prior-deg of the truth"""
        rng = np.random.default_rng(seed0 + 7919 * rank)
        pool = []
        for k in range(n_scans):
            while True:
                xy = rng.uniform(-spread, spread, 2)
                if not np.any((scene.lo[:, 0] - 1.5 < xy[0]) & (xy[0] < scene.hi[:, 0] + 1.5) & (scene.lo[:, 1] - 1.5 < xy[1]) & (xy[1] < scene.hi[:, 1] + 1.5)):
                    break
            pos = np.array([xy[0], xy[1], 1.8])
            q = synth.quat_from_rotvec([0, 0, rng.uniform(-np.pi, np.pi)])
            d = scanner.scan(pos, q, seed=seed0 + 100000 * rank + k)
            pos = pos - np.array([0.0, 0.0, float(np.float32(args.frame_z))])  # (the scan is body-frame data: only the pose moves with the frame)
            gp, gq = synth.perturb_pose(pos, q, seed=seed0 + 7 * k + rank, max_t=args.prior_t, max_deg=args.prior_deg)
            pool.append(dict(raw=d.cpu().numpy(), d=d, pos=pos, q=q, guess=synth.state_from_pose(gp, gq), seed=seed0 + 100000 * rank + k))
        return pool

    scans = make_pool(args.scan_pool, args.spread, args.seed)           # the timed workload: poses all over the 200 m map
    scans8 = make_pool(8, 4.0, args.seed + 500) if (rank == 0 and args.full and args.secondary) else []  # round 3's workload (8 scans within 4 m of one spot), timed beside it
    n_raw = int(np.mean([len(s["raw"]) for s in scans]))

    the_map = lio.Map(resolution=0.5, stencil=19, max_points=max(args.map_points, 1_000_000), max_voxels=max(args.map_points // 4, 1_000_000),
                      device=local_rank)
    # the map goes to HBM once; the raw scans live in torch tensors on the device (inputs resident before timing)
    torch.cuda.synchronize()
    the_map.add_device(d_map.data_ptr(), args.map_points)
    map_pts = d_map.cpu().numpy() if (args.full and rank == 0 and world == 1 and (args.cpu_scans > 0 or args.ref_scans > 0)) else None  # the CPU baselines' copy
    del d_map
    d_scans = [s["d"] for s in scans]
    torch.cuda.synchronize()
    n_streams = args.streams
    if n_streams <= 0:  # default: 12 scans in flight per GPU, fewer when the ranks of this node have to share few host CPUs
        n_streams = max(2, min(12, usable_cpus() // max(world, 1) - 1))
    if args.engine == "batch":
        n_streams = 1  # one per-scan engine for the latency / parity legs; the timed region runs on the batched engine
    engines = [lio.Engine(max_raw=1 << 18, max_ds=100000, shared_map=the_map) for _ in range(n_streams)]
    batch = lio.Batch(the_map, n_slots=args.slots, n_groups=args.groups, max_raw=1 << 17, max_ds=100000) if args.engine == "batch" else None

    def run_jobs(jl):
        return batch.process(jl) if batch is not None else lio.process_batch(engines, jl)
    for e in engines:
        e.set_flags(ekf_inited=True, first_scan=False, travel=0.0, first_lidar_time=-10.0)
    eng = engines[0]
    P0 = lio.init_cov()
    map_points, map_voxels = the_map.stats()

    def step(i, e=None):
        e = e or eng
        s = scans[i % len(scans)]
        e.set_state(s["guess"])
        e.set_cov(P0)
        rc = e.process_scan_device(d_scans[i % len(scans)].data_ptr(), len(s["raw"]), 1.0 + 0.1 * i)
        if rc != 3:
            raise RuntimeError(f"process_scan returned {rc}")

    # Setup, untimed: push enough launches through every engine's stream for the HIP runtime to finish growing its
    # per-queue pools -- a one-off ~35 ms stall shows up after roughly 190 scans (~5 000 kernel launches) of a fresh
    # process and never again (tools/experiments/README.md); a service hits it once at start-up.
    # The batched engine's first calls instantiate a graph per round in flight: the setup pushes two full sets of rounds through it.
    def job_of(i, pool=None):
        s = (pool or scans)[i % len(pool or scans)]
        return dict(dptr=s["d"].data_ptr(), n=len(s["raw"]), t=1.0 + 0.1 * i, state=s["guess"], cov=P0)

    run_jobs([job_of(i) for i in range(max(40 * n_streams, 2 * args.slots * args.groups if batch is not None else 0))])
    torch.cuda.synchronize()
    if args.warmup > 0:  # --warmup scans through the timed path itself
        lio.run_prepared(lio.PreparedJobs([job_of(i) for i in range(args.warmup)]), engines=engines, batch=batch)
        torch.cuda.synchronize()
    pose_err, ang_err, latency_ms = 0.0, 0.0, None
    if args.full:
        for i in range(args.warmup):
            step(i, engines[i % n_streams])
        # pose check outside the timed region: every pooled scan must land on its true pose
        for k in range(len(scans)):
            step(k)
            st = eng.get_state()
            pose_err = max(pose_err, float(np.linalg.norm(st[:3] - scans[k]["pos"])))
            ang_err = max(ang_err, float(synth.quat_angle(st[3:7], scans[k]["q"])))

        # single-stream latency of one scan (reported beside the throughput; not the timed region)
        torch.cuda.synchronize()
        l0 = time.perf_counter()
        for i in range(20):
            step(i)
        latency_ms = 1e3 * (time.perf_counter() - l0) / 20
    if args.full and batch is None:
        for e in engines:
            e.scan.enable_kernel_timing(1)  # the dominant kernel only: two event records per kNN launch in the timed region
            e.scan.kernel_times(reset=True)
    acc = dict(n_ds=0, n_pass=0, n_knn=0, pts=0)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # the timed region is ONE C-ABI call: the K = --steps independent scans (each with its own initial state / covariance), handed to
    # the device in batches by C++ (no Python in the loop), ms_per_step = t / K.  --min-seconds S > 0: the same list is repeated R times
    # inside the call instead, R from an untimed calibration pass so that the region lasts at least S, and ms_per_step = t / (K R).
    # ... and of the same scans one at a time through a ONE-slot batch: the whole registration (downsample chain, five passes of search / linearise /
    # filter step on the device) as one captured graph and one hipGraphLaunch, against the host-driven per-pass loop above
    latency_graph_ms = None
    if rank == 0 and world == 1 and args.full and args.secondary:  # (not in the short forms the profiling passes run: its one-slot launches would enter their per-kernel averages)
        try:
            b1 = lio.Batch(the_map, n_slots=1, n_groups=1, max_raw=1 << 17, max_ds=100000)
            for i in range(4):
                b1.process([job_of(i)])
            l0 = time.perf_counter()
            for i in range(20):
                b1.process([job_of(i)])
            latency_graph_ms = 1e3 * (time.perf_counter() - l0) / 20
            del b1
        except Exception:
            latency_graph_ms = None

    repeats = 1
    min_seconds = args.min_seconds or 0.0
    if min_seconds > 0:
        # calibration pass: long enough to fill every round in flight several times (a list shorter than slots x groups runs un-pipelined and
        # over-estimates the time per scan: round 4's first line had a 1.4 s region for --min-seconds 5)
        n_cal = max(8 * args.steps, 6 * args.slots * args.groups if batch is not None else 8 * n_streams)
        cal = lio.PreparedJobs([job_of(i) for i in range(n_cal)])
        lio.run_prepared(cal, engines=engines, batch=batch)  # (once untimed: graphs instantiated, pools grown)
        torch.cuda.synchronize()
        c0 = time.perf_counter()
        lio.run_prepared(cal, engines=engines, batch=batch)
        torch.cuda.synchronize()
        t_cal = max(time.perf_counter() - c0, 1e-6) * args.steps / n_cal  # seconds per --steps scans
        repeats = max(1, int(np.ceil(1.1 * min_seconds / t_cal)))
        if dist is not None:  # the same R on every rank
            tr = torch.tensor([float(repeats)], device=dev, dtype=torch.float64)
            dist.all_reduce(tr, op=dist.ReduceOp.MAX)
            repeats = int(tr.item())
    # K x R jobs walking through the WHOLE pool (job i = scan i mod pool): with --steps 20 the list used to be the first 20 scans repeated R times
    timed_jobs = [job_of(i) for i in range(args.steps * repeats)]
    prep = lio.PreparedJobs(timed_jobs)  # marshalled into the C ABI's job array BEFORE the clock starts: the timed region is the one C call
    cand0 = the_map.knn_candidates
    barrier()
    t0 = time.perf_counter()
    rc = lio.run_prepared(prep, engines=engines, batch=batch)
    torch.cuda.synchronize()
    t_local = time.perf_counter() - t0
    results = prep.results()
    if rc != 0 or any(r["rc"] != 3 for r in results):
        raise RuntimeError(f"process_batch failed: {rc} {[r['rc'] for r in results][:8]}")
    for i, r in enumerate(results):
        acc["n_ds"] += r["n_ds"]
        acc["n_pass"] += r["n_pass"]
        acc["n_knn"] += r["n_knn_pass"]
        acc["pts"] += len(scans[i % len(scans)]["raw"])
    n_timed = len(timed_jobs)
    barrier()
    t_max = t_local
    total_pts = acc["pts"]
    if dist is not None:
        tt = torch.tensor([t_local], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        t_max = float(tt.item())
        tp = torch.tensor([float(acc["pts"])], device=dev, dtype=torch.float64)
        dist.all_reduce(tp, op=dist.ReduceOp.SUM)
        total_pts = float(tp.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, results, len(scans))

    cand = the_map.knn_candidates - cand0
    S = 19
    n_ds_avg, n_pass_avg, n_knn_avg = acc["n_ds"] / n_timed, acc["n_pass"] / n_timed, acc["n_knn"] / n_timed
    # the checks below take scan i of the pool from job i of the timed call; a call shorter than the pool is completed by an untimed one
    pool_results = results[: len(scans)]
    if args.full and len(pool_results) < len(scans):
        rest = lio.PreparedJobs([job_of(i) for i in range(len(pool_results), len(scans))])
        lio.run_prepared(rest, engines=engines, batch=batch)
        pool_results = pool_results + rest.results()
    # ---- the same workload with the upload INCLUDED (t_scan upload excluded and included, both reported): the pool's clouds in
    # page-locked HOST memory, every job LIO_JOB_HOST_RAW -- the library copies a round's clouds to HBM on the round's stream, beside the kernels of the
    # other rounds in flight (the reference's path starts with this copy: slam/src/py_utils.cpp:149-181, slam_wrapper.cpp:64-84).  Same C call, same jobs.
    upload = None
    if args.full and batch is not None and args.upload_scans != 0:
        try:
            pinned = [lio.PinnedCloud(sc["raw"]) for sc in scans]

            def job_host(i):
                sc, pc = scans[i % len(scans)], pinned[i % len(scans)]
                return dict(dptr=pc.ptr, n=pc.n, t=1.0 + 0.1 * i, state=sc["guess"], cov=P0, flags=lio.JOB_HOST_RAW)

            n_up = args.upload_scans if args.upload_scans > 0 else int(max(4 * args.slots * args.groups, np.ceil(2.5 / max(t_local / n_timed, 3.5e-5))))
            lio.run_prepared(lio.PreparedJobs([job_host(i) for i in range(2 * args.slots * args.groups)]), batch=batch)  # (raw rings allocated, untimed)
            prep_up = lio.PreparedJobs([job_host(i) for i in range(n_up)])
            barrier()
            u0 = time.perf_counter()
            rc_up = lio.run_prepared(prep_up, batch=batch)
            torch.cuda.synchronize()
            t_up = time.perf_counter() - u0
            res_up = prep_up.results()
            same_up = rc_up == 0 and all(r["rc"] == 3 and np.array_equal(r["state"], pool_results[i % len(scans)]["state"]) for i, r in enumerate(res_up))
            bytes_up = float(sum(16 * len(scans[i % len(scans)]["raw"]) for i in range(n_up)))
            if dist is not None:
                tu = torch.tensor([t_up], device=dev, dtype=torch.float64)
                dist.all_reduce(tu, op=dist.ReduceOp.MAX)
                t_up = float(tu.item())
            upload = {"ms_per_step": round(1e3 * t_up / n_up, 4), "value": round(world * bytes_up / 16.0 / t_up, 1), "unit": "points/s", "timed_scans": n_up,
                      "timed_seconds": round(t_up, 4), "host_bytes_per_scan": int(bytes_up / n_up), "pcie_GBps": round(bytes_up / t_up / 1e9, 2),
                      "parity_ok": bool(same_up),
                      "what": "the timed region's jobs with the clouds in pinned host memory (lio_pinned_alloc) and LIO_JOB_HOST_RAW: hipMemcpyAsync of a round's "
                              "clouds on the round's stream, overlapped with the other rounds in flight; results bit-identical to the resident run's (parity_ok)"}
            del prep_up, pinned
        except Exception as ex:  # the headline must not depend on this leg
            upload = {"error": repr(ex)[-300:]}
    # ---- roofline of the dominant kernel (stencil kNN) ------------------------------------------------------------------------------
    # algorithmic bytes [SURVEY.md 8d]: B_knn = N_ds * (16 query + 16 * S slot probes) + 16 * (points resident in the probed voxels), per
    # scan and neighbour-search pass; the kernel's time from HIP events recorded on the streams it is launched on.  Timed OUTSIDE the
    # timed region (event records cost host time) with the device to the kernel itself -- one round in flight -- which is what
    # rocprofv3's per-kernel duration of the same command measures as well.
    others = {}

    def solo_leg(map_, sj):
        """one round in flight on its own batch object, HIP events around every kernel class (lio_batch_enable_kernel_timing), then the same jobs
        through the kNN kernel's counting variant: the figures of the dominant kernel's roofline for the jobs `sj` against `map_`"""
        solo = lio.Batch(map_, n_slots=args.slots, n_groups=1, max_raw=1 << 17, max_ds=100000)
        solo.process(sj[: 2 * args.slots])  # warm
        solo.enable_kernel_timing(True)
        solo.kernel_times(reset=True)
        c1 = map_.knn_candidates
        rc_s, res_s = solo.process(sj)
        kt = solo.kernel_times(reset=True)
        solo.enable_kernel_timing(False)
        n_search = sum(r["n_ds"] * r["n_knn_pass"] for r in res_s)  # queries, all searches
        searches = max(sum(r["n_knn_pass"] for r in res_s), 1)
        cand_pts = map_.knn_candidates - c1
        launches = max(int(kt["knn_launches"]), 1)
        rounds = max(int(kt["downsample_launches"]), 1)
        leg = {"us": kt["knn_us"] / launches, "launches": launches, "bytes": (n_search * (16 + 16 * S) + 16.0 * cand_pts) / launches,
               "queries_per_launch": n_search / launches, "candidates_per_query": cand_pts / max(n_search, 1),
               "others": {"downsample_chain_per_round": round(kt["downsample_us"] / rounds, 2),
                          "linearize_per_launch": round(kt["linearize_us"] / max(int(kt["linearize_launches"]), 1), 2),
                          "filter_pass_per_launch": round(kt["step_us"] / max(int(kt["step_launches"]), 1), 2),
                          "knn_per_scan_and_search": round(kt["knn_us"] / searches, 2),
                          "device_time_per_scan_one_round_in_flight": round((kt["downsample_us"] + kt["knn_us"] + kt["linearize_us"] + kt["step_us"]) / len(sj), 2)}}
        # the same jobs once more through the COUNTING variant of the kernel: the candidate points the pruned sweep really loads ("touched")
        solo.enable_kernel_timing(2)
        solo.kernel_times(reset=True)
        t0c, u0c = map_.knn_touched, map_.knn_unique
        solo.process(sj)
        kt2 = solo.kernel_times(reset=True)
        solo.enable_kernel_timing(False)
        leg["touched_bytes"] = (n_search * (16 + 16 * S) + 16.0 * (map_.knn_touched - t0c)) / max(int(kt2["knn_launches"]), 1)
        # UNIQUE bytes of a launch: every query's own point and stencil slots once, every DISTINCT candidate point the launch loads once (the
        # counting variant's bitmap over the pool, cleared before each launch) -- what the launch has to move at least once whatever its caches do
        leg["unique_bytes"] = (n_search * (16 + 16 * S) + 16.0 * (map_.knn_unique - u0c)) / max(int(kt2["knn_launches"]), 1)
        leg["unique_points_per_launch"] = (map_.knn_unique - u0c) / max(int(kt2["knn_launches"]), 1)
        del solo
        return leg

    def knn_roofline(leg, traffic_file):
        """the roofline object of the batched kNN kernel from a solo_leg.  `frac` is a UTILISATION: bytes that reach the memory side (PMC FETCH_SIZE x 2 +
        WRITE_SIZE per launch, profiles/<traffic_file>, collected in their own rocprofv3 --pmc passes of this workload) over the kernel's live HIP-event
        time over the 8 TB/s peak; without a PMC file of this workload, the bytes the kernel's loads REQUEST (its counting variant on the same jobs), an
        upper bound of what reaches HBM.  The reference algorithm's bytes (every point of the 19 stencil voxels of every query) are credit
        for work the exactly pruned sweep does not do: they stand beside it as frac_algorithmic and may exceed 1.  frac_valu = the kernel's VALU
        wave-instructions per launch over the chip's MEASURED issue rate (tools/valu_peak) over the same time."""
        us = leg["us"]
        per_s = 1.0 / (us * 1e-6) if us > 0 else 0.0
        alg = leg["bytes"] * per_s / 1e9
        touched = leg["touched_bytes"] * per_s / 1e9
        unique = leg.get("unique_bytes", 0.0) * per_s / 1e9
        traffic, valu_per_wave, valu_src = None, KNN_VALU_PER_WAVE_STATIC, "static ISA count (llvm-objdump of knn.o, loop body at the average trip counts)"
        valu_per_launch = None
        tpath = os.path.join(ROOT, "profiles", traffic_file)
        if os.path.exists(tpath):  # HBM bytes per launch + VALU instructions per wave from the PMC passes (tools/pmc_traffic.py, its own rocprofv3 --pmc runs)
            try:
                tj = json.load(open(tpath))
                if tj.get("slots_per_launch", args.slots) == args.slots and tj.get("scan_pool", args.scan_pool) == args.scan_pool:
                    traffic = tj.get("hbm_bytes_per_launch")
                    if tj.get("valu_wave_instructions_per_launch"):
                        valu_per_launch = float(tj["valu_wave_instructions_per_launch"])
                        valu_src = "PMC: SQ_INSTS_VALU per launch of this kernel on the same workload (profiles/%s, its own rocprofv3 --pmc pass)" % traffic_file
            except Exception:
                traffic = None
        waves = leg["queries_per_launch"] / 4.0  # sixteen lanes per query: four queries per wave-pass (a launched wave takes several in turn)
        measured = valu_src.startswith("PMC")
        if valu_per_launch is None:
            valu_per_launch = waves * valu_per_wave
        vp = measured_valu_peak(local_rank)
        peak_rate = vp["wave_insts_per_s"] if vp else None
        # (the static count is the metric map's: ~300 candidates per query; a sparser map sweeps fewer voxels per query, so without a PMC count of THIS
        # workload the figure is an upper bound and no fraction is formed from it)
        valu_ok = us > 0 and peak_rate and (measured or abs(leg["candidates_per_query"] - 300.0) < 60.0)
        frac_valu = round(valu_per_launch / peak_rate / (us * 1e-6), 4) if valu_ok else None
        mem = traffic * per_s / 1e9 if traffic else touched
        return dict(bound="hbm", limited_by="latency / VALU issue (no MFMA on this path): frac_valu beside the byte fractions",
                    kernel="knn_batch_kernel<2, false> (16 lanes per query, %d scans per launch)" % args.slots,
                    achieved=round(mem, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(mem / HBM_PEAK_GBS, 4),
                    frac_basis=("pmc: FETCH_SIZE x 2 + WRITE_SIZE per launch (profiles/%s) over the live HIP-event time" % traffic_file) if traffic
                               else "bytes the kernel's loads request (counting variant, same jobs): no PMC pass of this workload",
                    traffic=traffic,
                    achieved_algorithmic=round(alg, 1), frac_algorithmic=round(alg / HBM_PEAK_GBS, 4),
                    touched_bytes_per_launch=int(leg["touched_bytes"]), frac_touched=round(touched / HBM_PEAK_GBS, 4),
                    unique_bytes_per_launch=int(leg.get("unique_bytes", 0)), frac_unique=round(unique / HBM_PEAK_GBS, 4),
                    unique_candidate_points_per_launch=int(leg.get("unique_points_per_launch", 0)),
                    frac_hbm_traffic=(round(traffic * per_s / 1e9 / HBM_PEAK_GBS, 4) if traffic else None),
                    frac_valu=frac_valu, valu_peak_wave_insts_per_s=(round(peak_rate, 0) if peak_rate else None),
                    valu_wave_insts_per_launch=round(valu_per_launch, 0),
                    valu={"wave_instructions_per_launch": round(valu_per_launch, 0), "per_four_queries": round(valu_per_launch / max(waves, 1.0), 1),
                          "source": valu_src, "four_query_units_per_launch": round(waves, 1), "peak_measured": vp,
                          "issue_bound_us": (round(1e6 * valu_per_launch / peak_rate, 2) if peak_rate else None),
                          "frac_of_valu_issue_peak": frac_valu},
                    algorithmic_bytes_per_launch=int(leg["bytes"]), avg_launch_us=round(us, 2), launches=leg["launches"],
                    candidates_per_query=round(leg["candidates_per_query"], 1),
                    note="frac = memory-side bytes (PMC) or requested bytes over the kernel's time over 8 TB/s: a utilisation.  frac_unique = the bytes a launch "
                         "must move at least once (its queries, their stencil slots, every DISTINCT candidate point it loads: measured by the counting "
                         "variant's bitmap) over the same time: the floor of the traffic -- frac / frac_unique says how often a byte is re-fetched.  "
                         "frac_algorithmic = the reference "
                         "algorithm's bytes (every point of the 19 stencil voxels of every query) over the same time: credit for bytes the pruned sweep does "
                         "not read, may exceed 1.  frac_touched = the bytes the exactly pruned sweep asks for.  frac_valu = VALU wave-instructions per launch "
                         "over the measured issue rate (tools/valu_peak/valu_peak.hip, run in this process)")

    roofline = None
    if args.full:
        if batch is not None:
            leg = solo_leg(the_map, [job_of(i) for i in range(max(args.slots * 8, len(scans)))])
            iso_us, iso_bytes, iso_launches, others, touched_bytes = leg["us"], leg["bytes"], leg["launches"], leg["others"], leg["touched_bytes"]
            timed_region = None
        else:
            kt = dict(knn_us=0.0, linearize_us=0.0, finalize_us=0.0, knn_launches=0, linearize_launches=0, finalize_launches=0)
            for e in engines:
                k1 = e.scan.kernel_times(reset=True)
                for k in kt:
                    kt[k] += k1[k]
                e.scan.enable_kernel_timing(0)
            eng.scan.enable_kernel_timing(1)
            eng.scan.kernel_times(reset=True)
            cand1 = the_map.knn_candidates
            for i in range(32):
                step(i)
            k1 = eng.scan.kernel_times(reset=True)
            iso_launches = max(int(k1["knn_launches"]), 1)
            iso_us = k1["knn_us"] / iso_launches
            iso_bytes = n_ds_avg * (16 + 16 * S) + 16.0 * (the_map.knn_candidates - cand1) / iso_launches
            eng.scan.enable_kernel_timing(2)
            eng.scan.kernel_times(reset=True)
            for i in range(16):
                step(i)
            k2 = eng.scan.kernel_times(reset=True)
            eng.scan.enable_kernel_timing(0)
            others = {"linearize+report": round(k2["linearize_us"] / max(k2["linearize_launches"], 1), 2)}
            launches = max(int(kt["knn_launches"]), 1)
            knn_bytes = n_ds_avg * (16 + 16 * S) + 16.0 * cand / launches
            knn_us = kt["knn_us"] / launches
            shared = knn_bytes / (knn_us * 1e-6) / 1e9 if knn_us > 0 else 0.0
            timed_region = {"avg_launch_us": round(knn_us, 2), "launches": launches, "achieved": round(shared, 1), "frac": round(shared / HBM_PEAK_GBS, 4),
                            "streams": n_streams}
            kernel_name = "knn_kernel<2, 0> (16 lanes per query)"
        achieved = iso_bytes / (iso_us * 1e-6) / 1e9 if iso_us > 0 else 0.0
        # ---- the whole scan against the roofline, as SURVEY.md 8d defines it: B_scan = B_ds + n_knn B_knn + n_pass B_lin (+ B_ins, none against a
        # static map) over the scan's wall time in the timed region ----
        b_ds = 16.0 * n_raw + 16.0 * n_ds_avg
        b_knn = n_ds_avg * (16 + 16 * S) + 16.0 * cand / max(acc["n_knn"], 1)
        b_lin = n_ds_avg * (16 + 5 * 16) + 16.0 * n_ds_avg + 8 * 32 * np.ceil(n_ds_avg / 64)
        b_scan = b_ds + n_knn_avg * b_knn + n_pass_avg * b_lin
        # the device's own copy rate (report the fraction of the nominal AND of a measured peak): 1 GiB device-to-device copies,
        # read + write counted, torch events on torch's stream (nothing of the hot path is in flight here)
        copy_peak = None
        try:
            nbytes = 1 << 30
            src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            for _ in range(3):
                dst.copy_(src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            copy_peak = round(2.0 * nbytes * 10 / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)
            del src, dst
        except Exception:
            copy_peak = None
        t_scan = t_max / n_timed
        if batch is not None:
            roofline = knn_roofline(leg, "knn_batch_traffic.json")
        else:
            roofline = dict(bound="hbm", kernel=kernel_name, achieved=round(achieved, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(achieved / HBM_PEAK_GBS, 4),
                            traffic=None, algorithmic_bytes_per_launch=int(iso_bytes), avg_launch_us=round(iso_us, 2), launches=iso_launches, per_stream=timed_region)
        roofline.update(measured_copy_peak=copy_peak, frac_of_measured_copy_peak=(round(roofline["achieved"] / copy_peak, 4) if copy_peak else None),
                        timed_region=round(t_max, 4), timed_region_s=round(t_max, 4), other_kernels_us=others,
                        whole_scan={"algorithmic_bytes_per_scan": int(b_scan), "seconds_per_scan": t_scan, "credit_GBps": round(b_scan / t_scan / 1e9, 1),
                                    "credit_over_peak": round(b_scan / t_scan / 1e9 / HBM_PEAK_GBS, 4),
                                    "what": "SURVEY 8d's bytes of the REFERENCE algorithm per scan (every point of the 19 stencil voxels of every query counted) over "
                                            "the scan's wall time: credit for work the exactly pruned, cache-shared sweep does not do -- NOT a bandwidth utilisation (the "
                                            "kernels' own are roofline.frac and configs.*.roofline)",
                                    "terms": {"B_ds": int(b_ds), "B_knn": int(b_knn), "n_knn": round(n_knn_avg, 2), "B_lin": int(b_lin), "n_pass": round(n_pass_avg, 2),
                                              "B_ins": 0, "note": "B_ins = 0: the metric's map is static (BASELINE config 2 / the headline: independent scans against a "
                                                                  "fixed map, no map_incremental); the insert is timed in configs.config3_* and configs.sequence_batch"}})

    # ---- CPU baseline: the oracle restatement of the same path on a bounded sample of the same workload ---------
    cpu = None
    batch_vs_oracle = None
    if args.full and rank == 0 and world == 1 and args.cpu_scans > 0:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle  # test infrastructure; used here only as the timed CPU baseline / checker

        threads = min(8, usable_cpus())  # the reference parallelises the kNN loop over MP_PROC_NUM = 8 threads; fewer if the box has fewer
        o = oracle.Lio(res=0.5, stencil=19, capacity=1 << 40, threads=threads)
        o.map_add(map_pts)
        o.set_flags(ekf_inited=True, first_scan=False, travel=0.0, first_lidar_time=-10.0)
        t_cpu, pts_cpu, worst_dp, worst_da = 0.0, 0, 0.0, 0.0
        batch_dp, batch_da, batch_ds, batch_checked, pass_mismatch = 0.0, 0.0, 0.0, 0, []
        for i in range(args.cpu_scans):
            s = scans[i % len(scans)]
            parity = i < len(scans)
            if parity:  # equal histories: the neighbour cache (Nearest_Points) persists across scans on both sides
                o.reset_cache()
                eng.scan.reset()
            o.set_state(s["guess"])
            o.set_cov(P0)
            c0 = time.perf_counter()
            ds = oracle.voxel_downsample(s["raw"], 0.5)
            o.set_ds(ds)
            lo_passes = o.update()
            t_cpu += time.perf_counter() - c0
            pts_cpu += len(s["raw"])
            if parity:  # full-size parity: GPU pose vs oracle pose on the same scan
                step(i)
                sg, so = eng.get_state(), o.get_state()
                worst_dp = max(worst_dp, float(np.linalg.norm(sg[:3] - so[:3])))
                worst_da = max(worst_da, float(synth.quat_angle(sg[3:7], so[3:7])))
                if batch is not None and i < len(pool_results):
                    # ... and the TIMED path itself: the state the batched engine returned for this scan inside the timed region (job i of the timed
                    # list = scan i of the pool; jobs are independent scans, so every later repeat of it must carry the same bits -- checked below)
                    rb = pool_results[i]
                    if (rb["n_pass"], rb["n_knn_pass"]) != (len(lo_passes), sum(p["knn"] for p in lo_passes)):
                        pass_mismatch.append([i, rb["n_pass"], rb["n_knn_pass"], len(lo_passes), sum(p["knn"] for p in lo_passes)])
                    batch_dp = max(batch_dp, float(np.linalg.norm(rb["state"][:3] - so[:3])))
                    batch_da = max(batch_da, float(synth.quat_angle(rb["state"][3:7], so[3:7])))
                    batch_ds = max(batch_ds, float(np.abs(rb["state"] - so).max()))
                    batch_checked += 1
        batch_vs_oracle = None
        if batch is not None:
            same = all(np.array_equal(results[i]["state"], pool_results[i % len(scans)]["state"]) for i in range(len(results)))
            batch_vs_oracle = {"max_dpos_m": batch_dp, "max_drot_rad": batch_da, "max_dstate": batch_ds, "scans_checked": batch_checked,
                               "all_timed_results_bit_identical_to_the_checked_ones": bool(same), "timed_results": len(results),
                               "pass_structure_mismatches": pass_mismatch, "parity_ok": bool(same and batch_ds <= 1e-9 and not pass_mismatch),
                               "note": f"state_out of the timed lio_batch_process call itself ({args.slots} slots x {args.groups} rounds in flight, one hipGraphLaunch per round) against the "
                                       "oracle's registration of the same scan; same pass / search counts required"}
            if not batch_vs_oracle["parity_ok"]:  # reported in the line (parity_ok: false) and on stderr; the measurement itself stands
                print(f"bench.py: PARITY FAILURE -- batched engine differs from the oracle on the timed jobs: {batch_vs_oracle}", file=sys.stderr)
        port = dict(value=round(pts_cpu / t_cpu, 1), unit="points/s", cores=threads, kind="port",
                    sample=f"{args.cpu_scans} scans of the same workload (oracle/lio_oracle.cpp: VoxelGrid + iVox kNN on {threads} OpenMP threads + "
                           f"esti_plane + iterated ESKF, rest single-threaded as in the reference), {t_cpu:.1f} s",
                    ms_per_scan=round(1e3 * t_cpu / args.cpu_scans, 2),
                    gpu_vs_oracle_pose={"max_dpos_m": worst_dp, "max_drot_rad": worst_da}, batch_vs_oracle_pose=batch_vs_oracle)
        cpu = port
        # ---- the reference's OWN code on the same workload: laserMapping.cpp / iVox / IKFoM compiled from /root/reference with the
        # flags of its CMakeLists.txt (oracle/ref_fastlio.cpp, prebuilt into oracle/_ref by build(); travels to the GPU box) -----
        import ref_fastlio  # oracle/ref_fastlio.py

        if args.ref_scans > 0 and ref_fastlio.available(release=True):
            del o
            ref_fastlio.use_release_build()
            R = ref_fastlio.RefFastLio()
            R.set_logging(False)
            R.map_add(map_pts)
            R.set_nearby(18)
            t_ref, pts_ref, ref_dp, ref_da = 0.0, 0, 0.0, 0.0
            per_scan = []  # (|dpos|, |drot|, GPU state) against the reference's own code, scan by scan
            for i in range(args.ref_scans):
                s = scans[i % len(scans)]
                parity = i < len(scans)
                if parity:
                    R.reset_cache()
                    eng.scan.reset()
                c0 = time.perf_counter()
                rc_ref, sr, _ = R.register(s["raw"], s["guess"], P0)
                t_ref += time.perf_counter() - c0
                pts_ref += len(s["raw"])
                if rc_ref != 3:
                    raise RuntimeError(f"reference registration returned {rc_ref}")
                if parity:  # GPU pose vs the reference's pose (neighbour order and dense-algebra rounding differ: tolerance, not bits)
                    step(i)
                    sg = eng.get_state()
                    ref_dp = max(ref_dp, float(np.linalg.norm(sg[:3] - sr[:3])))
                    ref_da = max(ref_da, float(synth.quat_angle(sg[3:7], sr[3:7])))
                    per_scan.append((float(np.linalg.norm(sg[:3] - sr[:3])), float(synth.quat_angle(sg[3:7], sr[3:7])), sg.copy(), np.array(sr, dtype=np.float64).copy()))
            # `R` is the reference's code built with ITS flags (-O3 -DNDEBUG: Eigen vectorised, the compiler free to contract) -- the build that is
            # timed.  The build the path is PINNED to is the other one (oracle/_ref/libref_fastlio.so: scalar Eigen, no contraction -- DESIGN.md
            # section 4: Eigen's operation order depends on the build, and esti_plane's 5 x 3 QR is ill-conditioned for planes through the map
            # frame's origin, which this scene's ground z = 0 is).  One build per process (both define the reference's file-scope globals): the
            # pinned build registers the same scans in a child process, once as it is (neighbours 1..4 in std::nth_element's order) and once with
            # every search's lists sorted into the oracle's canonical order (ref_fl_set_canonical).
            gvr = {"build": "the reference's own flags (-O3 -DNDEBUG, vectorised Eigen): the build that is timed", "max_dpos_m": ref_dp, "max_drot_rad": ref_da,
                   "scans": len(per_scan)}
            if per_scan:
                dps, das = np.array([p[0] for p in per_scan]), np.array([p[1] for p in per_scan])
                w = int(np.argmax(dps))
                gvr.update(median_dpos_m=float(np.median(dps)), p90_dpos_m=float(np.percentile(dps, 90)),
                           scans_beyond_1e_4_m_or_1e_5_rad=int(np.count_nonzero((dps > 1e-4) | (das > 1e-5))),
                           worst_scan={"index": w, "seed": scans[w]["seed"], "dpos_m": float(dps[w]), "drot_rad": float(das[w]),
                                       "pose_error_vs_truth_m": float(np.linalg.norm(per_scan[w][2][:3] - scans[w]["pos"]))})
                try:
                    import subprocess
                    import tempfile

                    del R
                    m_par = min(len(per_scan), args.parity_scans)
                    # the same scans once more with the neighbour lists in the reference's own ORDER (lio_map_set_tie_mode 2: every query through the
                    # reference's selection, a checker ~100 x the search's cost): what the pinned build is compared with AS IT IS, nothing sorted on either side
                    mode2 = {}
                    try:
                        the_map.set_tie_mode(2)
                        for i in range(m_par):
                            eng.scan.reset()
                            step(i)
                            mode2[f"gpu2_{i}"] = eng.get_state().copy()
                    finally:
                        the_map.set_tie_mode(1)
                    with tempfile.TemporaryDirectory(prefix="lio_bench_parity_") as td:
                        np.save(os.path.join(td, "map.npy"), map_pts)
                        np.savez(os.path.join(td, "scans.npz"), P0=P0, n=m_par, **{f"raw{i}": scans[i]["raw"] for i in range(m_par)},
                                 **{f"guess{i}": scans[i]["guess"] for i in range(m_par)}, **{f"gpu{i}": per_scan[i][2] for i in range(m_par)},
                                 **{f"rel{i}": per_scan[i][3] for i in range(m_par)}, **mode2)
                        pr = subprocess.run([sys.executable, BENCH_PY, "--config", "refparity", "--parity-dir", td], capture_output=True, text=True,
                                            timeout=600)
                    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("{")]
                    if pr.returncode != 0 or not line:
                        raise RuntimeError((pr.stderr or pr.stdout)[-300:])
                    gvr["pinned_build"] = json.loads(line[-1])
                except Exception as ex:
                    gvr["pinned_build"] = {"error": repr(ex)[-300:]}
            cpu = dict(value=round(pts_ref / t_ref, 1), unit="points/s", cores=min(8, usable_cpus()), host_cpus=usable_cpus(), kind="reference",
                       sample=f"{args.ref_scans} scans of the same workload through the reference's own laserMapping.cpp h_share_model + iVox + esekfom "
                              f"update_iterated_dyn_share_modified (oracle/_ref/libref_fastlio_release.so: -O3 -DNDEBUG, MP_EN with MP_PROC_NUM=8 as its "
                              f"CMakeLists.txt sets on x86_64; pcl::VoxelGrid replaced by the oracle's restatement), {t_ref:.1f} s",
                       ms_per_scan=round(1e3 * t_ref / args.ref_scans, 2),
                       gpu_vs_reference_pose=gvr, port=port)

    # ---- secondary configurations (BASELINE.json configs 2 and 3), outside the timed region, reported under `configs` ----
    configs = None
    if args.full and rank == 0 and world == 1 and args.secondary and batch is not None:
        configs = {}
        def timed_leg(b_, jl, seconds):
            """jl through the batch b_ once to warm, then repeated for about `seconds`: (ms per scan, points/s, results of the first pass)"""
            rc0, r0 = b_.process(jl)
            if rc0 != 0 or any(r["rc"] != 3 for r in r0):
                raise RuntimeError(f"secondary leg failed: {rc0}")
            pw = lio.PreparedJobs(jl)
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            lio.run_prepared(pw, batch=b_)
            torch.cuda.synchronize()
            reps = max(1, int(np.ceil(seconds / max(time.perf_counter() - w0, 1e-6))))
            pj = lio.PreparedJobs(jl * reps)
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            lio.run_prepared(pj, batch=b_)
            torch.cuda.synchronize()
            dt = time.perf_counter() - w0
            return 1e3 * dt / pj.n, sum(j["n"] for j in jl) * reps / dt, r0, pj.n

        try:
            # round 3's workload beside the headline: 8 scans within 4 m of one spot of the SAME map, same engine object
            j8 = [job_of(i, scans8) for i in range(args.slots * args.groups * 2)]
            ms8, pps8, r8, n8 = timed_leg(batch, j8, 1.5)
            leg8 = solo_leg(the_map, [job_of(i, scans8) for i in range(args.slots * 8)])
            configs["pool8_one_spot"] = {"workload": "round 3's timed workload: 8 distinct scans within +-4 m of the map's centre (everything L2 / Infinity-Cache resident), "
                                                     "beside the headline's pool of %d scans spread over +-%.0f m" % (len(scans), args.spread),
                                         "ms_per_scan": round(ms8, 4), "points_per_s": round(pps8, 1), "scans_timed": n8,
                                         "n_ds_avg": round(float(np.mean([r["n_ds"] for r in r8])), 1), "passes_avg": round(float(np.mean([r["n_pass"] for r in r8])), 2),
                                         "roofline": {k: v for k, v in knn_roofline(leg8, "knn_batch_traffic_pool8.json").items() if k != "note"}}
        except Exception as ex:  # the headline must not depend on the secondary legs
            configs["pool8_one_spot"] = {"error": repr(ex)[-400:]}
        try:
            # config 2: the same 64 x 1875 scans against a 1e6-point map, through the same batched engine
            d2 = synth_gpu.sample_surface(scene, 1_000_000, dev, seed=2, sigma=0.01)
            map2 = lio.Map(resolution=0.5, stencil=19, max_points=1_000_000, max_voxels=1_000_000, device=local_rank)
            torch.cuda.synchronize()
            map2.add_device(d2.data_ptr(), 1_000_000)
            map2_pts = d2.cpu().numpy()
            del d2
            b2 = lio.Batch(map2, n_slots=args.slots, n_groups=args.groups, max_raw=1 << 17, max_ds=100000)
            j2 = [job_of(i) for i in range(max(args.slots * args.groups * 2, len(scans)))]
            ms2, pps2, r2, n2 = timed_leg(b2, j2, 2.0)
            pe2 = max(float(np.linalg.norm(r2[i]["state"][:3] - scans[i % len(scans)]["pos"])) for i in range(len(j2)))
            del b2
            leg2 = solo_leg(map2, [job_of(i) for i in range(max(args.slots * 8, len(scans)))])
            c2 = {"workload": "64x%d scans (the headline's pool of %d) vs 1000000-pt static map, batched engine" % (args.n_az, len(scans)), "ms_per_scan": round(ms2, 4),
                  "points_per_s": round(pps2, 1), "scans_timed": n2,
                  "n_ds_avg": round(float(np.mean([r["n_ds"] for r in r2])), 1), "passes_avg": round(float(np.mean([r["n_pass"] for r in r2])), 2),
                  "pose_error_vs_truth_m": pe2, "roofline": knn_roofline(leg2, "knn_batch_traffic_config2.json"), "cpu_baseline": None}
            c2["roofline"]["other_kernels_us"] = leg2["others"]
            del map2
            if args.ref_scans > 0:  # same-run baseline: the reference's own code on a bounded sample of the same scans against the same 1e6 points
                import ref_fastlio

                if ref_fastlio.available(release=True):
                    ref_fastlio.use_release_build()
                    R2 = ref_fastlio.RefFastLio()
                    R2.set_logging(False)
                    R2.map_add(map2_pts)
                    R2.set_nearby(18)
                    m2 = min(40, args.ref_scans)
                    t_r2, p_r2, e_r2, dps2, das2, rel2 = 0.0, 0, 0.0, [], [], []
                    for i in range(m2):
                        sc2 = scans[i % len(scans)]
                        R2.reset_cache()
                        c0 = time.perf_counter()
                        rc_r2, sr2, _ = R2.register(sc2["raw"], sc2["guess"], P0)
                        t_r2 += time.perf_counter() - c0
                        p_r2 += len(sc2["raw"])
                        rel2.append(np.array(sr2, dtype=np.float64).copy())
                        if rc_r2 == 3:
                            dps2.append(float(np.linalg.norm(r2[i]["state"][:3] - sr2[:3])))
                            das2.append(float(synth.quat_angle(r2[i]["state"][3:7], sr2[3:7])))
                    e_r2 = max(dps2) if dps2 else 0.0
                    gvr2 = {"build": "the reference's own flags (-O3 -DNDEBUG, vectorised Eigen)", "scans": len(dps2), "max_dpos_m": e_r2,
                            "max_drot_rad": max(das2) if das2 else 0.0, "median_dpos_m": float(np.median(dps2)) if dps2 else None,
                            "scans_beyond_1e_4_m_or_1e_5_rad": int(np.count_nonzero((np.array(dps2) > 1e-4) | (np.array(das2) > 1e-5)))}
                    c2["cpu_baseline"] = dict(value=round(p_r2 / t_r2, 1), unit="points/s", cores=min(8, usable_cpus()), host_cpus=usable_cpus(), kind="reference",
                                              sample=f"{m2} scans of the same workload through the reference's own laserMapping.cpp h_share_model + iVox + esekfom update "
                                                     f"(oracle/_ref/libref_fastlio_release.so, MP_PROC_NUM=8) against the same 1e6 map points, {t_r2:.1f} s",
                                              ms_per_scan=round(1e3 * t_r2 / m2, 2), gpu_vs_reference_pose_max_dpos_m=e_r2, gpu_vs_reference_pose=gvr2)
                    del R2
                    try:  # ... and the build the path is PINNED to, in a child process (one build per process), with the release build's poses beside the GPU's
                        import subprocess
                        import tempfile

                        with tempfile.TemporaryDirectory(prefix="lio_bench_parity2_") as td:
                            np.save(os.path.join(td, "map.npy"), map2_pts)
                            np.savez(os.path.join(td, "scans.npz"), P0=P0, n=m2, **{f"raw{i}": scans[i % len(scans)]["raw"] for i in range(m2)},
                                     **{f"guess{i}": scans[i % len(scans)]["guess"] for i in range(m2)}, **{f"gpu{i}": r2[i]["state"] for i in range(m2)},
                                     **{f"rel{i}": rel2[i] for i in range(m2)})
                            pr = subprocess.run([sys.executable, BENCH_PY, "--config", "refparity", "--parity-dir", td], capture_output=True, text=True,
                                                timeout=600)
                        line = [ln for ln in pr.stdout.splitlines() if ln.startswith("{")]
                        if pr.returncode != 0 or not line:
                            raise RuntimeError((pr.stderr or pr.stdout)[-300:])
                        gvr2["pinned_build"] = json.loads(line[-1])
                    except Exception as ex:
                        gvr2["pinned_build"] = {"error": repr(ex)[-300:]}
            configs["config2_1e6_map"] = c2
        except Exception as ex:  # the headline must not depend on the secondary legs
            configs["config2_1e6_map"] = {"error": repr(ex)[-400:]}
        # configs 3 and 4 run as their own processes (their own maps: 1e7 points grown by map_incremental, a 5e7-point NDT target; this
        # process idles meanwhile, its few GB of HBM do not matter on a 288 GB part); each prints the JSON line
        # `bench.py --config stream|localize` prints, embedded here
        import subprocess

        for key, extra in (("config3_stream_to_1e7_points", ["--config", "stream", "--grow-to", "10000000", "--steps", "6000", "--lru", "0"]),
                           ("config3_stream_lru_1e5_300_sweeps", ["--config", "stream", "--steps", "300", "--lru", "100000", "--ref-scans", "300"]),
                           ("config4_localize_5e7_map", ["--config", "localize", "--steps", "200", "--scan-pool", "32"]),
                           ("config5_merge_8_submaps_1_gpu", ["--config", "merge", "--steps", "256", "--warmup", "64", "--scan-pool", "64", "--min-seconds", "2"]),
                           ("sequence_batch", ["--config", "sequences", "--steps", "24", "--slots", "128", "--groups", "2"])):
            try:
                pr = subprocess.run([sys.executable, BENCH_PY, "--full-line", "--seed", str(args.seed)] + extra, capture_output=True, text=True, timeout=900)
                line = [ln for ln in pr.stdout.splitlines() if ln.startswith("{")]
                if pr.returncode != 0 or not line:
                    raise RuntimeError((pr.stderr or pr.stdout)[-400:])
                j = json.loads(line[-1])
                configs[key] = {"ms_per_scan": j["ms_per_step"], "points_per_s": j["value"], **j["config"],
                                "roofline": j.get("roofline"), "cpu_baseline": j.get("cpu_baseline"), "pose_error_vs_truth_m": j.get("pose_error_vs_truth_m")}
                for extra_key in ("drift", "collective", "latency", "knn_on_this_map", "parity", "one_session_at_a_time", "device_us_per_round", "pose_error_vs_truth"):
                    if j.get(extra_key):
                        configs[key][extra_key] = j[extra_key]
            except Exception as ex:  # the headline must not depend on the secondary legs
                configs[key] = {"error": repr(ex)[-500:]}

    # N > 1: the metric's ranks are replicas (no data-path collective); the native communicator of the C ABI (lio_comm_*: RCCL over xGMI, what
    # config 5's joint registration runs on) is brought up once OUTSIDE the timed region and its small-message all-gather timed, so that a
    # multi-GPU run leaves a measured collective latency and the communicator's own rank count in the line
    collective = None
    if args.full and dist is not None:
        try:
            collective = rccl_probe(dist, rank, world, local_rank)
        except Exception as ex:  # the probe must never cost the run its line
            collective = {"error": repr(ex)[-300:]}
    if rank == 0:
        value = total_pts / t_max
        out = {
            "metric": "registered points/sec (120k-pt scan vs 1e7-pt map, full iterate-to-converge)",
            "value": round(value, 1), "unit": "points/s", "n_gpus": world, "rccl_ranks": (collective or {}).get("rccl_ranks", 1 if world == 1 else None),
            "collective": collective, "steps": args.steps, "warmup": args.warmup,
            "repeats": repeats, "timed_scans": n_timed, "timed_seconds": round(t_max, 4),
            "ms_per_step": round(1e3 * t_max / n_timed, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 per-point geometry / f64 transforms and reductions", "data": "synthetic",
            "config": {"workload": f"64x{args.n_az} synthetic scan (~{n_raw} pts) vs {map_points}-pt static map ({map_voxels} voxels of 0.5 m), "
                                   "voxel downsample + iterated ESKF update to convergence (map_incremental excluded: the map is static), one scan per step, "
                                   f"scans sharded across GPUs; {len(scans)} distinct scans per GPU, sensor positions uniform over +-{args.spread:.0f} m of the 200 m scene",
                       "scan_pool": len(scans), "scan_seeds": [scans[0]["seed"], scans[-1]["seed"]], "spread_m": args.spread, "frame_z_m": args.frame_z,
                       "n_raw": n_raw, "n_ds_avg": round(n_ds_avg, 1), "passes_avg": round(n_pass_avg, 2),
                       "knn_passes_avg": round(n_knn_avg, 2), "stencil": 19,
                       "knn_candidates_per_query": round(cand / max(n_ds_avg * acc["n_knn"], 1), 1),
                       "map_bytes_hbm": the_map.nbytes,
                       "engine": ("batched: %d scans per launch, %d rounds in flight, filter loop on the device, 1 host thread" % (args.slots, args.groups))
                                 if batch is not None else ("%d engines, one host thread + stream each" % n_streams),
                       "single_stream_latency_ms_per_scan": (round(latency_ms, 4) if latency_ms is not None else None),
                       "single_scan_one_graph_latency_ms": (round(latency_graph_ms, 4) if latency_graph_ms else None)},
            "pose_error_vs_truth": {"max_dpos_m": pose_err, "max_drot_rad": ang_err,
                                    "note": "the reference's algorithm itself: at most four ESKF iterations from a prior 0.3 m / 2 deg off; the GPU pose "
                                            "equals the oracle's and the reference's own (cpu_baseline.gpu_vs_*_pose)"} if args.full else None,
            "batch_vs_oracle_pose": batch_vs_oracle, "upload_included": upload, "roofline": roofline, "cpu_baseline": cpu, "configs": configs,
        }
        emit(out, "metric")
    if dist is not None:
        if collective and "did not come up" in str(collective.get("error", "")):  # a worker thread is stuck inside ncclCommInitRank: leave without the teardown
            sys.stdout.flush()
            os._exit(0)
        dist.destroy_process_group()
