#!/usr/bin/env python3
"""bench.py -- decoded shots/s + logical error rate of the MI355X sliding-window BP-OSD decoder.

Workload (BASELINE.json configs[2], the configuration the metric is quoted on): [[144,12,12]] bivariate-bicycle code,
custom circuit, R = 12 (= d) noisy rounds, p = 0.003 on all four channels, Z basis -> detector error model
1008 x 9504 (33192 edges); decoder = flooding min-sum BP (ms_scaling_factor 1.0 = ldpc's default, the reference
wrapper does not expose it) with max_iter = 50, then OSD-0; one window over the whole history (BASELINE.json names
no W/F).  `--window W F` switches to a sliding window.

A step = one pass of the hot path (detector record on device -> logical predictions + mismatch count on device)
over one batch of `--shots` DEM-sampled shots.  Inputs are generated on the device before the timed region.
One process per GPU; shots are independent so ranks share nothing but the final (errors, shots) all-reduce.

Prints ONE JSON line on rank 0: the headline and the statistics of the timed steps.  A plain run does nothing else; `--full`
adds the kernel-event pass (`roofline`), `through_api`, `cpu_baseline` and `other_configs`.  `--dump-outputs DIR` saves what the
last timed step computed (inputs are seeded: the same arguments give the same inputs).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
NUM_CU = 256               # ... 256 CUs, 4 SIMD-32 each, 2.4 GHz max clock
CLOCK_HZ = 2.4e9

_CPU = {}


def _cpu_worker(lo_hi):
    """One slice of the CPU baseline: the oracle (double precision, ldpc's update order, exact LLRs) through the same window plan."""
    import oracle as orc
    lo, hi = lo_hi
    t = time.perf_counter()
    ref, _ = orc.sliding_window_decode(_CPU["wins"], _CPU["nz"], _CPU["det"][lo:hi], _CPU["prm"])
    return lo, ref, time.perf_counter() - t


def cpu_baseline(args, circ, hz, lz, R, W, F, batch, gpu_decode, gpu_value):
    """SURVEY.md 8(d).  Denominator A (preferred): `ldpc.BpOsdDecoder` -- the reference's own decoder (decoder/bposd.py:5) -- through
    the restated per-shot loop on the same saved syndromes, whenever `import ldpc` works on this host: `cpu_baseline.kind` =
    "reference", the port kept beside it as `cpu_baseline_port`.  Denominator B (always measured): oracle/qd_oracle.c, kind "port",
    timed on one core and on every core this process may use (decoders rebuilt per worker, shot slices over a multiprocessing
    pool), on a bounded sample of the first timed batch.  ldpc is absent in the build container and on the GPU box
    (profiles/r02_probe_ldpc_stim.txt), so there the line carries B alone and says why (`cpu_baseline.reference_probe`)."""
    import multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as orc
    from quits_amd.decoder.base import spacetime, window_count
    ncpu = len(os.sched_getaffinity(0))
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            ncpu = max(1, min(ncpu, int(int(q) / int(per))))
    except (OSError, ValueError):
        pass
    ns1 = min(args.cpu_shots, args.shots)
    nsa = min(args.shots, ns1 * ncpu)
    # batch = (detectors, observables) of the first timed step, torch tensors on the device or host arrays; gpu_decode(host
    # detector array) -> host predictions of the HIP path on the same shots (tests/test_refhooks.py passes a stand-in: no GPU there)
    to_np = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    det_h = to_np(batch[0][:nsa])
    obs_h = to_np(batch[1][:nsa])
    ncr, _, _ = window_count(R, W, F)
    checks, commits, priors, updates = spacetime(circ, hz, W, F, ncr)
    wins = [{"H": checks[k], "L": commits[k], "priors": priors[k], "U": updates[k] if k < ncr else None,
             "row0": F * k * hz.shape[0]} for k in range(len(checks))]
    _CPU.update(wins=wins, nz=hz.shape[0], det=det_h, lz=lz,
                prm=orc.make_params(args.bp_method, args.schedule, args.max_iter, args.osd_method, args.osd_order, 1.0, orc.FORM_LDPC_F64))
    orc.use_native(True)      # this host's own -O3 -march=native build of the port (oracle/_native/, never shipped)
    orc.lib()
    _, ref1, cpu1_s = _cpu_worker((0, ns1))
    res = {}
    if ncpu > 1:
        sl = [(i * nsa // ncpu, (i + 1) * nsa // ncpu) for i in range(ncpu)]
        t = time.perf_counter()
        with mp.get_context("fork").Pool(ncpu) as pool:          # children never touch the GPU
            parts = sorted(pool.map(_cpu_worker, sl), key=lambda r: r[0])
        cpua_s = time.perf_counter() - t
        ref = np.concatenate([p[1] for p in parts])
    else:
        ref, cpua_s = ref1, cpu1_s
    cpu_fail = int((ref != obs_h[:len(ref)]).any(axis=1).sum())
    gpu_pred = np.asarray(gpu_decode(det_h[:len(ref)]))
    gpu_fail = int((gpu_pred != obs_h[:len(ref)]).any(axis=1).sum())
    # paired comparison on the common shots: discordant counts and McNemar's z -- "within 1 sigma" is read off these
    cf = (ref != obs_h[:len(ref)]).any(axis=1)
    gf = (gpu_pred != obs_h[:len(ref)]).any(axis=1)
    only_cpu, only_gpu = int((cf & ~gf).sum()), int((gf & ~cf).sum())
    pooled = (cpu_fail + gpu_fail) / (2.0 * len(ref))
    paired = {"fail_cpu_only": only_cpu, "fail_gpu_only": only_gpu,
              "mcnemar_z": (only_gpu - only_cpu) / float(np.sqrt(max(1, only_cpu + only_gpu))),
              "delta_ler_in_sigma_unpaired": (gpu_fail - cpu_fail) / float(np.sqrt(max(1e-30, 2.0 * pooled * (1.0 - pooled) * len(ref)))),
              "note": "same syndromes through both decoders; the CPU column computes in double on the exact channel LLRs, the device on "
                      "LLRs rounded once to the grid (non-converged min-sum is chaotic: discordant shots are expected in both directions)"}
    sample = ("first %d shots of the first timed batch, same window plan and parameters; oracle/qd_oracle.c (double precision, ldpc's "
              "update order, exact LLRs)")
    res["cpu_baseline"] = {
        "value": len(ref) / cpua_s, "unit": "shots/s", "cores": ncpu, "kind": "port",
        "sample": sample % len(ref) + ", %d processes over shot slices" % ncpu, "build": orc.build_info()["flags"],
        "label": "own C port of ldpc's published algorithm (ldpc itself is absent here and on the GPU box): a readable restatement, "
                 "not a tuned CPU decoder -- any GPU/CPU ratio quoted from it carries that caveat",
        "ler": cpu_fail / len(ref), "gpu_ler_same_sample": gpu_fail / len(ref),
        "shots_with_identical_prediction": float((ref == gpu_pred).all(axis=1).mean()), "paired": paired,
        "speedup_vs_all_cores": gpu_value / (len(ref) / cpua_s)}
    res["cpu_baseline_1core"] = {"value": ns1 / cpu1_s, "unit": "shots/s", "cores": 1, "kind": "port", "sample": sample % ns1 + ", one thread",
                                 "speedup_vs_cpu_core": gpu_value / (ns1 / cpu1_s)}
    # ---- denominator A: ldpc itself, when this host has it
    import refhooks
    ldpc_cls, ldpc_info = refhooks.probe_ldpc()
    if ldpc_cls is None or args.osd_method.startswith("lsd"):
        res["cpu_baseline"]["reference_probe"] = "ldpc.bposd_decoder.BpOsdDecoder not importable on this host (%s): the port is the only CPU denominator" % ldpc_info \
            if ldpc_cls is None else "BP-LSD run: the ldpc leg times BpOsdDecoder only"
        return res
    nref = min(len(ref), max(ncpu, int(args.ref_shots) * ncpu))
    opts = dict(bp_method=args.bp_method, schedule=args.schedule, max_iter=args.max_iter, osd_method=args.osd_method, osd_order=args.osd_order)
    rpred, n1, t1, ta = refhooks.ldpc_window_loop(det_h[:nref], circ, hz, _CPU["lz"], W, F, opts, ncpu=ncpu, cls=ldpc_cls)
    rf = (rpred != obs_h[:nref]).any(axis=1)
    gfr = gf[:nref]
    o_ref, o_gpu = int((rf & ~gfr).sum()), int((gfr & ~rf).sum())
    res["cpu_baseline_port"] = res["cpu_baseline"]
    res["cpu_baseline"] = {
        "value": nref / ta, "unit": "shots/s", "cores": ncpu, "kind": "reference",
        "sample": "first %d shots of the first timed batch through ldpc %s BpOsdDecoder(%s) in the reference's per-shot loop "
                  "(sliding_window.py:143-186 restated), %d processes over shot slices" % (nref, ldpc_info, ", ".join("%s=%r" % kv for kv in sorted(opts.items())), ncpu),
        "one_core_shots_per_s": n1 / t1, "ler": float(rf.mean()), "gpu_ler_same_sample": float(gfr.mean()),
        "shots_with_identical_prediction": float((rpred == gpu_pred[:nref]).all(axis=1).mean()),
        "port_identical_prediction": float((rpred == ref[:nref]).all(axis=1).mean()),
        "paired": {"fail_ref_only": o_ref, "fail_gpu_only": o_gpu, "mcnemar_z": (o_gpu - o_ref) / float(np.sqrt(max(1, o_ref + o_gpu)))},
        "speedup_vs_all_cores": gpu_value / (nref / ta)}
    return res


def through_api(args, circ, hz, lz, W, F, sampler, device_resident_rate):
    """The drop-in call itself, as the reference's users make it (bposd.py:54-86; doc/06B_end_to_end_demo_bb.ipynb cell 5 calls it
    once per physical error rate): sliding_window_bposd_circuit_mem(bool ndarray [N, detectors] on the HOST, circuit, hz, lz, W, F,
    ...) -> int64 ndarray [N, k].  Timed cold (empty plan cache: DEM extraction, spacetime(), graph upload, workspaces) and warm
    (same arguments again: the cached plan; the samples stream through pinned staging buffers beside the decoding)."""
    from quits_amd.decoder import sliding_window_bposd_circuit_mem
    from quits_amd.decoder import sliding_window as sw
    ndet = int(sampler.m) if hasattr(sampler, "m") else None
    N = int(args.api_shots)
    pieces, obs_pieces = [], []
    done = 0
    while done < N:
        nb = min(1 << 17, N - done)
        det, obs = sampler.sample(nb, seed=7, shot0=done)
        pieces.append(det.cpu().numpy().astype(np.bool_))
        obs_pieces.append(obs.cpu().numpy())
        done += nb
        if sum(p.nbytes for p in pieces) >= (1 << 30):
            break
    det_host = np.concatenate(pieces)                       # plain (pageable) host memory, as a caller would hold it
    obs_host = np.concatenate(obs_pieces)
    N = det_host.shape[0]
    del pieces, obs_pieces
    kw = dict(max_iter=args.max_iter, osd_order=args.osd_order, bp_method=args.bp_method, schedule=args.schedule, osd_method=args.osd_method)
    sw.plan_cache_clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pred = sliding_window_bposd_circuit_mem(det_host, circ, hz, lz, W, F, **kw)
    cold = time.perf_counter() - t0
    warm = []
    for _ in range(3):
        t0 = time.perf_counter()
        pred2 = sliding_window_bposd_circuit_mem(det_host, circ, hz, lz, W, F, **kw)
        warm.append(time.perf_counter() - t0)
    assert pred.dtype == np.int64 and pred.shape == (N, obs_host.shape[1]) and np.array_equal(pred, pred2)
    info = sw.plan_cache_info()
    # the notebooks' pattern: the same call at ANOTHER physical error rate (a new plan, but the circuit's structure is known:
    # quits_amd/dem.py replays the probabilities instead of analysing the circuit again)
    other_p_s = None
    try:
        import helpers
        from quits_amd.dem import Circuit
        if args.code == "bb144":
            p2 = 0.002 if abs(args.p - 0.002) > 1e-9 else 0.004
            circ2 = Circuit(helpers.circuit_text("bb144_custom_r12_p%g" % p2))
        else:
            fixture_p = {"bb72": 0.003, "hgp225": 0.01, "qlp1020": 0.003}[args.code]
            name = {"bb72": "bb72_custom_r6_p0.003", "hgp225": "hgp225_cardinal_r3_p0.01", "qlp1020": "qlp1020_cardinal_r20_p0.003"}[args.code]
            circ2 = Circuit(helpers.circuit_text_at_p(name, fixture_p, (args.p_override or fixture_p) * 0.5))
        nsmall = min(N, 65536)
        t0 = time.perf_counter()
        sliding_window_bposd_circuit_mem(det_host[:nsmall], circ2, hz, lz, W, F, **kw)
        other_p_s = time.perf_counter() - t0
    except Exception as exc:      # (a fixture that is not there: the measurement is optional)
        other_p_s = "skipped: %s" % exc
    pl = float((pred != obs_host).any(axis=1).mean())
    best = min(warm)
    return {"call": "sliding_window_bposd_circuit_mem(bool ndarray [%d, %d] on the host, circuit, hz, lz, %d, %d, ...) -> int64 [%d, %d]"
                    % (N, det_host.shape[1], W, F, N, pred.shape[1]),
            "shots": N, "cold_s": cold, "warm_s": warm, "warm_shots_per_s": N / best, "cold_shots_per_s": N / cold,
            "warm_over_device_resident": (N / best) / device_resident_rate, "logical_error_rate": pl,
            "plan_cache": info, "first_call_at_another_p_s": other_p_s,
            "note": "cold = empty plan cache (DEM extraction + spacetime() + graph upload + workspaces inside the call); warm = the "
                    "same call again (cached plan; host array streamed in pinned pieces beside the decoding, predictions back through "
                    "a pinned buffer, .astype(int64) on the host included); first_call_at_another_p_s = the call on 65 536 shots with the "
                    "same circuit at another physical error rate (new plan; DEM structure replayed, graphs and workspaces built)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shots", type=int, default=1048576,
                    help="shots per step per GPU: 2^20 >= the 10^6 shots BASELINE configs[2] names, so one step is one whole experiment point "
                         "(decoded in chunks of 65536: a chunk's OSD runs beside the next chunk's BP; the one post-processing stage nothing "
                         "hides is exposed once per step -- per 16 chunks instead of round 5's 4)")
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--p", type=float, default=0.003)
    ap.add_argument("--bp-method", default="minimum_sum", choices=["minimum_sum", "product_sum"])
    ap.add_argument("--schedule", default="parallel", choices=["parallel", "serial"],
                    help="anything but minimum_sum + parallel runs in the one-message-per-edge kernel (bp_general.hip)")
    ap.add_argument("--osd-method", default="osd_0", choices=["osd_0", "osd_cs", "osd_e", "osd_off", "lsd_0", "lsd_cs", "lsd_e"],
                    help="lsd_*: BP-LSD instead of BP-OSD (--osd-order carries lsd_order)")
    ap.add_argument("--osd-order", type=int, default=0)
    ap.add_argument("--p-override", type=float, default=None, help="physical error rate for the non-headline codes")
    ap.add_argument("--code", default="bb144", choices=["bb144", "bb72", "hgp225", "qlp1020"],
                    help="bb144 = the headline (BASELINE configs[2]); bb72 = configs[1]; hgp225 = configs[0] (their circuits at their p)")
    ap.add_argument("--window", type=int, nargs=2, default=None, metavar=("W", "F"))
    ap.add_argument("--cpu-shots", type=int, default=6500, help="bounded CPU-baseline sample PER CORE (rank 0, N=1 only): 16 cores x 6500 = 104 000 paired shots, ~20 s")
    ap.add_argument("--ref-shots", type=int, default=1000, help="shots PER CORE of the ldpc leg of the CPU baseline (only when `import ldpc` works)")
    ap.add_argument("--sampler", default="auto", choices=["auto", "dem", "stim"],
                    help="inputs: stim = circuit.compile_detector_sampler(seed).sample(..., separate_observables=True) as simulation.py:23-27 "
                         "(host-sampled, --stim-batches distinct batches cycled); dem = the device DEM sampler; auto = stim when importable")
    ap.add_argument("--stim-batches", type=int, default=2, help="distinct Stim-sampled batches (host sampling is slow: the steps cycle through them)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-api", action="store_true", help="skip the drop-in call measurement (through_api)")
    ap.add_argument("--api-shots", type=int, default=1000000, help="shots of the through_api call (host bool array; capped at 1 GiB)")
    ap.add_argument("--dry-run-backend", default=None, help=argparse.SUPPRESS)   # tests: rank plumbing + collectives on CPU (gloo), no decoding
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the `other_configs` array (the other BASELINE configs and window shapes, each timed for two short steps)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, everything else the line can carry: the kernel-event pass and `roofline`, `through_api`, "
                         "`cpu_baseline` and `other_configs` (each still subject to its --no-* switch); a plain run times the steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR: predictions.npy (float32 [shots, observables]; a fixed "
                         "seeded sample of rows when the whole array would pass 64 MB) and mismatches.npy (float64 [1]); "
                         "_rank<r> is appended to the names when --gpus > 1")
    args = ap.parse_args()

    from quits_amd import parallel
    rank, world, local_rank = parallel.env_rank_world()
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d (launch N>1 with torch.distributed.run)" % (args.gpus, world))
    if args.dry_run_backend:
        # the N > 1 branch without a GPU: join the group, barrier, the (errors, shots) SUM and the elapsed-time MAX
        dist = parallel.init_distributed(args.dry_run_backend)
        if dist is not None:
            dist.barrier()
        lo, hi = parallel.shard_range(args.shots * world, rank, world)
        n_err, n_shots = parallel.reduce_counts(dist, rank + 1, hi - lo)
        tmax = parallel.reduce_max(dist, float(rank + 1))
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world, "errors": n_err, "shots": n_shots, "tmax": tmax}))
        if dist is not None:
            dist.destroy_process_group()
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU; the decoder has no CPU fallback")
    # QD_BENCH_SHARE_GPU=1 + QD_BENCH_DIST_BACKEND=gloo: the N > 1 branch on a box with fewer GPUs than ranks (ranks share devices,
    # the 16-byte reductions go over gloo) -- a plumbing check of this code path on hardware, never a scaling measurement
    share = os.environ.get("QD_BENCH_SHARE_GPU") == "1"
    torch.cuda.set_device(local_rank % torch.cuda.device_count() if share else local_rank)
    dist = parallel.init_distributed(os.environ.get("QD_BENCH_DIST_BACKEND", "nccl"))      # "nccl" is RCCL on ROCm; None for a single process

    out = run(args, rank, world, dist, full=args.full, kernel_pass=args.full, dump_dir=args.dump_outputs)
    if args.full and rank == 0 and world == 1 and not args.no_other_configs and args.code == "bb144" and args.window is None \
            and args.osd_method == "osd_0" and not (args.bp_method != "minimum_sum" or args.schedule != "parallel"):
        out["other_configs"] = other_configs(args)
        # the same list once more, compact and LAST in the line: the driver's record keeps the tail of stdout (VERDICT r5 weak 10:
        # four of thirteen entries were cut) -- [name, shots/s, BP ms per launch, post-processing ms per launch, roofline frac, LER]
        out["other_configs_summary"] = [[r["name"], round(r["value"]), round(r["bp_ms_per_launch"], 2), round(r["post_ms_per_launch"], 2),
                                         round(r["roofline"]["frac"], 3), round(r["logical_error_rate"], 5)] if "error" not in r
                                        else [r["name"], r["error"]] for r in out["other_configs"]]
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


# The other BASELINE.json configurations and the window shapes / options the reference's users run, each timed by the same code as
# the headline for a few short steps ("make every BASELINE config driver-timed").  N = 1 only; the headline line is
# measured first and is not affected.
OTHER_CONFIGS = [
    # name, overrides
    ("configs[1] bb72 single window", dict(code="bb72", shots=262144, steps=3, warmup=1)),
    ("configs[1] bb72 W=3 F=1", dict(code="bb72", window=[3, 1], shots=393216, steps=2, warmup=1)),       # (six chunks: two groups of the driver's three lanes)
    ("configs[2] bb144 W=3 F=1", dict(window=[3, 1], shots=393216, steps=2, warmup=1)),
    ("configs[2] bb144 W=5 F=3", dict(window=[5, 3], shots=393216, steps=2, warmup=1)),
    ("configs[3] bb144 p=1e-3", dict(p=0.001, shots=262144, steps=3, warmup=1)),
    ("configs[3] bb144 p=6e-3", dict(p=0.006, shots=262144, steps=3, warmup=1)),
    ("configs[2] bb144 headline window, osd_cs(1)", dict(osd_method="osd_cs", osd_order=1, shots=131072, steps=2, warmup=1)),
    ("configs[2] bb144 headline window, bp-lsd lsd_cs(1)", dict(osd_method="lsd_cs", osd_order=1, shots=262144, steps=2, warmup=1)),
    ("configs[4] qlp1020 W=3 F=1 p=1e-3 osd_0", dict(code="qlp1020", window=[3, 1], p_override=0.001, shots=65536, steps=2, warmup=1)),     # (8192 shots per step: 21.5 k, 32 768: 22.7 k, 65 536 = two chunks of 32 768 through the two-stream driver: 23.5 k shots/s)
    ("configs[4] qlp1020 W=3 F=1 p=1e-3 osd_cs(1)", dict(code="qlp1020", window=[3, 1], p_override=0.001, osd_method="osd_cs", osd_order=1,
                                                        shots=8192, steps=2, warmup=1)),
    ("configs[4] qlp1020 W=3 F=1 p=3e-3 (fixture p) osd_0", dict(code="qlp1020", window=[3, 1], shots=8192, steps=2, warmup=1)),
    ("reference settings (bposd.py:54 defaults + max_iter=10, osd_order=1) bb144 W=5 F=3",
     dict(window=[5, 3], bp_method="product_sum", schedule="serial", max_iter=10, osd_method="osd_cs", osd_order=1,
          shots=163840, steps=2, warmup=1)),
    ("configs[0] hgp225 R=3 p=0.01 W=3 F=1, reference settings", dict(code="hgp225", window=[3, 1], bp_method="product_sum", schedule="serial",
                                                                     max_iter=10, osd_method="osd_cs", osd_order=1, shots=65536, steps=2, warmup=1)),
]


def other_configs(args):
    import copy
    import gc
    res = []
    only = os.environ.get("QD_BENCH_OTHER_ONLY")            # substring filter (development)
    for name, ov in OTHER_CONFIGS:
        if only and only not in name:
            continue
        a = copy.copy(args)
        for k, v in ov.items():
            setattr(a, k, v)
        t0 = time.perf_counter()
        try:
            o = run(a, 0, 1, None, full=False)
            rf = o["roofline"]
            rec = {"name": name, "workload": o["config"]["workload"], "value": o["value"], "unit": "shots/s", "ms_per_step": o["ms_per_step"],
                   "shots_per_step": a.shots, "steps": a.steps, "logical_error_rate": o["logical_error_rate"], "ler_sigma": o["ler_sigma"],
                   "bp_converged_frac": o["bp_converged_frac"], "mean_bp_iters": o["mean_bp_iters"],
                   "bp_kernel": rf.get("kernel"), "bp_ms_per_launch": rf.get("avg_launch_ms"),
                   "post_ms_per_launch": rf.get("osd_kernel_ms_per_launch"),
                   "roofline": {"bound": rf["bound"], "frac": rf["frac"], "achieved": rf["achieved"], "peak": rf["peak"], "unit": rf["unit"]},
                   "wall_s": None}
            if "kernel_model" in rf:
                rec["roofline"]["kernel_model_frac"] = rf["kernel_model"]["frac"]
            if "osd" in rf:
                rec["post_kernel"] = rf["osd"]["kernel"]
                rec["post_us_per_shot"] = rf["osd"]["us_per_shot"]
        except Exception as exc:           # one configuration failing must not take the headline line with it
            rec = {"name": name, "error": "%s: %s" % (type(exc).__name__, exc)}
        rec["wall_s"] = time.perf_counter() - t0
        res.append(rec)
        gc.collect()
        torch.cuda.empty_cache()
    return res


DUMP_BYTES = 64 * 10 ** 6


def dump_outputs(dump_dir, pred, mismatches, suffix=""):
    """--dump-outputs: the logical predictions (uint8 [shots, observables] on the device) and the mismatch count of one step.
    Rows are sampled with a fixed seed when the float32 array would exceed DUMP_BYTES."""
    os.makedirs(dump_dir, exist_ok=True)
    p = pred.cpu().numpy()
    rows = max(1, (DUMP_BYTES - 4096) // (4 * max(1, p.shape[1])))
    if p.shape[0] > rows:
        p = p[np.sort(np.random.default_rng(2026).choice(p.shape[0], rows, replace=False))]
    np.save(os.path.join(dump_dir, "predictions%s.npy" % suffix), p.astype(np.float32))
    np.save(os.path.join(dump_dir, "mismatches%s.npy" % suffix), np.array([int(mismatches.item())], dtype=np.float64))


def run(args, rank, world, dist, full=True, kernel_pass=True, dump_dir=None):
    """One configuration: set up, warm up, time args.steps steps.  kernel_pass: the same steps again with the library's kernel
    events on, for `roofline`; full: `through_api` and `cpu_baseline` as well (rank 0, N = 1)."""
    import helpers
    from quits_amd import parallel
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.decoder.device import DemSampler, count_mismatch
    from quits_amd.decoder.sliding_window import build_circuit_plan
    from quits_amd.dem import Circuit

    if args.code == "bb144":
        R, cname = 12, "bb144_custom_r12_p%g" % args.p
    elif args.code == "bb72":
        R, cname = 6, "bb72_custom_r6_p0.003"
    elif args.code == "qlp1020":
        R, cname = 20, "qlp1020_cardinal_r20_p0.003"          # BASELINE configs[4]: ~1000 qubits, W=3 F=1 (pass --window 3 1)
    else:
        R, cname = 3, "hgp225_cardinal_r3_p0.01"
    text = helpers.circuit_text(cname)
    fixture_p = {"bb144": args.p, "bb72": 0.003, "hgp225": 0.01, "qlp1020": 0.003}[args.code]
    if args.code != "bb144" and args.p_override is not None and args.p_override != fixture_p:
        text = helpers.circuit_text_at_p(cname, fixture_p, args.p_override)      # same text the reference emits at that rate
        cname += "@p=%g" % args.p_override
    circ = Circuit(text)
    code = helpers.code(args.code)
    hz, lz = code["hz"], code["lz"]
    H, Lobs, pri = detector_error_model_to_matrix(circ)
    m, n = H.shape
    E = int(H.nnz)
    W, F = (R + 2, 1) if args.window is None else args.window
    general = not (args.bp_method == "minimum_sum" and args.schedule == "parallel")
    opts = dict(bp_method=args.bp_method, schedule=args.schedule, max_iter=args.max_iter, osd_method=args.osd_method,
                osd_order=args.osd_order)
    plan = build_circuit_plan(circ, hz, W, F, R, dict(opts), dict(opts))
    decs = plan.decoders()
    for d in decs:
        d.reserve(min(args.shots, 1 << 16))

    # ---- synthetic inputs, resident in HBM before the timed region
    sampler = DemSampler(H, Lobs, pri)
    nbatch = args.steps + args.warmup
    batches = []
    import refhooks
    stim_mod, stim_info = refhooks.probe_stim() if args.sampler != "dem" else (None, "--sampler dem")
    if args.sampler == "stim" and stim_mod is None:
        raise SystemExit("--sampler stim, but stim is not importable (%s)" % stim_info)
    if stim_mod is not None:
        # SURVEY.md 8(d) "Synthetic inputs": Stim's own detector sampler on the reference's circuit, seed S + rank per shard, S = 1
        # (the reference tests' value); sampled on the host before the timed region, a few distinct batches cycled over the steps
        nd = max(1, min(nbatch, args.stim_batches))
        distinct = []
        for j in range(nd):
            d_h, o_h = refhooks.stim_sample(text, args.shots, seed=1 + rank + 1000 * j)
            distinct.append((torch.from_numpy(d_h).to("cuda"), torch.from_numpy(o_h).to("cuda")))
        batches = [distinct[i % nd] for i in range(nbatch)]
        data_note = "synthetic (stim %s compile_detector_sampler on the reference's circuit, %d distinct batches of %d shots cycled)" % (stim_info, nd, args.shots)
    else:
        for i in range(nbatch):
            shot0 = (rank * nbatch + i) * args.shots
            batches.append(sampler.sample(args.shots, seed=1, shot0=shot0))
        data_note = "synthetic"
    torch.cuda.synchronize()

    def step(i, stats=None):
        det, obs = batches[i]
        pred = plan.decode(det, stats)
        return count_mismatch(pred, obs), pred

    # warm-up: the same loop body as the timed region (count accumulation and per-step statistics included), so that nothing is
    # loaded lazily inside the timed region -- a rocprofv3 timeline showed a one-off 14 ms host stall at the first `fails += c`
    # (profiles/r03f_bench_under_trace.json: 60.5 ms per step timed vs 55.6 ms for the same steps run again)
    fails_w = torch.zeros((1,), dtype=torch.int64, device="cuda")
    stats_w = []
    for i in range(args.warmup):
        c, _ = step(i, stats_w)
        fails_w += c
    del stats_w
    torch.cuda.synchronize()

    # ---- the timed region: K steps, no event recording inside (the per-launch hipEventCreate/Record pairs were
    # part of the number)
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fails = torch.zeros((1,), dtype=torch.int64, device="cuda")
    stats = []
    for i in range(args.warmup, nbatch):
        c, pred = step(i, stats)
        fails += c
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    elapsed = parallel.reduce_max(dist, elapsed, "cuda")
    # the path's only collective: 16 bytes over RCCL
    n_err, n_shots = parallel.reduce_counts(dist, int(fails.item()), args.shots * args.steps, "cuda")
    if dump_dir:
        dump_outputs(dump_dir, pred, c, "_rank%d" % rank if world > 1 else "")

    pipelined = bool(plan.pipeline and args.shots >= 2 * plan.chunk)
    st = torch.cat([t for (_, t) in stats])
    iters = (st & 0x3FFF).to(torch.int64)
    total_iters = int(iters.sum().item())
    conv_frac = float(((st >> 16) & 1).float().mean().item())
    osd_frac = float(((st >> 17) & 1).float().mean().item())
    off_grid = int(((st >> 14) & 3).ne(0).sum().item())
    value = n_shots / elapsed
    pl = n_err / n_shots
    dinfo = decs[0].info()
    out = {
        "metric": "decoded shots/sec + logical-error-rate, [[144,12,12]] BB code, d rounds, p=0.003",
        "value": value, "unit": "shots/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": data_note,
        "sampler": "stim" if stim_mod is not None else "device DEM sampler (qd_sample_dem_kernel: e ~ Bernoulli(priors), s = He, o = Le); stim: %s" % stim_info,
        "arithmetic": ("f32 on channel LLRs rounded to multiples of 2^-%d: exact (no operation rounds; certified per shot), i.e. the "
                       "result ldpc's f64 BpDecoder returns for those LLRs; %d of %d shot-windows left the fine grid"
                       % (dinfo["llr_grid_bits"], off_grid, st.numel())) if dinfo["llr_grid_bits"] >= 0 else "f32, float(log((1-p)/p)) LLRs",
        "config": {"workload": "%s circuit %s, R=%d, Z basis; DEM %dx%d (E=%d); "
                               "%s %s BP max_iter=%d ms_scaling=1.0 + %s(%d); W=%d F=%d (%d window%s)"
                               % ({"bb144": "BB [[144,12,12]]", "bb72": "BB [[72,12,6]]", "hgp225": "HGP [[225,9,6]]", "qlp1020": "QLP [[1020,136]]"}[args.code],
                                  cname, R, m, n, E, args.bp_method, args.schedule, args.max_iter, args.osd_method, args.osd_order, W, F, len(plan.windows),
                                  "" if len(plan.windows) == 1 else "s"),
                   "shots_per_step_per_gpu": args.shots, "parallelism": "shots sharded over %d GPU(s), no data-path collective" % world},
        "logical_error_rate": pl, "ler_sigma": float(np.sqrt(max(pl * (1 - pl), 1e-30) / n_shots)),
        "lfr_per_round": 1.0 - (1.0 - pl) ** (1.0 / R),
        "bp_converged_frac": conv_frac, "osd_frac": osd_frac, "mean_bp_iters": total_iters / max(1, st.numel()),
        "pipeline": {"osd_beside_next_chunk_bp": pipelined, "chunk_shots": plan.chunk,
                     "note": "timed region: chunk i's post-processing on a second stream beside chunk i+1's BP (two workspaces); "
                             "ms_per_step_with_kernel_events and the roofline's per-kernel times are from a pass with the kernels back to back"},
        # early exit makes the work data-dependent -- shot-windows by BP iterations used (index = iterations)
        "bp_iters_hist": torch.bincount(iters.clamp(max=args.max_iter), minlength=args.max_iter + 1).tolist(),
    }
    if not kernel_pass:
        plan.release_workspaces()
        return out

    # ---- the same K steps once more with the library's HIP events on (recorded on the launch stream around each kernel):
    # per-kernel device time for the roofline object
    # (kernels back to back on one stream in this pass: the per-kernel times the roofline is priced on are those of a kernel that
    # has the GPU to itself, as under rocprofv3 --kernel-trace of a QD_NO_PIPELINE=1 run; the timed region above overlaps them)
    pipeline_setting = plan.pipeline
    plan.pipeline = False
    for d in decs:
        d.set_profiling(True)
        d.profile(reset=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for i in range(args.warmup, nbatch):
        step(i)
    torch.cuda.synchronize()
    elapsed_ev = time.perf_counter() - t1
    plan.pipeline = pipeline_setting
    prof = {"bp_ms": 0.0, "osd_ms": 0.0, "bp_launches": 0, "osd_launches": 0}
    for d in decs:
        pr = d.profile(reset=True)
        d.set_profiling(False)
        for k in prof:
            prof[k] += pr[k]
    bp_s = prof["bp_ms"] / 1e3
    nlaunch = max(1, prof["bp_launches"])

    # ---- per-window work of one BP iteration of one shot
    #   B_iter = (4E + 2n) * 4 bytes of message traffic (what an HBM-resident formulation moves);
    #   LDS kernel: wave-steps of the check pass (64 checks x one edge) and of the bit pass (64 faults x one gather), padded as
    #   the kernel pads them (slots sorted by degree, a wavefront runs to its largest degree; check trips in fours)
    from scipy.sparse import csr_matrix, csc_matrix
    per_dec = {}
    for w in plan.windows:
        info = w["graph"].info()
        rec = {"b_iter": (4 * info["nnz"] + 2 * info["n"]) * 4, "n": info["n"], "m": info["m"], "nnz": info["nnz"]}
        per_dec[id(w["dec"])] = rec
    def wave_steps(Hm):
        rdeg = np.sort(np.diff(csr_matrix(Hm).indptr))[::-1]
        cdeg = np.sort(np.diff(csc_matrix(Hm).indptr))[::-1]
        ws_c = sum((int(rdeg[i:i + 64].max()) + 3) // 4 * 4 for i in range(0, len(rdeg), 64))
        ws_b = sum(int(cdeg[i:i + 64].max()) for i in range(0, len(cdeg), 64))
        return ws_c, ws_b
    for w, Hm in zip(plan.windows, plan.window_matrices()):
        per_dec[id(w["dec"])]["ws"] = wave_steps(Hm)
    algo_bytes = 0
    ws_c_tot = ws_b_tot = 0
    hbm_algo = 0
    for (k, s_t) in stats:
        rec = per_dec[id(plan.windows[k]["dec"])]
        it_k = int((s_t & 0x3FFF).to(torch.int64).sum().item())
        algo_bytes += it_k * rec["b_iter"]
        ws_c_tot += it_k * rec["ws"][0]
        ws_b_tot += it_k * rec["ws"][1]
        nf = int((((s_t >> 16) & 1) == 0).sum().item())
        hbm_algo += s_t.numel() * (rec["m"] + 4 * ((rec["n"] + 31) // 32) + 4) + nf * 4 * ((rec["n"] + 63) // 64 * 64)

    # HBM bytes per BP launch from the PMC passes of tools/profile_bench.sh (rocprofv3 cannot run inside this process);
    # only quoted when the committed profile was taken on this exact workload.
    traffic, traffic_src, sq_counters = None, None, None
    pmc_path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(pmc_path):
        try:
            pm = json.load(open(pmc_path))
            key = "p%g_it%d_W%d_F%d_shots%d" % (args.p, args.max_iter, W, F, min(args.shots, plan.chunk))      # per BP launch (one chunk)
            kname = (("qd_bp_scatter_wide_kernel" if decs[0].info().get("scatter_wide_kernel") else "qd_bp_scatter_kernel")
                     if decs[0].info().get("scatter_kernel") else "qd_bp_minsum_kernel")
            if key in pm and not general and args.code == "bb144" and pm[key].get("kernel", "qd_bp_minsum_kernel") == kname:
                traffic, traffic_src = pm[key]["bp_bytes_per_launch"], pm[key]["source"]
                sq_counters = pm[key].get("sq_counters")
        except (ValueError, KeyError):
            pass

    if general:
        achieved = (algo_bytes / bp_s / 1e9) if bp_s > 0 else 0.0
        # what the kernel itself moves per shot-iteration (csrc/bp_general.hip), in units of E edges, n faults, m detectors:
        #   serial:   suffix pass 8E (+4m), level pass 9E in + 8E out + 4n, convergence test 4E + m
        #   flooding: check pass 20E (min-sum) / 24E (product-sum: tanh plane), bit pass 8E + 4n, convergence test 4E + m
        ps = args.bp_method == "product_sum"
        def k_iter(rec):
            E_, n_, m_ = rec["nnz"], rec["n"], rec["m"]
            return (29 * E_ + 4 * n_ + 5 * m_) if args.schedule == "serial" else ((36 if ps else 32) * E_ + 4 * n_ + m_)
        kern_bytes = sum(int((s_t & 0x3FFF).to(torch.int64).sum().item()) * k_iter(per_dec[id(plan.windows[k]["dec"])]) for (k, s_t) in stats)
        roofline = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                    "traffic": traffic, "kernel": "qd_bp_edge_kernel", "avg_launch_ms": prof["bp_ms"] / nlaunch,
                    "algorithmic_bytes_per_launch": algo_bytes / nlaunch,
                    "kernel_model": {"bytes_per_launch": kern_bytes / nlaunch, "GBps": kern_bytes / bp_s / 1e9 if bp_s > 0 else 0.0,
                                     "frac": kern_bytes / bp_s / 1e9 / HBM_PEAK_GBS if bp_s > 0 else 0.0,
                                     "note": "bytes the kernel's own loads and stores add up to per shot-iteration (29E+4n+5m serial, "
                                             "32E/36E+4n+m flooding), cache hits included: an upper bound on its HBM traffic"},
                    "note": "one message per edge in HBM: algorithmic bytes = sum over shots of BP iterations x (4E+2n)*4 B (SURVEY.md "
                            "8d).  The serial schedule keeps a running prefix per row and a suffix per edge (one load of each per "
                            "edge instead of bp.hpp's row rescan); it is bound by the latency of one dependency level (a few faults "
                            "per level, one barrier each), not by bandwidth, see DESIGN.md"}
    else:
        # The LDS kernel's messages never leave the CU, so HBM cannot bound it ("report ... LDS bytes as the bound").
        # What bounds it is vector-ALU issue: wave-instructions per edge from the compiler's assembly
        # (profiles/k1_issue_model.json <- tools/isa_histogram.py), peak = 4 SIMDs x one wave-instruction per 2 clk
        # (MI355X_MICROARCH.md: a wave64 instruction issues over 2 cycles on a SIMD-32) = 2.0 per CU per clk at 2.4 GHz.
        mdl = {"check_pass_loop_4_edges": {"valu_fast": 16, "valu_slow": 38}, "bit_pass_gather_blocks": {"valu_fast": 31, "valu_slow": 34},
               "bit_pass_gathers": 8}
        mp = os.path.join(ROOT, "profiles", "k1_issue_model.json")
        if os.path.exists(mp):
            try:
                mdl = json.load(open(mp))["summary"]
            except (ValueError, KeyError):
                pass
        cf, cs = mdl["check_pass_loop_4_edges"]["valu_fast"] / 4.0, mdl["check_pass_loop_4_edges"]["valu_slow"] / 4.0
        bf, bs = (mdl["bit_pass_gather_blocks"][k] / float(mdl["bit_pass_gathers"]) for k in ("valu_fast", "valu_slow"))
        scatter = bool(decs[0].info().get("scatter_kernel"))
        if scatter:
            # scatter kernel (bp_scatter.hip): both passes walk the CHECKS' edges -- gather pass (minima, signs, decision parity) and
            # scatter pass (one ds_add_u32 per edge); per-edge counts from profiles/k1s_issue_model.json <- tools/isa_histogram.py
            ms = {"gather_pass_loop_4_edges": {"valu_fast": 26, "valu_slow": 32}, "scatter_pass_plain_block": {"valu_fast": 6, "valu_slow": 9},
                  "scatter_pass_edges_in_block": 3}
            # (the several-checks-per-lane kernel of bp_scatter_wide.hip -- the headline's -- has its own count: profiles/k1sw_issue_model.json,
            #  from this round's assembly, profiles/r05_k1sw_isa_loops.txt)
            wide = bool(decs[0].info().get("scatter_wide_kernel"))
            model_src = "profiles/k1sw_issue_model.json <- profiles/r05_k1sw_isa_loops.txt" if wide else "profiles/k1s_issue_model.json <- profiles/r03z_k1s_isa_histogram.txt"
            try:
                ms = json.load(open(os.path.join(ROOT, "profiles", "k1sw_issue_model.json" if wide else "k1s_issue_model.json")))["summary"]
            except (OSError, ValueError, KeyError):
                model_src = "built-in counts (profiles/k1s*_issue_model.json not readable)"
            slow_clk = float(ms.get("slow_class_clk", 4))
            cf, cs = ms["gather_pass_loop_4_edges"]["valu_fast"] / 4.0, ms["gather_pass_loop_4_edges"]["valu_slow"] / 4.0
            bf, bs = (ms["scatter_pass_plain_block"][k] / float(ms["scatter_pass_edges_in_block"]) for k in ("valu_fast", "valu_slow"))
            ws_b_tot = ws_c_tot                                                          # the scatter pass pads like the gather pass
        n_inst = ws_c_tot * (cf + cs) + ws_b_tot * (bf + bs)
        if not scatter:
            slow_clk, model_src = 4.0, "profiles/k1_issue_model.json <- profiles/r02_k1_isa_histogram.txt"
        issue_clk = ws_c_tot * (2 * cf + slow_clk * cs) + ws_b_tot * (2 * bf + slow_clk * bs)   # SIMD-cycles: fast class 2 clk, slow class 3 (K1sw model: measured 1.5 x) or 4 (older models)
        if scatter:
            lds_clk = ws_c_tot * 2 + ws_b_tot * 4                                        # ds_read_b32 2 cycles; ds_add_u32 ~4 (1.75 ns measured, conflict-free)
            lds_bytes = (ws_c_tot + ws_b_tot) * 64 * 4
        else:
            lds_clk = ws_c_tot * 2 + ws_b_tot * 4                                        # ds_read_b32 2 cycles, ds_read_b128 4 (conflict-free)
            lds_bytes = ws_c_tot * 64 * 4 + ws_b_tot * 64 * 16
        peak_inst = NUM_CU * 2.0 * CLOCK_HZ / 1e9
        ach_inst = n_inst / bp_s / 1e9 if bp_s > 0 else 0.0
        roofline = {
            "bound": "valu", "achieved": ach_inst, "peak": peak_inst, "unit": "G wave-instructions/s", "frac": ach_inst / peak_inst,
            "traffic": traffic, "traffic_source": traffic_src, "kernel": ("qd_bp_scatter_wide_kernel" if decs[0].info().get("scatter_wide_kernel") else "qd_bp_scatter_kernel") if scatter else "qd_bp_minsum_kernel",
            "avg_launch_ms": prof["bp_ms"] / nlaunch,
            "algorithmic_instructions_per_launch": n_inst / nlaunch,
            "model": ("VALU wave-instructions = check-side wave-steps x (%.2f gather pass + %.2f scatter pass) (per edge, from "
                      "%s), summed over the BP iterations each shot really ran; per-check overhead "
                      "outside the two edge loops is not counted, so `achieved` is a floor" % (cf + cs, bf + bs, model_src)) if scatter else
                     ("VALU wave-instructions = check-pass wave-steps x %.2f + bit-pass wave-steps x %.2f (per edge, from "
                      "profiles/r02_k1_isa_histogram.txt), summed over the BP iterations each shot really ran; per-node overhead "
                      "outside the two edge loops is not counted, so `achieved` is a floor" % (cf + cs, bf + bs)),
            # the same instructions priced by class: add / sub / xor / fma / v_bitop3 issue in 2 clk per wavefront per SIMD, shifts / bit-field
            # extracts / cvt / compares / cndmask / min / max / med3 / carry ops in 3 (K1sw model: tools/microbench/valu_rates.hip measured
            # 1.5 x, profiles/r05_valu_rates.txt) or 4 (the older models' estimate, profiles/r01f_valu_issue_rates.txt)
            "frac_priced_by_class": issue_clk / (bp_s * NUM_CU * 4 * CLOCK_HZ) if bp_s > 0 else 0.0,
            # the same fraction from the hardware counters of the COMMITTED PMC pass (profiles/pmc_traffic.json <- tools/profile_bench.sh; all
            # VALU instructions, overhead included) -- read from that file, NOT measured in this run (rocprofv3 cannot run inside this process)
            "frac_from_committed_profile_sq_counters": (sq_counters or {}).get("frac_of_2_per_cu_clk"), "sq_counters_committed_profile": sq_counters,
            "lds": {"achieved": lds_bytes / bp_s / 1e9 if bp_s > 0 else 0.0, "peak": NUM_CU * 256 * CLOCK_HZ / 1e9, "unit": "GB/s",
                    "frac_of_conflict_free_cycles": lds_clk / (bp_s * NUM_CU * CLOCK_HZ) if bp_s > 0 else 0.0,
                    "note": ("4 B gathered and 4 B added (ds_add_u32) per edge and iteration; LDS-array cycles at ds_read_b32 2 clk "
                             "(MI355X_MICROARCH.md) and ds_add_u32 ~4 clk per wavefront (profiles/r03z_lds_atomic_rates.txt: 1.75 ns "
                             "conflict-free, 2.2 ns scattered); bank conflicts add to it") if scatter else
                            ("gathers only (4 B per check-pass edge, 16 B per bit-pass edge); LDS-array cycles at the conflict-free "
                             "rate of MI355X_MICROARCH.md (ds_read_b32 2 clk, ds_read_b128 4 clk per wavefront); bank conflicts add to it "
                             "(tools/lds_model.py, profiles/r02_pmc_*)")},
            "hbm": {"achieved": hbm_algo / bp_s / 1e9 if bp_s > 0 else 0.0, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": hbm_algo / bp_s / 1e9 / HBM_PEAK_GBS if bp_s > 0 else 0.0,
                    "algorithmic_bytes_per_launch": hbm_algo / nlaunch,
                    "traffic_over_algorithmic": (traffic / (hbm_algo / nlaunch)) if traffic else None,
                    "note": "detector bytes in, packed decisions + status out, posteriors of the shots that go to OSD"},
            "hbm_resident_equivalent": {"bytes_per_launch": algo_bytes / nlaunch, "GBps": algo_bytes / bp_s / 1e9 if bp_s > 0 else 0.0,
                                        "note": "SURVEY.md 8(d) B_iter = (4E+2n)*4 per shot-iteration: what a one-message-per-edge "
                                                "layout in HBM would have to move in the same time (not bytes that cross HBM here)"},
        }
    roofline["osd_kernel_ms_per_launch"] = prof["osd_ms"] / max(1, prof["osd_launches"])
    # ---- the post-processing stage ("give the OSD kernels a roofline").  OSD-0 reads a shot's posteriors (4 n_pad bytes,
    # L2-resident after BP wrote them: a few passes per tier), its syndrome and writes the packed correction; the elimination itself
    # is GF(2) row work in registers / LDS.  Neither HBM nor the vector ALU bounds it: a shot is a chain of dependent barrier rounds
    # (tools/osd_timing.py counts them), so the object reports the chain beside the two hardware ceilings.
    if not args.osd_method.startswith("lsd") and args.osd_method != "osd_off":
        osd_mask = ((st >> 17) & 1) == 1
        n_osd = int(osd_mask.sum().item())
        piv = ((st >> 20) & 0xFFF)[osd_mask].to(torch.float64)
        mean_piv = float(piv.mean().item()) if n_osd else 0.0
        osd_s = prof["osd_ms"] / 1e3
        rec0 = per_dec[id(plan.windows[0]["dec"])]
        n_pad0, m0 = (rec0["n"] + 63) // 64 * 64, rec0["m"]
        osd_bytes = n_osd * (4 * n_pad0 + m0 + 4 * ((rec0["n"] + 31) // 32) + 8)
        mw0 = (m0 + 63) // 64
        # 64-bit word operations of a Gauss-Jordan elimination in T-form that stops after `piv` pivots: every pivot adds the pivot row's
        # Q words (ceil(k / 64) of them so far) and the batch word to, on average, half of the m rows -- an upper estimate of the useful work
        words = float((piv * (m0 / 2.0) * (1.0 + (piv / 64.0 + 1.0) / 2.0)).sum().item()) if n_osd else 0.0
        osd_pm = None
        try:
            osd_pm = json.load(open(pmc_path)).get("osd_" + key)
        except Exception:
            pass
        kern = dinfo_post = decs[0].info().get("post_kernel", "?")
        roofline["osd"] = {
            "kernel": kern, "avg_launch_ms": prof["osd_ms"] / max(1, prof["osd_launches"]), "shots_per_launch": n_osd / max(1, prof["osd_launches"]),
            "mean_pivots": mean_piv, "us_per_shot": 1e6 * osd_s / max(1, n_osd),
            "bound": "latency (dependent barrier rounds per shot); neither ceiling below is approached",
            "hbm": {"algorithmic_bytes_per_launch": osd_bytes / max(1, prof["osd_launches"]), "achieved": osd_bytes / osd_s / 1e9 if osd_s > 0 else 0.0,
                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": osd_bytes / osd_s / 1e9 / HBM_PEAK_GBS if osd_s > 0 else 0.0,
                    "traffic": (osd_pm or {}).get("bytes_per_launch"), "traffic_source": (osd_pm or {}).get("source")},
            "gf2_words": {"per_launch": words / max(1, prof["osd_launches"]), "achieved": words / osd_s / 1e9 if osd_s > 0 else 0.0,
                          "peak": NUM_CU * 64 * 2.0 * CLOCK_HZ / 1e9 / 2.0, "unit": "G 64-bit word-XORs/s",
                          "frac": (words / osd_s / 1e9) / (NUM_CU * 64 * 2.0 * CLOCK_HZ / 1e9 / 2.0) if osd_s > 0 else 0.0,
                          "note": "pivots x rows/2 x (Q words + batch word) per shot (an upper estimate of the row additions) against 2 wave-"
                                  "instructions per CU-clock x 64 lanes / 2 instructions per 64-bit XOR"},
            "sq_counters": (osd_pm or {}).get("sq_counters"),
            "chain": (osd_pm or {}).get("chain"),
        }

    out["ms_per_step_with_kernel_events"] = 1e3 * elapsed_ev / args.steps
    out["roofline"] = roofline

    if full and rank == 0 and world == 1 and not args.no_api and args.osd_method.startswith("osd"):
        out["through_api"] = through_api(args, circ, hz, lz, W, F, sampler, value)
    if full and rank == 0 and world == 1 and not args.no_cpu:
        out.update(cpu_baseline(args, circ, hz, lz, R, W, F, batches[args.warmup],
                                lambda d: plan.decode(torch.from_numpy(np.ascontiguousarray(d)).to("cuda")).cpu().numpy(), value))
    plan.release_workspaces()
    return out


if __name__ == "__main__":
    main()
