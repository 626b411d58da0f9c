#!/usr/bin/env python3
"""Time Relay-BP beside min-sum + OSD, in one session, on the same DEM-sampled shots.

    python tools/relay_timing.py [--points 0.001:1048576,0.003:1048576,0.006:1048576] [--reps 5] --out profiles/relay_bp_timing.json
    python tools/relay_timing.py --part qlp [--shots 65536] [--reps 5] --out profiles/relay_qlp_timing.json
    python tools/relay_timing.py --part headline --marginals lds|device|auto [--shots 262144] --out FILE      (QUITS_AMD_LIB names the library)
    python tools/relay_timing.py --part collect --this FILE [FILE ...] --parent FILE [FILE ...] --out profiles/relay_headline_forms.json

--part bb144 (the default): circuit bb144_custom_r12 (BB [[144,12,12]], 12 rounds), the whole history as one window, at each physical error
rate p of `--points` (p:shots).  Per point the same shots go through
  relay          RelayConfig() (80 + 60 x 60 iterations), osd_off
  relay_nconv5   the same with stop_nconv = 5
  ms50_osd0      minimum_sum / parallel / max_iter 50 + osd_0 (the headline configuration)
  ms50_osdcs1    the same BP + osd_cs of order 1
and each records shots/s (median of `--reps` plan.decode calls after a warm-up, host clock around a device synchronise) and the logical error
rate with its binomial sigma; the relay rows also the mean iterations per shot and the share of shots no leg solved.  No target: the
numbers are what they are.

--part qlp: the same rows without relay_nconv5 on QLP [[1020,136]], 20 rounds, W = 3 / F = 1 at p = 1e-3 -- the circuit and the 20 windows of
bench.py's configs[4] row (the fixture circuit with its noise literal replaced).  The windows of 1350 x 18 300 / 18 900 take Relay-BP's
device-marginal form by the automatic choice; the file records each decoder's form and LDS bytes.

--part headline: RelayConfig() on the bb144 window at p = 3e-3, one RelayBatchDecoder with the marginals where `--marginals` says, `--shots`
shots in batches of 65 536.  One process per run, so that the parent commit's library (QUITS_AMD_LIB; it knows "auto" only, and that is its
LDS form) and this one can alternate in one session; --part collect puts the runs into one file: the LDS form must sit inside the parent's
own run-to-run spread, the device form's number is recorded for information."""
import argparse
import json
import math
import os
import statistics
import sys
import time

W, F = 14, 1                                                         # R + 2 rounds of detectors: one window


def wall(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(round((time.perf_counter() - t0) * 1e3, 3))
    return out


def decode_row(plan, det, obs, shots, reps, relay):
    """One row of a point: a warm-up call (its predictions and status words are the row's), then `reps` timed calls."""
    import torch
    from quits_amd import _lib
    with plan.in_use():
        stats = []
        pred = plan.decode(det, stats)
        torch.cuda.synchronize()
        ms_list = wall(lambda: plan.decode(det), reps)
        errors = int((pred != obs).any(dim=1).sum())
        st = torch.cat([s for _, s in stats]).cpu().numpy()
        ler = errors / shots
        row = {"ms": ms_list, "shots_per_s": round(shots / (statistics.median(ms_list) * 1e-3), 1), "errors": errors, "ler": ler,
               "sigma": math.sqrt(max(ler * (1 - ler), 0.0) / shots), "mean_iterations": float((st & _lib.STATUS_ITER_MASK).mean()),
               "bp_unconverged_share": float(((st & _lib.STATUS_CONVERGED) == 0).mean())}
        if relay:
            legs = (st & _lib.STATUS_RELAY_LEG_MASK) >> _lib.STATUS_RELAY_LEG_SHIFT
            solved = (st & _lib.STATUS_CONVERGED) != 0
            row["unsolved_share"] = row.pop("bp_unconverged_share")
            row["solved_in_leg0_share"] = float((solved & (legs == 0)).mean())
            row["max_iterations"] = int((st & _lib.STATUS_ITER_MASK).max())
    plan.release_workspaces()
    return row


def save(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(json.dumps(res) + "\n")


def part_bb144(args, m):
    ms = dict(bp_method="minimum_sum", schedule="parallel", max_iter=50)
    configs = [("relay", m.RelayBpDecoder, m.relay_options(m.RelayConfig())),
               ("relay_nconv5", m.RelayBpDecoder, m.relay_options(m.RelayConfig(stop_nconv=5))),
               ("ms50_osd0", m.BpOsdDecoder, dict(ms, osd_method="osd_0", osd_order=0)),
               ("ms50_osdcs1", m.BpOsdDecoder, dict(ms, osd_method="osd_cs", osd_order=1))]
    cd = m.helpers.code("bb144")
    res = {"device": m.torch.cuda.get_device_name(0), "library_version": int(m._lib.load().qd_version()),
           "workload": "bb144_custom_r12, one window, DEM-sampled shots (seed 7)", "reps": args.reps,
           "method": "host clock around a device synchronise, one warm-up call before each series of %d; one session" % args.reps, "points": []}
    for item in args.points.split(","):
        p_txt, shots = item.split(":")
        p, shots = float(p_txt), int(shots)
        circ = m.Circuit(m.helpers.circuit_text("bb144_custom_r12_p%s" % p_txt))
        H, L, pri = m.detector_error_model_to_matrix(circ.detector_error_model())
        det, obs = m.DemSampler(H, L, pri).sample(shots, seed=7)
        point = {"p": p, "shots": shots, "window": list(H.shape), "rows": {}}
        for name, cls, opts in configs:
            plan = m.cached_circuit_plan(circ, cd["hz"], W, F, H.shape[0] // cd["hz"].shape[0] - 2, cls, cls, opts, opts)
            point["rows"][name] = row = decode_row(plan, det, obs, shots, args.reps, cls is m.RelayBpDecoder)
            print(p, name, json.dumps(row), flush=True)
        res["points"].append(point)
        save(args.out, res)                                          # after every point: a later point's trouble keeps the earlier ones
    print(json.dumps(res))


def part_qlp(args, m):
    name, p_fix, p, R = "qlp1020_cardinal_r20_p0.003", 0.003, 0.001, 20
    ms = dict(bp_method="minimum_sum", schedule="parallel", max_iter=50)
    configs = [("relay", m.RelayBpDecoder, m.relay_options(m.RelayConfig())),
               ("ms50_osd0", m.BpOsdDecoder, dict(ms, osd_method="osd_0", osd_order=0)),
               ("ms50_osdcs1", m.BpOsdDecoder, dict(ms, osd_method="osd_cs", osd_order=1))]
    cd = m.helpers.code("qlp1020")
    circ = m.Circuit(m.helpers.circuit_text_at_p(name, p_fix, p))
    H, L, pri = m.detector_error_model_to_matrix(circ.detector_error_model())
    shots = args.shots or (1 << 16)
    det, obs = m.DemSampler(H, L, pri).sample(shots, seed=7)
    res = {"device": m.torch.cuda.get_device_name(0), "library_version": int(m._lib.load().qd_version()),
           "workload": "%s at p = %g, W = 3 / F = 1, %d rounds, DEM-sampled shots (seed 7)" % (name, p, R), "p": p, "shots": shots, "reps": args.reps,
           "dem": list(H.shape), "method": "host clock around a device synchronise, one warm-up call before each series of %d; one session" % args.reps,
           "rows": {}}
    for rname, cls, opts in configs:
        plan = m.cached_circuit_plan(circ, cd["hz"], 3, 1, R, cls, cls, opts, opts)
        row = decode_row(plan, det, obs, shots, args.reps, cls is m.RelayBpDecoder)
        row["windows"], row["lanes"], row["chunk"] = len(plan.windows), int(plan.lanes), int(plan.chunk)
        if cls is m.RelayBpDecoder:
            infos = [(d.graph.m, d.graph.n, d.info()) for d in plan.decoders()]
            row["decoders"] = [{"window": [mm, nn], "relay_marginals": i["relay_marginals"], "relay_lds_bytes": i["relay_lds_bytes"]} for mm, nn, i in infos]
        res["rows"][rname] = row
        print(rname, json.dumps(row), flush=True)
        save(args.out, res)
    print(json.dumps(res))


def part_headline(args, m):
    from quits_amd.decoder.device import RelayBatchDecoder, WindowGraph
    circ = m.Circuit(m.helpers.circuit_text("bb144_custom_r12_p0.003"))
    H, L, pri = m.detector_error_model_to_matrix(circ.detector_error_model())
    shots = args.shots or (1 << 18)
    smp = m.DemSampler(H, L, pri)
    det = m.torch.cat([smp.sample(1 << 16, 7, s)[0] for s in range(0, shots, 1 << 16)])[:shots]
    wg = WindowGraph(H, pri)
    dec = RelayBatchDecoder(wg, m.RelayConfig(), marginals=args.marginals) if args.marginals != "auto" else RelayBatchDecoder(wg, m.RelayConfig())
    dec.reserve(1 << 16)
    bits = m.torch.empty((shots, wg.words), dtype=m.torch.int32, device="cuda")
    status = m.torch.empty((shots,), dtype=m.torch.int32, device="cuda")

    def run():
        for c0 in range(0, shots, 1 << 16):
            dec.decode(det[c0:c0 + (1 << 16)], err_bits=bits[c0:c0 + (1 << 16)], status=status[c0:c0 + (1 << 16)])

    run()
    m.torch.cuda.synchronize()
    import hashlib
    res = {"library": os.path.relpath(m._lib.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "library_version": int(m._lib.load().qd_version()), "marginals": args.marginals, "info": dec.info(),
           "shots": shots, "window": list(H.shape), "ms": wall(run, args.reps),
           "outputs_sha1": hashlib.sha1(bits.cpu().numpy().tobytes() + status.cpu().numpy().tobytes()).hexdigest()}
    print(json.dumps(res))
    save(args.out, res)


def part_collect(args):
    def load(paths):
        return [json.load(open(p)) for p in paths]

    def summary(runs):
        v = [x for r in runs for x in r["ms"]]
        return {"median": round(statistics.median(v), 3), "min": min(v), "max": max(v), "runs": len(runs)} if v else None

    this, parent = load(args.this), load(args.parent)
    lds = [r for r in this if r["info"].get("relay_marginals") == "lds"]
    dev = [r for r in this if r["info"].get("relay_marginals") == "device"]
    p, l, d = summary(parent), summary(lds), summary(dev)
    out = {"workload": "bb144_custom_r12_p0.003, one window, RelayConfig(), osd_off, %d DEM-sampled shots in batches of 65536" % parent[0]["shots"],
           "parent_ms": p, "this_lds_ms": l, "this_device_ms": d,
           "parent_spread_frac": round((p["max"] - p["min"]) / p["median"], 4), "lds_vs_parent_frac": round(l["median"] / p["median"] - 1, 4),
           "lds_inside_parent_spread": p["min"] <= l["median"] <= p["max"],          # the median inside the parent's [min, max] ...
           "lds_difference_below_parent_spread": abs(l["median"] - p["median"]) <= p["max"] - p["min"],          # ... or at least no farther from its median
           "device_vs_lds_frac": round(d["median"] / l["median"] - 1, 4) if d else None,
           "same_outputs": len({r["outputs_sha1"] for r in this + parent}) == 1, "runs": {"this": this, "parent": parent}}
    print(json.dumps({k: out[k] for k in out if k != "runs"}))
    save(args.out, out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", default="bb144", choices=["bb144", "qlp", "headline", "collect"])
    ap.add_argument("--points", default="0.001:1048576,0.003:1048576,0.006:1048576")
    ap.add_argument("--shots", type=int, default=0)
    ap.add_argument("--marginals", default="auto", choices=["auto", "lds", "device"])
    ap.add_argument("--this", nargs="+")
    ap.add_argument("--parent", nargs="+")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.part == "collect":
        return part_collect(args)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(here, "tests"), here):
        sys.path.insert(0, p)
    import types
    import torch
    import helpers
    from quits_amd import _lib
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.decoder.bposd import BpOsdDecoder
    from quits_amd.decoder.device import DemSampler
    from quits_amd.decoder.plan import cached_circuit_plan
    from quits_amd.decoder.relaybp import RelayBpDecoder, relay_options
    from quits_amd.dem import Circuit
    from quits_amd.relay import RelayConfig
    m = types.SimpleNamespace(torch=torch, helpers=helpers, _lib=_lib, detector_error_model_to_matrix=detector_error_model_to_matrix,
                              BpOsdDecoder=BpOsdDecoder, DemSampler=DemSampler, cached_circuit_plan=cached_circuit_plan, RelayBpDecoder=RelayBpDecoder,
                              relay_options=relay_options, Circuit=Circuit, RelayConfig=RelayConfig)
    {"bb144": part_bb144, "qlp": part_qlp, "headline": part_headline}[args.part](args, m)


if __name__ == "__main__":
    main()
