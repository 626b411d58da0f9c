#!/usr/bin/env python3
"""Time the fault-level outputs (corrections, sampled faults, the fault spectrum) against the paths they sit next to.

    python tools/fault_outputs_timing.py run [--root DIR] [--parts decode,sample,spectrum] [--shots 1048576] [--reps 5] --out FILE
    python tools/fault_outputs_timing.py collect --this FILE [FILE ...] --parent FILE [FILE ...] --out profiles/fault_outputs_timing.json

Circuit bb144_custom_r12, the whole history as one window, minimum_sum / parallel / max_iter = 50 / osd_0 (the headline configuration).
  decode    plan.decode on `--shots` resident DEM-sampled shots without `correction`, `--reps` calls after a warm-up, host clock around a
            device synchronise; the same with `correction` where the package under --root has it.  Run the part on this commit and on a
            checkout of its parent (--root), alternating the two in one session: the parent's spread is the margin within which the path
            without `correction` must be unchanged.
  sample    DemSampler.sample against DemSampler.sample_faults, 2^18 shots a call.
  spectrum  get_fault_spectrum against get_circuit_mem_pL(sampler='dem') on `--shots` shots, same seed and batch.
`collect` puts the runs' files into one JSON with the medians and the overheads."""
import argparse
import json
import os
import sys
import time

NAME = "bb144_custom_r12_p0.003"
KW = dict(max_iter=50, osd_order=0, bp_method="minimum_sum", schedule="parallel", osd_method="osd_0")
W, F = 14, 1                                                         # R + 2 rounds of detectors: one window


def wall(fn, reps):
    import torch
    fn()                                                             # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(round((time.perf_counter() - t0) * 1e3, 3))
    return out


def run(args):
    root = os.path.abspath(args.root)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(here, "tests"), root):                    # fixtures from this tree, the package from --root
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import helpers
    import quits_amd
    from quits_amd import _lib
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.decoder.bposd import BpOsdDecoder
    from quits_amd.decoder.device import DemSampler
    from quits_amd.decoder.plan import cached_circuit_plan
    from quits_amd.dem import Circuit
    from quits_amd.simulation import get_circuit_mem_pL
    assert os.path.abspath(quits_amd.__file__).startswith(root), quits_amd.__file__
    circ = Circuit(helpers.circuit_text(NAME))
    cd = helpers.code("bb144")
    H, L, pri = detector_error_model_to_matrix(circ.detector_error_model())
    smp = DemSampler(H, L, pri)
    opts = {'bp_method': KW["bp_method"], 'max_iter': KW["max_iter"], 'schedule': KW["schedule"], 'osd_method': KW["osd_method"],
            'osd_order': KW["osd_order"]}
    plan = cached_circuit_plan(circ, cd["hz"], W, F, smp.m // cd["hz"].shape[0] - 2, BpOsdDecoder, BpOsdDecoder, opts, opts)
    has = hasattr(plan, "nfaults")
    res = {"root": root, "library_version": int(_lib.load().qd_version()), "fault_outputs": has, "shots": args.shots, "window": list(H.shape),
           "chunk": int(plan.chunk), "lanes": int(plan.lanes)}
    parts = args.parts.split(",")
    with plan.in_use():
        if "decode" in parts:
            det = torch.cat([smp.sample(1 << 18, 7, s)[0] for s in range(0, args.shots, 1 << 18)])[:args.shots]
            ref = plan.decode(det)
            res["decode_ms"] = wall(lambda: plan.decode(det), args.reps)
            if has:
                corr = torch.empty((args.shots, (plan.nfaults + 31) // 32), dtype=torch.int32, device="cuda")
                pred = plan.decode(det, None, corr)
                assert torch.equal(pred, ref), "predictions change with `correction`"
                res["decode_correction_ms"] = wall(lambda: plan.decode(det, None, corr), args.reps)
                res["decode_ms_after"] = wall(lambda: plan.decode(det), args.reps)
                res["correction_bytes_per_shot"] = 4 * corr.shape[1]
            del det
        if "sample" in parts:
            res["sample_ms"] = wall(lambda: smp.sample(1 << 18, 7), args.reps)
            if has:
                res["sample_faults_ms"] = wall(lambda: smp.sample_faults(1 << 18, 7), args.reps)
                res["sample_ms_after"] = wall(lambda: smp.sample(1 << 18, 7), args.reps)
    if "spectrum" in parts:
        a = (circ, cd["hz"], cd["lz"], W, F, args.shots)
        get_circuit_mem_pL(*a, sampler="dem", seed=3, **KW)          # warm-up: workspaces, lanes
        mem = [get_circuit_mem_pL(*a, sampler="dem", seed=3, **KW) for _ in range(3)]
        res["mem_pL_s"] = [round(r.seconds, 4) for r in mem]
        res["mem_pL_errors"] = int(mem[0].errors)
        if has:
            from quits_amd.simulation import get_fault_spectrum
            get_fault_spectrum(*a, seed=3, **KW)
            sp = [get_fault_spectrum(*a, seed=3, **KW) for _ in range(3)]
            assert (sp[0].shots, sp[0].errors) == (mem[0].shots, mem[0].errors)
            res["spectrum_s"] = [round(r.seconds, 4) for r in sp]
            res["spectrum"] = {"errors": sp[0].errors, "residual_shots": sp[0].residual_shots, "lightest": sp[0].lightest,
                               "mean_faults": float((np.arange(256) * sp[0].shots_by_faults).sum() / sp[0].shots)}
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


def collect(args):
    import statistics

    def load(paths):
        return [json.load(open(p)) for p in paths]

    def pool(runs, key):
        return [x for r in runs for x in r.get(key, [])]

    def med(v):
        return round(statistics.median(v), 3) if v else None

    this, parent = load(args.this), load(args.parent)
    out = {"workload": "%s, one window, %s" % (NAME, KW), "runs": {"this": this, "parent": parent}}
    p, t, tc = pool(parent, "decode_ms"), pool(this, "decode_ms") + pool(this, "decode_ms_after"), pool(this, "decode_correction_ms")
    out["decode"] = {"parent_ms": {"median": med(p), "min": min(p), "max": max(p)}, "this_ms": {"median": med(t), "min": min(t), "max": max(t)},
                     "this_with_correction_ms": {"median": med(tc), "min": min(tc), "max": max(tc)},
                     "parent_spread_frac": round((max(p) - min(p)) / med(p), 4), "this_vs_parent_frac": round(med(t) / med(p) - 1, 4),
                     "correction_overhead_frac": round(med(tc) / med(t) - 1, 4)}
    s, sf = pool(this, "sample_ms") + pool(this, "sample_ms_after"), pool(this, "sample_faults_ms")
    if s and sf:
        out["sample"] = {"sample_ms": med(s), "sample_faults_ms": med(sf), "overhead_frac": round(med(sf) / med(s) - 1, 4)}
    m, sp = pool(this, "mem_pL_s"), pool(this, "spectrum_s")
    if m and sp:
        out["spectrum"] = {"mem_pL_s": med(m), "spectrum_s": med(sp), "overhead_frac": round(med(sp) / med(m) - 1, 4)}
    line = json.dumps(out)
    print(json.dumps({k: out[k] for k in out if k != "runs"}))
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r.add_argument("--parts", default="decode,sample,spectrum")
    r.add_argument("--shots", type=int, default=1 << 20)
    r.add_argument("--reps", type=int, default=5)
    r.add_argument("--out", required=True)
    c = sub.add_parser("collect")
    c.add_argument("--this", nargs="+", required=True)
    c.add_argument("--parent", nargs="+", required=True)
    c.add_argument("--out", required=True)
    args = ap.parse_args()
    (run if args.cmd == "run" else collect)(args)


if __name__ == "__main__":
    main()
