#!/usr/bin/env python3
"""Time the soft outputs (per-shot records, the post-selected experiment) against the paths they sit next to, and read the acceptance curves.

    python tools/soft_outputs_timing.py run [--root DIR] [--parts decode,experiment,curves] [--shots 1048576] [--reps 5] --out FILE
    python tools/soft_outputs_timing.py collect --this FILE [FILE ...] --parent FILE [FILE ...] --out profiles/soft_outputs_timing.json

Circuit bb144_custom_r12 at p = 3e-3, the whole history as one window, minimum_sum / parallel / max_iter = 50 / osd_0 (the headline configuration).
  decode      plan.decode on `--shots` resident DEM-sampled shots without `soft`, `--reps` calls after a warm-up, host clock around a device
              synchronise; where the package under --root has soft outputs, the same with `correction` alone and with `correction` + `soft`.
              Run the part on this commit and on a checkout of its parent (--root), alternating the two in one session: the two issue the same
              launches without `soft`, so the parent's own spread is the margin within which that path must be unchanged.
  experiment  get_postselected_pL against get_circuit_mem_pL(sampler='dem') on `--shots` shots, same seed and batch.
  curves      pL at 0, 1, 5 and 20 % rejection by every field, `--curve_shots` shots, for OSD-0, OSD-CS order 1 and Relay-BP.
`collect` puts the runs' files into one JSON with the medians, both spreads and the overheads."""
import argparse
import json
import os
import sys
import time

NAME = "bb144_custom_r12_p0.003"
KW = dict(max_iter=50, osd_order=0, bp_method="minimum_sum", schedule="parallel", osd_method="osd_0")
W, F = 14, 1                                                         # R + 2 rounds of detectors: one window
REJECT = (0.0, 0.01, 0.05, 0.20)


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
    has = hasattr(plan, "commit_weights")
    res = {"root": "this" if root == here else "parent", "library_version": int(_lib.load().qd_version()), "soft_outputs": has, "shots": args.shots, "window": list(H.shape),
           "chunk": int(plan.chunk), "lanes": int(plan.lanes)}
    parts = args.parts.split(",")
    with plan.in_use():
        if "decode" in parts:
            det = torch.cat([smp.sample(1 << 18, 7, s)[0] for s in range(0, args.shots, 1 << 18)])[:args.shots]
            ref = plan.decode(det)
            res["decode_ms"] = wall(lambda: plan.decode(det), args.reps)
            if has:
                corr = torch.empty((args.shots, (plan.nfaults + 31) // 32), dtype=torch.int32, device="cuda")
                rec = torch.empty((args.shots, 6), dtype=torch.int64, device="cuda")
                pred = plan.decode(det, None, corr, rec)
                assert torch.equal(pred, ref), "predictions change with `soft`"
                res["decode_correction_ms"] = wall(lambda: plan.decode(det, None, corr), args.reps)
                res["decode_soft_ms"] = wall(lambda: plan.decode(det, None, corr, rec), args.reps)
                res["decode_ms_after"] = wall(lambda: plan.decode(det), args.reps)
                res["weight_table_bytes"] = 4 * int(plan.nfaults)
                del corr, rec
            del det
    a = (circ, cd["hz"], cd["lz"], W, F)
    if "experiment" in parts:
        get_circuit_mem_pL(*a, args.shots, sampler="dem", seed=3, **KW)          # warm-up: workspaces, lanes
        mem = [get_circuit_mem_pL(*a, args.shots, sampler="dem", seed=3, **KW) for _ in range(3)]
        res["mem_pL_s"] = [round(r.seconds, 4) for r in mem]
        res["mem_pL_errors"] = int(mem[0].errors)
        if has:
            from quits_amd.simulation import get_postselected_pL
            get_postselected_pL(*a, args.shots, sampler="dem", seed=3, **KW)
            ps = [get_postselected_pL(*a, args.shots, sampler="dem", seed=3, **KW) for _ in range(3)]
            assert (ps[0].shots, ps[0].errors) == (mem[0].shots, mem[0].errors)
            res["postselected_s"] = [round(r.seconds, 4) for r in ps]
    if "curves" in parts and has:
        from quits_amd.relay import RelayConfig
        from quits_amd.simulation import get_postselected_pL
        from quits_amd.soft import FIELDS
        curves = {}
        for name, kw in (("osd_0", dict(KW)), ("osd_cs_1", dict(KW, osd_method="osd_cs", osd_order=1)), ("relay_bp", dict(relay=RelayConfig()))):
            r = get_postselected_pL(*a, args.curve_shots, sampler="dem", seed=3, **kw)
            entry = {"shots": r.shots, "errors": r.errors, "pL": r.pL, "sigma": r.sigma, "seconds": round(r.seconds, 3), "shifts": [int(s) for s in r.shifts]}
            for f in FIELDS:                                         # (NaN -- nothing kept -- is written as null)
                entry[f] = [{k: (None if isinstance(v, float) and v != v else v) for k, v in dict(r.at_rejection(f, x), asked=x).items()} for x in REJECT]
            curves[name] = entry
        res["curves"] = curves
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

    def summary(v):
        return {"median": round(statistics.median(v), 3), "min": min(v), "max": max(v), "spread_frac": round((max(v) - min(v)) / statistics.median(v), 4)} if v else None

    this, parent = load(args.this), load(args.parent)
    out = {"workload": "%s, one window, %s" % (NAME, KW), "runs": {"this": this, "parent": parent}}
    p, t = pool(parent, "decode_ms"), pool(this, "decode_ms") + pool(this, "decode_ms_after")
    tc, ts = pool(this, "decode_correction_ms"), pool(this, "decode_soft_ms")
    if p and t:
        out["decode"] = {"parent_ms": summary(p), "this_ms": summary(t), "this_with_correction_ms": summary(tc), "this_with_soft_ms": summary(ts),
                         "this_vs_parent_frac": round(statistics.median(t) / statistics.median(p) - 1, 4),
                         "inside_parent_spread": bool(min(p) <= statistics.median(t) <= max(p)),
                         "soft_over_correction_frac": round(statistics.median(ts) / statistics.median(tc) - 1, 4) if tc and ts else None}
    m, ps = pool(this, "mem_pL_s"), pool(this, "postselected_s")
    if m and ps:
        out["experiment"] = {"mem_pL_s": summary(m), "postselected_s": summary(ps), "overhead_frac": round(statistics.median(ps) / statistics.median(m) - 1, 4)}
    for r in this:
        if "curves" in r:
            out["curves"] = r["curves"]
    line = json.dumps(out)
    print(json.dumps({k: out[k] for k in out if k not in ("runs", "curves")}))
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r.add_argument("--parts", default="decode,experiment,curves")
    r.add_argument("--shots", type=int, default=1 << 20)
    r.add_argument("--curve_shots", type=int, default=1 << 18)
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
