#!/usr/bin/env python3
"""Shrink every failing shot of a headline run to a 1-minimal failing set, and say what it costs beside finding the failures.

    python tools/shrink_timing.py [--shots 1048576] [--relay-shots 1048576] [--runs osd0,osdcs1,relay] --out profiles/shrink_timing.json

Circuit bb144_custom_r12 at p = 0.003, the whole history as one window, DEM-sampled shots of one seed, minimum_sum / parallel / max_iter = 50
with OSD-0 and with OSD-CS order 1, and Relay-BP (RelayConfig() without a post-processor).  Per run, in one session:
  spectrum_s            get_fault_spectrum on the same shots (Relay-BP: get_relay_mem_pL with sampler='dem'): what finding the failures costs;
  run                   get_minimal_failures as a user calls it: parents, rounds, decodes, trials per parent, both weight histograms, the
                        lightest set and the lightest residual, and its wall time by part (find / shrink / final);
  profiled              the same call with profile=True -- a device synchronise around every plan.decode of the shrink, host clock -- which
                        splits the shrink into the plan.decode calls ("shrink_decode_s") and everything else ("shrink_other_s": the step
                        kernels, the tallies, the per-round read of the live count, and the idle time the synchronises add).
The decode time of the same rounds is existing code and is the reference for the split.  A warm-up call builds the plan first."""
import argparse
import json
import os
import sys
import time

NAME = "bb144_custom_r12_p0.003"
MINSUM = dict(max_iter=50, bp_method="minimum_sum", schedule="parallel")
W, F = 14, 1                                                         # R + 2 rounds of detectors: one window
SEED = 7


def sparse(hist):
    return {int(w): int(c) for w, c in enumerate(hist) if c}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shots", type=int, default=1 << 20)
    ap.add_argument("--relay-shots", type=int, default=None, help="shots of the Relay-BP run (default: --shots)")
    ap.add_argument("--runs", default="osd0,osdcs1,relay")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(here, "tests"), here):
        sys.path.insert(0, p)
    import torch
    import helpers
    from quits_amd import _lib
    from quits_amd.dem import Circuit
    from quits_amd.relay import RelayConfig
    from quits_amd.simulation import get_fault_spectrum, get_minimal_failures, get_relay_mem_pL, get_relay_minimal_failures
    circ = Circuit(helpers.circuit_text(NAME))
    cd = helpers.code("bb144")
    a = (circ, cd["hz"], cd["lz"], W, F)
    cfg = RelayConfig()
    runs = {
        "osd0": (lambda n, **kw: get_minimal_failures(*a, n, osd_method="osd_0", osd_order=0, seed=SEED, **MINSUM, **kw),
                 lambda n: get_fault_spectrum(*a, n, osd_method="osd_0", osd_order=0, seed=SEED, **MINSUM), args.shots),
        "osdcs1": (lambda n, **kw: get_minimal_failures(*a, n, osd_method="osd_cs", osd_order=1, seed=SEED, **MINSUM, **kw),
                   lambda n: get_fault_spectrum(*a, n, osd_method="osd_cs", osd_order=1, seed=SEED, **MINSUM), args.shots),
        "relay": (lambda n, **kw: get_relay_minimal_failures(*a, n, relay=cfg, osd_method="osd_off", seed=SEED, **kw),
                  lambda n: get_relay_mem_pL(*a, n, relay=cfg, osd_method="osd_off", seed=SEED, sampler="dem"),
                  args.shots if args.relay_shots is None else args.relay_shots),
    }
    res = {"device": torch.cuda.get_device_name(0), "library_version": int(_lib.load().qd_version()),
           "workload": "%s, one window, DEM-sampled shots (seed %d), %s" % (NAME, SEED, MINSUM), "relay": str(cfg),
           "method": "host clock around a device synchronise; one session; a 4096-shot warm-up call per run builds the plan", "runs": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in [r for r in args.runs.split(",") if r]:
        shrink_fn, find_fn, shots = runs[name]
        say = lambda what: print("%s: %s (%.1f s)" % (name, what, time.perf_counter() - t_run), file=sys.stderr, flush=True)
        t_run = time.perf_counter()
        shrink_fn(4096)
        say("warm")
        t0 = time.perf_counter()
        spec = find_fn(shots)
        spectrum_wall = time.perf_counter() - t0
        say("failures found")
        r = shrink_fn(shots)
        say("shrunk")
        q = shrink_fn(shots, profile=True)
        say("shrunk again with the profiling synchronises")
        same = (q.errors, q.parents, q.rounds, q.decodes, q.lightest, q.lightest_residual) == (r.errors, r.parents, r.rounds, r.decodes, r.lightest, r.lightest_residual)
        res["runs"][name] = {
            "shots": r.shots, "errors": r.errors, "errors_of_find_run": int(spec.errors), "parents": r.parents, "parents_truncated": r.parents_truncated,
            "all_minimal": bool(r.minimal.all()), "rounds": r.rounds, "decodes": r.decodes,
            "mean_trials_per_parent": round(float(r.trials.mean()), 2) if r.parents else None, "max_trials": int(r.trials.max()) if r.parents else None,
            "mean_start_weight": round(float(r.start_weights.mean()), 2) if r.parents else None,
            "mean_weight": round(float(r.weights.mean()), 3) if r.parents else None,
            "start_weight_hist": sparse(r.start_weight_hist), "weight_hist": sparse(r.weight_hist), "residual_weight_hist": sparse(r.residual_weight_hist),
            "lightest": r.lightest, "lightest_residual": r.lightest_residual,
            "spectrum_s": round(float(spec.seconds), 4), "spectrum_wall_s": round(spectrum_wall, 4),
            "run": {"seconds": round(r.seconds, 4), **{k + "_s": round(v, 4) for k, v in r.timing.items()}},
            "profiled": {"seconds": round(q.seconds, 4), "same_result": bool(same), "shrink_s": round(q.timing["shrink"], 4),
                         "shrink_decode_s": round(q.timing["shrink_decode"], 4),
                         "shrink_other_s": round(q.timing["shrink"] - q.timing["shrink_decode"], 4),
                         **{k: round(v, 5) for k, v in q.timing.items() if k.startswith("trial_") and (name == "relay" or k != "trial_later_leg_share")}},
            "shrink_over_find": round(r.timing["shrink"] / float(spec.seconds), 3) if spec.seconds else None,
        }
        with open(args.out, "w") as fh:                               # after every run: a later run that is cut short loses nothing
            fh.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
