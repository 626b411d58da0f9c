#!/usr/bin/env python3
"""Time Relay-BP beside min-sum + OSD on the headline window, in one session, on the same DEM-sampled shots.

    python tools/relay_timing.py [--points 0.001:1048576,0.003:1048576,0.006:1048576] [--reps 5] --out profiles/relay_bp_timing.json

Circuit bb144_custom_r12 (BB [[144,12,12]], 12 rounds), the whole history as one window, at each physical error rate p of `--points`
(p:shots).  Per point the same shots go through
  relay          RelayConfig() (80 + 60 x 60 iterations), osd_off
  relay_nconv5   the same with stop_nconv = 5
  ms50_osd0      minimum_sum / parallel / max_iter 50 + osd_0 (the headline configuration)
  ms50_osdcs1    the same BP + osd_cs of order 1
and each records shots/s (median of `--reps` plan.decode calls after a warm-up, host clock around a device synchronise) and the logical error
rate with its binomial sigma; the relay rows also the mean iterations per shot and the share of shots no leg solved.  No target: the
numbers are what they are."""
import argparse
import json
import math
import os
import statistics
import sys
import time

W, F = 14, 1                                                         # R + 2 rounds of detectors: one window


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", default="0.001:1048576,0.003:1048576,0.006:1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(here, "tests"), here):
        sys.path.insert(0, p)
    import numpy as np
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
    cd = helpers.code("bb144")
    ms = dict(bp_method="minimum_sum", schedule="parallel", max_iter=50)
    configs = [("relay", RelayBpDecoder, relay_options(RelayConfig())),
               ("relay_nconv5", RelayBpDecoder, relay_options(RelayConfig(stop_nconv=5))),
               ("ms50_osd0", BpOsdDecoder, dict(ms, osd_method="osd_0", osd_order=0)),
               ("ms50_osdcs1", BpOsdDecoder, dict(ms, osd_method="osd_cs", osd_order=1))]
    res = {"device": torch.cuda.get_device_name(0), "library_version": int(_lib.load().qd_version()),
           "workload": "bb144_custom_r12, one window, DEM-sampled shots (seed 7)", "reps": args.reps,
           "method": "host clock around a device synchronise, one warm-up call before each series of %d; one session" % args.reps, "points": []}
    for item in args.points.split(","):
        p_txt, shots = item.split(":")
        p, shots = float(p_txt), int(shots)
        circ = Circuit(helpers.circuit_text("bb144_custom_r12_p%s" % p_txt))
        H, L, pri = detector_error_model_to_matrix(circ.detector_error_model())
        det, obs = DemSampler(H, L, pri).sample(shots, seed=7)
        point = {"p": p, "shots": shots, "window": list(H.shape), "rows": {}}
        for name, cls, opts in configs:
            plan = cached_circuit_plan(circ, cd["hz"], W, F, H.shape[0] // cd["hz"].shape[0] - 2, cls, cls, opts, opts)
            with plan.in_use():
                stats = []
                pred = plan.decode(det, stats)                       # warm-up; its predictions and status words are the row's
                torch.cuda.synchronize()
                ms_list = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    plan.decode(det)
                    torch.cuda.synchronize()
                    ms_list.append(round((time.perf_counter() - t0) * 1e3, 3))
                errors = int((pred != obs).any(dim=1).sum())
                st = torch.cat([s for _, s in stats]).cpu().numpy()
                ler = errors / shots
                row = {"ms": ms_list, "shots_per_s": round(shots / (statistics.median(ms_list) * 1e-3), 1), "errors": errors, "ler": ler,
                       "sigma": math.sqrt(max(ler * (1 - ler), 0.0) / shots), "mean_iterations": float((st & _lib.STATUS_ITER_MASK).mean()),
                       "bp_unconverged_share": float(((st & _lib.STATUS_CONVERGED) == 0).mean())}
                if cls is RelayBpDecoder:
                    legs = (st & _lib.STATUS_RELAY_LEG_MASK) >> _lib.STATUS_RELAY_LEG_SHIFT
                    solved = (st & _lib.STATUS_CONVERGED) != 0
                    row["unsolved_share"] = row.pop("bp_unconverged_share")
                    row["solved_in_leg0_share"] = float((solved & (legs == 0)).mean())
                    row["max_iterations"] = int((st & _lib.STATUS_ITER_MASK).max())
            plan.release_workspaces()
            point["rows"][name] = row
            print(p, name, json.dumps(row), flush=True)
        res["points"].append(point)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:                             # after every point: a later point's trouble keeps the earlier ones
            fh.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
