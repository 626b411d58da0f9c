#!/usr/bin/env python3
"""Time the stratified DEM sampler beside the sampler and the decoder it feeds, in one session.

    python tools/stratified_timing.py [--shots 1048576] [--reps 5] --out profiles/stratified_sampler_timing.json

Circuit bb144_custom_r12, the whole history as one window, minimum_sum / parallel / max_iter = 50 / osd_0 (the headline configuration).
  strata_k8, strata_k52   StratifiedDemSampler.sample_faults of `--shots` rows with 8 / 52 faults each (the mean fault count is 51.6), in calls
                          of 2^18 rows;
  dem                     DemSampler.sample_faults on the same count, same calls;
  decode                  plan.decode of `--shots` resident shots (the k = 52 rows).
Host clock around a device synchronise, `--reps` calls after a warm-up each.  The experiment stays decoder-bound while the stratified sampler
takes at most a tenth of the decode time: `sampler_over_decode` says what it takes."""
import argparse
import json
import os
import statistics
import sys
import time

NAME = "bb144_custom_r12_p0.003"
KW = dict(max_iter=50, osd_order=0, bp_method="minimum_sum", schedule="parallel", osd_method="osd_0")
W, F = 14, 1                                                         # R + 2 rounds of detectors: one window
CALL = 1 << 18


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shots", type=int, default=1 << 20)
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
    from quits_amd.decoder.device import DemSampler, StratifiedDemSampler
    from quits_amd.decoder.plan import cached_circuit_plan
    from quits_amd.dem import Circuit
    circ = Circuit(helpers.circuit_text(NAME))
    cd = helpers.code("bb144")
    H, L, pri = detector_error_model_to_matrix(circ.detector_error_model())
    t0 = time.perf_counter()
    smp = StratifiedDemSampler(H, L, pri, 255)
    table_s = time.perf_counter() - t0
    dem = DemSampler(H, L, pri)
    opts = {'bp_method': KW["bp_method"], 'max_iter': KW["max_iter"], 'schedule': KW["schedule"], 'osd_method': KW["osd_method"],
            'osd_order': KW["osd_order"]}
    plan = cached_circuit_plan(circ, cd["hz"], W, F, smp.m // cd["hz"].shape[0] - 2, BpOsdDecoder, BpOsdDecoder, opts, opts)
    pieces = [(s, min(CALL, args.shots - s)) for s in range(0, args.shots, CALL)]
    words = (smp.nfaults + 31) // 32
    fb = torch.empty((CALL, words), dtype=torch.int32, device="cuda")

    def strata_run(k):
        for s, n in pieces:
            smp.sample_faults(k, 7, s, fb[:n], shots=n)

    def dem_run():
        for s, n in pieces:
            dem.sample_faults(n, 7, s, fb[:n])

    res = {"device": torch.cuda.get_device_name(0), "library_version": int(_lib.load().qd_version()), "workload": "%s, one window, %s" % (NAME, KW),
           "window": list(H.shape), "shots": args.shots, "rows_per_call": CALL, "table": smp.info(), "table_build_s": round(table_s, 3),
           "mean_faults": float(np.sum(pri)), "pmf": {"k8": float(smp.pmf[8]), "k52": float(smp.pmf[52]), "at_most_8": float(smp.pmf[:9].sum())}}
    with plan.in_use():
        res["strata_k8_ms"] = wall(lambda: strata_run(8), args.reps)
        res["strata_k52_ms"] = wall(lambda: strata_run(52), args.reps)
        res["dem_ms"] = wall(dem_run, args.reps)
        det = torch.cat([smp.sample_faults(52, 7, s, shots=n)[0] for s, n in pieces])
        res["decode_ms"] = wall(lambda: plan.decode(det), args.reps)
        res["strata_k52_ms_after"] = wall(lambda: strata_run(52), args.reps)
    med = lambda v: round(statistics.median(v), 3)
    worst = max(med(res["strata_k8_ms"]), med(res["strata_k52_ms"] + res["strata_k52_ms_after"]))
    res["median_ms"] = {"strata_k8": med(res["strata_k8_ms"]), "strata_k52": med(res["strata_k52_ms"] + res["strata_k52_ms_after"]), "dem": med(res["dem_ms"]),
                        "decode": med(res["decode_ms"])}
    res["sampler_over_decode"] = round(worst / med(res["decode_ms"]), 4)
    res["decoder_bound"] = bool(worst <= 0.1 * med(res["decode_ms"]))
    res["method"] = "host clock around a device synchronise, one warm-up call before each series of %d; one session" % args.reps
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
