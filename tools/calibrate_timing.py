#!/usr/bin/env python3
"""Time the prior fit (quits_amd/calibrate.py, csrc/calibrate.hip) and measure what it gives back.

    python tools/calibrate_timing.py [--parts timing,convergence,circuit,decoder] [--shots 1048576] [--reps 5] --out profiles/calibrate_timing.json

Circuit bb144_custom_r12 at p = 3e-3 (1008 detectors x 9504 hyperedges), one session; host clock around a device synchronise, medians of
--reps after a warm-up.
  timing       qd_bit_planes and qd_parity_counts on --shots resident DEM-sampled shots, next to DemSampler.sample and plan.decode (min-sum 50,
               OSD-0, one window) of the same shots, the whole estimate_priors call on them, and the numpy mirror on 2^16 of them.
  convergence  median relative error and rms z = (raw - p) / stderr against the model's priors at 2^18, 2^20 and 2^22 shots of DemSampler.
  circuit      the same with sampler='circuit': the frame sampler's shots fitted on the extractor's hyperedges, with the columns beyond |z| = 4.
  decoder      a drifted truth -- every prior times a log-uniform factor in [1/3, 3], fixed seed -- sampled --shots times; min-sum 50 + OSD-0 and
               OSD-CS(1) decode those shots with the truth, with the nominal model and with the model fitted from --shots other shots.
The file is rewritten after every part."""
import argparse
import json
import os
import statistics
import sys
import time

NAME = "bb144_custom_r12_p0.003"
BP = dict(max_iter=50, bp_method="minimum_sum", schedule="parallel")


def wall(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(round((time.perf_counter() - t0) * 1e3, 3))
    return {"median_ms": statistics.median(out), "all_ms": out}


def z_summary(res, truth, np, list_beyond=None):
    z = (res.raw - truth) / res.stderr
    out = {"shots": int(res.shots), "median_rel_err": float(np.median(np.abs(res.raw / truth - 1))), "rms_z": float(np.sqrt((z ** 2).mean())),
           "mean_z": float(z.mean()), "share_beyond_3": float((np.abs(z) > 3).mean()), "max_abs_z": float(np.abs(z).max()),
           "clipped": int(len(res.clipped)), "unidentified": int(len(res.unidentified)), "seconds": round(res.seconds, 3)}
    if list_beyond is not None:
        far = np.flatnonzero(np.abs(z) > list_beyond)
        out["columns_beyond_%g" % list_beyond] = [{"column": int(j), "weight": int(res.table.weight[j]), "detectors": [int(d) for d in res.table.detectors(j)],
                                                   "model": float(truth[j]), "raw": float(res.raw[j]), "stderr": float(res.stderr[j]), "z": float(z[j])}
                                                  for j in far[:64]]
        out["count_beyond_%g" % list_beyond] = int(len(far))
        by_w = {}
        for w in np.unique(res.table.weight):
            sel = res.table.weight == w
            by_w[int(w)] = {"columns": int(sel.sum()), "mean_z": float(z[sel].mean()), "rms_z": float(np.sqrt((z[sel] ** 2).mean()))}
        out["by_weight"] = by_w
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parts", default="timing,convergence,circuit,decoder")
    ap.add_argument("--shots", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="18,20,22", help="log2 of the shot counts of the convergence and circuit parts")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(here, "tests"), here):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import helpers
    from quits_amd import _lib
    from quits_amd import calibrate as qc
    from quits_amd.decoder import decode_dem
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.decoder.device import DemSampler
    from quits_amd.dem import Circuit
    circ = Circuit(helpers.circuit_text(NAME))
    H, L, pri = detector_error_model_to_matrix(circ.detector_error_model())
    pri = np.asarray(pri, dtype=np.float64)
    table = qc.hyperedge_table(H, L)
    res = {"workload": NAME, "library_version": int(_lib.load().qd_version()), "device": torch.cuda.get_device_name(0), "model": list(H.shape),
           "counters": int(table.total), "weights": {int(w): int((table.weight == w).sum()) for w in np.unique(table.weight)}}
    parts = args.parts.split(",")
    sizes = [1 << int(x) for x in args.sizes.split(",")]

    def save():
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res) + "\n")

    def sample(smp, shots, seed):
        parts_ = [smp.sample(min(1 << 18, shots - s), seed, s) for s in range(0, shots, 1 << 18)]
        return torch.cat([d for d, _ in parts_]), torch.cat([o for _, o in parts_])

    if "timing" in parts:
        N = args.shots
        smp = DemSampler(H, L, pri)
        det, _ = sample(smp, N, 7)
        counter = qc.ParityCounter(table)
        planes = counter.planes(det)
        row = torch.zeros(table.total, dtype=torch.int64, device="cuda")
        t = {"shots": N, "tasks": counter.tasks, "planes_bytes": int(planes.numel() * 8), "det_bytes": int(det.numel())}
        t["bit_planes"] = wall(lambda: counter.planes(det, planes), args.reps)
        t["parity_counts"] = wall(lambda: counter.count_planes(planes, (N + 63) // 64, row), args.reps)
        one = torch.zeros(table.total, dtype=torch.int64, device="cuda")
        counter.count_planes(planes, (N + 63) // 64, one)
        small = 1 << 16
        host = det[:small].cpu().numpy()
        t0 = time.perf_counter()
        ref = qc.parity_counts_mirror(host, table, blocks=1)[0][0]
        t["mirror_65536_shots_s"] = round(time.perf_counter() - t0, 3)
        chk = torch.zeros(table.total, dtype=torch.int64, device="cuda")
        counter.add(det[:small], chk)
        t["device_equals_mirror_on_65536"] = bool(np.array_equal(chk.cpu().numpy(), ref))
        batched = qc.estimate_priors((H, L, pri), det)
        t["one_call_equals_batched"] = bool(np.array_equal(batched.counts.sum(axis=0), one.cpu().numpy()))
        counter.close()
        del planes, row, one, chk
        t["estimate_priors_on_resident_shots"] = wall(lambda: qc.estimate_priors((H, L, pri), det), 3)
        t0 = time.perf_counter()
        qc.fit_priors(batched.counts, batched.block_shots, table, pri)
        t["fit_host_s"] = round(time.perf_counter() - t0, 3)
        t["dem_sampler_sample"] = wall(lambda: sample(smp, N, 7), args.reps)
        opts = dict(BP, osd_method="osd_0", osd_order=0)
        decode_dem(circ, det[:1 << 16], **opts)                                   # builds the cached plan
        t["decode_minsum50_osd0"] = wall(lambda: decode_dem(circ, det, **opts), args.reps)
        res["timing"] = t
        save()
        del det

    if "convergence" in parts:
        res["convergence_dem_sampler"] = [z_summary(qc.estimate_priors(circ, shots=n, seed=1, sampler="dem"), pri, np) for n in sizes]
        save()

    if "circuit" in parts:
        res["extractor_against_frame_sampler"] = [z_summary(qc.estimate_priors(circ, shots=n, seed=1, sampler="circuit"), pri, np, list_beyond=4.0) for n in sizes]
        save()

    if "decoder" in parts:
        N = args.shots
        rng = np.random.default_rng(20261021)
        truth = pri * np.exp(rng.uniform(-np.log(3.0), np.log(3.0), len(pri)))
        smp = DemSampler(H, L, truth)
        fit = qc.estimate_priors((H, L, pri), sample(smp, N, 11)[0])
        det, obs = sample(smp, N, 12)
        obs_h = obs.cpu().numpy().astype(np.int64)
        texts = {"truth": qc.model_dem_text(table, truth), "nominal": qc.model_dem_text(table, pri), "fitted": fit.dem_text()}
        d = {"shots": N, "drift": "log-uniform in [1/3, 3], numpy default_rng(20261021)", "fit": z_summary(fit, truth, np),
             "fitted_median_rel_err": float(np.median(np.abs(fit.priors / truth - 1))), "nominal_median_rel_err": float(np.median(np.abs(pri / truth - 1)))}
        for dec, opts in (("minsum50_osd0", dict(BP, osd_method="osd_0", osd_order=0)), ("minsum50_osdcs1", dict(BP, osd_method="osd_cs", osd_order=1))):
            d[dec] = {}
            for which, text in texts.items():
                t0 = time.perf_counter()
                pred = decode_dem(text, det, **opts)
                errors = int((pred != obs_h).any(axis=1).sum())
                pL = errors / N
                d[dec][which] = {"errors": errors, "pL": pL, "sigma": (pL * (1 - pL) / N) ** 0.5, "seconds": round(time.perf_counter() - t0, 3)}
                res["decoder_on_drifted_truth"] = d
                save()
        res["decoder_on_drifted_truth"] = d
        save()
    print(json.dumps({k: v for k, v in res.items() if k != "extractor_against_frame_sampler"}))


if __name__ == "__main__":
    main()
