#!/usr/bin/env python3
"""Decode rate of the reference's standard window size on the project's large code, whose windows are off-chip.

    python tools/large_window_timing.py [--shots 16384] [--reps 2] [--oracle-shots 64] [--out profiles/large_window_timing.json]

QLP [[1020,136]], cardinal circuit, 20 rounds at p = 1e-3; flooding min-sum (max_iter 50) + OSD-0.  Detector samples come from the DEM
sampler on the device.  After a warm-up call, `reps` calls of the sliding-window plan's decode() are timed (wall clock around a device
synchronisation) for (W, F) = (5, 3) -- seven windows, six of them 2250 x 30 900 / 31 500 and off-chip: the one-message-per-edge BP kernel
with its messages in HBM and qd_osd0_offchip_kernel -- and, for context, for (3, 1), whose twenty windows of 1350 x 18 900 run in the
on-chip kernels.  The CPU oracle's rate over 16 processes on `oracle-shots` of the same shots is the third figure.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import helpers  # noqa: E402

NAME, ROUNDS, P = "qlp1020_cardinal_r20_p0.003", 20, 0.001
OPTS = dict(bp_method="minimum_sum", schedule="parallel", max_iter=50, osd_method="osd_0", osd_order=0)


def oracle_rate(circ, hz, det, W, F, procs):
    """Shots per second of oracle.sliding_window_decode over `procs` processes (shot slices), and its predictions."""
    import multiprocessing as mp
    import oracle as orc
    from quits_amd.decoder.base import spacetime, window_count
    nz = hz.shape[0]
    ncr, _, _ = window_count(ROUNDS, W, F)
    checks, commits, priors, updates = spacetime(circ, hz, W, F, ncr)
    wins = [{"H": checks[k], "L": commits[k], "priors": priors[k], "U": updates[k] if k < ncr else None, "row0": F * k * nz}
            for k in range(len(checks))]
    prm = ("minimum_sum", "parallel", OPTS["max_iter"], "osd_0", 0, 1.0, orc.FORM_LDPC_F64)
    parts = [p for p in np.array_split(np.ascontiguousarray(det), procs) if len(p)]
    with mp.get_context("fork").Pool(len(parts)) as pool:
        t0 = time.perf_counter()
        res = pool.map(helpers._sw_worker, [(wins, nz, p, prm, True) for p in parts])
        dt = time.perf_counter() - t0
    return len(det) / dt, np.concatenate([r[0] for r in res], axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--oracle-shots", type=int, default=64)
    ap.add_argument("--oracle-procs", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_window_timing.json"))
    a = ap.parse_args()
    import oracle as orc
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.dem import Circuit
    circ = Circuit(helpers.circuit_text_at_p(NAME, 0.003, P))
    H, L, pri = detector_error_model_to_matrix(circ)
    hz = helpers.code("qlp1020")["hz"]
    # the oracle first: its fork pool must not inherit an initialised device
    det_o = orc.sample_dem(H, L, pri, seed=7, shot0=0, B=a.oracle_shots)[0]
    o_rate, o_pred = oracle_rate(circ, hz, det_o, 5, 3, a.oracle_procs)

    import torch
    from quits_amd.decoder.device import DemSampler
    from quits_amd.decoder.sliding_window import build_circuit_plan
    det, obs = DemSampler(H, L, pri).sample(a.shots, seed=7)
    row = dict(circuit=NAME, p=P, rounds=ROUNDS, shots=a.shots, reps=a.reps, options=OPTS, device=torch.cuda.get_device_name(0))
    for W, F in ((5, 3), (3, 1)):
        plan = build_circuit_plan(circ, hz, W, F, ROUNDS, dict(OPTS), dict(OPTS))
        info = [d.info() for d in plan.decoders()]
        shapes = sorted({(d.graph.m, d.graph.n) for d in plan.decoders()}, reverse=True)
        plan.decode(det[:min(a.shots, 2048)])                        # warm-up: code objects, workspaces of the first chunk
        pred, secs = None, []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pred = plan.decode(det)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        best = min(secs)
        key = "W%dF%d" % (W, F)
        row[key] = dict(windows=len(plan.windows), window_shapes=shapes, off_chip_decoders=sum(1 for i in info if i["post_kernel"] == "qd_osd0_offchip_kernel"),
                        edge_kernel_decoders=sum(1 for i in info if i["edge_kernel"]), chunk=plan.chunk, pipelined=bool(plan.pipeline),
                        seconds=[round(s, 4) for s in secs], shots_per_s=round(a.shots / best),
                        logical_error_rate=float((pred != obs).any(dim=1).float().mean()))
        if (W, F) == (5, 3):
            n = min(a.oracle_shots, a.shots)
            row[key]["equals_oracle_on_first_shots"] = bool(np.array_equal(pred[:n].cpu().numpy(), o_pred[:n]))
        plan.release_workspaces()
        del plan
        torch.cuda.empty_cache()
    row["oracle_W5F3"] = dict(processes=a.oracle_procs, shots=a.oracle_shots, shots_per_s=round(o_rate, 2))
    row["W5F3_over_oracle"] = round(row["W5F3"]["shots_per_s"] / o_rate, 1)
    row["W5F3_over_W3F1"] = round(row["W5F3"]["shots_per_s"] / row["W3F1"]["shots_per_s"], 4)
    line = json.dumps(row)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
