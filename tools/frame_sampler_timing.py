#!/usr/bin/env python3
"""Time the circuit-level frame sampler against the DEM sampler and the headline decode on the same shots.

    python tools/frame_sampler_timing.py [--shots 1048576] [--reps 5] [--out profiles/frame_sampler_timing.json]

Circuit bb144_custom_r12_p0.003.  After one warm-up of each, device events time `reps` calls of CircuitSampler.sample and
DemSampler.sample (2^20 shots each) and one headline decode (minimum_sum, parallel, max_iter=50, OSD-0, the whole history as one
window) of the circuit-sampled shots; the median call is reported.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import helpers  # noqa: E402


def timed(fn, reps):
    import torch
    out, ms = None, []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, float(np.median(ms)), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.decoder.device import BatchDecoder, CircuitSampler, DemSampler, WindowGraph
    from quits_amd.dem import Circuit
    name = "bb144_custom_r12_p0.003"
    text = helpers.circuit_text(name)
    H, L, pri = detector_error_model_to_matrix(Circuit(text).detector_error_model())
    cs, ds = CircuitSampler(text), DemSampler(H, L, pri)
    dec = BatchDecoder(WindowGraph(H, pri), "minimum_sum", "parallel", 50, "osd_0")
    B = a.shots
    cs.sample(B, seed=1), ds.sample(B, seed=1)                      # warm-up
    (det, obs), c_ms, c_all = timed(lambda: cs.sample(B, seed=7), a.reps)
    _, d_ms, d_all = timed(lambda: ds.sample(B, seed=7), a.reps)
    dec.decode(det[:65536])
    _, dec_ms, dec_all = timed(lambda: dec.decode(det), max(1, a.reps // 2))
    torch.cuda.synchronize()
    row = dict(circuit=name, shots=B, info=cs.info(),
               circuit_sampler_ms=round(c_ms, 3), dem_sampler_ms=round(d_ms, 3), headline_decode_ms=round(dec_ms, 3),
               circuit_sampler_shots_per_s=round(B / c_ms * 1e3), dem_sampler_shots_per_s=round(B / d_ms * 1e3),
               headline_decode_shots_per_s=round(B / dec_ms * 1e3),
               circuit_sampler_over_decode=round(c_ms / dec_ms, 4),
               all_ms=dict(circuit_sampler=[round(x, 3) for x in c_all], dem_sampler=[round(x, 3) for x in d_all],
                           headline_decode=[round(x, 3) for x in dec_all]),
               device=torch.cuda.get_device_name(0))
    line = json.dumps(row)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
