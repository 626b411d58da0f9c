#!/usr/bin/env python3
"""Time the bit-packing kernels (csrc/bitpack.hip) and the headline call fed with bit-packed host samples.

    python tools/packed_input_timing.py --part kernels|dropin [--shots 1048576] [--out profiles/packed_input_timing.json]

  kernels   qd_unpack_b8 and qd_pack_b8 over 2^20 rows of 1008 bits (126 packed bytes, 1008 unpacked), device events, median of 5 calls
            after a warm-up, with the bytes each has to move (packed + unpacked) per second beside the 8 TB/s HBM peak; unpack again with
            bit0 = 3 (rows of 127 packed bytes: every group reads two source bytes, every row starts at an odd address).
  dropin    sliding_window_bposd_circuit_mem on bb144_custom_r12 at p = 0.003, the whole history as one window, minimum_sum / parallel /
            max_iter = 50 / osd_0 (the headline configuration), `--shots` shots from a host bool array and from host PackedSamples of the same
            shots: wall time of three calls each, alternating, after one warm-up call each, in one process.  The expectation is that the
            packed call is not slower than the unpacked one beyond the spread of the unpacked call's own three repetitions.
Each part is one GPU step; the parts merge into the file named by --out, and the part's JSON is printed on one line."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import helpers  # noqa: E402

NAME = "bb144_custom_r12_p0.003"
KW = dict(max_iter=50, osd_order=0, bp_method="minimum_sum", schedule="parallel", osd_method="osd_0")
W, F = 14, 1                                                         # R + 2 rounds of detectors: one window
HBM_PEAK_GBPS = 8000.0


def timed(fn, reps=5):
    import torch
    fn()                                                             # warm-up
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def kernels(B=1 << 20, nbits=1008):
    import torch
    from quits_amd.samples import pack_b8_into, unpack_b8_into
    g = torch.Generator(device="cuda").manual_seed(1)
    out = {"rows": B, "bits": nbits, "hbm_peak_GBps": HBM_PEAK_GBPS}
    bits = torch.empty((B, nbits), dtype=torch.uint8, device="cuda")
    for tag, bit0 in (("unpack", 0), ("unpack_bit0_3", 3)):
        nb = (bit0 + nbits + 7) // 8
        packed = torch.randint(0, 256, (B, nb), dtype=torch.uint8, device="cuda", generator=g)
        row = timed(lambda: unpack_b8_into(packed, bit0, nbits, bits))
        row["bytes"] = B * (nb + nbits)
        row["GBps"] = round(row["bytes"] / row["median_ms"] / 1e6, 1)
        row["fraction_of_peak"] = round(row["GBps"] / HBM_PEAK_GBPS, 4)
        out[tag] = row
    packed = torch.empty((B, (nbits + 7) // 8), dtype=torch.uint8, device="cuda")
    row = timed(lambda: pack_b8_into(bits, packed))
    row["bytes"] = B * (packed.shape[1] + nbits)
    row["GBps"] = round(row["bytes"] / row["median_ms"] / 1e6, 1)
    row["fraction_of_peak"] = round(row["GBps"] / HBM_PEAK_GBPS, 4)
    out["pack"] = row
    return out


def dropin(shots):
    from quits_amd.decoder import sliding_window_bposd_circuit_mem
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.decoder.device import DemSampler
    from quits_amd.dem import Circuit
    from quits_amd.samples import PackedSamples
    circ = Circuit(helpers.circuit_text(NAME))
    cd = helpers.code("bb144")
    H, L, pri = detector_error_model_to_matrix(circ)
    det = DemSampler(H, L, pri).sample(shots, seed=2026)[0].cpu().numpy().astype(bool)
    packed = PackedSamples.pack(det)

    def call(samples):
        t0 = time.perf_counter()
        pred = sliding_window_bposd_circuit_mem(samples, circ, cd["hz"], cd["lz"], W, F, **KW)
        return time.perf_counter() - t0, pred

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, ref = call(det)                                           # warm-up: builds the plan, sizes the workspaces and the staging buffers
        _, got = call(packed)
        same = bool(np.array_equal(ref, got))
        t_u, t_p = [], []
        for _ in range(3):
            t_u.append(call(det)[0])
            t_p.append(call(packed)[0])
    out = {"shots": shots, "host_bytes_unpacked": int(det.nbytes), "host_bytes_packed": int(packed.data.nbytes), "identical_predictions": same,
           "unpacked_s": [round(t, 4) for t in t_u], "packed_s": [round(t, 4) for t in t_p]}
    out["unpacked_spread_s"] = round(max(t_u) - min(t_u), 4)
    out["packed_minus_unpacked_median_s"] = round(float(np.median(t_p) - np.median(t_u)), 4)
    out["unpacked_shots_per_s"] = round(shots / float(np.median(t_u)))
    out["packed_shots_per_s"] = round(shots / float(np.median(t_p)))
    out["packed_not_slower_beyond_spread"] = bool(np.median(t_p) - np.median(t_u) <= max(t_u) - min(t_u))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=("kernels", "dropin"), required=True)
    ap.add_argument("--shots", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = kernels() if args.part == "kernels" else dropin(args.shots)
    print(json.dumps({args.part: res}))
    if args.out:
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                doc = json.load(fh)
        doc[args.part] = res
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
