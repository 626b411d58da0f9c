#!/usr/bin/env python3
"""Time qd_bp_minsum_kernel (csrc/bp_kernels.hip) by itself on the headline window.

    python tools/gather_minsum_timing.py [--shots 65536] [--reps 5] [--max-iter 50] --out FILE.json

Window fixture bb144_custom_r12_p0.003 (BB [[144,12,12]], 12 rounds, the whole history: 1008 x 9504), shots from the DEM sampler (seed 7),
decoded by BatchDecoder(raw_llr=True, osd_method="osd_off"): float LLRs as they are, which keeps the window out of the scatter kernel and
in the gather-form kernel, with no post-processor behind it.  Records the milliseconds of `--reps` decode calls after a warm-up (host clock
around a device synchronise), their median as shots/s, and a checksum of the outputs so that two libraries can be compared: run it once
per library (QUITS_AMD_LIB) in alternation and compare the medians with the spread between runs of the same library."""
import argparse
import json
import os
import statistics
import sys
import time
import zlib


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shots", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(here, "tests"), here):
        sys.path.insert(0, p)
    import torch
    import helpers
    from quits_amd import _lib
    from quits_amd.decoder.device import BatchDecoder, DemSampler, WindowGraph
    name = "bb144_custom_r12_p0.003"
    H, L, pri = helpers.dem_matrices(name)
    det, _ = DemSampler(H, L, pri).sample(args.shots, seed=7)
    wg = WindowGraph(H, pri)
    dec = BatchDecoder(wg, raw_llr=True, osd_method="osd_off", max_iter=args.max_iter)
    info = dec.info()
    assert info["llr_grid_bits"] == -1 and not info["scatter_kernel"] and not info["edge_kernel"], info
    bits, st = dec.decode(det)                                      # warm-up; its outputs are the run's
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        dec.decode(det)
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    st_h = st.cpu().numpy()
    res = {"device": torch.cuda.get_device_name(0), "library": _lib.LIB_PATH, "window": list(H.shape), "fixture": name, "shots": args.shots,
           "max_iter": args.max_iter, "ms": ms, "shots_per_s": round(args.shots / (statistics.median(ms) * 1e-3), 1),
           "mean_iterations": float((st_h & _lib.STATUS_ITER_MASK).mean()), "converged_share": float(((st_h & _lib.STATUS_CONVERGED) != 0).mean()),
           "crc32_err_bits": zlib.crc32(bits.cpu().numpy().tobytes()), "crc32_status": zlib.crc32(st_h.tobytes())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
