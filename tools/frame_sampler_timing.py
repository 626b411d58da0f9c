#!/usr/bin/env python3
"""Time the circuit-level frame sampler against the DEM sampler and the headline decode on the same shots.

    python tools/frame_sampler_timing.py [--shots 1048576] [--reps 5] [--out profiles/frame_sampler_timing.json]
    python tools/frame_sampler_timing.py --channels [--parent-lib OLD/libquits_amd.so [--rounds 4]] [--out profiles/frame_sampler_channels_timing.json]

Circuit bb144_custom_r12_p0.003.  After one warm-up of each, device events time `reps` calls of CircuitSampler.sample and
DemSampler.sample (2^20 shots each) and one headline decode (minimum_sum, parallel, max_iter=50, OSD-0, the whole history as one
window) of the circuit-sampled shots; the median call is reported.  Prints one JSON line.

--channels times the biased-noise path instead: the same circuit with every DEPOLARIZE1(p) rewritten as PAULI_CHANNEL_1(p/3, p/3, p/3)
and every DEPOLARIZE2(p) as the uniform 15-entry PAULI_CHANNEL_2 -- the same distribution through the threshold tables -- next to the
unchanged text, `shots` shots each, median and min - max of `reps` calls after a warm-up.  With --parent-lib the unchanged text is timed
with that library too (an older build of libquits_amd.so, which need not know the channel opcodes): --rounds rounds, in each the parent
library and then this one, `reps` calls each, a library's calls pooled over the rounds.  Every measurement runs in a child process of its
own (QUITS_AMD_LIB names the library), one after the other; this process does not touch the GPU."""
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


def _stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), all_ms=[round(x, 3) for x in ms])


def sampler_only(a):
    """Child of --channels: time CircuitSampler.sample on the unchanged text and, if this library knows the channel opcodes, on the
    rewritten one.  Prints one JSON line."""
    import torch
    import channel_circuits
    from quits_amd import _lib
    from quits_amd.decoder.device import CircuitSampler
    name = "bb144_custom_r12_p0.003"
    text = helpers.circuit_text(name)
    version = int(_lib.load().qd_version())
    row = dict(library=os.path.basename(_lib.LIB_PATH), library_version=version, device=torch.cuda.get_device_name(0))
    texts = [("depolarize", text)] + ([("pauli_channel", channel_circuits.uniform(text))] if version >= 106 else [])
    for key, t in texts:
        cs = CircuitSampler(t)
        cs.sample(a.shots, seed=1)                                 # warm-up
        _, _, ms = timed(lambda: cs.sample(a.shots, seed=7), a.reps)
        row[key] = dict(_stats(ms), info=cs.info())
    torch.cuda.synchronize()
    print(json.dumps(row), flush=True)


def channels(a):
    import subprocess

    def child(lib):
        env = dict(os.environ)
        if lib:
            env["QUITS_AMD_LIB"] = os.path.abspath(lib)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--sampler-only", "--shots", str(a.shots), "--reps", str(a.reps)],
                             env=env, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            raise RuntimeError("timing child failed (%d): %s" % (out.returncode, out.stderr[-2000:]))
        return json.loads(out.stdout.strip().splitlines()[-1])
    row = dict(circuit="bb144_custom_r12_p0.003", shots=a.shots, reps=a.reps,
               rewrite="DEPOLARIZE1(p) -> PAULI_CHANNEL_1(p/3 x 3), DEPOLARIZE2(p) -> PAULI_CHANNEL_2(p/15 x 15)")
    if a.parent_lib:
        # A B A B ...: one child per library and round, the two libraries alternating, so that drift over the session falls on both alike;
        # a library's calls of all rounds are pooled
        runs = {"parent_library": [], "this_library": []}
        for _ in range(max(1, a.rounds)):
            runs["parent_library"].append(child(a.parent_lib))
            runs["this_library"].append(child(None))
        for side, lst in runs.items():
            row[side] = dict(lst[0])
            for key in ("depolarize", "pauli_channel"):
                if key in lst[0]:
                    row[side][key] = dict(_stats([x for r in lst for x in r[key]["all_ms"]]), info=lst[0][key]["info"],
                                          round_medians_ms=[r[key]["median_ms"] for r in lst])
        row["order"] = "alternating, parent library first, %d rounds of %d calls per library" % (max(1, a.rounds), a.reps)
    else:
        row["this_library"] = child(None)
    new = row["this_library"]
    row["pauli_channel_over_depolarize"] = round(new["pauli_channel"]["median_ms"] / new["depolarize"]["median_ms"], 4)
    if a.parent_lib:
        old = row["parent_library"]["depolarize"]
        row["depolarize_over_parent"] = round(new["depolarize"]["median_ms"] / old["median_ms"], 4)
        row["depolarize_within_parent_range"] = bool(old["min_ms"] <= new["depolarize"]["median_ms"] <= old["max_ms"])
    line = json.dumps(row)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--channels", action="store_true", help="time the PAULI_CHANNEL_1/2 rewrite next to the unchanged circuit")
    ap.add_argument("--parent-lib", default=None, help="with --channels: an older libquits_amd.so to time the unchanged circuit with")
    ap.add_argument("--rounds", type=int, default=4, help="with --parent-lib: rounds of (parent library, this library), alternating")
    ap.add_argument("--sampler-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.sampler_only:
        return sampler_only(a)
    if a.channels:
        return channels(a)
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
