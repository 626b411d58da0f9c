#!/usr/bin/env python3
"""Time the device-resident memory experiment (quits_amd.simulation.get_circuit_mem_pL) and its bookkeeping kernels.

    python tools/mem_experiment_timing.py [--shots 4194304] [--big-shots 67108864] [--out profiles/mem_experiment_timing.json]

Circuit bb144_custom_r12, the whole history as one window, minimum_sum / parallel / max_iter = 50 / osd_0 (the headline configuration).
  tally     qd_shot_flags_fold + qd_tally_batch (flags and fail mask on) over 2^20 decoded headline shots, k = 12, and qd_tally_batch
            over 65 536 random rows of k = 136; device events, median of 5 calls after a warm-up, next to CircuitSampler.sample of the
            same 2^20 shots in the same run and to the bytes the kernels have to read at least.
  end_to_end  get_circuit_mem_pL on `--shots` shots at p = 3e-3 against the sum of its parts measured in the same process: plan.decode
            alone on resident samples (three calls: their spread is the yardstick), the sampler alone, fold + tally alone.
  big_point   one p = 1e-3 point of `--big-shots` shots, max_errors unset: shots/s, LER +- sigma, peak host RSS.
Prints one JSON line; --out writes it to a file as well."""
import argparse
import json
import os
import resource
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import helpers  # noqa: E402

NAME = "bb144_custom_r12_p0.003"
KW = dict(max_iter=50, osd_order=0, bp_method="minimum_sum", schedule="parallel", osd_method="osd_0")
W, F = 14, 1                                                         # R + 2 rounds of detectors: one window


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


def tally_cost(plan, sampler, B=1 << 20):
    import torch
    from quits_amd.decoder.device import Tally, shot_flags_fold
    det, obs = sampler.sample(B, 7)
    stats = []
    pred = plan.decode(det, stats)
    status = torch.cat([st for _, st in stats])
    flags = torch.zeros((B,), dtype=torch.uint8, device="cuda")
    mask = torch.zeros((B // 64,), dtype=torch.int64, device="cuda")
    k = pred.shape[1]
    t = Tally(k)

    def fold_and_tally():
        shot_flags_fold(status, flags)
        t.add(pred, obs, flags, mask)
    row = dict(shots=B, k=k, fold_plus_tally=timed(fold_and_tally), tally_alone=timed(lambda: t.add(pred, obs, flags, mask)),
               sampler=timed(lambda: sampler.sample(B, 7)), min_bytes=2 * k * B + B + 4 * B)
    row["fold_plus_tally_over_sampler"] = round(row["fold_plus_tally"]["median_ms"] / row["sampler"]["median_ms"], 5)
    row["fold_plus_tally_GBps"] = round(row["min_bytes"] / row["fold_plus_tally"]["median_ms"] / 1e6, 1)
    del det, pred, obs
    Bw, kw = 1 << 16, 136
    g = torch.Generator(device="cuda").manual_seed(1)
    p = torch.randint(0, 2, (Bw, kw), dtype=torch.uint8, device="cuda", generator=g)
    o = p ^ (torch.rand((Bw, kw), device="cuda", generator=g) < 0.01).to(torch.uint8)
    fw = torch.zeros((Bw,), dtype=torch.uint8, device="cuda")
    mw = torch.zeros((Bw // 64,), dtype=torch.int64, device="cuda")
    tw = Tally(kw)
    wide = dict(shots=Bw, k=kw, tally_alone=timed(lambda: tw.add(p, o, fw, mw)), min_bytes=2 * kw * Bw + Bw)
    wide["GBps"] = round(wide["min_bytes"] / wide["tally_alone"]["median_ms"] / 1e6, 1)
    return dict(k12=row, k136=wide)


def end_to_end(text, cd, plan, sampler, N):
    import torch
    from quits_amd.decoder.device import Tally, shot_flags_fold
    from quits_amd.simulation import get_circuit_mem_pL
    get_circuit_mem_pL(text, cd["hz"], cd["lz"], W, F, 1 << 18, **KW, seed=3)          # warm-up: workspaces, lane decoders, streams
    runs = [get_circuit_mem_pL(text, cd["hz"], cd["lz"], W, F, N, **KW, seed=5) for _ in range(2)]
    batch = runs[0].batch

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def sample_all():
        for s0 in range(0, N, batch):
            sampler.sample(min(batch, N - s0), 5, s0)
    t_sample = wall(sample_all)
    pieces = [sampler.sample(min(batch, N - s0), 5, s0) for s0 in range(0, N, batch)]
    kept = []

    def decode_all():
        kept.clear()
        for det, _ in pieces:
            stats = []
            kept.append((plan.decode(det, stats), stats))
    t_decode = [wall(decode_all) for _ in range(3)]
    t = Tally(plan.nobs)

    def tally_all():
        for (det, obs), (pred, stats) in zip(pieces, kept):
            flags = torch.zeros((det.shape[0],), dtype=torch.uint8, device="cuda")
            at = 0
            for _, st in stats:
                shot_flags_fold(st, flags[at:at + st.shape[0]])
                at += st.shape[0]
            t.add(pred, obs, flags)
    t_tally = wall(tally_all)
    assert int(t.counts()[1]) == runs[0].errors == runs[1].errors
    parts = float(np.median(t_decode)) + t_sample + t_tally
    best = min(r.seconds for r in runs)
    return dict(shots=N, batch=batch, chunk=plan.chunk, errors=runs[0].errors, pL=runs[0].pL, sigma=runs[0].sigma,
                experiment_seconds=[round(r.seconds, 4) for r in runs], experiment_shots_per_s=round(N / best),
                decode_alone_seconds=[round(x, 4) for x in t_decode], sampler_alone_seconds=round(t_sample, 4), tally_alone_seconds=round(t_tally, 4),
                sum_of_parts_seconds=round(parts, 4), experiment_over_sum_of_parts=round(best / parts, 4),
                decode_alone_spread=round((max(t_decode) - min(t_decode)) / float(np.median(t_decode)), 4))


def big_point(cd, N):
    from quits_amd.simulation import get_circuit_mem_pL
    text = helpers.circuit_text_at_p(NAME, 0.003, 0.001)
    get_circuit_mem_pL(text, cd["hz"], cd["lz"], W, F, 1 << 18, **KW, seed=3)          # plan, workspaces
    r = get_circuit_mem_pL(text, cd["hz"], cd["lz"], W, F, N, **KW, seed=2026)
    return dict(p=0.001, shots=r.shots, errors=r.errors, pL=r.pL, sigma=r.sigma, seconds=round(r.seconds, 3), shots_per_s=round(r.shots_per_s),
                per_observable_errors=r.per_observable_errors.tolist(), flagged=r.flagged, failing_shots_kept=int(r.failing_shots.shape[0]),
                failures_truncated=r.failures_truncated, peak_host_rss_MB=round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=1 << 22)
    ap.add_argument("--big-shots", type=int, default=1 << 26, help="0 skips the p = 1e-3 point")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from quits_amd.decoder.bposd import BpOsdDecoder
    from quits_amd.decoder.device import CircuitSampler
    from quits_amd.decoder.plan import cached_circuit_plan
    from quits_amd.dem import Circuit
    text = helpers.circuit_text(NAME)
    cd = helpers.code("bb144")
    circ = Circuit(text)
    opts = {k: KW[k] for k in ("bp_method", "max_iter", "schedule", "osd_method", "osd_order")}
    plan = cached_circuit_plan(circ, cd["hz"], W, F, 12, BpOsdDecoder, BpOsdDecoder, opts, opts)
    assert len(plan.windows) == 1
    sampler = CircuitSampler(text)
    row = dict(circuit=NAME, decoder=KW, device=torch.cuda.get_device_name(0))
    row["tally"] = tally_cost(plan, sampler)
    row["end_to_end"] = end_to_end(text, cd, plan, sampler, a.shots)
    if a.big_shots:
        row["big_point"] = big_point(cd, a.big_shots)
    line = json.dumps(row)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
