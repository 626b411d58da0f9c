#!/usr/bin/env python3
"""Time the random information-set estimate of the distance (quits_amd/distance.py, csrc/distance.hip).

    python tools/distance_timing.py [--seed 1] [--headline-seconds 120] [--model-seconds 60] [--rate-seconds 2] --out profiles/distance_timing.json

Models, each in one session on one estimator:
  the four golden codes (hx with lx), QLP [[1020,136]] in three selections of its 136 logicals (0-63, 64-127, 128-135),
  bb72_custom_r6_p0.003 and bb144_custom_r12_p0.003 (the headline circuit).
Per model: trials / s (host clock around each batch's launch and the device synchronise that reads its records; one warm-up trial first);
the lightest weight and the trial that first reached it after 2^10, 2^14 and 2^18 trials of --seed (a checkpoint that --model-seconds does
not reach is recorded as null); every run goes on in batches until --rate-seconds are spent, so that the rate is not that of a few
milliseconds, the headline circuit's until --headline-seconds are spent; the lightest witness is regenerated and checked on the host; and the numpy mirror's time for the first 8 trials of the same seed, whose records must equal the device's.
Nothing else exists to measure against."""
import argparse
import json
import os
import sys
import time

CHECKPOINTS = (1 << 10, 1 << 14, 1 << 18)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--headline-seconds", type=float, default=120.0)
    ap.add_argument("--model-seconds", type=float, default=60.0)
    ap.add_argument("--rate-seconds", type=float, default=2.0)
    ap.add_argument("--models", default="")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(here, "tests"), here):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import helpers
    from quits_amd import _lib
    from quits_amd import distance as qd
    from quits_amd.dem import Circuit
    from quits_amd.search import _matrices

    def code(name):
        cd = helpers.code(name)
        return cd["hx"], cd["lx"]

    models = [("bb72_code", lambda: code("bb72"), None), ("bb90_code", lambda: code("bb90"), None), ("bb144_code", lambda: code("bb144"), None),
              ("hgp225_code", lambda: code("hgp225"), None),
              ("qlp1020_code_obs0_63", lambda: code("qlp1020"), list(range(0, 64))), ("qlp1020_code_obs64_127", lambda: code("qlp1020"), list(range(64, 128))),
              ("qlp1020_code_obs128_135", lambda: code("qlp1020"), list(range(128, 136))),
              ("bb72_custom_r6_p0.003", lambda: _matrices(Circuit(helpers.circuit_text("bb72_custom_r6_p0.003"))), None),
              ("bb144_custom_r12_p0.003", lambda: _matrices(Circuit(helpers.circuit_text("bb144_custom_r12_p0.003"))), None)]
    only = [x for x in args.models.split(",") if x]
    res = {"device": torch.cuda.get_device_name(0), "library_version": int(_lib.load().qd_version()), "seed": args.seed,
           "method": "host clock around each batch's launch and the synchronising read of its records; one session per model, one warm-up trial",
           "model_seconds_limit": args.model_seconds, "rate_seconds": args.rate_seconds, "headline_seconds_limit": args.headline_seconds, "models": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name, make, obs in models:
        if only and name not in only:
            continue
        H, L = make()
        m = qd.prepare(H, L, obs)
        est = qd.DistanceEstimator(m)
        try:
            info = est.info()
            est.run(args.seed, 0, 1)
            est.reset()
            batch = max(1024, 8 * info["trials_in_flight"])
            run = {"shape": [m.ndet, m.n], "observables": len(m.observables), **{k: info[k] for k in ("lds_bytes", "threads", "workspace_bytes", "trials_in_flight", "columns_per_block")},
                   "batch": batch, "checkpoints": {}}
            headline = name == "bb144_custom_r12_p0.003"
            best, done, spent, first8 = None, 0, 0.0, None
            marks = list(CHECKPOINTS)
            limit = args.headline_seconds if headline else args.model_seconds
            floor = args.headline_seconds if headline else args.rate_seconds
            while marks or spent < floor:
                if marks and spent > limit:
                    for c in marks:
                        run["checkpoints"][str(c)] = None
                    marks = []
                    continue
                cnt = min(batch, marks[0] - done) if marks else batch
                t1 = time.perf_counter()
                rec = est.run(args.seed, done, cnt)
                spent += time.perf_counter() - t1
                if first8 is None:
                    first8 = rec[:8].copy()
                best = qd._lightest(rec, done, 1, best)
                done += cnt
                if marks and done == marks[0]:
                    run["checkpoints"][str(marks.pop(0))] = None if best is None else {"weight": best[0], "first_trial": best[1][0][0], "seconds": round(spent, 4)}
                    print("%s: %d trials, %.2f s, lightest %s" % (name, done, spent, best and best[0]), file=sys.stderr, flush=True)
            run.update(trials=done, seconds=round(spent, 4), trials_per_s=round(done / spent, 1), rank=est.info()["rank"],
                       weight=None if best is None else best[0], first_trial=None if best is None else best[1][0][0])
            hist = est.hist()
            run["hist"] = {str(w): int(c) for w, c in enumerate(hist) if c}
        finally:
            est.close()
        if best is not None:
            e, mask = qd.kernel_vector(m, None, args.seed, best[1][0][0], best[1][0][1])
            qd.check_vector(H, L, e, mask, m.observables)
            assert len(e) == best[0]
            run["witness"], run["witness_mask"] = [int(j) for j in e], int(mask)
        t1 = time.perf_counter()
        ref, _ = qd.distance_mirror(m, None, 8, seed=args.seed)
        run["mirror_seconds_8_trials"] = round(time.perf_counter() - t1, 4)
        run["mirror_equals_device_8_trials"] = bool(np.array_equal(ref, first8))
        run["speedup_over_mirror"] = round(run["trials_per_s"] * run["mirror_seconds_8_trials"] / 8, 1)
        res["models"][name] = run
        print("%s: %d trials in %.2f s (%.0f / s), weight %s at trial %s" % (name, done, spent, done / spent, run["weight"], run["first_trial"]),
              file=sys.stderr, flush=True)
        with open(args.out, "w") as fh:                               # after every model: a later one that is cut short loses nothing
            fh.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
