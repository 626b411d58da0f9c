"""`python -m quits_amd predict`: decode a file of detector samples against a detector error model, as the `predict` commands Stim users
know do (sinter / pymatching: --dem, --in, --in_format, --out, --out_format).

    python -m quits_amd predict --dem model.dem --in shots.b8 --in_format b8 --out predictions.01 --out_format 01

Without --checks_per_round / --window / --commit the model is decoded over its whole history (quits_amd.decoder.decode_dem); with all three
by the sliding-window decoder (quits_amd.decoder.sliding_window_bposd_circuit_mem), the detectors being rounds of --checks_per_round.
--corrections_out FILE (--corrections_format b8 | 01 | hits, default b8) also writes every shot's correction, one bit per fault of the model
in the column order of detector_error_model_to_matrix (quits_amd.decoder.sliding_window_corrections / decode_dem_corrections).
--soft_out FILE also writes every shot's soft record (quits_amd/soft.py: weight faults events iters post tail), six decimal integers on one
line per shot (quits_amd.decoder.sliding_window_soft_outputs / decode_dem_soft_outputs).
Exit status: 0 done, 1 unreadable input, 2 bad arguments, or no GPU / no library (the decoder has no CPU fallback).

`python -m quits_amd search`: the directed search for light undetectable logical faults (quits_amd/search.py states it) on the device; one
JSON object on stdout: outcome, weight, levels_completed, level_sizes, total_states, logical_masks, witnesses and the limits used.

    python -m quits_amd search --circuit memory.stim --max_event_set 4 --max_fault_degree 4

--mirror runs the numpy mirror of the kernels on the CPU instead (small models only); nothing else falls back to it.

`python -m quits_amd distance`: the random information-set estimate of the distance (quits_amd/distance.py states it) on the device; one
JSON object on stdout: weight (an upper bound), witnesses, masks, trials, first_trial, hist, rank, seed, observables, seconds.

    python -m quits_amd distance --circuit memory.stim --trials 65536 --target 6

--mirror as above.

`python -m quits_amd calibrate`: fit the priors of a model's hyperedges to a file of detector samples (quits_amd/calibrate.py states the fit);
the counting runs on the device.  --out receives the model with the fitted priors as .dem text, which every command here takes as --dem;
--stderr_out one line per column: prior, jackknife standard error, flag (ok, clipped or unidentified).  One JSON object on stdout: shots,
columns, clipped, unidentified, median_rel_stderr and max_rel_stderr (stderr / prior), seconds.

    python -m quits_amd calibrate --circuit memory.stim --in shots.b8 --in_format b8 --out fitted.dem

--mirror as above.  Exit statuses as `predict`.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np


def _parser():
    from .samples import FORMATS
    ap = argparse.ArgumentParser(prog="python -m quits_amd", description="MI355X sliding-window BP-OSD decoder: command line.")
    sub = ap.add_subparsers(dest="command", required=True)
    p = sub.add_parser("predict", help="predict observable flips from detector samples",
                       description="Predict the observable flips of every shot of a detector sample file.")
    model = p.add_mutually_exclusive_group(required=True)
    model.add_argument("--dem", metavar="FILE", help="detector error model, Stim's .dem text")
    model.add_argument("--circuit", metavar="FILE", help="Stim circuit text (its detector error model is extracted here)")
    p.add_argument("--in", dest="inp", metavar="FILE", required=True, help="detector samples")
    p.add_argument("--in_format", choices=FORMATS, required=True)
    p.add_argument("--in_includes_appended_observables", action="store_true",
                   help="every shot of --in holds the observables after the detectors (stim sample/detect --append_observables)")
    p.add_argument("--out", metavar="FILE", required=True, help="predicted observable flips, one shot per record")
    p.add_argument("--out_format", choices=FORMATS, required=True)
    p.add_argument("--obs_in", metavar="FILE", help="actual observable flips: prints one JSON line {\"shots\": .., \"errors\": ..}")
    p.add_argument("--obs_in_format", choices=FORMATS, help="default: --in_format")
    p.add_argument("--bp_method", default="product_sum")
    p.add_argument("--schedule", default="serial")
    p.add_argument("--max_iter", type=int, default=2)
    p.add_argument("--osd_method", default="osd_cs")
    p.add_argument("--osd_order", type=int, default=0)
    p.add_argument("--checks_per_round", type=int, metavar="NZ", help="detectors per round (sliding window; with --window and --commit)")
    p.add_argument("--window", type=int, metavar="W", help="rounds per window")
    p.add_argument("--commit", type=int, metavar="F", help="rounds committed per window")
    p.add_argument("--corrections_out", metavar="FILE",
                   help="also write every shot's correction, one bit per fault of the model (the columns of detector_error_model_to_matrix)")
    p.add_argument("--corrections_format", choices=("b8", "01", "hits"), default="b8")
    p.add_argument("--soft_out", metavar="FILE",
                   help="also write every shot's soft record: weight faults events iters post tail, six decimal integers per line (quits_amd/soft.py)")
    q = sub.add_parser("search", help="search for light undetectable logical faults",
                       description="Breadth-first search over small detection-event sets for an undetectable logical fault (quits_amd/search.py).")
    model = q.add_mutually_exclusive_group(required=True)
    model.add_argument("--dem", metavar="FILE", help="detector error model, Stim's .dem text")
    model.add_argument("--circuit", metavar="FILE", help="Stim circuit text (its detector error model is extracted here)")
    q.add_argument("--max_event_set", type=int, default=6, metavar="K", help="detectors a state may hold (1 .. 8)")
    q.add_argument("--max_fault_degree", type=int, default=6, metavar="D", help="detectors an admitted fault may flip (1 .. 16)")
    q.add_argument("--no_increase", action="store_true", help="do not follow faults that enlarge the detection-event set")
    q.add_argument("--max_weight", type=int, help="stop after this many levels")
    q.add_argument("--max_states", type=int, help="distinct states the search may hold (default: what half of the free device memory holds)")
    q.add_argument("--keep", type=int, default=16, help="witnesses to return")
    q.add_argument("--observables", metavar="I,J,..", help="rows of the observable matrix to search (at most 64; default: all)")
    q.add_argument("--mirror", action="store_true", help="run the numpy mirror on the CPU instead of the device")
    d = sub.add_parser("distance", help="estimate the distance from random information sets",
                       description="Random column orders of the check matrix, one elimination each; the lightest kernel vector that flips an "
                                   "observable is an upper bound on the distance (quits_amd/distance.py).")
    model = d.add_mutually_exclusive_group(required=True)
    model.add_argument("--dem", metavar="FILE", help="detector error model, Stim's .dem text")
    model.add_argument("--circuit", metavar="FILE", help="Stim circuit text (its detector error model is extracted here)")
    d.add_argument("--trials", type=int, default=1 << 16, help="trials to run (default 65536)")
    d.add_argument("--seed", type=int, default=0)
    d.add_argument("--target", type=int, metavar="W", help="stop after the first batch that reaches this weight")
    d.add_argument("--max_seconds", type=float, metavar="T", help="stop after the first batch that ends past this time")
    d.add_argument("--keep", type=int, default=16, help="witnesses to return")
    d.add_argument("--observables", metavar="I,J,..", help="rows of the observable matrix to watch (at most 64; default: all)")
    d.add_argument("--mirror", action="store_true", help="run the numpy mirror on the CPU instead of the device")
    c = sub.add_parser("calibrate", help="fit a model's priors to detector samples",
                       description="Fit the prior of every hyperedge of a detector error model to detector samples, with jackknife standard "
                                   "errors (quits_amd/calibrate.py).")
    model = c.add_mutually_exclusive_group(required=True)
    model.add_argument("--dem", metavar="FILE", help="detector error model, Stim's .dem text")
    model.add_argument("--circuit", metavar="FILE", help="Stim circuit text (its detector error model is extracted here)")
    c.add_argument("--in", dest="inp", metavar="FILE", required=True, help="detector samples")
    c.add_argument("--in_format", choices=FORMATS, required=True)
    c.add_argument("--in_includes_appended_observables", action="store_true",
                   help="every shot of --in holds the observables after the detectors (they are not read)")
    c.add_argument("--out", metavar="FILE", required=True, help="the model with the fitted priors, .dem text")
    c.add_argument("--blocks", type=int, default=16, help="jackknife blocks (default 16)")
    c.add_argument("--stderr_out", metavar="FILE", help="one line per column: prior stderr flag")
    c.add_argument("--mirror", action="store_true", help="count with the numpy mirror on the CPU instead of the device")
    return ap


def calibrate(args, ap) -> int:
    from .dem import Circuit, as_dem
    from . import calibrate as qc
    from .samples import read_shots
    if args.blocks < 1:
        ap.error("--blocks must be positive")
    with open(args.dem or args.circuit, "r") as fh:
        text = fh.read()
    model = text if args.dem else Circuit(text)
    dem = as_dem(model)
    ndet, nobs = dem.num_detectors, dem.num_observables
    rec = read_shots(args.inp, args.in_format, ndet, nobs if args.in_includes_appended_observables else 0)
    det = rec.field(0, ndet)
    if args.mirror:
        res = qc.estimate_priors_mirror(model, det, blocks=args.blocks)
    else:
        res = qc.estimate_priors(model, det, blocks=args.blocks)
    with open(args.out, "w") as fh:
        fh.write(res.dem_text())
    if args.stderr_out:
        flag = np.zeros(len(res.priors), np.int64)
        flag[res.clipped], flag[res.unidentified] = 1, 2
        with open(args.stderr_out, "w") as fh:
            fh.writelines("%.17g %.17g %s\n" % (p, e, ("ok", "clipped", "unidentified")[f]) for p, e, f in zip(res.priors, res.stderr, flag))
    print(json.dumps(res.to_json()))
    return 0


def distance(args, ap) -> int:
    from .dem import Circuit
    from . import distance as qd
    with open(args.dem or args.circuit, "r") as fh:
        text = fh.read()
    model = text if args.dem else Circuit(text)
    obs = None if args.observables is None else [int(x) for x in args.observables.split(",") if x.strip()]
    if args.mirror:
        res = qd.estimate_distance_mirror(model, trials=args.trials, seed=args.seed, keep=args.keep, observables=obs)
    else:
        res = qd.estimate_distance(model, trials=args.trials, seed=args.seed, target=args.target, max_seconds=args.max_seconds, keep=args.keep,
                                   observables=obs)
    print(json.dumps(res.to_json()))
    return 0


def search(args, ap) -> int:
    from .dem import Circuit
    from . import search as ls
    with open(args.dem or args.circuit, "r") as fh:
        text = fh.read()
    model = text if args.dem else Circuit(text)
    obs = None if args.observables is None else [int(x) for x in args.observables.split(",") if x.strip()]
    opts = dict(max_event_set=args.max_event_set, max_fault_degree=args.max_fault_degree, no_increase=args.no_increase, max_weight=args.max_weight,
                max_states=args.max_states, keep=args.keep, observables=obs)
    if args.mirror:
        res = ls.search_mirror(*ls._matrices(model), **opts)
    else:
        res = ls.find_undetectable_logical_errors(model, **opts)
    print(json.dumps(res.to_json()))
    return 0


def predict(args, ap) -> int:
    from . import _lib
    from .dem import Circuit, as_dem
    from .samples import read_shots, write_shots
    sliding = [args.checks_per_round, args.window, args.commit]
    if any(v is not None for v in sliding) and not all(v is not None for v in sliding):
        ap.error("--checks_per_round, --window and --commit go together")
    if all(v is not None for v in sliding) and min(sliding) < 1:
        ap.error("--checks_per_round, --window and --commit must be positive")
    with open(args.dem or args.circuit, "r") as fh:
        text = fh.read()
    model = text if args.dem else Circuit(text)
    dem = as_dem(model)
    ndet, nobs = dem.num_detectors, dem.num_observables
    rec = read_shots(args.inp, args.in_format, ndet, nobs if args.in_includes_appended_observables else 0)
    det = rec.field(0, ndet)
    actual = rec.field(ndet, nobs) if args.in_includes_appended_observables else None
    if args.obs_in:
        actual = read_shots(args.obs_in, args.obs_in_format or args.in_format, nobs)
        if len(actual) != len(det):
            raise ValueError("%s holds %d shots, %s holds %d" % (args.obs_in, len(actual), args.inp, len(det)))
    _lib.require_gpu()
    opts = dict(max_iter=args.max_iter, osd_order=args.osd_order, bp_method=args.bp_method, schedule=args.schedule, osd_method=args.osd_method)
    if args.window is not None:
        import warnings
        from .decoder import sliding_window_bposd_circuit_mem, sliding_window_corrections, sliding_window_soft_outputs
        nz = args.checks_per_round
        if ndet % nz:
            raise ValueError("the model's %d detectors are not whole rounds of %d" % (ndet, nz))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")           # (whole-history notice of the reference: not an error here)
            decode = sliding_window_corrections if args.corrections_out else sliding_window_bposd_circuit_mem
            if args.soft_out:
                opts["corrections"] = bool(args.corrections_out)
                decode = sliding_window_soft_outputs
            pred = decode(det, model, np.zeros((nz, 1), np.uint8), np.zeros((nobs, 1), np.uint8), args.window, args.commit, **opts)
    elif args.soft_out:
        from .decoder import decode_dem_soft_outputs
        pred = decode_dem_soft_outputs(model, det, corrections=bool(args.corrections_out), **opts)
    else:
        from .decoder import decode_dem, decode_dem_corrections
        pred = (decode_dem_corrections if args.corrections_out else decode_dem)(model, det, **opts)
    soft = None
    if args.soft_out:
        pred, soft, corrections = pred if args.corrections_out else (pred + (None,))
    elif args.corrections_out:
        pred, corrections = pred
    if args.corrections_out:
        write_shots(args.corrections_out, corrections, args.corrections_format)
    if soft is not None:
        with open(args.soft_out, "w") as fh:
            fh.writelines("%d %d %d %d %d %d\n" % tuple(int(v) for v in row) for row in soft)
    write_shots(args.out, pred.astype(np.uint8), args.out_format, num_detectors=0)
    if actual is not None:
        import torch
        from .decoder.device import Tally
        tally = Tally(nobs)
        if len(det):
            from .decoder.pipeline import _to_device_samples
            tally.add(torch.from_numpy(pred.astype(np.uint8)).to("cuda"), _to_device_samples(actual))
        counts = tally.counts()
        print(json.dumps({"shots": int(counts[0]), "errors": int(counts[1])}))
    return 0


def main(argv=None) -> int:
    ap = _parser()
    args = ap.parse_args(argv)
    try:
        return {"search": search, "distance": distance, "calibrate": calibrate}.get(args.command, predict)(args, ap)
    except RuntimeError as exc:                      # no GPU, no library, a library error: the package's own text
        print(str(exc), file=sys.stderr)
        return 2
    except (ValueError, OSError, NotImplementedError) as exc:
        print("quits_amd %s: %s" % (args.command, exc), file=sys.stderr)
        return 1


if __name__ == "__main__":
    sys.exit(main())
