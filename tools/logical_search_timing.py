#!/usr/bin/env python3
"""Time the search for light undetectable logical faults level by level (quits_amd/search.py, csrc/logical_search.hip).

    python tools/logical_search_timing.py [--seconds 600] [--runs bb72_k6,bb144_k4,bb144_k6] --out profiles/logical_search_timing.json

Runs, each in one session on one search object with the default max_states (what half of the free device memory holds):
  bb72_k6     bb72_custom_r2_xbasis_mixed, K = D = 6
  bb144_k4    bb144_custom_r12_p0.003 (the headline circuit), K = D = 4
  bb144_k6    the same, K = D = 6
Each runs to `found`, to `capacity`, to `space`, or until the next level is expected not to fit into --seconds (the last level's time times
the last growth factor, added to the time spent): a level is queued whole and cannot be cut short, so the limit is applied between levels and
the run then ends as `time`.  Per level: states, candidates looked up in the visited set, seconds (host clock around the level's launches and
the device synchronise that reads its counters) and states / s.  Per run: the bytes the search allocated (its own statement and the drop of
the device's free memory across the allocation) and, as the only baseline at hand, the numpy mirror on the same model for the levels it
finishes inside --mirror-seconds (a level expected to end after that is not run).  Stim is not installed here: there is no reference timing."""
import argparse
import json
import os
import sys
import time

RUNS = {"bb72_k6": ("bb72_custom_r2_xbasis_mixed", 6, 6), "bb144_k4": ("bb144_custom_r12_p0.003", 4, 4), "bb144_k6": ("bb144_custom_r12_p0.003", 6, 6)}


def mirror_levels(ls, m, seconds):
    """Level sizes and seconds of the mirror, stopping before a level that is expected to end after `seconds` (the last level's time
    times the last growth factor)."""
    eng = ls._MirrorEngine(m, None)
    out, t0 = [], time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        if len(out) >= 2 and time.perf_counter() - t0 + out[-1]["seconds"] * out[-1]["states"] / max(1, out[-2]["states"]) > seconds:
            break
        t1 = time.perf_counter()
        new = eng.start() if not out else eng.step()
        out.append({"states": int(new), "seconds": round(time.perf_counter() - t1, 4)})
        if not new or eng.found():
            break
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--mirror-seconds", type=float, default=60.0)
    ap.add_argument("--runs", default="bb72_k6,bb144_k4,bb144_k6")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(here, "tests"), here):
        sys.path.insert(0, p)
    import torch
    import helpers
    from quits_amd import _lib
    from quits_amd import search as ls
    from quits_amd.dem import Circuit
    res = {"device": torch.cuda.get_device_name(0), "library_version": int(_lib.load().qd_version()),
           "method": "host clock around each level's launches and the synchronising read of its counters; one session per run",
           "seconds_limit": args.seconds, "mirror_seconds_limit": args.mirror_seconds, "runs": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in [r for r in args.runs.split(",") if r]:
        circuit, K, D = RUNS[name]
        H, L = ls._matrices(Circuit(helpers.circuit_text(circuit)))
        m = ls.prepare(H, L, K, D)
        free0 = torch.cuda.mem_get_info()[0]
        max_states = ls.default_max_states(free0)
        t0 = time.perf_counter()
        eng = ls.LogicalSearcher(m, max_states)
        torch.cuda.synchronize()
        run = {"circuit": circuit, "shape": list(H.shape), "max_event_set": K, "max_fault_degree": D, "max_states": max_states,
               "table_slots": eng.table_size, "chunk_states": eng.chunk_states, "longest_row": m.max_row, "bytes_stated": eng.bytes,
               "bytes_free_drop": int(free0 - torch.cuda.mem_get_info()[0]), "create_seconds": round(time.perf_counter() - t0, 4), "levels": []}
        outcome, spent = None, 0.0
        try:
            while outcome is None:
                lv = run["levels"]
                if len(lv) >= 2 and lv[-2]["states"]:
                    expect = lv[-1]["seconds"] * lv[-1]["states"] / lv[-2]["states"]
                    if spent + expect > args.seconds:
                        outcome = "time"
                        run["next_level_expected_seconds"] = round(expect, 2)
                        break
                t1 = time.perf_counter()
                new = eng.start() if not lv else eng.step()
                dt = time.perf_counter() - t1
                spent += dt
                if new is None:
                    outcome = "capacity"
                    run["overflowing_level_seconds"] = round(dt, 4)
                    break
                found = eng.found()
                if new == 0:
                    outcome = "space"
                    break
                lv.append({"level": len(lv) + 1, "states": int(new), "candidates": int(eng.candidates[-1]), "seconds": round(dt, 5),
                           "states_per_s": round(new / dt, 1), "candidates_per_s": round(eng.candidates[-1] / dt, 1)})
                print("%s: level %d, %d states, %.3f s" % (name, len(lv), new, dt), file=sys.stderr, flush=True)
                if found:
                    outcome = "found"
                    found.sort()
                    run["weight"], run["logical_masks"] = len(lv), len(found)
                    e = ls.witness_of(eng.chain(found[0][1]))
                    ls.check_witness(H, L, e, found[0][0], m.observables, len(lv), D)
                    run["witness"], run["witness_weight"] = [int(j) for j in e], len(e)
        finally:
            eng.close()
        run.update(outcome=outcome, levels_completed=len(run["levels"]), total_states=sum(x["states"] for x in run["levels"]), search_seconds=round(spent, 4))
        run["mirror"] = mirror_levels(ls, m, args.mirror_seconds)
        res["runs"][name] = run
        with open(args.out, "w") as fh:                               # after every run: a later run that is cut short loses nothing
            fh.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
