#!/usr/bin/env python3
"""Run every experiment driver of quits_amd.simulation once and print what it returned, one JSON line per call, so that two trees can be
compared byte for byte.

    python tools/experiment_identity.py [--root DIR] [--lib FILE] > FILE

--root: the tree whose `quits_amd` is imported (default: this one); --lib: the built library both trees load (QUITS_AMD_LIB).  The fixtures
come from this tree's tests/.  Circuit bb72_custom_r6_p0.003, W = 3, F = 1, minimum_sum / parallel / max_iter = 20 / osd_0, seed 11.
A line holds every field of the result except seconds, shots_per_s and timing; an array is written as the SHA-256 of its bytes with its
shape and dtype."""
import argparse
import dataclasses
import hashlib
import json
import os
import sys

NAME = "bb72_custom_r6_p0.003"
W, F, SEED = 3, 1, 11
MINSUM = dict(bp_method="minimum_sum", schedule="parallel", max_iter=20, osd_method="osd_0", osd_order=0)
SKIP = ("seconds", "shots_per_s", "timing")


def plain(x):
    import numpy as np
    if dataclasses.is_dataclass(x):
        return {f.name: plain(getattr(x, f.name)) for f in dataclasses.fields(x) if f.name not in SKIP}
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "shape": list(a.shape), "dtype": str(a.dtype)}
    if isinstance(x, dict):
        return {str(k): plain(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [plain(v) for v in x]
    if isinstance(x, np.generic):
        return x.item()
    return x


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--root", default=here)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    if a.lib:
        os.environ["QUITS_AMD_LIB"] = os.path.abspath(a.lib)
    for p in (os.path.join(here, "tests"), root):                    # fixtures from this tree, the package from --root
        sys.path.insert(0, p)
    import numpy as np
    import helpers
    import quits_amd
    from quits_amd import shrink as sk
    from quits_amd import simulation as sim
    from quits_amd.relay import RelayConfig
    assert os.path.abspath(quits_amd.__file__).startswith(root + os.sep), quits_amd.__file__
    text = helpers.circuit_text(NAME)
    cd = helpers.code("bb72")
    base = (text, cd["hz"], cd["lz"], W, F)
    cfg = RelayConfig(pre_iter=20, num_sets=3, set_max_iter=20)

    def show(call, result):
        print(json.dumps({"call": call, "result": plain(result)}, sort_keys=True), flush=True)

    for sampler in ("circuit", "dem"):
        for extra in ({"batch": 192}, {}, {"max_errors": 8}, {"batch": 192, "max_errors": 8}, {"shard": (1, 3)}):
            show("get_circuit_mem_pL %s %s" % (sampler, sorted(extra.items())),
                 sim.get_circuit_mem_pL(*base, 4096, **MINSUM, seed=SEED, sampler=sampler, **extra))
    show("get_relay_mem_pL", sim.get_relay_mem_pL(*base, 512, relay=cfg, seed=SEED))
    for sampler in ("circuit", "dem"):
        show("get_postselected_pL %s" % sampler, sim.get_postselected_pL(*base, 4096, **MINSUM, seed=SEED, sampler=sampler))
    for extra in ({"batch": 192}, {}):
        show("get_fault_spectrum %s" % sorted(extra.items()), sim.get_fault_spectrum(*base, 4096, **MINSUM, seed=SEED, **extra))
    show("get_stratified_pL", sim.get_stratified_pL(*base, {0: 64, 14: 1024}, **MINSUM, seed=SEED))
    mf = sim.get_minimal_failures(*base, 4096, **MINSUM, seed=SEED)
    show("get_minimal_failures", mf)
    show("get_minimal_failures strata", sim.get_minimal_failures(*base, 0, **MINSUM, seed=SEED, shots_per_weight={14: 1024}))
    show("get_relay_minimal_failures", sim.get_relay_minimal_failures(*base, 512, relay=cfg, osd_method="osd_off", seed=SEED))
    shots = mf.parent_shots[:16]
    show("replay_shots circuit", sim.replay_shots(text, shots, SEED))
    show("replay_shots dem", sim.replay_shots(text, shots, SEED, "dem"))
    parents = sim.replay_faults(text, shots, SEED)
    show("replay_faults", parents)
    show("replay_strata_faults", sim.replay_strata_faults(text, 14, np.arange(16), SEED))
    show("shrink_fault_sets bool", sim.shrink_fault_sets(*base, parents, **MINSUM))
    show("shrink_fault_sets packed", sim.shrink_fault_sets(*base, sk.pack_sets(parents), **MINSUM))


if __name__ == "__main__":
    main()
