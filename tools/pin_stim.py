#!/usr/bin/env python3
"""Pins quits_amd/dem.py (the detector error model restated from memory) and the samplers against Stim ITSELF, the day Stim is at hand.

Stim is an external C++ wheel that is not installed where this repository is built and tested (profiles/r02_probe_ldpc_stim.txt), so
nothing Stim-made has ever been compared with this package's extractor (VERDICT.md coverage row a5).  This script is
the route in, as tools/pin_ldpc.py is for `ldpc`: where `import stim` works -- any laptop -- it writes, for every circuit of
tests/golden/circuits/index.json,

  tests/golden/stim_pin/<name>.dem      Stim's own `circuit.detector_error_model(decompose_errors=False)`, printed (gzipped to
                                        <name>.dem.gz where the text exceeds 1 MiB, the limit for a committed file)

and for bb72_custom_r6_p0.003 and hgp225_cardinal_r3_p0.01 also

  tests/golden/stim_pin/<name>.b8       4096 shots of Stim's detector sampler, seed 1, format b8, observables appended after the detectors.

The files are data and travel; tests/test_stim_pin.py picks them up when present (quits_amd.dem.parse_dem and quits_amd.samples.read_shots
read them) and runs the same comparison on a stand-in of its own while they are absent.

Without Stim: prints one line and exits 0.  Nothing is ever fetched."""
import argparse
import gzip
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SAMPLED = ("bb72_custom_r6_p0.003", "hgp225_cardinal_r3_p0.01")
SHOTS, SEED = 4096, 1
LIMIT = 1 << 20


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "stim_pin"))
    args = ap.parse_args()
    try:
        import stim
    except ImportError as exc:
        print("stim not importable (%s): nothing to pin; quits_amd/dem.py stays unpinned against Stim" % exc)
        return 0
    import helpers
    os.makedirs(args.out, exist_ok=True)
    for name in sorted(helpers.circuit_index()):
        circuit = stim.Circuit(helpers.circuit_text(name))
        text = str(circuit.detector_error_model(decompose_errors=False)) + "\n"
        path = os.path.join(args.out, name + ".dem")
        if len(text.encode()) > LIMIT:
            path += ".gz"
            with gzip.open(path, "wb", compresslevel=9, mtime=0) as fh:
                fh.write(text.encode())
        else:
            with open(path, "w", newline="\n") as fh:
                fh.write(text)
        print("%-40s %8d detectors %3d observables -> %s" % (name, circuit.num_detectors, circuit.num_observables, os.path.relpath(path, ROOT)))
        if name in SAMPLED:
            rec = circuit.compile_detector_sampler(seed=SEED).sample(shots=SHOTS, append_observables=True, bit_packed=True)
            path = os.path.join(args.out, name + ".b8")
            rec.tofile(path)
            print("%-40s %8d shots of %d bytes (stim %s, seed %d) -> %s" % (name, rec.shape[0], rec.shape[1], stim.__version__, SEED, os.path.relpath(path, ROOT)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
