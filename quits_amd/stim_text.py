"""Parser for the Stim circuit dialect that QUITS emits.

The reference builds its circuits as *text* (`/root/reference/src/quits/circuit.py:30-279`) and
only wraps the text in `stim.Circuit` at the very end (`qldpc_code/bb.py:301`,
`circuit_construction/cardinal.py:267`, `zxcoloration.py:270`).  Stim is not installed in the
build image, so the decoder front end reads the same text itself.

Ops understood: R RX H CX M MX MR TICK X_ERROR Z_ERROR DEPOLARIZE1
DEPOLARIZE2 DETECTOR OBSERVABLE_INCLUDE REPEAT{...} (one level; nesting is accepted too).

Biased noise.  PAULI_CHANNEL_1(px, py, pz) / PAULI_CHANNEL_2(pIX ... pZZ, 15 entries) are what the reference emits when an
ErrorModel field is a tuple (`circuit.py:115,139,171`); Y_ERROR(p) is their one-Pauli sibling.  `flatten(text)` refuses all
three, as it always has: a detector error model of a channel needs Stim's approximate-disjoint-error conversion, which the
caller has to ask for.  `flatten(text, channels=True)` accepts them: `Op.args` carries the parenthesised list and `Op.arg`
its sum (the probability that the site does anything).  The frame sampler (frame.py) always parses this way; the DEM
extractor (dem.py) does and then applies Stim's opt-in rule.  Noisy measurements M(p) flip a record, not the frame, are never
emitted by the reference and stay refused in both modes.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

_GATES = {"R", "RX", "H", "CX", "M", "MX", "MR"}
_NOISE = {"X_ERROR", "Z_ERROR", "DEPOLARIZE1", "DEPOLARIZE2"}
_CHANNELS = {"PAULI_CHANNEL_1": 3, "PAULI_CHANNEL_2": 15, "Y_ERROR": 1}     # accepted by flatten(channels=True): argument count
_ANNOT = {"DETECTOR", "OBSERVABLE_INCLUDE"}
_IGNORED = {"TICK", "QUBIT_COORDS", "SHIFT_COORDS"}
_COORD_ARGS = {"DETECTOR", "QUBIT_COORDS", "SHIFT_COORDS"}     # parenthesised arguments are coordinates: ignored
_UNSUPPORTED = {"PAULI_CHANNEL_1", "PAULI_CHANNEL_2", "Y_ERROR", "CORRELATED_ERROR", "E",
                "ELSE_CORRELATED_ERROR", "MPP", "MY", "RY", "MRX", "MRY", "CZ", "CY", "SWAP",
                "S", "S_DAG", "SQRT_X", "X", "Y", "Z", "CNOT", "ZCX"}


@dataclass(frozen=True)
class Op:
    """One flattened circuit instruction.

    name    : gate / noise / annotation mnemonic
    arg     : parenthesised argument (probability, or observable index), 0.0 if none; for PAULI_CHANNEL_1/2 the sum of args
    targets : qubit indices, or (for DETECTOR / OBSERVABLE_INCLUDE) *absolute* measurement indices
    args    : the parenthesised list of PAULI_CHANNEL_1 (px, py, pz), PAULI_CHANNEL_2 (IX ... ZZ) and Y_ERROR (p); () elsewhere
    """
    name: str
    arg: float
    targets: Tuple[int, ...]
    args: Tuple[float, ...] = ()


class CircuitSyntaxError(ValueError):
    pass


def _parse_line(line: str, channels: bool = False):
    head, _, rest = line.partition(" ")
    arg = 0.0
    if "(" in head or (rest.startswith("(")):
        # e.g. "X_ERROR(0.003) 1 2"  (the reference never puts a space before '(')
        name, _, tail = line.partition("(")
        argtxt, _, rest = tail.partition(")")
        name = name.strip()
        if name.upper() in _COORD_ARGS:
            # DETECTOR(x, y, t) / QUBIT_COORDS(x, y) / SHIFT_COORDS(...): coordinates carry no decoding information
            return name.upper(), 0.0, rest.split()
        if channels and name.upper() in _CHANNELS:
            try:
                args = tuple(float(x) for x in argtxt.split(","))
            except ValueError as exc:
                raise CircuitSyntaxError(f"bad argument list in {line!r}") from exc
            return name.upper(), args, rest.split()
        if "," in argtxt:
            raise NotImplementedError(
                f"{name} with a multi-parameter channel is not supported (reference emits it only for "
                "tuple-valued ErrorModel fields, circuit.py:115,139,171); use scalar rates")
        arg = float(argtxt)
    else:
        name = head
    return name.strip().upper(), arg, rest.split()


def _channel_op(name: str, args, toks, ln: str) -> Op:
    """Op of a PAULI_CHANNEL_1 / PAULI_CHANNEL_2 / Y_ERROR line (flatten(channels=True))."""
    if not isinstance(args, tuple) or len(args) != _CHANNELS[name]:
        raise CircuitSyntaxError(f"{name} takes {_CHANNELS[name]} argument(s): {ln!r}")
    try:
        qs = tuple(int(t) for t in toks)
    except ValueError as exc:
        raise CircuitSyntaxError(f"bad qubit target in {ln!r}") from exc
    if name == "PAULI_CHANNEL_2" and len(qs) % 2:
        raise CircuitSyntaxError(f"{name} needs an even number of targets")
    total = 0.0
    for p in args:                                              # left to right in float64, as frame.py accumulates its thresholds
        if not p >= 0.0:
            raise ValueError(f"negative probability in {ln!r}")
        total += p
    if total > 1.0 + 1e-9:
        raise ValueError(f"the probabilities of {ln!r} add up to more than 1")
    return Op(name, total, qs, args)


def flatten(text: str, channels: bool = False) -> Tuple[List[Op], int, int, int]:
    """Expand REPEAT blocks and resolve rec[-k] to absolute measurement indices.

    channels=True accepts PAULI_CHANNEL_1, PAULI_CHANNEL_2 and Y_ERROR (module docstring); the default refuses them.
    Returns (ops, num_measurements, num_detectors, num_observables).
    """
    lines = [ln.split("#", 1)[0].strip() for ln in text.splitlines()]
    lines = [ln for ln in lines if ln]
    ops: List[Op] = []
    state = {"meas": 0, "det": 0, "obs": 0}

    def run(block: List[str]):
        i = 0
        while i < len(block):
            ln = block[i]
            if ln.upper().startswith("REPEAT"):
                parts = ln.replace("{", " { ").split()
                if len(parts) < 3 or parts[2] != "{":
                    raise CircuitSyntaxError(f"malformed REPEAT header: {ln!r}")
                count = int(parts[1])
                depth, j = 1, i + 1
                while j < len(block):
                    if block[j].upper().startswith("REPEAT"):
                        depth += 1
                    elif block[j] == "}":
                        depth -= 1
                        if depth == 0:
                            break
                    j += 1
                if depth != 0:
                    raise CircuitSyntaxError("unterminated REPEAT block")
                body = block[i + 1:j]
                for _ in range(count):
                    run(body)
                i = j + 1
                continue
            if ln == "}":
                raise CircuitSyntaxError("unbalanced '}'")
            name, arg, toks = _parse_line(ln, channels)
            if name in _IGNORED:
                pass
            elif channels and name in _CHANNELS:
                ops.append(_channel_op(name, arg, toks, ln))
            elif name in _GATES or name in _NOISE:
                try:
                    qs = tuple(int(t) for t in toks)
                except ValueError as exc:
                    raise CircuitSyntaxError(f"bad qubit target in {ln!r}") from exc
                if name in ("M", "MX", "MR") and arg != 0.0:
                    # Stim's measurement-flip noise M(p): the reference models measurement errors with X_ERROR / Z_ERROR
                    # before the measurement instead (circuit.py:201-246); dropping the argument would silently empty the DEM
                    raise NotImplementedError(f"{name}({arg:g}): noisy-measurement arguments are outside the QUITS dialect "
                                              "handled here (the reference emits X_ERROR/Z_ERROR before M/MX/MR)")
                if name in ("CX", "DEPOLARIZE2") and len(qs) % 2:
                    raise CircuitSyntaxError(f"{name} needs an even number of targets")
                ops.append(Op(name, arg, qs))
                if name in ("M", "MX", "MR"):
                    state["meas"] += len(qs)
            elif name in _ANNOT:
                recs = []
                for t in toks:
                    if not (t.startswith("rec[-") and t.endswith("]")):
                        raise CircuitSyntaxError(f"unsupported target {t!r} in {ln!r}")
                    k = int(t[5:-1])
                    idx = state["meas"] - k
                    if idx < 0:
                        raise CircuitSyntaxError(f"{t} looks before the first measurement")
                    recs.append(idx)
                if name == "DETECTOR":
                    ops.append(Op(name, float(state["det"]), tuple(recs)))
                    state["det"] += 1
                else:
                    obs = int(arg)
                    ops.append(Op(name, float(obs), tuple(recs)))
                    state["obs"] = max(state["obs"], obs + 1)
            elif name in _UNSUPPORTED:
                raise NotImplementedError(f"Stim instruction {name} is outside the QUITS dialect handled here")
            else:
                raise CircuitSyntaxError(f"unknown instruction {name!r}")
            i += 1

    run(lines)
    return ops, state["meas"], state["det"], state["obs"]
