"""Biased-noise test circuits, made by rewriting the golden circuit texts (no fixtures of their own): every DEPOLARIZE1(p)
becomes a PAULI_CHANNEL_1 and every DEPOLARIZE2(p) a PAULI_CHANNEL_2 -- what the reference's circuit writer emits when an
ErrorModel field is a tuple."""
import re

# Z-biased one-qubit noise; twelve distinct two-qubit weights and three zeros (components 4 = XI, 9 = YX, 14 = ZY)
W1 = (0.1, 0.1, 0.8)
_RAW2 = (1, 2, 3, 0, 5, 6, 7, 8, 0, 10, 11, 12, 13, 0, 15)
W2 = tuple(x / sum(_RAW2) for x in _RAW2)

_DEP = re.compile(r"DEPOLARIZE([12])\(([^)]*)\)")


def rewrite(text, one, two):
    """one(p) -> the 3 arguments replacing DEPOLARIZE1(p), two(p) -> the 15 replacing DEPOLARIZE2(p); printed with repr."""
    def sub(m):
        p = float(m.group(2))
        args = one(p) if m.group(1) == "1" else two(p)
        assert len(args) == (3 if m.group(1) == "1" else 15)
        return "PAULI_CHANNEL_%s(%s)" % (m.group(1), ", ".join(repr(float(a)) for a in args))
    out, n = _DEP.subn(sub, text)
    assert n > 0
    return out


def biased(text, scale=1.0):
    """The same total probability per site (times `scale`), split by W1 / W2."""
    return rewrite(text, lambda p: [scale * p * w for w in W1], lambda p: [scale * p * w for w in W2])


def uniform(text):
    """DEPOLARIZE1(p) -> PAULI_CHANNEL_1(p/3, p/3, p/3), DEPOLARIZE2(p) -> the uniform 15-entry channel: the same distribution."""
    return rewrite(text, lambda p: [p / 3.0] * 3, lambda p: [p / 15.0] * 15)


def independent_equivalent(text):
    """Every component gets the extractor's own independent-equivalent probability of the depolarizing channel, so that the
    approximate-disjoint conversion of the rewritten circuit and the exact conversion of the original fold the same numbers."""
    from quits_amd.dem import _mechanism_probability
    from quits_amd.stim_text import Op
    return rewrite(text, lambda p: [_mechanism_probability(Op("DEPOLARIZE1", p, ()))] * 3,
                   lambda p: [_mechanism_probability(Op("DEPOLARIZE2", p, ()))] * 15)


# exercises the partial last group of four sites: 5 targets, 6 targets, 7 pairs
SYNTHETIC = """R 0 1 2 3 4 5 6 7 8 9 10 11 12 13
RX 14 15
Y_ERROR(0.3) 0 1 2 3 4
H 5
PAULI_CHANNEL_1(0.05, 0.1, 0.2) 0 3 5 6 7 14
H 5
CX 0 1 2 3 4 5 6 7 8 9 10 11 12 13
PAULI_CHANNEL_2(%s) 0 1 2 3 4 5 6 7 8 9 10 11 12 14
X_ERROR(0.1) 1 2
Y_ERROR(0.02) 15 14
DEPOLARIZE2(0.2) 1 2 13 0
PAULI_CHANNEL_1(0.05, 0.1, 0.2) 9 15
MR 1 3 5 7
M 0 2 4 6 8 9 10 11 12 13 1 3
MX 14 15
DETECTOR rec[-1]
DETECTOR rec[-2]
DETECTOR rec[-3] rec[-17]
DETECTOR rec[-4] rec[-18]
DETECTOR rec[-5]
DETECTOR rec[-6]
DETECTOR rec[-7] rec[-8]
DETECTOR rec[-9]
DETECTOR rec[-10] rec[-15]
DETECTOR rec[-11]
DETECTOR rec[-12] rec[-16]
OBSERVABLE_INCLUDE(0) rec[-13] rec[-14]
OBSERVABLE_INCLUDE(1) rec[-1] rec[-2]
""" % ", ".join(repr(0.4 * w) for w in W2)
