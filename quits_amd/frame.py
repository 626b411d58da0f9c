"""Host compile step of the circuit-level Pauli-frame sampler (csrc/frame_sampler.hip, qd_circuit_* in include/quits_amd.h).

The sampler does what Stim's detector sampler does for the QUITS dialect (`stim_text.flatten`): per shot, detection
events and observable flips, each the parity of measurement flips relative to the noiseless circuit.  It propagates a
Pauli frame -- per qubit an X-flip bit and a Z-flip bit -- through the circuit:

    R, RX        clear both bits              M     record X
    H            swap X and Z                 MX    record Z
    CX c t       X[t] ^= X[c]; Z[c] ^= Z[t]   MR    record X, then clear both
    X_ERROR      flip X                       Z_ERROR  flip Z
    DEPOLARIZE1  Pauli 1 + r mod 3            DEPOLARIZE2  v = 1 + r mod 15: first target v >> 2, second v & 3
                 (Pauli codes 1 = X, 2 = Y = both bits, 3 = Z)
    Y_ERROR      flip X and Z                 PAULI_CHANNEL_1 / PAULI_CHANNEL_2  one component by cumulative thresholds (below)

Assumption: every DETECTOR and OBSERVABLE_INCLUDE is deterministic in the noiseless circuit, so the frame needs no gauge
randomisation (Stim randomises the Z part of a frame at resets and measurements; here the frame starts and stays exact).
The DEM extractor (dem.py) relies on the same assumption.  Circuits that break it would get wrong samples from both.

Random stream.  Noise sites are numbered in flattened program order: one per target of X_ERROR / Z_ERROR / Y_ERROR /
DEPOLARIZE1 / PAULI_CHANNEL_1, one per target pair of DEPOLARIZE2 / PAULI_CHANNEL_2, and each noise instruction starts at
the next multiple of 4.  Shot s, site j draws
    r = Philox4x32-10(key = (seed lo, seed hi), counter = (s lo, s hi, j >> 2, 1))[j & 3]
(qd_sample_dem's convention with counter word 3 = 1 instead of 0, so the two streams never coincide) and fires iff
r < floor(p * 2^32) (oq_prob_threshold).  The Pauli of a firing depolarizing site is drawn from the same r; `r mod K`
over r < thr is biased by at most K / thr relative (about 2e-7 for K = 15 at p = 3e-3).  The stream depends only on
(seed, shot, site), not on how the kernel lays out shots, so shot0 offsets and shards compose.

Biased noise (the reference's tuple-valued ErrorModel fields).  The sites and the draw r are the ones above.
    Y_ERROR(p)            fires iff r < prob_threshold(p) and flips both bits.
    PAULI_CHANNEL_1/2     A channel with probabilities p_1 .. p_K (K = 3: X, Y, Z; K = 15: IX, IY, IZ, XI, .. ZZ; Stim's argument
                          order, which is ErrorModel's) gets integer thresholds T_k = prob_threshold(p_1 + .. + p_k), the partial
                          sums accumulated left to right in float64, T_0 = 0.  Component k is applied iff T_{k-1} <= r < T_k, and
                          the site does nothing iff r >= T_K: component k has probability exactly (T_k - T_{k-1}) / 2^32, with no
                          modulo bias, and a component of probability 0 is never drawn.
                          PAULI_CHANNEL_1: component k is Pauli k.  PAULI_CHANNEL_2: the first target gets Pauli k >> 2, the
                          second k & 3 (0 = I) -- DEPOLARIZE2's mapping of v.
A circuit without these three instructions compiles to the program, and samples the bits, it did before they existed.

compile_circuit() turns a circuit into the flat int32 program the kernel walks (layout below), numbers the sites,
tabulates the thresholds, sizes the measurement ring from the largest rec look-back and checks the LDS budget.
Pure host code.

Program layout (int32 words; every instruction starts with opcode, count):
    OP_R  / OP_H   n, q[n]                    (RX is OP_R: both clear the frame)
    OP_CX          n pairs, (c, t)[n]
    OP_M / OP_MX / OP_MR   n, (q, ring slot)[n]
    OP_XERR / OP_ZERR / OP_DEP1   n, threshold index, first site, q[n]
    OP_DEP2        n pairs, threshold index, first site, (a, b)[n]
    OP_DET         k, detector index, ring slot[k]
    OP_FLUSH       count, first detector       (write detectors first .. first + count - 1, count <= 64)
    OP_OBS         k, observable index, ring slot[k]
    OP_YERR        n, threshold index, first site, q[n]
    OP_PC1         n, table index, first site, q[n]
    OP_PC2         n pairs, table index, first site, (a, b)[n]
`table index` is the first of 3 (OP_PC1) / 15 (OP_PC2) consecutive entries of the thresholds array, the channel's T_1 .. T_K;
equal tables are stored once.
A gate instruction whose targets repeat a qubit is split into sequential parts with distinct qubits each, so the
kernel's lanes may apply one part's targets in parallel.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .stim_text import flatten

OP_R, OP_H, OP_CX, OP_M, OP_MX, OP_MR, OP_XERR, OP_ZERR, OP_DEP1, OP_DEP2, OP_DET, OP_FLUSH, OP_OBS = range(13)
OP_YERR, OP_PC1, OP_PC2 = range(13, 16)

LDS_BUDGET = 64 * 1024          # bytes of LDS one wavefront (64 shots) may hold: frames + measurement ring + observables

_GATE_OP = {"R": OP_R, "RX": OP_R, "H": OP_H, "CX": OP_CX, "M": OP_M, "MX": OP_MX, "MR": OP_MR}
_NOISE_OP = {"X_ERROR": OP_XERR, "Z_ERROR": OP_ZERR, "DEPOLARIZE1": OP_DEP1, "DEPOLARIZE2": OP_DEP2,
             "Y_ERROR": OP_YERR, "PAULI_CHANNEL_1": OP_PC1, "PAULI_CHANNEL_2": OP_PC2}
_NOISE_CODES = frozenset(_NOISE_OP.values())
_PAIR_CODES = (OP_DEP2, OP_PC2)


@dataclass
class CompiledCircuit:
    program: np.ndarray        # int32 [program_len]
    thresholds: np.ndarray     # uint32 [nthr]: floor(p * 2^32), one per distinct noise probability; then the channels' tables
    nq: int                    # qubits (frame words per Pauli part)
    nmeas: int
    ndet: int
    nobs: int
    nsites: int                # noise sites (targets of the one-qubit noise instructions, pairs of DEPOLARIZE2 / PAULI_CHANNEL_2)
    site_span: int             # site numbers used, the alignment gaps included
    lookback: int              # largest rec[-k] look-back
    ring: int                  # measurement ring length: max(lookback, widest measurement instruction)
    lds_bytes: int             # per wavefront

    @property
    def first_sites(self) -> np.ndarray:
        """First site of every noise instruction, in program order."""
        out, pc, prog = [], 0, self.program
        while pc < len(prog):
            op, n = int(prog[pc]), int(prog[pc + 1])
            if op in _NOISE_CODES:
                out.append(int(prog[pc + 3]))
            pc += _length(op, n)
        return np.asarray(out, np.int64)


def _length(op: int, n: int) -> int:
    if op in (OP_R, OP_H):
        return 2 + n
    if op in (OP_CX, OP_M, OP_MX, OP_MR):
        return 2 + 2 * n
    if op in (OP_XERR, OP_ZERR, OP_DEP1, OP_YERR, OP_PC1):
        return 4 + n
    if op in _PAIR_CODES:
        return 4 + 2 * n
    if op in (OP_DET, OP_OBS):
        return 3 + n
    if op == OP_FLUSH:
        return 3
    raise ValueError("bad opcode %d" % op)


def prob_threshold(p: float) -> int:
    """floor(p * 2^32) clamped to [0, 2^32 - 1]: the rule of oq_prob_threshold / qd_sample_dem."""
    t = np.floor(float(p) * 4294967296.0)
    return int(min(max(t, 0.0), 4294967295.0))


def channel_thresholds(args) -> tuple:
    """T_1 .. T_K of a Pauli channel: prob_threshold of the partial sums, accumulated left to right in float64."""
    out, acc = [], 0.0
    for p in args:
        acc += float(p)
        out.append(prob_threshold(acc))
    return tuple(out)


def _split_distinct(groups):
    """Split a list of target groups (1 qubit, or a CX pair) into runs in which no qubit appears twice."""
    parts, cur, seen = [], [], set()
    for g in groups:
        if len(set(g)) != len(g):
            raise ValueError("CX with control equal to target %s" % (g,))
        if seen.intersection(g):
            parts.append(cur)
            cur, seen = [], set()
        cur.append(g)
        seen.update(g)
    if cur:
        parts.append(cur)
    return parts


def compile_circuit(circuit, lds_budget: int = LDS_BUDGET) -> CompiledCircuit:
    """Circuit text (or anything whose str() is the text: quits_amd.dem.Circuit, stim.Circuit) -> CompiledCircuit.
    Raises NotImplementedError if one wavefront's frames + ring + observables exceed `lds_budget` bytes."""
    ops, nmeas, ndet, nobs = flatten(str(circuit), channels=True)
    nq = 0
    for op in ops:
        if op.name in _GATE_OP or op.name in _NOISE_OP:
            if op.targets:
                nq = max(nq, 1 + max(op.targets))
    # look-back: how far behind the running measurement count an annotation reaches
    lookback, m = 0, 0
    for op in ops:
        if op.name in ("M", "MX", "MR"):
            m += len(op.targets)
        elif op.name in ("DETECTOR", "OBSERVABLE_INCLUDE") and op.targets:
            lookback = max(lookback, m - min(op.targets))
    # the ring holds every measurement an annotation can still read; it is at least as long as the widest measurement
    # instruction so that no two lanes of one instruction write the same slot
    widest = max([len(op.targets) for op in ops if op.name in ("M", "MX", "MR")] + [1])
    ring = max(lookback, widest)
    lds = 8 * (2 * nq + ring + nobs)
    if lds > lds_budget:
        raise NotImplementedError(
            "circuit needs %d B of LDS per wavefront (%d qubits x 16 B frames + %d-measurement ring x 8 B + %d observables x 8 B); "
            "the frame sampler's budget is %d B" % (lds, nq, ring, nobs, lds_budget))

    prog = []
    thr_index = {}
    tables, table_index = [], {}        # the channels' cumulative tables, laid out after the scalar thresholds
    fixups = []                         # program words holding a table index relative to the first table
    site = nsites = 0
    m = 0
    for op in ops:
        nm = op.name
        if nm in _GATE_OP:
            code = _GATE_OP[nm]
            if code == OP_CX:
                groups = [tuple(op.targets[i:i + 2]) for i in range(0, len(op.targets), 2)]
            else:
                groups = [(q,) for q in op.targets]
            for part in _split_distinct(groups):
                prog += [code, len(part)]
                for g in part:
                    if code in (OP_M, OP_MX, OP_MR):
                        prog += [g[0], m % ring]
                        m += 1
                    else:
                        prog += list(g)
        elif nm in _NOISE_OP:
            code = _NOISE_OP[nm]
            if code in (OP_PC1, OP_PC2):
                tab = channel_thresholds(op.args)
                if tab not in table_index:
                    table_index[tab] = len(tables)
                    tables += tab
                idx = table_index[tab]
                fixups.append(len(prog) + 2)
            else:
                t = prob_threshold(op.arg)
                idx = thr_index.setdefault(t, len(thr_index))
            n = len(op.targets) // 2 if code in _PAIR_CODES else len(op.targets)
            if code == OP_PC2 and any(op.targets[2 * i] == op.targets[2 * i + 1] for i in range(n)):
                raise ValueError("PAULI_CHANNEL_2 with both targets of a pair equal %s" % (op.targets,))
            site = (site + 3) & ~3
            prog += [code, n, idx, site] + list(op.targets)
            site += n
            nsites += n
        elif nm == "DETECTOR":
            d = int(op.arg)
            prog += [OP_DET, len(op.targets), d] + [k % ring for k in op.targets]
            if d % 64 == 63 or d == ndet - 1:
                base = d & ~63
                prog += [OP_FLUSH, d - base + 1, base]
        elif nm == "OBSERVABLE_INCLUDE":
            prog += [OP_OBS, len(op.targets), int(op.arg)] + [k % ring for k in op.targets]
    assert m == nmeas
    nscalar = max(len(thr_index), 1)
    thresholds = np.zeros(nscalar + len(tables), np.uint32)
    for t, i in thr_index.items():
        thresholds[i] = t
    thresholds[nscalar:] = tables
    for w in fixups:
        prog[w] += nscalar
    return CompiledCircuit(np.asarray(prog, np.int32), thresholds, nq, nmeas, ndet, nobs, nsites, site, lookback, ring, lds)
