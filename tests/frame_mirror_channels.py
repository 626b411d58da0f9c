"""CPU restatement of the frame sampler WITH biased noise (test infrastructure; the specification of Y_ERROR, PAULI_CHANNEL_1 and
PAULI_CHANNEL_2 in qd_sample_circuit).

Written from the sampling contract in quits_amd/frame.py's docstring and sharing nothing with quits_amd/frame.py or the kernel
but the text parser (stim_text.flatten(channels=True)); Philox and the bit packing come from tests/frame_mirror.py, whose own
sampler this one must equal on every circuit without the new instructions (tests/test_frame_channels.py):

  * frames, gates, measurements, detectors and observables as in frame_mirror.py;
  * one site per target of X_ERROR / Z_ERROR / Y_ERROR / DEPOLARIZE1 / PAULI_CHANNEL_1, one per target pair of DEPOLARIZE2 /
    PAULI_CHANNEL_2, each noise instruction starting at the next multiple of 4;
  * shot s, site j: r = Philox4x32-10(key = (seed lo, seed hi), counter = (s lo, s hi, j >> 2, 1))[j & 3];
  * X_ERROR / Z_ERROR / Y_ERROR fire iff r < floor(p 2^32); DEPOLARIZE1 then applies Pauli 1 + r mod 3, DEPOLARIZE2
    v = 1 + r mod 15 as (v >> 2, v & 3); Y_ERROR flips both bits;
  * a channel with probabilities p_1 .. p_K has T_k = floor(2^32 (p_1 + .. + p_k)) (clamped to 2^32 - 1), the sums accumulated
    left to right in float64, T_0 = 0, and applies component k iff T_{k-1} <= r < T_k: Pauli k for PAULI_CHANNEL_1, Paulis
    (k >> 2, k & 3) for the pair of PAULI_CHANNEL_2 (1 = X, 2 = Y, 3 = Z, 0 = I).

sample(..., components=True) also returns, per channel instruction, the drawn component of every (site, shot), 0 = none."""
import numpy as np

from frame_mirror import _M32, _S32, _paulis_to_masks, _unpack, philox, threshold
from quits_amd.stim_text import flatten

_ONE = ("X_ERROR", "Z_ERROR", "Y_ERROR", "DEPOLARIZE1", "PAULI_CHANNEL_1")
_TWO = ("DEPOLARIZE2", "PAULI_CHANNEL_2")


def parse(text):
    return flatten(text, channels=True)


def channel_thresholds(args):
    """T_1 .. T_K."""
    out, acc = [], 0.0
    for p in args:
        acc += float(p)
        out.append(threshold(acc))
    return out


def draws(seed, shot0, B, site0, n):
    """r of sites site0 .. site0 + n - 1 (site0 a multiple of 4) for shots shot0 .. shot0 + B - 1: uint64 [n, B] of 32-bit words."""
    assert site0 % 4 == 0
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    shots = np.uint64(shot0) + np.arange(B, dtype=np.uint64)
    groups = (n + 3) // 4
    ctr = np.uint64(site0 >> 2) + np.arange(groups, dtype=np.uint64)
    r = philox((shots & _M32)[None, :], (shots >> _S32)[None, :], ctr[:, None], 1, k0, k1)
    return np.stack(r, axis=1).reshape(groups * 4, B)[:n]


def component(r, table):
    """Component index per draw: k with T_{k-1} <= r < T_k, 0 if r >= T_K.  Written as the definition, interval by interval."""
    comp = np.zeros(r.shape, np.int64)
    lo = 0
    for k, hi in enumerate(table, start=1):
        comp[(r >= np.uint64(lo)) & (r < np.uint64(hi))] = k
        lo = hi
    return comp


def _site_paulis(op, r):
    """Pauli code per target and shot, int [len(targets), B] (0 = none), and the component array of a channel (else None)."""
    nm = op.name
    nt = len(op.targets)
    if nm in ("X_ERROR", "Z_ERROR", "Y_ERROR"):
        code = {"X_ERROR": 1, "Y_ERROR": 2, "Z_ERROR": 3}[nm]
        return np.where(r < np.uint64(threshold(op.arg)), code, 0), None
    if nm == "DEPOLARIZE1":
        return np.where(r < np.uint64(threshold(op.arg)), 1 + (r % np.uint64(3)).astype(np.int64), 0), None
    if nm == "PAULI_CHANNEL_1":
        comp = component(r, channel_thresholds(op.args))
        return comp, comp
    comp = None
    if nm == "DEPOLARIZE2":
        v = np.where(r < np.uint64(threshold(op.arg)), 1 + (r % np.uint64(15)).astype(np.int64), 0)
    else:
        v = comp = component(r, channel_thresholds(op.args))
    pauli = np.empty((nt, r.shape[1]), np.int64)
    pauli[0::2], pauli[1::2] = v >> 2, v & 3
    return pauli, comp


def run(text, seed, shot0, B, parsed=None, components=False):
    ops, nmeas, ndet, nobs = parsed if parsed is not None else parse(text)
    W = (B + 63) // 64
    nq = 1 + max([max(op.targets) for op in ops if op.name not in ("DETECTOR", "OBSERVABLE_INCLUDE") and op.targets] + [-1])
    X = np.zeros((nq, W), np.uint64)
    Z = np.zeros((nq, W), np.uint64)
    meas = np.zeros((nmeas, W), np.uint64)
    det = np.zeros((ndet, W), np.uint64)
    obs = np.zeros((nobs, W), np.uint64)
    drawn = []
    m = site = 0
    for op in ops:
        nm, t = op.name, list(op.targets)
        if nm in ("R", "RX"):
            X[t] = 0
            Z[t] = 0
        elif nm == "H":
            for q in t:                                     # left to right; a repeated qubit is swapped twice
                X[q], Z[q] = Z[q].copy(), X[q].copy()
        elif nm == "CX":
            if len(set(t)) == len(t):
                c, u = t[0::2], t[1::2]
                X[u] ^= X[c]
                Z[c] ^= Z[u]
            else:
                for c, u in zip(t[0::2], t[1::2]):
                    X[u] ^= X[c]
                    Z[c] ^= Z[u]
        elif nm in ("M", "MX", "MR"):
            for q in t:
                meas[m] = Z[q] if nm == "MX" else X[q]
                m += 1
                if nm == "MR":
                    X[q] = 0
                    Z[q] = 0
        elif nm in _ONE or nm in _TWO:
            n = len(t) // 2 if nm in _TWO else len(t)
            site = (site + 3) // 4 * 4
            if n:
                pauli, comp = _site_paulis(op, draws(seed, shot0, B, site, n))
                xm, zm = _paulis_to_masks(pauli > 0, pauli)
                np.bitwise_xor.at(X, np.asarray(t, np.int64), xm)
                np.bitwise_xor.at(Z, np.asarray(t, np.int64), zm)
                if components and comp is not None:
                    drawn.append((nm, site, comp.astype(np.int8)))
            site += n
        elif nm == "DETECTOR":
            for k in t:
                det[int(op.arg)] ^= meas[k]
        elif nm == "OBSERVABLE_INCLUDE":
            for k in t:
                obs[int(op.arg)] ^= meas[k]
        else:
            raise AssertionError(nm)
    assert m == nmeas
    out = (_unpack(det, B), _unpack(obs, B))
    return out + (drawn,) if components else out


def sample(text, seed, shot0, B, parsed=None, components=False):
    """What qd_sample_circuit(seed, shot0, B) must return, bit for bit; with components=True a third entry, the list of
    (instruction name, first site, component int8 [sites, B]) of the channel instructions in program order."""
    return run(text, seed, shot0, B, parsed, components)
