"""CPU restatement of the circuit-level frame sampler (test infrastructure; the specification of qd_sample_circuit).

Written from the contract alone -- the frame rules, the site numbering and the random stream of quits_amd/frame.py's docstring --
and sharing nothing with quits_amd/frame.py or the kernel but the text parser (stim_text.flatten):

  * a Pauli frame per qubit, X and Z bits, bit-sliced: shot b is bit b & 63 of word b >> 6 (as in dem_forward.py);
  * R / RX clear both, H swaps, CX c t: X[t] ^= X[c] then Z[c] ^= Z[t], M / MR record X, MX records Z, MR clears after;
    targets apply left to right (an instruction that repeats a qubit is walked one target at a time);
  * noise sites in flattened program order, one per target of X_ERROR / Z_ERROR / DEPOLARIZE1, one per target pair of
    DEPOLARIZE2, each noise instruction starting at the next multiple of 4;
  * shot s, site j: r = Philox4x32-10(key = (seed lo, seed hi), counter = (s lo, s hi, j >> 2, 1))[j & 3], fires iff
    r < floor(p 2^32); DEPOLARIZE1 applies Pauli 1 + r mod 3, DEPOLARIZE2 v = 1 + r mod 15 as (v >> 2, v & 3), 1 = X, 2 = Y, 3 = Z;
  * detector / observable = XOR of the recorded measurement flips it names.

Philox is vectorised over shots and counters in uint64 arithmetic (every product of two 32-bit words fits)."""
import numpy as np

from quits_amd.stim_text import flatten

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on broadcastable arrays of 32-bit words (any integer dtype); returns four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(x).astype(np.uint64) & _M32 for x in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _M32)
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def threshold(p):
    return int(min(max(np.floor(float(p) * 4294967296.0), 0.0), 4294967295.0))


def _pack(bits):
    """bool [k, B] -> uint64 [k, words]: bit b of row i = bits[i, b]."""
    k, B = bits.shape
    W = (B + 63) // 64
    pad = np.zeros((k, W * 64), np.uint8)
    pad[:, :B] = bits
    return np.packbits(pad, axis=1, bitorder="little").view("<u8").astype(np.uint64)


def _unpack(words, B):
    """uint64 [k, words] -> uint8 [B, k]."""
    if words.shape[0] == 0:
        return np.zeros((B, 0), np.uint8)
    return np.unpackbits(np.ascontiguousarray(words).astype("<u8").view(np.uint8), axis=1, bitorder="little")[:, :B].T.copy()


def _paulis_to_masks(fire, pauli):
    """fire bool [k, B], pauli int [k, B] (1 X, 2 Y, 3 Z) -> (X-flip words, Z-flip words) [k, words]."""
    return _pack(fire & ((pauli == 1) | (pauli == 2))), _pack(fire & (pauli >= 2))


def random_noise(seed, shot0, B):
    """The sampler's noise: a function (name, p, first_site, targets) -> (X words, Z words) per target."""
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    shots = np.uint64(shot0) + np.arange(B, dtype=np.uint64)

    def noise(name, p, site0, targets):
        nt = len(targets)
        n = nt // 2 if name == "DEPOLARIZE2" else nt
        t = threshold(p)
        if t == 0 or n == 0:
            z = np.zeros((nt, (B + 63) // 64), np.uint64)
            return z, z.copy()
        groups = (n + 3) // 4
        ctr = np.uint64(site0 >> 2) + np.arange(groups, dtype=np.uint64)
        r = philox((shots & _M32)[None, :], (shots >> _S32)[None, :], ctr[:, None], 1, k0, k1)     # 4 x [groups, B]
        r = np.stack(r, axis=1).reshape(groups * 4, B)[:n]                                         # site-major [n, B]
        fire = r < np.uint64(t)
        if name == "X_ERROR":
            return _pack(fire), np.zeros((n, (B + 63) // 64), np.uint64)
        if name == "Z_ERROR":
            return np.zeros((n, (B + 63) // 64), np.uint64), _pack(fire)
        if name == "DEPOLARIZE1":
            return _paulis_to_masks(fire, 1 + (r % np.uint64(3)).astype(np.int64))
        v = 1 + (r % np.uint64(15)).astype(np.int64)
        pa, pb = v >> 2, v & 3
        xa, za = _paulis_to_masks(fire, pa)
        xb, zb = _paulis_to_masks(fire, pb)
        X = np.empty((nt, xa.shape[1]), np.uint64)
        Z = np.empty_like(X)
        X[0::2], X[1::2], Z[0::2], Z[1::2] = xa, xb, za, zb
        return X, Z
    return noise


def forced_noise(components):
    """Shot b carries exactly the fault component components[b], numbered as tests/dem_forward.py numbers them (noise
    instructions with p > 0 only: X_ERROR / Z_ERROR 1 per target, DEPOLARIZE1 X, Y, Z per target, DEPOLARIZE2 the 15 non-identity
    pairs (pa, pb) in order 4 pa + pb per pair)."""
    comps = np.asarray(components, np.int64)
    B = len(comps)
    state = {"c": 0}

    def noise(name, p, site0, targets):
        nt = len(targets)
        per = {"X_ERROR": 1, "Z_ERROR": 1, "DEPOLARIZE1": 3, "DEPOLARIZE2": 15}[name]
        nsite = nt // 2 if name == "DEPOLARIZE2" else nt
        pauli = np.zeros((nt, B), np.int64)
        if p > 0:
            c0 = state["c"]
            state["c"] += per * nsite
            sel = (comps >= c0) & (comps < c0 + per * nsite)
            for b in np.flatnonzero(sel):
                s, k = divmod(int(comps[b] - c0), per)
                if name == "X_ERROR":
                    pauli[s, b] = 1
                elif name == "Z_ERROR":
                    pauli[s, b] = 3
                elif name == "DEPOLARIZE1":
                    pauli[s, b] = 1 + k
                else:
                    v = 1 + k
                    pauli[2 * s, b], pauli[2 * s + 1, b] = v >> 2, v & 3
        return _paulis_to_masks(pauli > 0, pauli)
    return noise


def _distinct(qs):
    return len(set(qs)) == len(qs)


def run(text, B, noise, parsed=None):
    """Propagate frames of B shots through the circuit with the given noise function -> (det uint8 [B, ndet], obs uint8 [B, nobs])."""
    ops, nmeas, ndet, nobs = parsed if parsed is not None else flatten(text)
    W = (B + 63) // 64
    nq = 1 + max([max(op.targets) for op in ops if op.name not in ("DETECTOR", "OBSERVABLE_INCLUDE") and op.targets] + [-1])
    X = np.zeros((nq, W), np.uint64)
    Z = np.zeros((nq, W), np.uint64)
    meas = np.zeros((nmeas, W), np.uint64)
    det = np.zeros((ndet, W), np.uint64)
    obs = np.zeros((nobs, W), np.uint64)
    m = 0
    site = 0
    for op in ops:
        nm, t = op.name, list(op.targets)
        if nm in ("R", "RX"):
            X[t] = 0
            Z[t] = 0
        elif nm == "H":
            if _distinct(t):
                X[t], Z[t] = Z[t].copy(), X[t].copy()
            else:
                for q in t:
                    X[q], Z[q] = Z[q].copy(), X[q].copy()
        elif nm == "CX":
            if _distinct(t):
                c, u = t[0::2], t[1::2]
                X[u] ^= X[c]
                Z[c] ^= Z[u]
            else:
                for c, u in zip(t[0::2], t[1::2]):
                    X[u] ^= X[c]
                    Z[c] ^= Z[u]
        elif nm in ("M", "MX", "MR"):
            if nm == "MR" and not _distinct(t):
                for q in t:
                    meas[m] = X[q]
                    X[q] = 0
                    Z[q] = 0
                    m += 1
            else:
                meas[m:m + len(t)] = Z[t] if nm == "MX" else X[t]
                m += len(t)
                if nm == "MR":
                    X[t] = 0
                    Z[t] = 0
        elif nm in ("X_ERROR", "Z_ERROR", "DEPOLARIZE1", "DEPOLARIZE2"):
            site = (site + 3) // 4 * 4
            xm, zm = noise(nm, op.arg, site, t)
            np.bitwise_xor.at(X, np.asarray(t, np.int64), xm)
            np.bitwise_xor.at(Z, np.asarray(t, np.int64), zm)
            site += len(t) // 2 if nm == "DEPOLARIZE2" else len(t)
        elif nm == "DETECTOR":
            d = int(op.arg)
            for k in t:
                det[d] ^= meas[k]
        elif nm == "OBSERVABLE_INCLUDE":
            o = int(op.arg)
            for k in t:
                obs[o] ^= meas[k]
    assert m == nmeas
    return _unpack(det, B), _unpack(obs, B)


def sample(text, seed, shot0, B, parsed=None):
    """What qd_sample_circuit(seed, shot0, B) must return, bit for bit."""
    return run(text, B, random_noise(seed, shot0, B), parsed)
