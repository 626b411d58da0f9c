"""Stratified sampling of a detector error model: shots conditioned on exactly k faults firing (subset sampling).

The law.  Faults fire independently with priors p_j; with the odds w_j = p_j / (1 - p_j) a fault set S has probability
prod_j (1 - p_j) * prod_{j in S} w_j, so conditioned on |E| = k it has probability prod_{j in S} w_j / e_k(w), e_k the k-th elementary
symmetric polynomial.  The sampler walks the faults in ascending index with r faults still to place and includes fault j with probability

    q[j][r] = w_j e_{r-1}(w_{j+1..}) / e_r(w_{j..}),

which draws S from exactly that law; inclusion is forced when n - j = r, and the walk ends when r = 0.

The stream.  The decision for fault j of shot s uses word j & 3 of Philox4x32-10 with key = (seed lo, seed hi) and counter
(s lo, s hi, j >> 2, 2) -- the DEM sampler's last counter word is 0, the frame sampler's 1 -- and the fault is included iff

    word < floor(q[j][r] 2^32)   or   n - j == r.

So a row depends on (seed, s, k) alone, not on batch boundaries or on how a kernel is parallelised, and every decision has the 2^-32
resolution of the DEM sampler's thresholds.  `sample_mirror` is this paragraph in numpy: the specification of qd_sample_dem_strata
(csrc/strata_sampler.hip).

The estimator.  P(|E| = k) is the Poisson-binomial pmf (`fault_count_pmf`), f(k) = P(fail | k faults) is measured per stratum, and

    pL = sum_k pmf_k f_k,   sigma^2 = sum_k pmf_k^2 f_k (1 - f_k) / N_k,   pL <= truth <= pL + unsampled_mass,

unsampled_mass = the pmf of the strata without shots plus the tail above the table (`estimate`)."""
from __future__ import annotations

import math

import numpy as np

KMAX_LIMIT = 255              # the last bin of QD_FAULT_HIST: a stratum beyond it could not be told from its neighbours in the histograms
UNREACHABLE = 0               # the threshold of a state (j, r) no walk reaches: e_r(w_{j..}) = 0
STREAM = 2                    # last Philox counter word of this sampler

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on broadcastable arrays of 32-bit words; four uint64 arrays of 32-bit words.  (Every product of two 32-bit words fits
    a uint64.)  The generator of qd_internal.h, restated; tests check it against the oracle's C function."""
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


def _checked_priors(priors, kmax):
    p = np.ascontiguousarray(priors, dtype=np.float64).reshape(-1)
    if p.size == 0:
        raise ValueError("no faults")
    if not np.all((p >= 0.0) & (p < 1.0)):              # (also refuses NaN)
        raise ValueError("priors must lie in [0, 1): a fault that always fires has infinite odds")
    kmax = int(kmax)
    if kmax < 0 or kmax > KMAX_LIMIT:
        raise ValueError("kmax = %d outside 0 .. %d (the last bin of the fault histograms)" % (kmax, KMAX_LIMIT))
    return p, kmax


def strata_thresholds(priors, kmax):
    """uint32 [n, kmax + 1]: floor(q[j][r] 2^32), clipped to 2^32 - 1.  Column 0 is 0 (nothing left to place: never included).  A state no
    walk reaches -- r exceeds the number of faults with p > 0 among j .. n - 1 -- holds UNREACHABLE (0).

    The recursion runs backwards over j on the RATIOS rho[j][r] = e_r(w_{j..}) / e_{r-1}(w_{j..}), never on the polynomials themselves (whose
    rows, however rescaled, span more than the double range near the end of the list and turn reachable states into 0 / 0):

        q[j][r] = w_j / (rho[j+1][r] + w_j),      rho[j][1] = rho[j+1][1] + w_j,
        rho[j][r] = rho[j+1][r-1] (rho[j+1][r] + w_j) / (rho[j+1][r-1] + w_j)   (r >= 2),

    from rho[n][.] = 0, with rho = 0 exactly where e_r = 0.  Only positive numbers are added, multiplied and divided, so the relative error
    of every rho and q is a few ulp per step: about 3 n 2^-53, far below one threshold unit (2^-32) for any n that fits a device.  A fault
    of prior 0 leaves rho as it is and gets threshold 0.  Where w_j > 0 and r equals the number of positive priors left, q = 1 and the
    threshold is 2^32 - 1; the rule `n - j == r` covers that case exactly when no prior 0 lies behind j -- with one behind it the
    decision misses with probability 2^-32, the resolution of every other decision."""
    p, kmax = _checked_priors(priors, kmax)
    n = p.shape[0]
    w = p / (1.0 - p)
    thr = np.full((n, kmax + 1), UNREACHABLE, dtype=np.uint32)
    if kmax == 0:
        return thr
    rho = np.zeros(kmax + 2, dtype=np.float64)          # rho[r], r = 1 .. kmax of the suffix behind j; rho[0] unused, rho[kmax + 1] scratch
    left = 0                                            # positive priors in that suffix: rho[r] > 0 for r <= left, 0 beyond
    for j in range(n - 1, -1, -1):
        wj = w[j]
        if wj == 0.0:
            continue                                    # e(w_{j..}) = e(w_{j+1..}); every q is 0
        top = min(left + 1, kmax)                       # states r = 1 .. top are reachable from here
        q = wj / (rho[1:top + 1] + wj)
        thr[j, 1:top + 1] = np.minimum(np.floor(q * 4294967296.0), 4294967295.0).astype(np.uint32)
        new = np.zeros_like(rho)
        new[1] = rho[1] + wj
        if top >= 2:
            new[2:top + 1] = rho[1:top] * ((rho[2:top + 1] + wj) / (rho[1:top] + wj))
        rho = new
        left += 1
    return thr


def fault_count_pmf(priors, kmax):
    """(pmf float64 [kmax + 1], tail): P(|E| = k) for k <= kmax and P(|E| > kmax), the Poisson-binomial law of the model.  One forward pass
    P_j[k] = P_{j-1}[k] (1 - p_j) + P_{j-1}[k - 1] p_j; the mass that leaves bin kmax is summed as it leaves, so the tail is not a
    difference from 1.  Only non-negative numbers are added: each entry is good to a few n ulp."""
    p, kmax = _checked_priors(priors, kmax)
    pmf = np.zeros(kmax + 1, dtype=np.float64)
    pmf[0] = 1.0
    tail = 0.0
    for pj in p:
        if pj == 0.0:
            continue
        tail += pmf[kmax] * pj
        pmf[1:] = pmf[1:] * (1.0 - pj) + pmf[:-1] * pj
        pmf[0] *= 1.0 - pj
    return pmf, float(tail)


def check_ks(ks, shots, priors, kmax):
    """`ks` (an int or `shots` ints) as an int32 array of length `shots`, refused outside 0 .. min(kmax, number of faults with p > 0)."""
    k = np.asarray(ks)
    if k.size and k.dtype.kind not in "iu":
        raise ValueError("fault counts must be integers")
    k = np.ascontiguousarray(np.broadcast_to(k.astype(np.int64), (int(shots),)) if k.ndim == 0 else k.reshape(-1).astype(np.int64))
    if k.shape[0] != int(shots):
        raise ValueError("%d fault counts for %d shots" % (k.shape[0], int(shots)))
    positive = int(np.count_nonzero(np.asarray(priors) > 0.0))
    if k.size and (int(k.min()) < 0 or int(k.max()) > min(int(kmax), positive)):
        raise ValueError("fault counts must lie in 0 .. min(kmax = %d, %d faults with p > 0); got %d .. %d"
                         % (int(kmax), positive, int(k.min()), int(k.max())))
    return k.astype(np.int32)


def sample_faults_mirror(priors, ks, seed, shots, thresholds=None):
    """The walk alone: bool [len(shots), n], row i = the fault set of shot shots[i] of `seed`'s stream with ks[i] faults.  `shots`: a count
    (shots 0 .. shots - 1) or an array of shot indices, any order, repeats allowed."""
    p = np.ascontiguousarray(priors, dtype=np.float64).reshape(-1)
    n = p.shape[0]
    s = np.arange(int(shots), dtype=np.uint64) if np.ndim(shots) == 0 else np.asarray(shots).astype(np.uint64).reshape(-1)
    kmax = int(np.max(ks)) if thresholds is None else thresholds.shape[1] - 1
    r = check_ks(ks, s.shape[0], p, kmax).astype(np.int64)
    thr = strata_thresholds(p, kmax) if thresholds is None else thresholds
    E = np.zeros((s.shape[0], n), dtype=bool)
    rows = np.arange(s.shape[0])
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    words = None
    for j in range(n):
        if not r.any():
            break
        if j & 3 == 0 or words is None:
            words = philox4x32_10(s & _M32, s >> _S32, j >> 2, STREAM, k0, k1)
        inc = (r > 0) & ((words[j & 3] < thr[j, r].astype(np.uint64)) | (n - j == r))
        E[rows[inc], j] = True
        r = r - inc
    return E


def sample_mirror(H, L, priors, ks, seed, shots):
    """Plain numpy restatement of the stratified sampler: (det uint8 [B, m], obs uint8 [B, nobs], fault bits bool [B, n]); det = H E and
    obs = L E over GF(2).  `ks`: an int or one int per row; `shots`: a count or an array of shot indices."""
    from scipy.sparse import csr_matrix
    E = sample_faults_mirror(priors, ks, seed, shots)
    Ei = csr_matrix(E.astype(np.int32))
    det = np.asarray((Ei @ csr_matrix(H).astype(np.int32).T).todense()) & 1
    obs = np.asarray((Ei @ csr_matrix(L).astype(np.int32).T).todense()) & 1
    return det.astype(np.uint8), obs.astype(np.uint8), E


def estimate(shots_by_faults, errors_by_faults, pmf, tail):
    """(pL, sigma, unsampled_mass) of a stratified run: pL = sum over the sampled k of pmf_k f_k with f_k = errors_k / shots_k,
    sigma = sqrt(sum pmf_k^2 f_k (1 - f_k) / shots_k), unsampled_mass = the pmf of the strata without shots + tail."""
    s = np.asarray(shots_by_faults, dtype=np.float64)
    e = np.asarray(errors_by_faults, dtype=np.float64)
    pmf = np.asarray(pmf, dtype=np.float64)
    if s.shape != e.shape or s.ndim != 1 or pmf.shape[0] > s.shape[0]:
        raise ValueError("shots, errors: one-dimensional and equally long, at least as long as the pmf")
    if np.any(e > s) or np.any(s < 0) or np.any(e < 0) or np.any(s[pmf.shape[0]:] > 0):
        raise ValueError("more errors than shots, negative counts, or shots in a stratum the pmf does not cover")
    s, e = s[:pmf.shape[0]], e[:pmf.shape[0]]
    on = s > 0
    f = e[on] / s[on]
    pL = float(np.sum(pmf[on] * f))
    sigma = math.sqrt(float(np.sum(pmf[on] ** 2 * f * (1.0 - f) / s[on])))
    return pL, sigma, float(np.sum(pmf[~on]) + tail)
