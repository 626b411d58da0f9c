"""Relay-BP: flooding min-sum BP run as a chain of legs, every fault carrying a memory strength gamma_j that mixes its previous marginal
into its prior (after Mueller et al. 2025, "Improved belief propagation is sufficient for real-time decoding of quantum memory").

Host side, numpy only: the configuration, the table of memory strengths and `relay_mirror`, the definition of the decoder in float32
numpy -- the CPU reference of qd_bp_relay_kernel (csrc/bp_relay.hip), which must return the same bits.

The definition.  A window has check matrix H (m x n) and priors p_j; L0_j = float32(log((1 - p_j) / p_j)), the log in double.  Every
operation below is IEEE float32, rounded once, nothing fused.  Leg 0 runs `pre_iter` iterations with gamma_j = gamma0, leg r >= 1 runs
`set_max_iter` iterations with gamma_j = gammas[r - 1][j].  A shot keeps its marginals M_j (L0_j at the start) from leg to leg.

  start of a leg:   a_j = fl(fl(1 - gamma_j) L0_j), every check->fault message mu_ij = +0
  iteration t = 1.. of the leg:
    1. Lam_j = fl(a_j + fl(gamma_j M_j))
    2. P_j = Lam_j + the messages mu_ij of the previous iteration, added one at a time in ascending row index i
    3. nu_ji = fl(P_j - mu_ij)
    4. check i, syndrome bit s_i: nu is negative iff nu <= 0 (-0.0 included); the new mu_ij has magnitude
       fl(alpha min(FLT_MAX, min_{j' != j} |nu_j'i|)) and is negative iff s_i + #{j' != j: nu_j'i negative} is odd
       (alpha = ms_scaling_factor; 0 means 1 - 2^-t)
    5. M_j = Lam_j + the new messages, in the order of step 2
    6. e_j = [M_j <= 0];  7. if H e = s the leg ends with candidate e

A candidate weighs sum_j e_j w_j, w_j = llround(L0_j 2^16) (int64); it replaces the best one only if strictly lighter.  The decode stops
after `stop_nconv` candidates or the last leg and returns the best candidate, or, without one, the e of the last iteration run.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from . import strata

ITER_LIMIT = 16383          # QD_STATUS_ITER_MASK: the status word's iteration field holds the total over all legs
GAMMA_LIMIT = 1.5
MAX_SETS = 1023             # the status word's leg field, bits 20..29
_FLT_MAX = np.float32(np.finfo(np.float32).max)


@dataclasses.dataclass(frozen=True)
class RelayConfig:
    """Budgets and memory strengths of a Relay-BP decode.  The defaults are this project's, after the published gross-code settings as
    remembered (80 + 60 x 60 iterations, gamma0 = 0.125, gamma uniform in [-0.24, 0.66]); they reproduce no published number."""
    pre_iter: int = 80
    num_sets: int = 60
    set_max_iter: int = 60
    gamma0: float = 0.125
    gamma_min: float = -0.24
    gamma_max: float = 0.66
    stop_nconv: int = 1
    seed: int = 0

    def __post_init__(self):
        for name in ("pre_iter", "num_sets", "set_max_iter", "stop_nconv", "seed"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError("RelayConfig.%s must be an integer, not %r" % (name, v))
        if self.pre_iter < 1 or self.set_max_iter < 1:
            raise ValueError("pre_iter and set_max_iter must be at least 1")
        if self.num_sets < 0 or self.num_sets > MAX_SETS:
            raise ValueError("num_sets = %d outside 0 .. %d" % (self.num_sets, MAX_SETS))
        if self.stop_nconv < 1:
            raise ValueError("stop_nconv must be at least 1")
        for name in ("gamma0", "gamma_min", "gamma_max"):
            check_gamma(getattr(self, name), name)
        if self.gamma_min > self.gamma_max:
            raise ValueError("gamma_min %r > gamma_max %r" % (self.gamma_min, self.gamma_max))
        if self.total_iter > ITER_LIMIT:
            raise ValueError("pre_iter + num_sets * set_max_iter = %d exceeds %d, the status word's iteration field" % (self.total_iter, ITER_LIMIT))

    @property
    def total_iter(self) -> int:
        return int(self.pre_iter) + int(self.num_sets) * int(self.set_max_iter)


def check_gamma(g, what="gamma"):
    """ValueError unless every memory strength is finite and |gamma| < 1.5 (a guard against runaway magnitudes)."""
    a = np.asarray(g, dtype=np.float64)
    if not np.all(np.isfinite(a)) or (a.size and float(np.max(np.abs(a))) >= GAMMA_LIMIT):
        raise ValueError("%s must be finite with |gamma| < %g" % (what, GAMMA_LIMIT))


def relay_gammas(n: int, cfg: RelayConfig) -> np.ndarray:
    """float32 [num_sets, n]: gamma[r][j] = float32(gamma_min + (gamma_max - gamma_min) (x + 0.5) 2^-32) in double, x = word j & 3 of
    Philox4x32-10 with key = seed and counter = (j >> 2, r, 0, 3) -- the samplers' last counter words are 0, 1 and 2.  The same table for
    every shot and every window of n faults."""
    n = int(n)
    if n < 1:
        raise ValueError("no faults")
    out = np.empty((cfg.num_sets, n), dtype=np.float32)
    if cfg.num_sets == 0:
        return out
    j = np.arange(n, dtype=np.uint64)
    r = np.arange(cfg.num_sets, dtype=np.uint64)[:, None]
    seed = int(cfg.seed) & (2 ** 64 - 1)
    words = strata.philox4x32_10((j >> np.uint64(2))[None, :], r, 0, 3, seed & 0xFFFFFFFF, seed >> 32)
    x = np.choose((j & np.uint64(3)).astype(np.intp)[None, :], [w.astype(np.float64) for w in words])
    out[:] = (float(cfg.gamma_min) + (float(cfg.gamma_max) - float(cfg.gamma_min)) * (x + 0.5) * 2.0 ** -32).astype(np.float32)
    return out


def prior_llr32(priors) -> np.ndarray:
    """float32(log((1 - p) / p)), the log in double: the channel LLRs as qd_graph_create keeps them."""
    p = np.asarray(priors, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.log((1.0 - p) / p).astype(np.float32)


def candidate_weights(llr0) -> np.ndarray:
    """int64 w_j = llround(L0_j 2^16), from the float32 value in double (halves away from zero)."""
    x = np.asarray(llr0, dtype=np.float32).astype(np.float64) * 65536.0
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5)).astype(np.int64)


def check_table(gammas, cfg: RelayConfig, n: int) -> np.ndarray:
    """The table of a decode as contiguous float32 [num_sets, n]; `None`: relay_gammas(n, cfg)."""
    if gammas is None:
        return relay_gammas(n, cfg)
    g = np.ascontiguousarray(gammas, dtype=np.float32)
    if g.shape != (cfg.num_sets, n):
        raise ValueError("gammas has shape %s, the decode needs (%d, %d)" % (g.shape, cfg.num_sets, n))
    check_gamma(g, "gammas")
    return g


class _Graph:
    """Edge lists of H in the two orders the definition sums in, padded to rectangles with one dummy edge (index E)."""

    def __init__(self, H):
        from scipy.sparse import csr_matrix
        H = csr_matrix(H)
        H.sort_indices()
        self.m, self.n = H.shape
        self.rows = np.repeat(np.arange(self.m), np.diff(H.indptr)).astype(np.intp)
        self.cols = H.indices.astype(np.intp)
        E = self.E = len(self.cols)
        rdeg, cdeg = np.diff(H.indptr), np.bincount(self.cols, minlength=self.n)
        self.epos = (np.arange(E) - H.indptr[self.rows]).astype(np.intp)             # position of an edge inside its row
        self.row_edges = np.full((self.m, max(1, int(rdeg.max(initial=0)))), E, dtype=np.intp)
        self.row_edges[self.rows, self.epos] = np.arange(E)
        self.row_faults = np.concatenate((self.cols, [self.n]))[self.row_edges]      # the dummy edge's fault: column n, never set
        order = np.lexsort((self.rows, self.cols))                                  # by column, rows ascending inside
        cstart = np.concatenate(([0], np.cumsum(cdeg)))
        self.col_edges = np.full((self.n, max(1, int(cdeg.max(initial=0)))), E, dtype=np.intp)
        self.col_edges[self.cols[order], np.arange(E) - cstart[self.cols[order]]] = order


def relay_mirror(H, priors, syndromes, cfg: RelayConfig, gammas=None, ms_scaling_factor=1.0, marginals=False, trace=None):
    """The definition in the module docstring, float32 numpy, vectorised over shots and edges; the sequential adds are a loop over the
    column weight.  Returns (errors uint8 [B, n], solved bool [B], iterations int32 [B], leg_of_output int32 [B], candidates int32 [B]):
    `solved` = a candidate was found (or the syndrome was zero: zero correction, no iteration, no candidate), `iterations` the total over
    all legs, `leg_of_output` the leg of the returned candidate (the last leg run where there is none).  marginals=True appends the final
    M (float32 [B, n]); `trace`, a dict, receives "nu_zero" and "nu_neg_zero": how many fault->check messages equal to +-0, and to -0, the run saw."""
    G = _Graph(H)
    m, n, E = G.m, G.n, G.E
    llr0 = prior_llr32(np.broadcast_to(np.asarray(priors, dtype=np.float64), (n,)))
    gam = check_table(gammas, cfg, n)
    check_gamma(cfg.gamma0, "gamma0")
    syn = (np.asarray(syndromes).reshape(-1, m) & 1).astype(np.uint8)
    B = syn.shape[0]
    w = candidate_weights(llr0)
    alpha_fixed = np.float32(ms_scaling_factor)
    one = np.float32(1.0)

    M = np.broadcast_to(llr0, (B, n)).copy()
    errors = np.zeros((B, n), dtype=np.uint8)
    solved = np.zeros(B, dtype=bool)
    iters = np.zeros(B, dtype=np.int32)
    leg_out = np.zeros(B, dtype=np.int32)
    ncand = np.zeros(B, dtype=np.int32)
    best_w = np.full(B, np.iinfo(np.int64).max, dtype=np.int64)
    done = ~syn.any(axis=1)
    solved[done] = True
    nu_zero = nu_neg_zero = 0

    for leg in range(cfg.num_sets + 1):
        idx = np.flatnonzero(~done)
        if idx.size == 0:
            break
        g = np.full(n, cfg.gamma0, dtype=np.float32) if leg == 0 else gam[leg - 1]
        a = (one - g) * llr0
        Ml, sl = M[idx], syn[idx]
        mu = np.zeros((idx.size, E + 1), dtype=np.float32)
        mu[:, E] = -0.0                                           # the dummy edge: x + (-0) = x for every x
        for t in range(1, (cfg.pre_iter if leg == 0 else cfg.set_max_iter) + 1):
            alpha = alpha_fixed if alpha_fixed != 0 else np.float32(1.0 - 2.0 ** -t)
            lam = a + g * Ml
            P = lam.copy()
            for k in range(G.col_edges.shape[1]):
                P = P + mu[:, G.col_edges[:, k]]
            nu = np.empty_like(mu)
            nu[:, :E] = P[:, G.cols] - mu[:, :E]
            nu[:, E] = np.inf
            if trace is not None:
                nu_zero += int(np.count_nonzero(nu[:, :E] == 0))
                nu_neg_zero += int(np.count_nonzero((nu[:, :E] == 0) & np.signbit(nu[:, :E])))
            neg = nu <= 0
            A = np.abs(nu)[:, G.row_edges]                        # [shots, m, row weight]
            arg = A.argmin(axis=2)
            min1 = np.take_along_axis(A, arg[:, :, None], axis=2)[:, :, 0]
            np.put_along_axis(A, arg[:, :, None], np.inf, axis=2)
            min2 = A.min(axis=2)
            min1, min2 = np.minimum(min1, _FLT_MAX) * alpha, np.minimum(min2, _FLT_MAX) * alpha
            par = (neg[:, G.row_edges].sum(axis=2) + sl) & 1
            mag = np.where(arg[:, G.rows] == G.epos, min2[:, G.rows], min1[:, G.rows])
            sgn = (par[:, G.rows] ^ neg[:, :E]).astype(bool)
            mu[:, :E] = np.where(sgn, -mag, mag)
            Ml = lam
            for k in range(G.col_edges.shape[1]):
                Ml = Ml + mu[:, G.col_edges[:, k]]
            e = np.concatenate([(Ml <= 0).astype(np.uint8), np.zeros((idx.size, 1), dtype=np.uint8)], axis=1)
            ok = ((e[:, G.row_faults].sum(axis=2) & 1) == sl).all(axis=1)
            if ok.any():
                hit = idx[ok]
                M[hit] = Ml[ok]
                iters[hit] += t
                ncand[hit] += 1
                solved[hit] = True
                cw = (e[ok, :n].astype(np.int64) * w).sum(axis=1)
                better = cw < best_w[hit]
                errors[hit[better]] = e[ok, :n][better]
                best_w[hit[better]] = cw[better]
                leg_out[hit[better]] = leg
                done[hit[ncand[hit] >= cfg.stop_nconv]] = True
                keep = ~ok
                idx, Ml, sl, mu = idx[keep], Ml[keep], sl[keep], mu[keep]
                if idx.size == 0:
                    break
        if idx.size:
            M[idx] = Ml
            iters[idx] += cfg.pre_iter if leg == 0 else cfg.set_max_iter
    unsolved = ~solved
    errors[unsolved] = (M[unsolved] <= 0).astype(np.uint8)
    leg_out[unsolved] = cfg.num_sets
    if trace is not None:
        trace["nu_zero"], trace["nu_neg_zero"] = nu_zero, nu_neg_zero
    out = (errors, solved, iters, leg_out, ncand)
    return out + (M,) if marginals else out
