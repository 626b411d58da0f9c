"""Fit the priors of a detector error model to detector samples: the p_ij method of the repetition- and surface-code experiments, generalised to
hyperedges.  Every decoder here takes its priors from a circuit's noise arguments or from a .dem somebody else weighted; this module asks the
samples instead.  The model contributes its hyperedges (the columns of H) and nothing else: L and the model's own priors are carried along but
never enter the fit.

Host side, numpy only: the definition, `hyperedge_table`, the numpy mirror of the counting kernels (`parity_counts_mirror`; the kernels are
csrc/calibrate.hip) and the fit (`fit_priors`, one function for device counts and mirror counts alike); then `ParityCounter`, the device
class, and `estimate_priors`.  The text below is the definition: the device must produce the mirror's integers bit for bit.

The model.  Independent mechanisms e_j, mechanism j flipping the detector set e_j with probability p_j.  The e_j are the columns of H: distinct,
non-empty, sorted ascending, s_j = |e_j| <= 10 (NotImplementedError beyond, naming the column and its weight, before any launch).

Why it inverts.  Write z_d = 1 - 2 x_d = +-1 for detector d of a shot.  A set T of detectors has prod_{d in T} z_d = prod_e (-1)^{f_e |e & T|},
f_e = 1 iff e fired; the mechanisms are independent and <(-1)^{f_e}> = 1 - 2 p_e, so <prod_{d in T} z_d> = prod_{e : |e & T| odd} (1 - 2 p_e).  With
lambda_e = -ln(1 - 2 p_e) that is -ln <prod_T z> = sum_e lambda_e [|e & T| odd].  Now fix a column e_j of size s and sum over its non-empty subsets
T with the sign (-1)^{|T| + 1}: mechanism e meets e_j in a = e & e_j, and sum_{T != 0} (-1)^{|T| + 1} [|a & T| odd] counts, over the choices of
T & a (odd size k, sign carried by |T| = k + |T - a|) and of T - a, sum_{k odd} C(|a|, k) * sum_{U subset of e_j - a} (-1)^{k + |U| + 1}.  The inner sum
over U is 0 unless e_j - a is empty, i.e. a = e_j, i.e. e contains e_j; then it is sum_{k odd} C(s, k) = 2^(s - 1).  So
    Lambda_j := 2^-(s - 1) sum_{T != 0} (-1)^{|T| + 1} (-ln <prod_T z>) = sum_{i : e_i contains e_j} lambda_i,
exactly the hyperedges that contain e_j, and the system is triangular in descending weight.

  counts       for column j and mask t = 1 .. 2^s_j - 1, bit i of t stands for the i-th smallest detector of e_j; c[k][j][t] = the number of shots
               of block k in which the XOR of the selected detectors is 1.  Stored flat, int64 [K, total], total = sum_j (2^s_j - 1); column j starts
               at ptr[j] and t - 1 indexes inside it.  Block k of N shots holds the shot indices [floor(k N / K), floor((k + 1) N / K)); K
               defaults to 16 and is capped at N.
  fit          float64.  c = sum_k c[k], z_{j,t} = 1 - 2 c[j][t] / N; Lambda_j as above, summed with t ascending;
               lambda_j = Lambda_j - sum_{i : e_i strictly contains e_j} lambda_i, columns in descending weight, supersets in ascending index;
               raw[j] = (1 - e^-lambda_j) / 2.
  clipping     priors[j] = raw[j] clipped to [min_prior, 1/2 - min_prior], min_prior = 0.5 / N by default ("half a count"); `clipped` lists the
               columns it changed.
  unidentified a column with a moment z <= 0, or with a proper superset that has one, keeps the model's prior, is listed in `unidentified`, and
               contributes its model lambda to its subsets.
  stderr       the delete-one-block jackknife: stderr[j] = sqrt((K - 1) / K * sum_k (r_j^(-k) - mean_k r_j^(-k))^2), r^(-k) the raw fit of the
               counts without block k on N - N_k shots.  (The naive sqrt(p / N) is wrong by a factor of about two: the estimate is a difference
               of logarithms of correlated moments.)  nan for K = 1.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import time

import numpy as np

MAX_WEIGHT = 10                         # QD_CALIB_MAX_WEIGHT
DEFAULT_BLOCKS = 16
DEFAULT_BATCH = 1 << 16


@dataclasses.dataclass
class HyperedgeTable:
    """ndet, n; col_ptr int64 [n + 1], col_det int32: the detectors of every column, ascending; weight int64 [n]; ptr int64 [n + 1]: the first
    counter of every column, total = ptr[n]; sup_ptr int64 [n + 1], sup_idx int64: the proper supersets of every column among the columns, in
    ascending index; H, L: the matrices the table was made from (L may be None)."""
    ndet: int
    n: int
    col_ptr: np.ndarray
    col_det: np.ndarray
    weight: np.ndarray
    ptr: np.ndarray
    total: int
    sup_ptr: np.ndarray
    sup_idx: np.ndarray
    H: object = None
    L: object = None

    def detectors(self, j):
        return self.col_det[self.col_ptr[j]:self.col_ptr[j + 1]]

    def supersets(self, j):
        return self.sup_idx[self.sup_ptr[j]:self.sup_ptr[j + 1]]


def hyperedge_table(H, L=None) -> HyperedgeTable:
    """The tables of the module docstring from a check matrix (detectors x columns).  ValueError for an empty column or two equal ones;
    NotImplementedError for a column of more than 10 detectors."""
    from scipy.sparse import csc_matrix
    Hc = csc_matrix(H).copy()
    Hc.sum_duplicates()
    Hc.data = (Hc.data % 2).astype(np.uint8)
    Hc.eliminate_zeros()
    Hc.sort_indices()
    ndet, n = Hc.shape
    col_ptr, col_det = Hc.indptr.astype(np.int64), Hc.indices.astype(np.int32)
    weight = np.diff(col_ptr)
    if n and weight.min() < 1:
        raise ValueError("column %d flips no detector: the samples say nothing about it" % int(np.argmin(weight)))
    if n and weight.max() > MAX_WEIGHT:
        j = int(np.argmax(weight > MAX_WEIGHT))
        raise NotImplementedError("column %d has weight %d: the fit counts the subsets of at most %d detectors a column" % (j, int(weight[j]), MAX_WEIGHT))
    sets = [tuple(int(d) for d in col_det[col_ptr[j]:col_ptr[j + 1]]) for j in range(n)]
    index = {}
    for j, e in enumerate(sets):
        if index.setdefault(e, j) != j:
            raise ValueError("columns %d and %d flip the same detectors: merge them (detector_error_model_to_matrix does)" % (index[e], j))
    sup = [[] for _ in range(n)]
    bits = [[i for i in range(MAX_WEIGHT) if (t >> i) & 1] for t in range(1 << MAX_WEIGHT)]
    for i, e in enumerate(sets):                         # i ascending: every list comes out in ascending index
        for t in range(1, (1 << len(e)) - 1):
            j = index.get(tuple(e[b] for b in bits[t]))
            if j is not None:
                sup[j].append(i)
    sup_ptr = np.zeros(n + 1, np.int64)
    sup_ptr[1:] = np.cumsum([len(s) for s in sup])
    sup_idx = np.array([i for s in sup for i in s], dtype=np.int64)
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum((np.int64(1) << weight) - 1)
    return HyperedgeTable(int(ndet), int(n), col_ptr, col_det, weight.astype(np.int64), ptr, int(ptr[n]), sup_ptr, sup_idx, Hc, None if L is None else csc_matrix(L))


def block_edges(shots, blocks=DEFAULT_BLOCKS) -> np.ndarray:
    """int64 [K + 1]: block k holds the shots [edges[k], edges[k + 1]), K = min(blocks, shots)."""
    shots, blocks = int(shots), int(blocks)
    if shots < 1:
        raise ValueError("there are no shots to fit")
    if blocks < 1:
        raise ValueError("blocks must be at least 1")
    K = min(blocks, shots)
    return np.array([k * shots // K for k in range(K + 1)], dtype=np.int64)


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------------
def _popcount_rows(x) -> np.ndarray:
    """Set bits of every row of a uint64 array."""
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x).sum(axis=1, dtype=np.int64)
    return _POP8[x.view(np.uint8)].sum(axis=1, dtype=np.int64)


_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def bit_planes_mirror(samples) -> np.ndarray:
    """uint64 [ndet, ceil(B / 64)]: bit b & 63 of word b >> 6 of plane d is the low bit of samples[b, d]; pad bits zero (qd_bit_planes)."""
    a = np.asarray(samples)
    a = a.view(np.uint8) if a.dtype == np.bool_ else (a & 1).astype(np.uint8)
    B, ndet = a.shape
    W = (B + 63) // 64
    packed = np.zeros((ndet, 8 * W), np.uint8)
    if B:
        packed[:, :(B + 7) // 8] = np.packbits(a.T, axis=1, bitorder="little")
    return packed.view("<u8").astype(np.uint64)


def _count_planes(planes, table, out):
    """out[ptr[j] + t - 1] += the shots whose detectors t of column j XOR to 1, from bit planes; the Gray-code walk of the kernel."""
    for s in np.unique(table.weight):
        cols = np.flatnonzero(table.weight == s)
        dets = table.col_det[table.col_ptr[cols][:, None] + np.arange(int(s))[None, :]]
        for c0 in range(0, len(cols), 4096):
            cc, dd = cols[c0:c0 + 4096], dets[c0:c0 + 4096]
            x = np.zeros((len(cc), planes.shape[1]), np.uint64)
            for k in range(1, 1 << int(s)):
                x ^= planes[dd[:, (k & -k).bit_length() - 1]]
                out[table.ptr[cc] + (k ^ (k >> 1)) - 1] += _popcount_rows(x)


def parity_counts_mirror(samples, table, blocks=DEFAULT_BLOCKS):
    """The counts of the module docstring in numpy: (counts int64 [K, total], block_shots int64 [K]).  samples: [N, ndet], bool or integer
    (the low bit counts).  The CPU reference of the kernels."""
    a = np.asarray(samples)
    if a.ndim != 2 or a.shape[1] != table.ndet:
        raise ValueError("samples must be [shots, %d], not %s" % (table.ndet, a.shape))
    edges = block_edges(a.shape[0], blocks)
    counts = np.zeros((len(edges) - 1, table.total), np.int64)
    for k in range(len(edges) - 1):
        _count_planes(bit_planes_mirror(a[edges[k]:edges[k + 1]]), table, counts[k])
    return counts, np.diff(edges)


# ---- the fit ------------------------------------------------------------------------------------------------------------------------------
def fit_moments(z, table, model_priors):
    """The fit of the module docstring from the moments z [total] (float64): (raw float64 [n], unidentified bool [n])."""
    z = np.asarray(z, dtype=np.float64)
    model_lam = -np.log1p(-2.0 * np.asarray(model_priors, dtype=np.float64))
    n = table.n
    Lam = np.zeros(n)
    bad = np.zeros(n, bool)
    for s in np.unique(table.weight):
        cols = np.flatnonzero(table.weight == s)
        acc = np.zeros(len(cols))
        for t in range(1, 1 << int(s)):                  # t ascending
            zt = z[table.ptr[cols] + t - 1]
            ok = zt > 0.0
            bad[cols[~ok]] = True
            term = -np.log(np.where(ok, zt, 1.0))
            acc = acc + term if bin(t).count("1") & 1 else acc - term
        Lam[cols] = acc / float(1 << (int(s) - 1))
    unid = bad.copy()
    for j in np.flatnonzero(np.diff(table.sup_ptr)):
        if bad[table.supersets(j)].any():
            unid[j] = True
    lam = np.zeros(n)
    for s in sorted((int(w) for w in np.unique(table.weight)), reverse=True):
        for j in np.flatnonzero(table.weight == s):
            if unid[j]:
                lam[j] = model_lam[j]
                continue
            above = 0.0
            for v in lam[table.supersets(j)].tolist():   # ascending index
                above += v
            lam[j] = Lam[j] - above
    return -np.expm1(-lam) / 2.0, unid


def model_dem_text(table: HyperedgeTable, priors, digits: int = 17) -> str:
    """The table's detector sets and observables with the given priors, as .dem text (dem_to_text): one error per column, in column order."""
    from .dem import DetectorErrorModel, dem_to_text
    from scipy.sparse import csc_matrix
    nobs = 0 if table.L is None else table.L.shape[0]
    Lc = csc_matrix((nobs, table.n), dtype=np.uint8) if table.L is None else csc_matrix(table.L)
    Lc.sort_indices()
    errors = [(float(priors[j]), tuple(int(d) for d in table.detectors(j)),
               tuple(int(o) for o, v in zip(Lc.indices[Lc.indptr[j]:Lc.indptr[j + 1]], Lc.data[Lc.indptr[j]:Lc.indptr[j + 1]]) if int(v) % 2))
              for j in range(table.n)]
    return dem_to_text(DetectorErrorModel(errors, table.ndet, nobs), digits)


@dataclasses.dataclass
class CalibrationResult:
    """What a fit returns.  priors: the fitted priors, clipped, an unidentified column keeping the model's; raw: before clipping; stderr: the
    jackknife standard error of raw; clipped, unidentified: int64 column indices, ascending; shots; counts: int64 [K, total], the sufficient
    statistic (module docstring); block_shots int64 [K]; table: the HyperedgeTable; model_priors; seconds."""
    priors: np.ndarray
    raw: np.ndarray
    stderr: np.ndarray
    clipped: np.ndarray
    unidentified: np.ndarray
    shots: int
    counts: np.ndarray
    block_shots: np.ndarray
    table: HyperedgeTable
    model_priors: np.ndarray
    seconds: float = 0.0

    def matrices(self):
        """(H, L, priors): what detector_error_model_to_matrix returns for the fitted model."""
        if self.table.L is None:
            raise ValueError("the table was made without an observable matrix")
        return self.table.H.copy(), self.table.L.copy(), self.priors.copy()

    def dem_text(self, digits: int = 17) -> str:
        """The model's detector sets and observables with the fitted priors, as .dem text: what every decoder here takes in place of a circuit."""
        return model_dem_text(self.table, self.priors, digits)

    def to_json(self) -> dict:
        rel = self.stderr / self.priors
        rel = rel[np.isfinite(rel)]
        return {"shots": int(self.shots), "columns": int(self.table.n), "clipped": int(len(self.clipped)), "unidentified": int(len(self.unidentified)),
                "median_rel_stderr": float(np.median(rel)) if len(rel) else None, "max_rel_stderr": float(rel.max()) if len(rel) else None,
                "seconds": float(self.seconds)}


def fit_priors(counts, block_shots, table, model_priors, min_prior=None) -> CalibrationResult:
    """The fit, the clipping and the jackknife of the module docstring from counts [K, total] (int64; real-valued counts are taken as they
    are) and the shots of every block.  One function for the device's counts and the mirror's."""
    t0 = time.perf_counter()
    counts = np.asarray(counts)
    if counts.ndim == 1:
        counts = counts[None, :]
    block_shots = np.asarray(block_shots, dtype=np.int64).reshape(-1)
    model_priors = np.asarray(model_priors, dtype=np.float64)
    K = counts.shape[0]
    if counts.shape != (K, table.total) or block_shots.shape != (K,) or model_priors.shape != (table.n,):
        raise ValueError("counts must be [K, %d], block_shots [K] and model_priors [%d]" % (table.total, table.n))
    N = int(block_shots.sum())
    if N < 1 or (block_shots < 0).any():
        raise ValueError("there are no shots to fit")
    min_prior = 0.5 / N if min_prior is None else float(min_prior)
    if not 0.0 <= min_prior < 0.25:
        raise ValueError("min_prior must lie in [0, 1/4)")
    c = counts.sum(axis=0)
    raw, unid = fit_moments(1.0 - 2.0 * c / N, table, model_priors)
    priors = np.clip(raw, min_prior, 0.5 - min_prior)
    clipped = np.flatnonzero((priors != raw) & ~unid)
    priors[unid] = model_priors[unid]
    stderr = np.full(table.n, np.nan)
    if K > 1:
        reps = np.stack([fit_moments(1.0 - 2.0 * (c - counts[k]) / (N - int(block_shots[k])), table, model_priors)[0] for k in range(K)])
        stderr = np.sqrt((K - 1) / K * ((reps - reps.mean(axis=0)) ** 2).sum(axis=0))
    return CalibrationResult(priors, raw, stderr, clipped.astype(np.int64), np.flatnonzero(unid).astype(np.int64), N, counts, block_shots, table,
                             model_priors, time.perf_counter() - t0)


# ---- the device ---------------------------------------------------------------------------------------------------------------------------
class ParityCounter:
    """The counting pass on the device (csrc/calibrate.hip): the column table is checked and uploaded here, before any launch; `add` turns a
    batch of detector rows into bit planes and adds its counts to one row of counters."""

    def __init__(self, table: HyperedgeTable, device=None):
        from . import _lib
        import torch
        self.L = _lib.require_calibrate(_lib.require_gpu())
        self.table = table
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.h = C.c_void_p()
        cp = np.ascontiguousarray(table.col_ptr, dtype=np.int64)
        cd = np.ascontiguousarray(table.col_det, dtype=np.int32)
        rc = self.L.qd_calib_create(table.ndet, table.n, cp.ctypes.data, cd.ctypes.data, self.device, C.byref(self.h))
        if rc == _lib.QD_ECAPACITY:
            raise NotImplementedError("quits_amd: prior fit: " + self.L.qd_last_error().decode(errors="replace"))
        _lib.check(rc)
        info = np.zeros(4, np.int64)
        _lib.check(self.L.qd_calib_info(self.h, info.ctypes.data))
        assert int(info[0]) == table.total, (int(info[0]), table.total)
        self.tasks = int(info[1])
        self._planes = None

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.qd_calib_destroy(self.h)
            self.h = C.c_void_p()
        self._planes = None

    __del__ = close

    def planes(self, det, out=None):
        """uint64 planes [ndet, ceil(B / 64)] (an int64 cuda tensor) of a cuda uint8 tensor [B, ndet] (unit stride inside a row)."""
        from . import _lib
        from .samples import _stream_ptr
        import torch
        assert det.is_cuda and det.dtype == torch.uint8 and det.dim() == 2 and (det.shape[1] <= 1 or det.stride(1) == 1)
        B, ndet = det.shape
        W = (B + 63) // 64
        if out is None:
            out = torch.empty((ndet, max(W, 1)), dtype=torch.int64, device=det.device)
        assert out.is_cuda and out.dtype == torch.int64 and out.dim() == 2 and out.shape[0] >= ndet and out.stride(0) >= W and (out.shape[1] <= 1 or out.stride(1) == 1)
        stride = det.stride(0) if B > 1 else max(det.stride(0), ndet)
        _lib.check(self.L.qd_bit_planes(C.c_void_p(det.data_ptr()), stride, ndet, B, C.c_void_p(out.data_ptr()), out.stride(0), _stream_ptr()))
        return out

    def count_planes(self, planes, nwords, row):
        """row (int64 cuda tensor [total]) += the counts of the first nwords words of the planes."""
        from . import _lib
        from .samples import _stream_ptr
        import torch
        assert planes.is_cuda and planes.dtype == torch.int64 and planes.dim() == 2 and planes.shape[0] >= self.table.ndet and planes.stride(0) >= nwords
        assert row.is_cuda and row.dtype == torch.int64 and row.dim() == 1 and row.shape[0] == self.table.total and (row.shape[0] <= 1 or row.stride(0) == 1)
        _lib.check(self.L.qd_parity_counts(self.h, C.c_void_p(planes.data_ptr()), planes.stride(0), int(nwords), C.c_void_p(row.data_ptr()), _stream_ptr()))

    def add(self, det, row):
        """row += the counts of the shots of `det` (cuda uint8 [B, ndet]); the planes buffer is kept between calls."""
        import torch
        B = det.shape[0]
        if det.shape[1] != self.table.ndet:
            raise ValueError("samples are %d detectors wide, the model has %d" % (det.shape[1], self.table.ndet))
        W = (B + 63) // 64
        if self._planes is None or self._planes.shape[1] < W or self._planes.device != det.device:
            self._planes = torch.empty((self.table.ndet, max(W, 1)), dtype=torch.int64, device=det.device)
        self.count_planes(self.planes(det, self._planes), W, row)


def _model(model):
    """(H, L, priors) from an (H, L) pair, an (H, L, priors) triple, circuit text, a Circuit, .dem text or a DEM."""
    from scipy.sparse import csc_matrix
    if isinstance(model, (tuple, list)) and len(model) in (2, 3):
        H, L = csc_matrix(model[0]), csc_matrix(model[1])
        priors = np.full(H.shape[1], np.nan) if len(model) == 2 else np.asarray(model[2], dtype=np.float64)
    else:
        from .decoder.base import detector_error_model_to_matrix
        H, L, priors = detector_error_model_to_matrix(model)
        H, L = csc_matrix(H), csc_matrix(L)
    if H.shape[1] != L.shape[1] or priors.shape != (H.shape[1],):
        raise ValueError("H has %d columns, L %d and there are %d priors: one of each per fault" % (H.shape[1], L.shape[1], priors.shape[0]))
    return H, L, priors


def _device_rows(samples, lo, hi):
    """Shots lo .. hi - 1 of any accepted form of samples as a cuda uint8 tensor [hi - lo, ndet]."""
    import torch
    from .samples import PackedSamples, unpack_b8_into
    if isinstance(samples, PackedSamples):
        data = samples.data[lo:hi]
        if not samples.is_cuda:
            b0, b1 = samples.bit0 >> 3, (samples.bit0 + samples.num_bits + 7) >> 3
            data = torch.from_numpy(np.ascontiguousarray(data[:, b0:b1])).to("cuda")
            bit0 = samples.bit0 & 7
        else:
            bit0 = samples.bit0
        out = torch.empty((hi - lo, samples.num_bits), dtype=torch.uint8, device=data.device)
        return unpack_b8_into(data, bit0, samples.num_bits, out) if out.numel() else out
    if isinstance(samples, torch.Tensor):
        t = samples[lo:hi]
        t = t.to("cuda") if not t.is_cuda else t
        t = t.to(torch.uint8) if t.dtype != torch.uint8 else t
        return t if t.shape[1] <= 1 or t.stride(1) == 1 else t.contiguous()
    a = np.asarray(samples[lo:hi])
    a = a.view(np.uint8) if a.dtype == np.bool_ else a.astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def estimate_priors(model, samples=None, *, shots=None, seed=0, sampler="dem", blocks=DEFAULT_BLOCKS, batch=None, min_prior=None) -> CalibrationResult:
    """Fit the priors of `model`'s hyperedges to detector samples, counting on the device.  model: circuit text, a Circuit, .dem text, a DEM,
    or an (H, L, priors) triple ((H, L): the model priors are nan, so an unidentified column has none to keep).  samples: a numpy bool / integer
    array [N, ndet], a cuda uint8 tensor or PackedSamples (host or device; `.field()` offsets honoured).  samples=None draws `shots` shots of
    `seed`'s stream from the model itself, batch after batch on the device -- sampler='dem': DemSampler on the model's own priors,
    'circuit': CircuitSampler on the circuit (the model must be one) -- and no host array per shot is made.  The shots are cut into `blocks`
    jackknife blocks (module docstring) and every block into batches of at most `batch` shots (default 65536): a batch never straddles a block
    edge, and the counts do not depend on it.  ValueError: a width mismatch or zero shots.  There is no CPU fall-back: without the library or
    a device this raises; `parity_counts_mirror` + `fit_priors` is the CPU path, called by name."""
    t0 = time.perf_counter()
    H, L, priors = _model(model)
    table = hyperedge_table(H, L)
    if sampler not in ("dem", "circuit"):
        raise ValueError("sampler must be 'dem' or 'circuit'")
    if samples is None:
        if shots is None:
            raise ValueError("give samples, or shots to draw from the model")
        N = int(shots)
    else:
        if getattr(samples, "ndim", 0) != 2:
            raise ValueError("samples must be [shots, detectors]")
        N = int(samples.shape[0])
        if int(samples.shape[1]) != table.ndet:
            raise ValueError("samples are %d detectors wide, the model has %d" % (int(samples.shape[1]), table.ndet))
    edges = block_edges(N, blocks)
    batch = DEFAULT_BATCH if batch is None else int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    import torch
    counter = ParityCounter(table)
    try:
        draw = None
        if samples is None:
            if sampler == "circuit":
                from .decoder.device import CircuitSampler
                from .dem import Circuit
                if not isinstance(model, str):
                    raise ValueError("sampler='circuit' needs a circuit, not matrices or a DEM")
                draw = CircuitSampler(model if isinstance(model, Circuit) else Circuit(model))
            else:
                from .decoder.device import DemSampler
                draw = DemSampler(H, L, priors)
            if draw.m != table.ndet:
                raise ValueError("the sampler draws %d detectors, the model has %d" % (draw.m, table.ndet))
        counts = torch.zeros((len(edges) - 1, table.total), dtype=torch.int64, device="cuda")
        for k in range(len(edges) - 1):
            for lo in range(int(edges[k]), int(edges[k + 1]), batch):
                hi = min(lo + batch, int(edges[k + 1]))
                det = draw.sample(hi - lo, seed, lo)[0] if draw is not None else _device_rows(samples, lo, hi)
                counter.add(det, counts[k])
        torch.cuda.synchronize()
        host = counts.cpu().numpy()
    finally:
        counter.close()
    res = fit_priors(host, np.diff(edges), table, priors, min_prior)
    res.seconds = time.perf_counter() - t0
    return res


def estimate_priors_mirror(model, samples, blocks=DEFAULT_BLOCKS, min_prior=None) -> CalibrationResult:
    """`estimate_priors` on the CPU through `parity_counts_mirror`: for tests and small inputs, called by name."""
    t0 = time.perf_counter()
    H, L, priors = _model(model)
    table = hyperedge_table(H, L)
    from .samples import PackedSamples
    a = np.asarray(samples.cpu()) if isinstance(samples, PackedSamples) else np.asarray(samples)
    if a.ndim != 2 or a.shape[1] != table.ndet:
        raise ValueError("samples are %s, the model has %d detectors" % (a.shape, table.ndet))
    counts, block_shots = parity_counts_mirror(a, table, blocks)
    res = fit_priors(counts, block_shots, table, priors, min_prior)
    res.seconds = time.perf_counter() - t0
    return res
