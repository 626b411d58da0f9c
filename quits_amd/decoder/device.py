"""Thin Python objects over the C ABI (include/quits_amd.h): device-resident window graphs, batch decoders and
GF(2) matrices.  PyTorch is used for device memory and streams only."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .. import _lib
from .base import as_csr_int32


def _torch():
    import torch
    return torch


def _stream_ptr():
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class _Handle:
    """Owner of one library object: `_h` is its handle, `_L` the library, `_destroy` the name of the function that frees it.  The object is
    freed with its owner; at interpreter shutdown, when the library may be gone first, a failing call is swallowed."""
    _destroy = None

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                getattr(self._L, self._destroy)(self._h)
            except Exception:
                pass
            self._h = None


def _seed64(seed):
    """A seed as the library takes it: any Python int, reduced mod 2^64."""
    return C.c_uint64(int(seed) & (2 ** 64 - 1))


def _sample_rows(shots, m, nobs):
    """(det uint8 [shots, m], obs uint8 [shots, nobs]) for a sampler to fill, on the current device."""
    torch = _torch()
    return torch.empty((shots, m), dtype=torch.uint8, device="cuda"), torch.empty((shots, nobs), dtype=torch.uint8, device="cuda")


def _fault_rows(fault_bits, shots, nfaults):
    """(fault_bits, its row stride): the caller's rows checked -- cuda int32 [shots, >= ceil(nfaults / 32)], unit stride inside a row -- or new
    rows of exactly that many words."""
    torch = _torch()
    words = (nfaults + 31) // 32
    if fault_bits is None:
        fault_bits = torch.empty((shots, words), dtype=torch.int32, device="cuda")
    assert fault_bits.is_cuda and fault_bits.dtype == torch.int32 and fault_bits.dim() == 2 and fault_bits.shape[0] == shots
    assert fault_bits.shape[1] >= words and (fault_bits.shape[1] <= 1 or fault_bits.stride(1) == 1)
    return fault_bits, fault_bits.stride(0) if shots > 1 else max(fault_bits.stride(0), fault_bits.shape[1])


def _check_mask(fail_mask, B):
    """The pointer of a fail mask over B shots: a contiguous cuda int64 tensor of at least ceil(B / 64) words."""
    torch = _torch()
    assert fail_mask.is_cuda and fail_mask.dtype == torch.int64 and fail_mask.dim() == 1 and fail_mask.is_contiguous()
    assert fail_mask.shape[0] >= (B + 63) // 64
    return _ptr(fail_mask)


class WindowGraph(_Handle):
    """Device copy of one window check matrix + priors (qd_graph).  Stands in for the sparse-matrix half of
    `BpOsdDecoder(pcm, channel_probs=...)` (reference sliding_window.py:149)."""
    _destroy = "qd_graph_destroy"

    def __init__(self, pcm, priors, device: Optional[int] = None):
        L = _lib.require_gpu()
        torch = _torch()
        self.device = torch.cuda.current_device() if device is None else int(device)
        rp, ci, (m, n) = as_csr_int32(pcm)
        pri = np.ascontiguousarray(np.broadcast_to(np.asarray(priors, dtype=np.float64), (n,)))
        self.m, self.n = int(m), int(n)
        self.words = (self.n + 31) // 32
        h = C.c_void_p()
        _lib.check(L.qd_graph_create(self.m, self.n, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                     pri.ctypes.data_as(C.c_void_p), self.device, C.byref(h)))
        self._h = h
        self._L = L
        self.priors = pri

    def info(self) -> dict:
        arr = (C.c_int32 * 14)()
        _lib.check(self._L.qd_graph_info_ex(self._h, arr, 14))
        keys = ("m", "n", "nnz", "max_row_weight", "max_col_weight", "bp_threads", "bp_lds_bytes", "osd_threads",
                "osd_lds_bytes", "rank", "scatter_walk_cycles", "scatter_walk_ideal", "scatter_threads", "scatter_checks_per_lane")
        return dict(zip(keys, [int(x) for x in arr]))


class BatchDecoder(_Handle):
    """qd_decoder: BP(+OSD-0) over a batch of shots for one window."""
    _destroy = "qd_decoder_destroy"

    def __init__(self, graph: WindowGraph, bp_method="minimum_sum", schedule="parallel", max_iter=0,
                 osd_method="osd_0", osd_order=0, ms_scaling_factor=1.0, edge_messages=False, raw_llr=False, off_chip=False):
        """bp_method 'minimum_sum' + schedule 'parallel' runs in the compressed LDS kernel; every other pair -- and that one
        too when `edge_messages` is set -- in the one-message-per-edge kernel (csrc/bp_general.hip).  `raw_llr` keeps the
        channel LLRs off the binary grid (QD_FLAG_RAW_LLR: round-1 float arithmetic, validation only).  `off_chip` decodes a window
        that fits the CU the way an off-chip window is decoded (QD_FLAG_OFF_CHIP: edge kernel with the exactness certificate,
        qd_osd0_offchip_kernel; validation only) -- a window that does not fit takes that path by itself."""
        self.graph = graph
        L = graph._L
        try:
            prm = _lib.QdParams(_lib.QD_BP[_norm(bp_method)], _lib.QD_SCHEDULE[_norm(schedule)], int(max_iter),
                                _lib.QD_OSD[_norm(osd_method)], int(osd_order), (1 if edge_messages else 0) | (2 if raw_llr else 0) | (4 if off_chip else 0),
                                float(ms_scaling_factor))
        except KeyError as exc:
            raise ValueError("unknown decoder option %s" % exc) from exc
        h = C.c_void_p()
        rc = L.qd_decoder_create(graph._h, C.byref(prm), C.byref(h))
        if rc == -2:
            raise NotImplementedError(L.qd_last_error().decode())
        _lib.check(rc)
        self._h = h
        self._L = L
        self.params = prm

    def info(self) -> dict:
        """Arithmetic of this decoder (qd_decoder_info): LLR grid bits (-1 = float LLRs as they are), coarse grid, kernel."""
        arr = (C.c_int32 * 4)()
        _lib.check(self._L.qd_decoder_info(self._h, arr))
        post = {0: "none", 1: "qd_osd0_sr_kernel", 2: "qd_osd0_reg_kernel", 3: "qd_osd0_reg_kernel<row form>", 4: "qd_osdcs_kernel",
                5: "qd_lsd0_kernel", 6: "qd_osd0_offchip_kernel"}.get(int(self._L.qd_decoder_postproc_kernel(self._h)), "?")
        fast = hasattr(self._L, "qd_decoder_fast_start") and int(self._L.qd_decoder_fast_start(self._h)) == 1
        return {"llr_grid_bits": int(arr[0]), "llr_coarse_bits": int(arr[1]), "edge_kernel": bool(arr[2]),
                "scatter_kernel": bool(arr[3]), "scatter_wide_kernel": int(arr[3]) == 2, "bp_fast_start": fast, "post_kernel": post}

    def set_workspace_limit(self, nbytes: int):
        """Cap the HBM message workspace of the one-message-per-edge BP kernel (product_sum / serial); no effect on the LDS kernel."""
        _lib.check(self._L.qd_decoder_set_workspace_limit(self._h, int(nbytes)))

    def release_workspace(self):
        """Give the device workspace back; the next decode sizes it again."""
        _lib.check(self._L.qd_decoder_release_workspace(self._h))

    def reserve(self, max_batch: int):
        _lib.check(self._L.qd_decoder_reserve(self._h, int(max_batch)))

    def decode(self, det, det_offset: int = 0, upd=None, err_bits=None, status=None, stage: int = 3, stream=None):
        """det: cuda uint8 [B, stride]; upd: cuda uint8 [B, rows] or None.
        stage 1 = BP only, 2 = OSD over the shots the preceding stage-1 call parked (same arguments), 3 = both.
        Returns (err_bits int32 [B, words], status int32 [B])."""
        torch = _torch()
        assert det.is_cuda and det.dtype == torch.uint8 and det.dim() == 2 and det.stride(1) == 1
        B = det.shape[0]
        g = self.graph
        if err_bits is None:
            err_bits = torch.empty((B, g.words), dtype=torch.int32, device=det.device)
        if status is None:
            status = torch.empty((B,), dtype=torch.int32, device=det.device)
        if upd is not None:
            assert upd.is_cuda and upd.dtype == torch.uint8 and upd.dim() == 2 and upd.stride(1) == 1
            up, us, ur = _ptr(upd), upd.stride(0), upd.shape[1]
        else:
            up, us, ur = C.c_void_p(0), 0, 0
        sp = _stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
        _lib.check(self._L.qd_decode_stage(self._h, _ptr(det), det.stride(0), int(det_offset), up, us, ur, B,
                                           _ptr(err_bits), _ptr(status), int(stage), sp))
        return err_bits, status

    def post_head_start(self, stream, microseconds: int = -1):
        """Two-stream drivers: behind a stage-1 call on `stream`, hold that stream briefly if this batch's post-processing is heavy (qd_decoder_post_head_start)."""
        _lib.check(self._L.qd_decoder_post_head_start(self._h, int(microseconds), C.c_void_p(stream.cuda_stream)))

    def osd0(self, det, llr, det_offset: int = 0, upd=None):
        """OSD-0 alone on caller-supplied posteriors llr: cuda float32 [B, n] (fault order).  Returns (err_bits, status)."""
        torch = _torch()
        assert det.is_cuda and det.dtype == torch.uint8 and det.dim() == 2 and det.stride(1) == 1
        assert llr.is_cuda and llr.dtype == torch.float32 and llr.shape == (det.shape[0], self.graph.n) and llr.is_contiguous()
        B = det.shape[0]
        err_bits = torch.empty((B, self.graph.words), dtype=torch.int32, device=det.device)
        status = torch.empty((B,), dtype=torch.int32, device=det.device)
        if upd is not None:
            up, us, ur = _ptr(upd), upd.stride(0), upd.shape[1]
        else:
            up, us, ur = C.c_void_p(0), 0, 0
        _lib.check(self._L.qd_osd0_batch(self._h, _ptr(det), det.stride(0), int(det_offset), up, us, ur, B, _ptr(llr),
                                         _ptr(err_bits), _ptr(status), _stream_ptr()))
        return err_bits, status

    def failed_llr(self, b: int):
        torch = _torch()
        out = torch.empty((self.graph.n,), dtype=torch.float32, device="cuda")
        _lib.check(self._L.qd_decoder_failed_llr(self._h, int(b), _ptr(out), _stream_ptr()))
        return out

    def debug_counters(self):
        arr = (C.c_uint64 * 16)()
        _lib.check(self._L.qd_decoder_debug_counters(self._h, arr))
        return [int(x) for x in arr]

    def set_profiling(self, on: bool):
        _lib.check(self._L.qd_decoder_set_profiling(self._h, 1 if on else 0))

    def profile(self, reset: bool = True) -> dict:
        arr = (C.c_double * 4)()
        _lib.check(self._L.qd_decoder_profile(self._h, arr, 1 if reset else 0))
        return {"bp_ms": arr[0], "osd_ms": arr[1], "bp_launches": int(arr[2]), "osd_launches": int(arr[3])}


class RelayBatchDecoder(BatchDecoder):
    """qd_decoder_create_relay: Relay-BP over a batch of shots for one window (csrc/bp_relay.hip; the definition is quits_amd/relay.py), then
    `osd_method`'s post-processor over the shots that found no candidate ("osd_off": they return their last hard decision).  `decode`,
    `info`, `profile` and the rest are BatchDecoder's.  `gammas`: float32 [cfg.num_sets, n] in fault order; None = relay_gammas(n, cfg).
    `marginals`: where the kernel keeps the marginals M_j -- "auto": in LDS wherever the whole state fits the CU, else in the decoder's
    device-memory workspace (4 bytes per fault and shot of a batch); "lds": in LDS or not at all (QdError -4 where that does not fit);
    "device": in the workspace even where LDS would do (QD_RELAY_FLAG_MARGINALS_DEVICE, validation).  Same results, bit for bit."""

    def __init__(self, graph: WindowGraph, cfg=None, osd_method="osd_off", osd_order=0, ms_scaling_factor=1.0, gammas=None, marginals="auto"):
        from .. import relay as _relay
        cfg = _relay.RelayConfig() if cfg is None else cfg
        if not isinstance(cfg, _relay.RelayConfig):
            raise TypeError("cfg must be a RelayConfig, not %r" % type(cfg).__name__)
        if _norm(marginals) not in ("auto", "lds", "device"):
            raise ValueError("marginals must be 'auto', 'lds' or 'device', not %r" % (marginals,))
        self.graph = graph
        self.cfg = cfg
        L = _lib.require_relay(graph._L)
        if _norm(marginals) != "auto":
            _lib.require_relay_forms(L)
        try:
            prm = _lib.QdParams(_lib.QD_BP["minimum_sum"], _lib.QD_SCHEDULE["parallel"], 0, _lib.QD_OSD[_norm(osd_method)], int(osd_order), 0,
                                float(ms_scaling_factor))
        except KeyError as exc:
            raise ValueError("unknown decoder option %s" % exc) from exc
        self.gammas = _relay.check_table(gammas, cfg, graph.n)
        rp = _lib.QdRelayParams(cfg.pre_iter, cfg.num_sets, cfg.set_max_iter, cfg.stop_nconv, float(cfg.gamma0),
                                _lib.RELAY_FLAG_MARGINALS_DEVICE if _norm(marginals) == "device" else 0)
        h = C.c_void_p()
        rc = L.qd_decoder_create_relay(graph._h, C.byref(prm), C.byref(rp), self.gammas.ctypes.data_as(C.c_void_p) if cfg.num_sets else C.c_void_p(0), C.byref(h))
        if rc == -2:
            raise NotImplementedError(L.qd_last_error().decode())
        _lib.check(rc)
        self._h = h
        self._L = L
        self.params = prm
        if _norm(marginals) == "lds" and self._relay_info()[0] != 1:
            # the library chose the device-memory form because the LDS form does not fit: with "lds" that is the capacity error
            _, used, lds_form, limit = self._relay_info()
            L.qd_decoder_destroy(self._h)
            self._h = None
            raise _lib.QdError(-4, "Relay-BP state of window %d x %d with the marginals in LDS (marginals='lds'): %d bytes of LDS, the CU has %d "
                                   "(%d bytes with the marginals in device memory: marginals='auto')" % (graph.m, graph.n, lds_form, limit, used))

    def _relay_info(self):
        if not hasattr(self._L, "qd_decoder_relay_info"):         # (a version 112 library named by QUITS_AMD_LIB: the LDS form is all it has)
            return [1, 0, 0, 0]
        arr = (C.c_int32 * 4)()
        _lib.check(self._L.qd_decoder_relay_info(self._h, arr))
        return [int(v) for v in arr]

    def info(self) -> dict:
        form, lds, _, _ = self._relay_info()
        return dict(super().info(), bp_kernel="qd_bp_relay_kernel", total_iter=self.cfg.total_iter, relay_marginals={1: "lds", 2: "device"}[form],
                    relay_lds_bytes=lds)


class GF2Matrix(_Handle):
    """Sparse GF(2) matrix on the device (qd_spmat), CSR."""
    _destroy = "qd_spmat_destroy"

    def __init__(self, mat, device: Optional[int] = None):
        L = _lib.require_gpu()
        torch = _torch()
        self.device = torch.cuda.current_device() if device is None else int(device)
        rp, ci, (r, c) = as_csr_int32(mat)
        self.shape = (int(r), int(c))
        h = C.c_void_p()
        _lib.check(L.qd_spmat_create(self.shape[0], self.shape[1], rp.ctypes.data_as(C.c_void_p),
                                     ci.ctypes.data_as(C.c_void_p), self.device, C.byref(h)))
        self._h = h
        self._L = L

    def xor_apply(self, err_bits, out, accumulate: bool, stream=None):
        """out[b, :nrows] (^)= A @ e_b mod 2, e_b = packed bits err_bits[b]."""
        sp = _stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
        _lib.check(self._L.qd_gf2_spmv_batch(self._h, _ptr(err_bits), err_bits.stride(0), err_bits.shape[0], _ptr(out),
                                             out.stride(0), 1 if accumulate else 0, sp))
        return out


def unpack_bits(bits, nbits: int):
    torch = _torch()
    L = _lib.load()
    out = torch.empty((bits.shape[0], nbits), dtype=torch.uint8, device=bits.device)
    _lib.check(L.qd_unpack_bits(_ptr(bits), bits.stride(0), int(nbits), bits.shape[0], _ptr(out), out.stride(0),
                                _stream_ptr()))
    return out


def count_mismatch(pred, obs) -> "object":
    """Device int64 scalar tensor: number of shots with pred != obs on any bit."""
    torch = _torch()
    L = _lib.load()
    assert pred.shape == obs.shape and pred.dtype == torch.uint8 and obs.dtype == torch.uint8
    pred = pred.contiguous()
    obs = obs.contiguous()
    cnt = torch.zeros((1,), dtype=torch.int64, device=pred.device)
    _lib.check(L.qd_count_mismatch(_ptr(pred), _ptr(obs), pred.shape[1], pred.shape[0], _ptr(cnt), _stream_ptr()))
    return cnt


def shot_flags_fold(status, flags):
    """flags[b] |= the QD_SHOT_* bits of one window's status words (qd_shot_flags_fold): _lib.SHOT_POST if the post-processor produced that
    window's output, SHOT_INCONSISTENT, SHOT_INEXACT, SHOT_COARSE.  status: cuda int32 [B], flags: cuda uint8 [B], both contiguous."""
    torch = _torch()
    L = _lib.require_experiment(_lib.load())
    assert status.is_cuda and status.dtype == torch.int32 and status.dim() == 1 and status.is_contiguous()
    assert flags.is_cuda and flags.dtype == torch.uint8 and flags.shape == status.shape and flags.is_contiguous()
    _lib.check(L.qd_shot_flags_fold(_ptr(status), status.shape[0], _ptr(flags), _stream_ptr()))
    return flags


class Tally:
    """Counters of a memory experiment, on the device (qd_tally_batch): shots, failing shots, both again per flag bit, mismatches per
    observable.  `add` accumulates and returns nothing to the host; `counts` does."""

    def __init__(self, k: int, device=None):
        torch = _torch()
        self._L = _lib.require_experiment(_lib.require_gpu())
        self.k = int(k)
        self.data = torch.zeros((_lib.TALLY_HEAD + self.k,), dtype=torch.int64, device="cuda" if device is None else device)

    def add(self, pred, obs, flags=None, fail_mask=None):
        """pred, obs: cuda uint8 [B, k] (row strides >= k: column slices are fine); flags: cuda uint8 [B] or None; fail_mask: cuda int64
        [>= ceil(B / 64)] or None -- written, not accumulated: bit l of word w is the fail bit of shot 64 w + l, zero past B."""
        torch = _torch()
        assert pred.is_cuda and obs.is_cuda and pred.dtype == torch.uint8 and obs.dtype == torch.uint8
        assert pred.dim() == 2 and pred.shape == obs.shape and pred.shape[1] == self.k
        B = pred.shape[0]
        if B == 0:
            return
        assert pred.stride(1) == 1 and obs.stride(1) == 1
        fp = mp = C.c_void_p(0)
        if flags is not None:
            assert flags.is_cuda and flags.dtype == torch.uint8 and flags.shape == (B,) and flags.is_contiguous()
            fp = _ptr(flags)
        if fail_mask is not None:
            mp = _check_mask(fail_mask, B)
        _lib.check(self._L.qd_tally_batch(_ptr(pred), pred.stride(0), _ptr(obs), obs.stride(0), self.k, B, fp, _ptr(self.data), mp, _stream_ptr()))

    def counts(self):
        """numpy int64 [10 + k] (synchronises): [0] shots, [1] failing shots, [2 + 2j], [3 + 2j] shots / failing shots with flag bit j,
        [10 + i] shots whose observable i mismatches."""
        return self.data.cpu().numpy()


def commit_bits(err_bits, nbits: int, out, out_bit0: int, stream=None):
    """Bits [out_bit0, out_bit0 + nbits) of every row of `out` = bits [0, nbits) of the same row of `err_bits` (qd_commit_bits); the other bits of
    `out` stay.  cuda int32 [B, words] tensors with unit stride inside a row.  Asynchronous on `stream` (default: the current one)."""
    torch = _torch()
    L = _lib.require_faults(_lib.load())
    assert err_bits.is_cuda and out.is_cuda and err_bits.dtype == torch.int32 and out.dtype == torch.int32
    assert err_bits.dim() == 2 and out.dim() == 2 and err_bits.shape[0] == out.shape[0]
    assert (err_bits.shape[1] <= 1 or err_bits.stride(1) == 1) and (out.shape[1] <= 1 or out.stride(1) == 1)
    B = out.shape[0]
    es = err_bits.stride(0) if B > 1 else max(err_bits.stride(0), err_bits.shape[1])
    os_ = out.stride(0) if B > 1 else max(out.stride(0), out.shape[1])
    if 32 * err_bits.shape[1] < nbits or 32 * out.shape[1] < out_bit0 + nbits:
        raise ValueError("rows of %d / %d words cannot hold %d bits / bits %d .. %d" % (err_bits.shape[1], out.shape[1], nbits, out_bit0, out_bit0 + nbits - 1))
    sp = _stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
    _lib.check(L.qd_commit_bits(_ptr(err_bits), es, int(nbits), B, _ptr(out), os_, int(out_bit0), sp))
    return out


class FaultStats:
    """Tallies of a memory experiment by fault weight, on the device (qd_fault_stats_batch): shots and failing shots by the number of sampled
    faults, the failing shots whose correction reproduces the syndrome by the weight of E xor C, the lightest of those and its shot.  `add`
    accumulates and returns nothing to the host; `result` does."""

    def __init__(self, device=None):
        torch = _torch()
        self._L = _lib.require_faults(_lib.require_gpu())
        dev = "cuda" if device is None else device
        self.hist = torch.zeros((3, _lib.FAULT_HIST), dtype=torch.int64, device=dev)
        self.counts = torch.zeros((4,), dtype=torch.int64, device=dev)
        self.best = torch.full((1,), -1, dtype=torch.int64, device=dev)          # all ones: no failing shot with a zero residual yet

    def add(self, faults, corr, nbits: int, residual, fail_mask, shot0: int = 0):
        """faults, corr: cuda int32 [B, words] of the same row stride, nbits bits each; residual: cuda uint8 [B, m] (H C xor det); fail_mask: cuda
        int64 [>= ceil(B / 64)], Tally.add's mask of the same batch; shot0: the global index of row 0."""
        torch = _torch()
        for t in (faults, corr):
            assert t.is_cuda and t.dtype == torch.int32 and t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1)
        B = faults.shape[0]
        assert corr.shape[0] == B and residual.shape[0] == B
        if B == 0:
            return
        stride = faults.stride(0) if B > 1 else min(faults.shape[1], corr.shape[1])
        assert B == 1 or corr.stride(0) == stride, "faults and corrections must share a row stride"
        assert 32 * min(faults.shape[1], corr.shape[1]) >= nbits
        assert residual.is_cuda and residual.dtype == torch.uint8 and residual.dim() == 2 and (residual.shape[1] <= 1 or residual.stride(1) == 1)
        mp = _check_mask(fail_mask, B)
        m = residual.shape[1]
        rs = residual.stride(0) if B > 1 else max(residual.stride(0), m)
        _lib.check(self._L.qd_fault_stats_batch(_ptr(faults), _ptr(corr), stride, int(nbits), _ptr(residual), rs, m, mp, B, int(shot0),
                                                _ptr(self.hist), _ptr(self.counts), _ptr(self.best), _stream_ptr()))

    def result(self):
        """(hist int64 [3, 256], counts int64 [4], lightest) on the host (synchronises); lightest = (weight, shot) or None."""
        best = int(self.best.cpu().numpy().view(np.uint64)[0])
        lightest = None if best == 2 ** 64 - 1 else (best >> 40, best & ((1 << 40) - 1))
        return self.hist.cpu().numpy(), self.counts.cpu().numpy(), lightest


def _check_soft(soft, B):
    torch = _torch()
    assert soft.is_cuda and soft.dtype == torch.int64 and soft.dim() == 2 and soft.shape[0] == B and soft.shape[1] >= _lib.SOFT_FIELDS
    assert B == 0 or soft.stride(1) == 1            # (an empty tensor's strides say nothing)
    return soft.stride(0) if B > 1 else max(soft.stride(0), soft.shape[1])


def soft_fold(status, soft, stream=None):
    """soft[b, 3:6] += (iterations, post-processed, bits 20 .. 31) of one window's status words (qd_soft_fold; quits_amd/soft.py).  status: cuda
    int32 [B], contiguous; soft: cuda int64 [B, >= 6] with unit stride inside a row, zeroed before the first window.  Asynchronous on `stream`."""
    torch = _torch()
    L = _lib.require_soft(_lib.load())
    assert status.is_cuda and status.dtype == torch.int32 and status.dim() == 1 and status.is_contiguous()
    B = status.shape[0]
    ss = _check_soft(soft, B)
    sp = _stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
    _lib.check(L.qd_soft_fold(_ptr(status), B, _ptr(soft), ss, sp))
    return soft


def soft_weigh(corr, nbits: int, weights, det, soft, stream=None):
    """soft[b, 0:3] = (sum of weights over the set bits of corr[b], their number, the detector bytes of det[b] with the low bit set)
    (qd_soft_weigh).  corr: cuda int32 [B, >= ceil(nbits / 32)]; weights: cuda int32 [nbits] (soft.fault_weights); det: cuda uint8 [B, m]; soft:
    cuda int64 [B, >= 6]; rows with unit stride inside.  Asynchronous on `stream` (default: the current one)."""
    torch = _torch()
    L = _lib.require_soft(_lib.load())
    assert corr.is_cuda and corr.dtype == torch.int32 and corr.dim() == 2 and det.is_cuda and det.dtype == torch.uint8 and det.dim() == 2
    assert corr.shape[0] == 0 or ((corr.shape[1] <= 1 or corr.stride(1) == 1) and (det.shape[1] <= 1 or det.stride(1) == 1))
    assert weights.is_cuda and weights.dtype == torch.int32 and weights.dim() == 1 and weights.is_contiguous() and weights.shape[0] >= nbits
    B, m = corr.shape[0], det.shape[1]
    assert det.shape[0] == B
    if 32 * corr.shape[1] < nbits:
        raise ValueError("rows of %d words cannot hold %d bits" % (corr.shape[1], nbits))
    ss = _check_soft(soft, B)
    if B == 0:
        return soft
    cs = corr.stride(0) if B > 1 else max(corr.stride(0), corr.shape[1])
    ds = det.stride(0) if B > 1 else max(det.stride(0), m)
    sp = _stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
    _lib.check(L.qd_soft_weigh(_ptr(corr), cs, int(nbits), _ptr(weights), _ptr(det), ds, m, B, _ptr(soft), ss, sp))
    return soft


def soft_tally(soft, shifts, fail_mask, hist, stream=None):
    """hist[f, 0, bin] += 1 for every row of `soft` and field f, hist[f, 1, bin] += 1 for the rows whose bit is set in fail_mask
    (qd_soft_tally; bin = soft.bin_of(value, shifts[f])).  soft: cuda int64 [B, >= 6]; shifts: six ints on the host; fail_mask: cuda int64
    [>= ceil(B / 64)] (Tally.add's) or None: plane 1 stays; hist: cuda int64 [6, 2, 1024], contiguous."""
    torch = _torch()
    L = _lib.require_soft(_lib.load())
    B = soft.shape[0]
    ss = _check_soft(soft, B)
    sh = np.ascontiguousarray(np.asarray(shifts, dtype=np.int32).reshape(-1))
    if sh.shape[0] != _lib.SOFT_FIELDS or sh.min() < 0 or sh.max() > 62:
        raise ValueError("shifts must be %d integers in 0 .. 62" % _lib.SOFT_FIELDS)
    assert hist.is_cuda and hist.dtype == torch.int64 and hist.shape == (_lib.SOFT_FIELDS, 2, _lib.SOFT_BINS) and hist.is_contiguous()
    mp = C.c_void_p(0)
    if fail_mask is not None:
        mp = _check_mask(fail_mask, B)
    sp = _stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
    _lib.check(L.qd_soft_tally(_ptr(soft), ss, B, sh.ctypes.data_as(C.c_void_p), mp, _ptr(hist), sp))
    return hist


class SoftTally:
    """Histograms of the soft records of a memory experiment, on the device (qd_soft_tally): per field, the shots and the failing shots by bin
    of width 2^shift.  `add` accumulates and returns nothing to the host; `result` does."""

    def __init__(self, shifts, device=None):
        torch = _torch()
        self._L = _lib.require_soft(_lib.require_gpu())
        self.shifts = np.ascontiguousarray(np.asarray(shifts, dtype=np.int32).reshape(-1))
        if self.shifts.shape[0] != _lib.SOFT_FIELDS or self.shifts.min() < 0 or self.shifts.max() > 62:
            raise ValueError("shifts must be %d integers in 0 .. 62" % _lib.SOFT_FIELDS)
        self.hist = torch.zeros((_lib.SOFT_FIELDS, 2, _lib.SOFT_BINS), dtype=torch.int64, device="cuda" if device is None else device)

    def add(self, soft, fail_mask=None):
        """soft: cuda int64 [B, >= 6]; fail_mask: Tally.add's mask of the same batch, or None (plane 1 is left alone)."""
        soft_tally(soft, self.shifts, fail_mask, self.hist)

    def result(self):
        """numpy int64 [6, 2, 1024] (synchronises)."""
        return self.hist.cpu().numpy()


class FaultShrinker:
    """The step of the fault-set shrinker on the device (qd_shrink_begin, qd_shrink_step; csrc/shrink.hip): quits_amd/shrink.py's walk, every
    live parent advancing one trial per round.  The decode is the caller's, so that any decoder -- or a scripted verdict -- drives it:

        shr.begin(packed_sets)
        while not shr.done:
            det, obs, fault, parent = shr.trials()          # cuda uint8 [A, m], uint8 [A, k], int32 [A], int32 [A]: row i = H (S \\ {j}), L (S \\ {j})
            shr.commit(fail_mask)                           # Tally.add's mask of those A rows: bit i = the decoder fails on row i
        res = shr.result()                                  # a quits_amd.shrink.ShrinkResult with packed sets, on the host

    Per round the host reads one number, the count of live parents, which sizes the next decode.  `sets`, `kept_det`, `kept_obs` are the
    current sets (cuda int32 [P, ceil(n / 32)]) and their H S and L S (cuda uint8), final once `done`."""

    def __init__(self, check_matrix, observable_matrix, device: Optional[int] = None):
        from scipy.sparse import csr_matrix
        H, Lm = csr_matrix(check_matrix), csr_matrix(observable_matrix)
        if H.shape[1] != Lm.shape[1]:
            raise ValueError("the check matrix has %d columns, the observable matrix %d" % (H.shape[1], Lm.shape[1]))
        self.H, self.L = GF2Matrix(H, device), GF2Matrix(Lm, device)
        self.Ht, self.Lt = GF2Matrix(H.T.tocsr(), device), GF2Matrix(Lm.T.tocsr(), device)
        self.m, self.n, self.k = int(H.shape[0]), int(H.shape[1]), int(Lm.shape[0])
        self.words = (self.n + 31) // 32
        self._L = _lib.require_shrink(self.Ht._L)
        self.P = self._A = 0
        self.rounds = 0
        self.sets = None

    def begin(self, packed_sets):
        """packed_sets: int32 [P, >= ceil(n / 32)] words, a cuda tensor or a host array; copied, the caller's rows stay as they are."""
        torch = _torch()
        if isinstance(packed_sets, torch.Tensor):
            t = packed_sets.to("cuda")
        else:
            t = torch.from_numpy(np.ascontiguousarray(packed_sets, dtype=np.int32)).to("cuda")
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] < self.words:
            raise ValueError("packed sets must be int32 [parents, >= %d] words" % self.words)
        self.sets = t[:, :self.words].clone().contiguous()
        P = self.P = int(t.shape[0])
        dev = self.sets.device
        self.state = torch.zeros((P, _lib.SHRINK_STATE), dtype=torch.int32, device=dev)
        self._live = [torch.empty((max(P, 1),), dtype=torch.int32, device=dev) for _ in range(2)]
        self._count = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.kept_det = torch.zeros((P, self.m), dtype=torch.uint8, device=dev)
        self.kept_obs = torch.zeros((P, self.k), dtype=torch.uint8, device=dev)
        self._det = torch.empty((P, self.m), dtype=torch.uint8, device=dev)
        self._obs = torch.empty((P, self.k), dtype=torch.uint8, device=dev)
        self._fault = torch.empty((max(P, 1),), dtype=torch.int32, device=dev)
        self._parent = torch.empty((max(P, 1),), dtype=torch.int32, device=dev)
        self.rounds = 0
        if P:
            self.H.xor_apply(self.sets, self.kept_det, accumulate=False)
            self.L.xor_apply(self.sets, self.kept_obs, accumulate=False)
            _lib.check(self._L.qd_shrink_begin(self.Ht._h, self.Lt._h, _ptr(self.sets), self.words, P, _ptr(self.state), _ptr(self._live[0]),
                                               _ptr(self._count), _ptr(self.kept_det), self.kept_det.stride(0), _ptr(self.kept_obs), self.kept_obs.stride(0),
                                               _ptr(self._det), self._det.stride(0), _ptr(self._obs), self._obs.stride(0), _ptr(self._fault),
                                               _ptr(self._parent), _stream_ptr()))
        self._A = P
        return self

    @property
    def done(self) -> bool:
        return self._A == 0

    @property
    def live(self) -> int:
        """The number of parents still walking = rows of the next `trials()`."""
        return self._A

    def trials(self):
        """(det uint8 [A, m], obs uint8 [A, k], fault int32 [A], parent int32 [A]) of this round, views into the shrinker's buffers: row i is the
        trial of parent[i] (ascending), the set without fault[i]; fault -1 is trial 0, the set itself."""
        A = self._A
        return self._det[:A], self._obs[:A], self._fault[:A], self._parent[:A]

    def commit(self, fail_mask):
        """The verdicts of this round's trials: a cuda int64 tensor of >= ceil(A / 64) words (Tally.add's fail mask of the A rows), or a bool
        sequence of length A.  Applies them, compacts the live list and emits the next round's trials; then reads the live count."""
        torch = _torch()
        A = self._A
        if A == 0:
            return 0
        if not (isinstance(fail_mask, torch.Tensor) and fail_mask.dtype == torch.int64):
            v = np.asarray(fail_mask.cpu().numpy() if isinstance(fail_mask, torch.Tensor) else fail_mask).astype(bool).reshape(-1)
            if v.shape[0] != A:
                raise ValueError("%d verdicts for %d trials" % (v.shape[0], A))
            pad = np.zeros(((A + 63) // 64) * 64, np.uint8)
            pad[:A] = v
            fail_mask = torch.from_numpy(np.packbits(pad, bitorder="little").view("<i8").copy()).to("cuda")
        _lib.check(self._L.qd_shrink_step(self.Ht._h, self.Lt._h, _ptr(self.sets), self.words, self.P, _ptr(self.state), _ptr(self._live[0]), A,
                                          _check_mask(fail_mask, A), _ptr(self._live[1]), _ptr(self._count), _ptr(self.kept_det), self.kept_det.stride(0),
                                          _ptr(self.kept_obs), self.kept_obs.stride(0), _ptr(self._det), self._det.stride(0), _ptr(self._obs),
                                          self._obs.stride(0), _ptr(self._fault), _ptr(self._parent), _stream_ptr()))
        self._live.reverse()
        self.rounds += 1
        self._A = int(self._count.cpu()[0])          # the round's one host read: it sizes the next decode
        return self._A

    def result(self):
        """quits_amd.shrink.ShrinkResult on the host (synchronises), `sets` as packed int32 [P, ceil(n / 32)] words."""
        from ..shrink import ShrinkResult
        if self.sets is None:
            raise RuntimeError("begin() has not been called")
        st = self.state.cpu().numpy().astype(np.int64)
        flags = st[:, 4]
        return ShrinkResult(self.sets.cpu().numpy(), (flags & _lib.SHRINK_FAILS) != 0, (flags & _lib.SHRINK_MINIMAL) != 0, st[:, 6].copy(),
                            st[:, 2].copy(), st[:, 3].copy())


def _shot_indices(indices):
    """int64 cuda tensor of shot indices from a tensor or any integer sequence."""
    torch = _torch()
    if isinstance(indices, torch.Tensor):
        if indices.dtype != torch.int64 or indices.dim() != 1:
            raise ValueError("shot indices must be a one-dimensional int64 tensor")
        idx = indices.to("cuda").contiguous()
    else:
        a = np.asarray(indices)
        if a.size and a.dtype.kind not in "iu":
            raise ValueError("shot indices must be integers")
        idx = torch.from_numpy(np.ascontiguousarray(a.reshape(-1).astype(np.int64))).to("cuda")
    if idx.numel() and int(idx.min()) < 0:
        raise ValueError("shot indices must not be negative")
    return idx


class DemSampler:
    """Device-side detector-error-model sampler (stands in for stim's detector sampler, simulation.py:23-27)."""

    def __init__(self, check_matrix, observable_matrix, priors, device: Optional[int] = None):
        from scipy.sparse import csr_matrix
        self.Ht = GF2Matrix(csr_matrix(check_matrix).T.tocsr(), device)
        self.Lt = GF2Matrix(csr_matrix(observable_matrix).T.tocsr(), device)
        self.m = self.Ht.shape[1]
        self.nobs = self.Lt.shape[1]
        self.priors = np.ascontiguousarray(priors, dtype=np.float64)
        assert self.priors.shape[0] == self.Ht.shape[0]

    def sample(self, shots: int, seed: int, shot0: int = 0):
        det, obs = _sample_rows(shots, self.m, self.nobs)
        L = self.Ht._L
        _lib.check(L.qd_sample_dem(self.Ht._h, self.Lt._h, self.priors.ctypes.data_as(C.c_void_p), _seed64(seed), int(shot0), int(shots), _ptr(det),
                                   det.stride(0), _ptr(obs), obs.stride(0), _stream_ptr()))
        return det, obs

    def sample_packed(self, shots: int, seed: int, shot0: int = 0):
        """`sample` bit-packed on the device (qd_pack_b8): (PackedSamples det, PackedSamples obs), CUDA tensors of ceil(m / 8) and
        ceil(nobs / 8) bytes per shot -- Stim's `sample(..., bit_packed=True, separate_observables=True)`."""
        from ..samples import PackedSamples
        det, obs = self.sample(shots, seed, shot0)
        return PackedSamples.pack(det), PackedSamples.pack(obs)

    def sample_shots(self, indices, seed: int):
        """Row b = shot indices[b] of this seed's stream (qd_sample_dem_shots): what `sample(1, seed, shot0=indices[b])` returns.  `indices`: an
        int64 cuda tensor or any integer sequence; any order, repeats allowed."""
        idx = _shot_indices(indices)
        n = idx.shape[0]
        det, obs = _sample_rows(n, self.m, self.nobs)
        L = _lib.require_experiment(self.Ht._L)
        _lib.check(L.qd_sample_dem_shots(self.Ht._h, self.Lt._h, self.priors.ctypes.data_as(C.c_void_p), _seed64(seed),
                                         _ptr(idx), n, _ptr(det), det.stride(0), _ptr(obs), obs.stride(0), _stream_ptr()))
        return det, obs


    @property
    def nfaults(self) -> int:
        return self.Ht.shape[0]

    def _sample_with_faults(self, idx, shots, seed, shot0, fault_bits):
        L = _lib.require_faults(self.Ht._L)
        det, obs = _sample_rows(shots, self.m, self.nobs)
        fault_bits, fs = _fault_rows(fault_bits, shots, self.nfaults)
        _lib.check(L.qd_sample_dem_faults(self.Ht._h, self.Lt._h, self.priors.ctypes.data_as(C.c_void_p), _seed64(seed),
                                          int(shot0), C.c_void_p(0) if idx is None else _ptr(idx), shots, _ptr(det), det.stride(0), _ptr(obs),
                                          obs.stride(0), _ptr(fault_bits), fs, _stream_ptr()))
        return det, obs, fault_bits

    def sample_faults(self, shots: int, seed: int, shot0: int = 0, fault_bits=None):
        """`sample` and which faults fired (qd_sample_dem_faults): (det, obs, fault_bits), fault_bits a cuda int32 [shots, ceil(n / 32)] tensor,
        bit j & 31 of word j >> 5 = fault j (a column of the check matrix) fired.  Same random stream: det and obs are `sample`'s.
        fault_bits: rows to write into instead (they may be wider; the words past ceil(n / 32) are left alone)."""
        return self._sample_with_faults(None, int(shots), seed, shot0, fault_bits)

    def sample_shots_faults(self, indices, seed: int, fault_bits=None):
        """`sample_shots` and which faults fired: row b is what `sample_faults(1, seed, shot0=indices[b])` returns."""
        idx = _shot_indices(indices)
        return self._sample_with_faults(idx, int(idx.shape[0]), seed, 0, fault_bits)


class StratifiedDemSampler(_Handle):
    """Device-side sampler of the detector error model conditioned on the number of faults (qd_sample_dem_strata): row b holds exactly ks[b]
    faults, drawn from the model's exact conditional law.  quits_amd/strata.py states the law, the random stream and the threshold table
    (computed here once, for 0 .. kmax faults, and kept in device memory); `pmf[k]` = P(|E| = k) and `tail` = P(|E| > kmax) weigh the strata.
    Returns what DemSampler.sample_faults returns."""
    _destroy = "qd_strata_destroy"

    def __init__(self, check_matrix, observable_matrix, priors, kmax: int, device: Optional[int] = None):
        from scipy.sparse import csr_matrix
        from .. import strata
        self.priors = np.ascontiguousarray(priors, dtype=np.float64)
        self.thresholds = strata.strata_thresholds(self.priors, kmax)            # (refuses priors outside [0, 1) and kmax > 255)
        self.kmax = int(kmax)
        self.pmf, self.tail = strata.fault_count_pmf(self.priors, self.kmax)
        self.Ht = GF2Matrix(csr_matrix(check_matrix).T.tocsr(), device)
        self.Lt = GF2Matrix(csr_matrix(observable_matrix).T.tocsr(), device)
        self.m = self.Ht.shape[1]
        self.nobs = self.Lt.shape[1]
        if self.priors.shape[0] != self.Ht.shape[0] or self.Lt.shape[0] != self.Ht.shape[0]:
            raise ValueError("%d priors, %d columns of the check matrix, %d of the observable matrix" % (self.priors.shape[0], self.Ht.shape[0], self.Lt.shape[0]))
        L = _lib.require_strata(_lib.require_faults(self.Ht._L))
        h = C.c_void_p()
        _lib.check(L.qd_strata_create(self.nfaults, self.kmax, self.thresholds.ctypes.data_as(C.c_void_p), self.Ht.device, C.byref(h)))
        self._h = h
        self._L = L

    @property
    def nfaults(self) -> int:
        return self.Ht.shape[0]

    def info(self) -> dict:
        arr = (C.c_int64 * 4)()
        _lib.check(self._L.qd_strata_info(self._h, arr))
        return dict(zip(("faults", "kmax", "table_bytes", "device"), [int(x) for x in arr]))

    def _sample(self, idx, shots, ks, seed, shot0, fault_bits):
        from .. import strata
        torch = _torch()
        if isinstance(ks, torch.Tensor):
            ks = ks.cpu().numpy()
        k = torch.from_numpy(strata.check_ks(ks, shots, self.priors, self.kmax)).to("cuda")
        det, obs = _sample_rows(shots, self.m, self.nobs)
        fault_bits, fs = _fault_rows(fault_bits, shots, self.nfaults)
        _lib.check(self._L.qd_sample_dem_strata(self._h, self.Ht._h, self.Lt._h, _seed64(seed), int(shot0),
                                                C.c_void_p(0) if idx is None else _ptr(idx), _ptr(k), shots, _ptr(det), det.stride(0), _ptr(obs),
                                                obs.stride(0), _ptr(fault_bits), fs, _stream_ptr()))
        return det, obs, fault_bits

    def sample_faults(self, ks, seed: int, shot0: int = 0, fault_bits=None, shots: Optional[int] = None):
        """(det, obs, fault_bits) of shots shot0 .. shot0 + shots - 1 of `seed`'s stream, row b with ks[b] faults.  ks: an int array (or int
        tensor) of length `shots`, or one int for every row -- then `shots` says how many rows (default 1).  Every count must lie in
        0 .. min(kmax, number of faults with p > 0): ValueError otherwise.  fault_bits: as in DemSampler.sample_faults."""
        if shots is None:
            shots = 1 if np.ndim(ks) == 0 else len(ks)
        if int(shot0) < 0:
            raise ValueError("shot0 must not be negative")
        return self._sample(None, int(shots), ks, seed, shot0, fault_bits)

    def sample_shots_faults(self, indices, ks, seed: int, fault_bits=None):
        """Row b = shot indices[b] with ks[b] faults (ks: one int for all, or one per row): what `sample_faults(ks[b], seed, shot0=indices[b])`
        returns.  `indices`: an int64 cuda tensor or any integer sequence; any order, repeats allowed."""
        idx = _shot_indices(indices)
        return self._sample(idx, int(idx.shape[0]), ks, seed, 0, fault_bits)


class CircuitSampler(_Handle):
    """Device-side circuit-level sampler (qd_sample_circuit): a Pauli-frame simulation of the circuit, what the reference gets from
    `circuit.compile_detector_sampler().sample(shots, separate_observables=True)` (simulation.py:8-28).  Same surface as DemSampler.
    `circuit`: circuit text, quits_amd.dem.Circuit, stim.Circuit, or a quits_amd.frame.CompiledCircuit.  The semantics, the random
    stream and its assumption (deterministic detectors) are in quits_amd/frame.py.  Biased noise (Y_ERROR, PAULI_CHANNEL_1,
    PAULI_CHANNEL_2) is sampled exactly and needs no `approximate_disjoint_errors`: that setting concerns detector error models only."""
    _destroy = "qd_circuit_destroy"

    def __init__(self, circuit, device: Optional[int] = None):
        from ..frame import CompiledCircuit, compile_circuit
        L = _lib.require_gpu()
        torch = _torch()
        self.device = torch.cuda.current_device() if device is None else int(device)
        cc = circuit if isinstance(circuit, CompiledCircuit) else compile_circuit(circuit)
        prog = np.ascontiguousarray(cc.program, dtype=np.int32)
        thr = np.ascontiguousarray(cc.thresholds, dtype=np.uint32)
        h = C.c_void_p()
        rc = L.qd_circuit_create(prog.ctypes.data_as(C.c_void_p), len(prog), cc.nq, cc.nmeas, cc.ndet, cc.nobs,
                                 thr.ctypes.data_as(C.c_void_p), len(thr), cc.ring, self.device, C.byref(h))
        if rc == -4:
            raise NotImplementedError(L.qd_last_error().decode())
        _lib.check(rc)
        self._h = h
        self._L = L
        self.compiled = cc
        self.m = cc.ndet
        self.nobs = cc.nobs

    def info(self) -> dict:
        arr = (C.c_int64 * 8)()
        _lib.check(self._L.qd_circuit_info(self._h, arr))
        keys = ("qubits", "sites", "lds_bytes", "measurements", "detectors", "observables", "ring", "program_words")
        return dict(zip(keys, [int(x) for x in arr]))

    def sample(self, shots: int, seed: int, shot0: int = 0):
        """(det uint8 [shots, m], obs uint8 [shots, nobs]) on the current device, shots shot0 .. shot0 + shots - 1."""
        det, obs = _sample_rows(shots, self.m, self.nobs)
        _lib.check(self._L.qd_sample_circuit(self._h, _seed64(seed), int(shot0), int(shots), _ptr(det),
                                             det.stride(0), _ptr(obs), obs.stride(0), _stream_ptr()))
        return det, obs

    def sample_packed(self, shots: int, seed: int, shot0: int = 0):
        """`sample` bit-packed on the device (qd_pack_b8): (PackedSamples det, PackedSamples obs), CUDA tensors of ceil(m / 8) and
        ceil(nobs / 8) bytes per shot -- Stim's `sample(..., bit_packed=True, separate_observables=True)`."""
        from ..samples import PackedSamples
        det, obs = self.sample(shots, seed, shot0)
        return PackedSamples.pack(det), PackedSamples.pack(obs)

    def sample_shots(self, indices, seed: int):
        """Row b = shot indices[b] of this seed's stream (qd_sample_circuit_shots): what `sample(1, seed, shot0=indices[b])` returns.
        `indices`: an int64 cuda tensor or any integer sequence; any order, repeats allowed."""
        idx = _shot_indices(indices)
        n = idx.shape[0]
        det, obs = _sample_rows(n, self.m, self.nobs)
        _lib.check(_lib.require_experiment(self._L).qd_sample_circuit_shots(self._h, _seed64(seed), _ptr(idx), n, _ptr(det),
                                                                            det.stride(0), _ptr(obs), obs.stride(0), _stream_ptr()))
        return det, obs


def _norm(x):
    return x.lower() if isinstance(x, str) else x
