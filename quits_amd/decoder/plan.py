"""DeviceWindowPlan: the windows of one sliding-window decoding problem, resident on the GPU, and the batched driver over them."""
from __future__ import annotations

import contextlib
import threading
from typing import NamedTuple, Optional

import numpy as np
from scipy.sparse import csr_matrix

from . import pipeline
from .base import commit_ranges, spacetime, window_count
from .plan_cache import _current_device, cached_plan, plan_key

_CHUNK = 1 << 16   # shots per device batch
_CHUNK_EDGE = 5 << 14   # ... when BP runs in the one-message-per-edge kernel: five 64-shot workgroups per CU are resident on 256 CUs and the kernel's
                        # time is per-workgroup latency (81 920 vs 65 536 shots per launch: +8 % shots/s, 98 304 -18 %; profiles/r03o)


class DriverEnv(NamedTuple):
    chunk_shots: Optional[int]        # QD_CHUNK_SHOTS: shots per chunk, as given (A/B switch, profiles/r03x_chunk_size_pipelined_ab.txt)
    general_ws_gb: Optional[float]    # QD_GENERAL_WS_GB: HBM budget of the per-edge BP kernel's message planes (set_workspace_limits)
    post_ws_gb: float                 # QD_POST_WS_GB: what the lanes' posterior workspaces may take (default 160 of the 288 GB)
    no_pipeline: bool                 # QD_NO_PIPELINE: everything on the caller's stream


def driver_env():
    """The driver's environment, read once per plan (DeviceWindowPlan.__init__ keeps it as `plan.env`); nothing on the decode path reads
    the environment.  The flag is true for any non-empty value other than '0' / 'false' / 'no' / 'off' (so QD_NO_PIPELINE=true still
    means what it says); the numbers raise ValueError when malformed, and empty counts as unset."""
    import os
    chunk, general, post = (os.environ.get(name) for name in ("QD_CHUNK_SHOTS", "QD_GENERAL_WS_GB", "QD_POST_WS_GB"))
    flag = os.environ.get("QD_NO_PIPELINE", "").strip().lower()
    return DriverEnv(int(chunk) if chunk else None, float(general) if general else None, float(post) if post else 160.0,
                     flag not in ("", "0", "false", "no", "off"))


def set_workspace_limits(decs, general_ws_gb):
    """The per-edge BP kernel (product_sum / serial) keeps its messages in HBM, one workspace per decoder: `decs`, the decoders that will
    hold message planes at once, split a fixed budget (QD_GENERAL_WS_GB, default 96) instead of each claiming the single-decoder default.
    One decoder gets the whole budget, and only if one was given (unset: the library's 48 GB)."""
    if len(decs) > 1:
        budget = (96.0 if general_ws_gb is None else general_ws_gb) * (1 << 30)
        for d in decs:
            d.set_workspace_limit(max(1 << 28, int(budget / len(decs))))
    elif general_ws_gb is not None:
        decs[0].set_workspace_limit(int(max(0.001, general_ws_gb) * (1 << 30)))


def _new_decoder(graph, kw):
    """The batch decoder of a window from its device options (_kwargs_for_device): Relay-BP where they carry a RelayConfig."""
    from .device import BatchDecoder, RelayBatchDecoder
    if "relay" in kw:
        kw = dict(kw)
        return RelayBatchDecoder(graph, kw.pop("relay"), **kw)
    return BatchDecoder(graph, **kw)


class DeviceWindowPlan:
    """Everything the batched driver needs, resident on the GPU: per window a decoder, the commit matrix L_k, the
    hand-off matrix U_k and the first detector row."""

    def __init__(self, checks, commits, priors, updates, row0, nz, nobs, dict1, dict2):
        from .device import GF2Matrix, WindowGraph
        self.nz, self.nobs = int(nz), int(nobs)
        self.windows = []
        nwin = len(checks)
        # where every window's committed columns lie in the space-time correction `decode(..., correction=...)` fills
        self.commit_ranges = commit_ranges(commits)
        self.nfaults = sum(nc for _, nc in self.commit_ranges)
        cache = {}
        for k in range(nwin):
            kw = dict(dict2 if k == nwin - 1 else dict1)
            kw.pop("error_rate", None)
            kw.pop("channel_probs", None)
            kw.pop("error_channel", None)
            key = (id(checks[k]), id(priors[k]), k == nwin - 1)    # the phenomenological windows share one matrix
            if key not in cache:
                graph = WindowGraph(checks[k], priors[k])
                cache[key] = (graph, _new_decoder(graph, kw))
            graph, dec = cache[key]
            Lk = csr_matrix(commits[k])
            if Lk.shape[1] < graph.n:     # L_k only spans the committed columns (base.py:170)
                Lk = csr_matrix((Lk.data, Lk.indices, Lk.indptr), shape=(Lk.shape[0], graph.n))
            U = None
            if k < nwin - 1:
                Uk = csr_matrix(updates[k])
                Uk = csr_matrix((Uk.data, Uk.indices, Uk.indptr), shape=(Uk.shape[0], graph.n))
                U = GF2Matrix(Uk)
            self.windows.append({"dec": dec, "graph": graph, "L": GF2Matrix(Lk), "U": U, "row0": int(row0[k]), "H": checks[k], "kw": kw, "priors": priors[k],
                                 "col0": self.commit_ranges[k][0], "ncommit": self.commit_ranges[k][1]})
        self.env = driver_env()
        decs = self.decoders()
        edge = any(d.info()["edge_kernel"] for d in decs)
        self.chunk = self.env.chunk_shots if self.env.chunk_shots is not None else (_CHUNK_EDGE if edge else _CHUNK)
        set_workspace_limits(decs, self.env.general_ws_gb)
        # calls of two or more chunks: the post-processing of one chunk beside the BP of another (pipeline.decode_pipelined);
        # QD_NO_PIPELINE=1 or plan.pipeline = False keeps everything on the caller's stream.  Not the default where BP runs in the
        # per-edge kernel: HBM-bound, it loses more to the co-running post-processor than the overlap returns (W = 5 / F = 3
        # windows with the reference's settings 219 k -> 209 k shots/s, profiles/r03x_pipelined_driver_multiwindow_ab.txt; forced on,
        # a wash: profiles/r05_pipeline_edge_ab.txt)
        self.pipeline = not self.env.no_pipeline and not edge
        # lanes of the pipelined driver: 2; 3 for plans of several windows -- a lane's next BP stage waits for its last post stage, which
        # runs beside the BP of the NEXT lane and, starved of wavefront slots by it, ends ~0.4 ms after it: with two lanes the BP stream
        # waits that long before every stage, with three the post stage has one more BP stage's time (profiles/r06_three_lanes_ab.txt)
        self.lanes = 3 if nwin > 1 else 2
        # every lane has its own decoders and every decoder its own posterior workspace (4 bytes per fault and shot of a chunk): a plan of many
        # large windows -- QLP [[1020,136]] W = 3: 18 decoders x 18 900 faults = 1.36 MB per shot and lane -- would not fit three lanes of
        # 65 536 shots (268 GB).  Lanes first, then the chunk, give way until the estimate fits QD_POST_WS_GB.
        if self.pipeline and self.env.chunk_shots is None:
            per_shot = workspace_bytes_per_shot(decs)
            self.lanes, self.chunk = fit_lanes_and_chunk(per_shot, self.lanes, self.chunk, self.env.post_ws_gb * (1 << 30))
        self.host_piece = self.lanes * self.chunk   # shots per staged piece of decode_host (one group of the pipelined driver's lanes)
        self._lane_decs = {id(d): [d] for d in decs}     # per decoder of the plan, the decoders of the two-stream driver's lanes (lane 0: itself)
        self._two_streams = None                         # pipeline.TwoStreams and pipeline.HostStaging, made at first use
        self._staging = None
        self._commit_weights = None                      # commit_weights(): the committed columns' log-likelihood weights, on the device
        self.device = _current_device()      # graphs, decoders and workspaces were created on this device
        self._lock = threading.RLock()       # one decode_host at a time per plan (staging buffers, side streams and workspaces are per plan);
                                             # re-entrant, and the plan cache takes it (non-blocking) before releasing an idle plan's workspaces

    def release_workspaces(self):
        """Hand the decoders' device workspaces and the staging buffers back (the plan itself -- graphs, decoders, matrices --
        stays): cached plans that are not the one in use hold no large allocations."""
        for lst in self._lane_decs.values():
            for d in lst:
                d.release_workspace()
        self._staging = None

    def window_matrices(self):
        """Host copies of the window check matrices, in window order (bench.py derives its work model from them)."""
        return [w["H"] for w in self.windows]

    def decoders(self):
        out = []
        for w in self.windows:
            if w["dec"] not in out:
                out.append(w["dec"])
        return out

    def lane_decoders(self):
        """Per window, the decoders of the two-stream driver's `self.lanes` lanes, each with its own workspaces; windows that share a
        decoder share its lanes' decoders.  Lanes that are missing are built here."""
        if any(len(lst) < self.lanes for lst in self._lane_decs.values()):
            for w in self.windows:
                lst = self._lane_decs[id(w["dec"])]
                while len(lst) < self.lanes:
                    lst.append(_new_decoder(w["graph"], w["kw"]))
            if any(d.info()["edge_kernel"] for d in self.decoders()):
                set_workspace_limits([d for lst in self._lane_decs.values() for d in lst], self.env.general_ws_gb)
        return [self._lane_decs[id(w["dec"])] for w in self.windows]

    def two_streams(self, device):
        """The two-stream driver's state (streams live on the device of the data)."""
        if self._two_streams is None:
            self._two_streams = pipeline.TwoStreams(device)
        return self._two_streams

    def check_correction(self, correction, N, device):
        import torch
        words = (self.nfaults + 31) // 32
        if not (isinstance(correction, torch.Tensor) and correction.is_cuda and correction.dtype == torch.int32 and correction.dim() == 2
                and correction.shape[0] == N and correction.shape[1] >= words and (correction.shape[1] <= 1 or correction.stride(1) == 1)):
            raise ValueError("correction must be a cuda int32 [%d, >= %d] tensor with unit stride inside a row" % (N, words))
        if correction.device != device:
            raise ValueError("correction lives on %s, the samples on %s" % (correction.device, device))

    def commit_priors(self):
        """float64 [nfaults] on the host: the priors of the committed columns, laid end to end like the correction."""
        pri = [np.broadcast_to(np.asarray(w["priors"], dtype=np.float64), (w["graph"].n,))[:w["ncommit"]] for w in self.windows]
        return np.concatenate(pri) if pri else np.zeros((0,))

    def commit_weights(self):
        """cuda int32 [nfaults]: quits_amd.soft.fault_weights of the committed columns' priors, laid end to end like the correction -- window k
        contributes priors_k[:ncommit_k].  Made once per plan and kept on its device."""
        if self._commit_weights is None:
            import torch
            from ..soft import fault_weights
            host = fault_weights(self.commit_priors())
            dev = torch.device("cuda", self.device) if self.device >= 0 else torch.device("cuda")
            self._commit_weights = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
        return self._commit_weights

    def check_soft(self, soft, correction, N, device):
        import torch
        if correction is None:
            raise ValueError("soft records are computed from the committed correction: pass `correction` along with `soft`")
        if not (isinstance(soft, torch.Tensor) and soft.is_cuda and soft.dtype == torch.int64 and soft.dim() == 2 and soft.shape[0] == N
                and soft.shape[1] == 6 and soft.stride(1) == 1):
            raise ValueError("soft must be a cuda int64 [%d, 6] tensor with unit stride inside a row" % N)
        if soft.device != device:
            raise ValueError("soft lives on %s, the samples on %s" % (soft.device, device))

    def decode(self, det, stats=None, correction=None, soft=None):
        """det: cuda uint8 [N, ndet]  ->  cuda uint8 [N, nobs] logical predictions.

        Chunks of `self.chunk` shots, windows inner.  `stats`, if given, receives (window index, status tensor) pairs.
        `correction`, if given, is a cuda int32 [N, >= ceil(nfaults / 32)] tensor that the call zero-fills and then fills with the space-time
        correction: bit j & 31 of word j >> 5 of row b = fault j of the whole model is in shot b's correction -- every window's committed
        columns at `commit_ranges[k]` (qd_commit_bits next to the window's acc ^= L_k e, on its stream).  Without it no launch is added.
        `soft`, if given (it needs `correction`), is a cuda int64 [N, 6] tensor that the call zero-fills and then fills with the shots' soft
        records (quits_amd/soft.py): qd_soft_fold behind every window's decode, qd_soft_weigh behind a chunk's last qd_commit_bits, with
        `commit_weights()`.  Without it no launch is added either.
        A call of two or more chunks runs a chunk's post-processing on a second stream beside the BP of the other chunks of its
        group (pipeline.decode_pipelined: headline 1.21 -> 1.30 M shots/s, BP-LSD order 1 690 k -> 866 k, p = 6e-3 320 k -> 355 k,
        W = 3 / F = 1 windows 511 k -> 539 k, identical outputs; profiles/r03x_pipelined_driver_ab.txt,
        r03x_pipelined_driver_multiwindow_ab.txt); results are delivered in order on the caller's stream.  QD_NO_PIPELINE=1 or
        `plan.pipeline = False` turns it off; it is off by default for plans whose BP runs in the per-edge kernel."""
        import torch
        N = det.shape[0]
        if self.pipeline and N >= 2 * self.chunk:
            if correction is None:
                if soft is not None:
                    self.check_soft(soft, correction, N, det.device)
                return pipeline.decode_pipelined(self, det, stats)
            if soft is None:
                return pipeline.decode_pipelined(self, det, stats, correction=correction)
            return pipeline.decode_pipelined(self, det, stats, correction=correction, soft=soft)
        pred = torch.zeros((N, self.nobs), dtype=torch.uint8, device=det.device)
        if correction is not None:
            from .device import commit_bits
            self.check_correction(correction, N, det.device)
            correction.zero_()
        if soft is not None:
            from .device import soft_fold, soft_weigh
            self.check_soft(soft, correction, N, det.device)
            weights = self.commit_weights()
            soft.zero_()
        for c0 in range(0, N, self.chunk):
            chunk = det[c0:c0 + self.chunk]
            acc = pred[c0:c0 + self.chunk]
            upd = None
            for k, w in enumerate(self.windows):
                err_bits, status = w["dec"].decode(chunk, w["row0"], upd)
                w["L"].xor_apply(err_bits, acc, accumulate=True)
                if correction is not None:
                    commit_bits(err_bits, w["ncommit"], correction[c0:c0 + self.chunk], w["col0"])
                if soft is not None:
                    soft_fold(status, soft[c0:c0 + self.chunk])
                    if k == len(self.windows) - 1:
                        soft_weigh(correction[c0:c0 + self.chunk], self.nfaults, weights, chunk, soft[c0:c0 + self.chunk])
                if w["U"] is not None:
                    upd = torch.empty((chunk.shape[0], self.nz), dtype=torch.uint8, device=det.device)
                    w["U"].xor_apply(err_bits, upd, accumulate=False)
                if stats is not None:
                    stats.append((k, status))
        return pred

    def decode_host(self, zcheck_samples, corrections=False):
        """The reference call's data path: host samples [N, ndet] (bool / uint8 / any integer numpy array, a torch tensor, or
        quits_amd.samples.PackedSamples on either side)
        -> int64 numpy [N, nobs] (reference sliding_window.py:160,186).  Host arrays are streamed: pieces of `self.host_piece`
        shots go through two pinned staging buffers and a copy stream, so that the host-side copy and the PCIe transfer of one
        piece run beside the decoding of the previous one, and the predictions come back through a pinned buffer
        (pipeline.decode_host_samples).  Tensors that already live on the GPU skip the staging.
        corrections=True: returns (predictions, PackedSamples of `nfaults` bits per shot on the host), the space-time corrections of
        `decode(..., correction=...)`; they come back through a pinned buffer of their own, piece by piece like the predictions."""
        import torch
        from ..samples import PackedSamples
        with self.in_use():
            dev = torch.device("cuda", self.device) if self.device >= 0 else torch.device("cuda")
            packed = isinstance(zcheck_samples, PackedSamples)
            on_gpu = zcheck_samples.data if packed and zcheck_samples.is_cuda else zcheck_samples
            if isinstance(on_gpu, torch.Tensor) and on_gpu.is_cuda:
                if on_gpu.device != dev:
                    raise RuntimeError("samples live on %s, the plan on %s" % (on_gpu.device, dev))
                det = pipeline._to_device_samples(zcheck_samples)
                if not corrections:
                    return self.decode(det).cpu().numpy().astype(np.int64)
                corr = torch.empty((det.shape[0], (self.nfaults + 31) // 32), dtype=torch.int32, device=dev)
                pred = self.decode(det, None, corr)
                return pred.cpu().numpy().astype(np.int64), pipeline.correction_words_to_packed(corr.cpu().numpy(), self.nfaults)
            if packed:
                a = zcheck_samples                                # (staged packed: pipeline.decode_host_samples)
            else:
                a = zcheck_samples.cpu().numpy() if isinstance(zcheck_samples, torch.Tensor) else np.asarray(zcheck_samples)
            if a.ndim != 2:
                raise ValueError("zcheck_samples must be a [shots, detectors] array")
            if a.shape[0] == 0:
                pred = np.zeros((0, self.nobs), dtype=np.int64)
                return (pred, pipeline.correction_words_to_packed(np.zeros((0, (self.nfaults + 31) // 32), np.int32), self.nfaults)) if corrections else pred
            if self._staging is None:
                self._staging = pipeline.HostStaging(dev)
            if not corrections:
                return pipeline.decode_host_samples(self, self._staging, a)
            return pipeline.decode_host_samples(self, self._staging, a, corrections=True)

    def in_use(self):
        """Context manager around a run of `decode` calls that owns the plan: checks the current device, takes the plan's lock and marks
        the workspaces live, so that the plan cache does not release them under the run (decode_host, simulation.get_circuit_mem_pL)."""
        import torch
        if self.device >= 0 and torch.cuda.current_device() != self.device:
            raise RuntimeError("this plan was built on cuda:%d but the current device is cuda:%d (plans are per device; the plan "
                               "cache keys on the current device)" % (self.device, torch.cuda.current_device()))

        @contextlib.contextmanager
        def held():
            with self._lock:
                self._ws_live = True             # (a concurrent cache lookup may have released them since this plan was handed out)
                yield self
        return held()


def workspace_bytes_per_shot(decs):
    """The estimate fit_lanes_and_chunk is given: what one shot of a chunk takes in the workspaces of one lane's decoders `decs` -- the posterior
    row, 4 bytes per padded fault (n_pad = n rounded up to 64), and the lists; a Relay-BP decoder whose marginals live in device memory
    (info()["relay_marginals"] == "device") keeps a second such row per shot.  QLP [[1020,136]] W = 3: 18 decoders x 2 x 75.6 KB."""
    total = 0
    for d in decs:
        row = 4 * ((d.graph.n + 63) // 64 * 64)
        total += row + 64
        if d.info().get("relay_marginals") == "device":
            total += row
    return total


def fit_lanes_and_chunk(per_shot_bytes, lanes, chunk, budget_bytes, min_chunk=8192):
    """(lanes, chunk) of the pipelined driver such that lanes x chunk x per_shot_bytes (the lanes' decoder workspaces) fits the budget: a third
    lane goes first (it is worth 2-5 %), then the chunk is halved (down to `min_chunk` shots: below that the launches are all tail)."""
    while lanes * chunk * per_shot_bytes > budget_bytes:
        if lanes > 2:
            lanes -= 1
        elif chunk // 2 >= min_chunk:
            chunk //= 2
        else:
            break
    return lanes, chunk


def _kwargs_for_device(d, cls):
    """Keyword arguments of plug-in class `cls` -> BatchDecoder options.  The post-processor follows the CLASS, as it does in
    ldpc: a BpLsdDecoder runs LSD whether or not the dict names `lsd_method` / `lsd_order` (ldpc's defaults 'lsd_0', 0).
    Keywords that do not change the algorithm here are dropped (`omp_thread_count`; `input_vector_type` 'syndrome' / 'auto';
    `random_schedule_seed` 0 / None and `serial_schedule_order` None = the natural serial order, which is what this build
    runs); legal ldpc keywords the device path does not implement raise NotImplementedError; the other class's post-processor
    options and unknown names raise TypeError naming the device path (ldpc's own classes take **kwargs and may ignore them:
    refusing is the safe side of "never a silent change of algorithm")."""
    from .bplsd import BpLsdDecoder, lsd_to_device_method
    from .relaybp import RelayBpDecoder, relay_device_kwargs
    if isinstance(cls, type) and issubclass(cls, RelayBpDecoder):        # its own keywords: the RelayConfig fields and the post-processor
        return relay_device_kwargs(d)
    common = ("bp_method", "schedule", "max_iter", "ms_scaling_factor")
    rates = ("error_rate", "channel_probs", "error_channel")
    d = dict(d)
    is_lsd = isinstance(cls, type) and issubclass(cls, BpLsdDecoder)
    own = ("lsd_method", "lsd_order", "bits_per_step") if is_lsd else ("osd_method", "osd_order")
    d.pop("omp_thread_count", None)
    if str(d.pop("input_vector_type", "syndrome")).lower() not in ("syndrome", "auto"):
        raise NotImplementedError("the device path decodes syndromes only (input_vector_type='syndrome')")
    if d.pop("random_schedule_seed", 0) not in (0, None) or d.pop("serial_schedule_order", None) is not None:
        raise NotImplementedError("the device path runs the serial schedule in natural fault order only (ldpc's default: "
                                  "random_schedule_seed=0, serial_schedule_order=None)")
    extra = [k for k in d if k not in common + rates + own]
    if extra:
        raise TypeError("%s on the device path does not take the keyword argument(s): %s" % (cls.__name__, ", ".join(sorted(extra))))
    out = {k: d[k] for k in d if k in common}
    if is_lsd:
        out["osd_method"], out["osd_order"] = lsd_to_device_method(d.get("lsd_method", "lsd_0"), d.get("lsd_order", 0),
                                                                   d.get("bits_per_step", 1))
    else:
        out.update({k: d[k] for k in d if k in own})
    return out


def build_circuit_plan(circuit, hz, W, F, num_rounds, dict1, dict2, decoder1=None, decoder2=None):
    from .bposd import BpOsdDecoder
    nz = hz.shape[0]
    num_cor_rounds, _, _ = window_count(num_rounds, W, F)
    checks, commits, priors, updates = spacetime(circuit, hz, W, F, num_cor_rounds)
    row0 = [F * k * nz for k in range(num_cor_rounds)] + [F * num_cor_rounds * nz]
    return DeviceWindowPlan(checks, commits, priors, updates, row0, nz, commits[0].shape[0],
                            _kwargs_for_device(dict1, decoder1 or BpOsdDecoder), _kwargs_for_device(dict2, decoder2 or BpOsdDecoder))


def phenom_window_set(hz, lz, W, F, num_rounds, rate_mid, rate_last):
    """The phenomenological variant's windows in spacetime()'s format (checks, commits, priors, updates): the analytic window
    matrices of reference sliding_window.py:56-68 with the slicing of :86,:88,:96,:99 written as matrices
    (commit = lz @ sum of the first F data blocks, by linearity; hand-off = measurement block F-1 of the decoded vector)."""
    from .sliding_window import phenom_window_matrices
    hz = np.asarray(hz) % 2
    lz = np.asarray(lz) % 2
    nz, nq = hz.shape
    num_cor_rounds, W_last, _ = window_count(num_rounds, W, F)
    h_mid, h_last = phenom_window_matrices(hz, W, F, W_last)
    commit_mid = csr_matrix(np.concatenate([np.tile(lz, (1, F)), np.zeros((lz.shape[0], h_mid.shape[1] - F * nq), int)], axis=1))
    commit_last = csr_matrix(np.concatenate([np.tile(lz, (1, W_last)), np.zeros((lz.shape[0], h_last.shape[1] - W_last * nq), int)], axis=1))
    sel = np.zeros((nz, h_mid.shape[1]), dtype=int)
    sel[np.arange(nz), W * nq + (F - 1) * nz + np.arange(nz)] = 1
    checks = [h_mid] * num_cor_rounds + [h_last]
    commits = [commit_mid] * num_cor_rounds + [commit_last]
    updates = [csr_matrix(sel)] * num_cor_rounds
    priors = [np.full(h_mid.shape[1], float(rate_mid))] * num_cor_rounds + [np.full(h_last.shape[1], float(rate_last))]
    return checks, commits, priors, updates


def build_phenom_plan(hz, lz, W, F, num_rounds, dict1, dict2, decoder1=None, decoder2=None):
    from .bposd import BpOsdDecoder
    nz = np.asarray(hz).shape[0]
    num_cor_rounds, _, _ = window_count(num_rounds, W, F)
    checks, commits, priors, updates = phenom_window_set(hz, lz, W, F, num_rounds, dict1["error_rate"], dict2["error_rate"])
    row0 = [F * k * nz for k in range(num_cor_rounds)] + [F * num_cor_rounds * nz]
    return DeviceWindowPlan(checks, commits, priors, updates, row0, nz, np.asarray(lz).shape[0],
                            _kwargs_for_device(dict1, decoder1 or BpOsdDecoder), _kwargs_for_device(dict2, decoder2 or BpOsdDecoder))


def cached_circuit_plan(circuit, hz, W, F, num_rounds, decoder1, decoder2, dict1, dict2):
    """The process-wide cache's plan for these arguments (plan_key's, kind 'circuit'), built on a miss."""
    return cached_plan(plan_key("circuit", circuit, hz, None, W, F, num_rounds, decoder1, decoder2, dict1, dict2),
                       lambda: build_circuit_plan(circuit, hz, W, F, num_rounds, dict1, dict2, decoder1, decoder2))


def cached_phenom_plan(hz, lz, W, F, num_rounds, decoder1, decoder2, dict1, dict2):
    """The same for the phenomenological windows (kind 'phenom')."""
    return cached_plan(plan_key("phenom", None, hz, lz, W, F, num_rounds, decoder1, decoder2, dict1, dict2),
                       lambda: build_phenom_plan(hz, lz, W, F, num_rounds, dict1, dict2, decoder1, decoder2))
