"""Monte-Carlo drivers around the decoder, mirroring `/root/reference/src/quits/simulation.py`.

  get_codecap_pL       <- simulation.py:31-61   code-capacity logical error rate of a decoder plug-in
  get_stim_mem_result  <- simulation.py:8-28    detector / observable samples of a memory circuit
  get_circuit_mem_result                        the same samples from the circuit itself on the device (Pauli-frame simulation)
  get_circuit_mem_pL                            a whole memory experiment on the device: sampler -> sliding-window BP-OSD -> tallies; what
                                                the reference's users write around the two calls above (tests/test_sliding_window.py:72-83),
                                                without a host array per shot
  get_relay_mem_pL                              the same experiment with the sliding-window Relay-BP decoder
  replay_shots                                  the samples of given shot indices again (both samplers are counter-based)
  get_postselected_pL                           the same experiment with a soft record per shot kept on the device (quits_amd/soft.py): the logical
                                                error rate that remains when the least certain fraction of the shots is discarded
  get_fault_spectrum                            the same experiment on DEM-sampled shots with the faults in view: shots and failures by the
                                                number of sampled faults, the residual E xor C of the failing shots, the lightest one seen
  replay_faults                                 which faults fired in given shots of the DEM sampler
  get_stratified_pL                             the same experiment on shots with a prescribed number of faults (subset sampling): f(k) where
                                                independent faults put no mass, pL = sum_k P(|E| = k) f(k) with an explicit truncation bound
  replay_strata_faults                          the fault sets of given shots of a stratum
  shrink_fault_sets                             given fault sets shrunk to 1-minimal failing ones on the device (quits_amd/shrink.py has the definition)
  get_minimal_failures                          the failing shots of such an experiment shrunk in one run: the lightest failing set (the exponent of
                                                pL ~ p^t for this decoder) and the lightest undetectable residual (a bound on the distance)
  get_relay_minimal_failures                    the same with the sliding-window Relay-BP decoder
  find_undetectable_logical_errors              a directed search for a light undetectable logical fault on the device, without decoder or
                                                sampler (quits_amd/search.py has the definition; re-exported from there)
  estimate_distance, estimate_code_distance     the random information-set estimate of the circuit-level or code distance on the device: an upper
                                                bound with its witnesses (quits_amd/distance.py has the definition; re-exported from there)
  estimate_priors                               the priors of a model's hyperedges fitted to detector samples, counted on the device, with
                                                jackknife standard errors (quits_amd/calibrate.py has the definition; re-exported from there)

`get_codecap_pL` keeps the reference's signature and its random stream (`np.random.seed(seed)` followed by one
`np.random.binomial(1, p, n)` per trial), so a given seed produces the same noise vectors as the reference.  With a plug-in
that decodes batches (`quits_amd.decoder.BpOsdDecoder`: it has `decode_batch`) all trials go through the device decoder in
one call; any other plug-in class runs the reference's per-trial loop on the host.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from .search import LogicalSearchResult, find_undetectable_logical_errors, search_mirror  # noqa: F401  (re-exported)
from .distance import DistanceResult, distance_mirror, estimate_code_distance, estimate_distance  # noqa: F401  (re-exported)
from .calibrate import CalibrationResult, estimate_priors  # noqa: F401  (re-exported)


def get_stim_mem_result(circuit, num_trials, seed=-1):
    """Detector and observable samples for a logical-memory circuit (simulation.py:8-28).

    A real `stim.Circuit` is sampled by Stim exactly like the reference does.  Anything else (circuit text or
    `quits_amd.dem.Circuit`; Stim is not a dependency of this package) is sampled at the level of its detector error
    model on the device: independent fault mechanisms with the model's probabilities, the same distribution for Pauli noise,
    not the same random stream.
    """
    if hasattr(circuit, "compile_detector_sampler"):
        sampler = circuit.compile_detector_sampler(seed=seed) if seed >= 0 else circuit.compile_detector_sampler()
        return sampler.sample(shots=num_trials, separate_observables=True)
    from .decoder.base import detector_error_model_to_matrix
    from .decoder.device import DemSampler
    from .dem import Circuit
    if not isinstance(circuit, Circuit):
        circuit = Circuit(str(circuit))
    H, L, priors = detector_error_model_to_matrix(circuit.detector_error_model())
    if seed < 0:
        seed = int(np.random.SeedSequence().entropy % (1 << 62))
    det, obs = DemSampler(H, L, priors).sample(int(num_trials), seed=int(seed))
    return det.cpu().numpy().astype(bool), obs.cpu().numpy().astype(bool)


def get_circuit_mem_result(circuit, num_trials, seed=-1):
    """Detector and observable samples of a memory circuit, drawn on the device by simulating the circuit itself
    (quits_amd.decoder.device.CircuitSampler, Pauli frames; quits_amd/frame.py states the semantics): the distribution the
    reference's `compile_detector_sampler().sample(..., separate_observables=True)` draws from, without Stim.  `circuit` is circuit
    text, a `quits_amd.dem.Circuit` or a `stim.Circuit`.  Returns numpy bool (det [num_trials, ndet], obs [num_trials, nobs])."""
    from .decoder.device import CircuitSampler
    if seed < 0:
        seed = int(np.random.SeedSequence().entropy % (1 << 62))
    det, obs = CircuitSampler(circuit).sample(int(num_trials), seed=int(seed))
    return det.cpu().numpy().astype(bool), obs.cpu().numpy().astype(bool)


def get_codecap_pL(code, p, num_trials, decoder, dict, basis='Z', seed=-1, tqdm_on=False):
    """Code-capacity logical error rate (simulation.py:31-61): i.i.d. bit flips with probability `p` on the data qubits,
    one decode of `H e` per trial, failure when the residual error anticommutes with a logical operator."""
    if seed >= 0:
        np.random.seed(seed)
    basis = basis.upper()
    if basis == 'Z':
        parity_check_matrix, logical_codewords = code.hz, code.lz
    elif basis == 'X':
        parity_check_matrix, logical_codewords = code.hx, code.lx
    else:
        raise ValueError("basis must be 'Z' or 'X'")
    bpd = decoder(parity_check_matrix, **dict)
    n = parity_check_matrix.shape[1]
    H = np.asarray(parity_check_matrix.todense() if hasattr(parity_check_matrix, "todense") else parity_check_matrix) % 2
    Lm = np.asarray(logical_codewords.todense() if hasattr(logical_codewords, "todense") else logical_codewords) % 2
    H = H.astype(np.int64); Lm = Lm.astype(np.int64)
    if hasattr(bpd, "decode_batch") and num_trials > 0:
        # same stream as `num_trials` successive binomial(1, p, n) calls of the legacy generator
        noise = np.random.binomial(1, p, (num_trials, n)).astype(np.int64)
        syndromes = (noise @ H.T) % 2
        decoded = np.asarray(bpd.decode_batch(syndromes.astype(np.uint8))).astype(np.int64)
        residual = (decoded + noise) % 2
        num_errors = int(((residual @ Lm.T) % 2).any(axis=1).sum())
        return num_errors / num_trials
    iterator = range(num_trials)
    if tqdm_on:
        from tqdm import tqdm
        iterator = tqdm(iterator)
    num_errors = 0
    for _ in iterator:
        noise = np.random.binomial(1, p, n)
        syndrome = H @ noise % 2
        decoded_error = np.asarray(bpd.decode(syndrome)).astype(np.int64)
        residual_error = (decoded_error + noise) % 2
        if (Lm @ residual_error % 2).any():
            num_errors += 1
    return num_errors / num_trials


# ---- a memory experiment on the device ------------------------------------------------------------------------------------------
def _rate(shots, errors):
    """(pL, sigma): `errors` / `shots` and its binomial standard deviation; NaN without shots."""
    if not shots:
        return float("nan"), float("nan")
    pL = errors / shots
    return pL, math.sqrt(pL * (1.0 - pL) / shots)


class _ByFaults:
    """The method the results with shots_by_faults / errors_by_faults share."""

    def failure_fraction(self):
        """f(w) = errors_by_faults[w] / shots_by_faults[w], float64 [256]; NaN where no shot had w faults (stratum w has no shots)."""
        s = self.shots_by_faults.astype(np.float64)
        return np.divide(self.errors_by_faults.astype(np.float64), s, out=np.full(s.shape, np.nan), where=s > 0)


def _fault_rows(bits, nfaults):
    """numpy bool [rows, nfaults] of packed fault words (a cuda int32 tensor: bit j & 31 of word j >> 5 = fault j)."""
    return np.unpackbits(np.ascontiguousarray(bits.cpu().numpy()).view(np.uint8), axis=1, bitorder="little")[:, :nfaults].astype(bool)


def _batch_step(batch):
    """`batch` rounded up to a multiple of 64, a word of the fail mask."""
    return (int(batch) + 63) // 64 * 64


def experiment_batches(num_trials, batch, rank=0, world=1):
    """[(shot0, n), ...]: the batches `get_circuit_mem_pL` issues, in order, for `rank` of `world`: the rank's contiguous slice of
    [0, num_trials) (parallel.shard_range) cut into pieces of `batch` shots, `batch` rounded up to a multiple of 64 (a word of the
    fail mask), the last piece taking what is left.  Shot indices are global."""
    from .parallel import shard_range
    if num_trials < 0 or batch < 1:
        raise ValueError("num_trials must be >= 0 and batch >= 1")
    lo, hi = shard_range(int(num_trials), int(rank), int(world))
    step = _batch_step(batch)
    return [(s, min(step, hi - s)) for s in range(lo, hi, step)]


def shots_before_stop(batches, failing_shots, max_errors):
    """The early-stop rule of `get_circuit_mem_pL`, as arithmetic: how many of `batches` (experiment_batches) are issued when the sorted
    global indices of the failing shots are `failing_shots`.  Batch i >= 2 is issued only if fewer than `max_errors` of the shots of batches
    0 .. i - 2 failed: the driver reads the count two batches behind, so that the read never waits for the batch in flight.  Returns the
    number of batches issued."""
    f = np.sort(np.asarray(failing_shots, dtype=np.int64))
    for i in range(2, len(batches)):
        end = batches[i - 2][0] + batches[i - 2][1]
        first = batches[0][0]
        if int(np.searchsorted(f, end, side="left") - np.searchsorted(f, first, side="left")) >= max_errors:
            return i
    return len(batches)


@dataclasses.dataclass
class MemExperimentResult:
    """What `get_circuit_mem_pL` returns.  shots, errors: decoded shots and those with a wrong prediction on any observable; pL = errors /
    shots with its binomial standard deviation sigma; per_observable_errors[i]: shots whose observable i was mispredicted; flagged[name] =
    (shots, errors) among the shots some window of which was post-processed ('post'), had a syndrome outside the window matrix's column
    space ('inconsistent'), may have seen float rounding ('inexact'), was decoded again on the coarse LLR grid ('coarse');
    failing_shots: ascending global indices of the first `keep_failures` failing shots (of this rank), failures_truncated if there were more."""
    shots: int
    errors: int
    pL: float
    sigma: float
    per_observable_errors: np.ndarray
    flagged: dict
    failing_shots: np.ndarray
    failures_truncated: bool
    seed: int
    sampler: str
    batch: int
    seconds: float
    shots_per_s: float

    @classmethod
    def from_counts(cls, counts, failing_shots=(), failures_truncated=False, seed=0, sampler="circuit", batch=0, seconds=0.0):
        """From the counter vector of decoder.device.Tally ([0] shots, [1] errors, [2 + 2j], [3 + 2j] per flag, [10 + i] per observable)."""
        from ._lib import SHOT_FLAG_NAMES, TALLY_HEAD
        c = np.asarray(counts, dtype=np.int64)
        shots, errors = int(c[0]), int(c[1])
        pL, sigma = _rate(shots, errors)
        flagged = {name: (int(c[2 + 2 * j]), int(c[3 + 2 * j])) for j, name in enumerate(SHOT_FLAG_NAMES)}
        return cls(shots, errors, pL, sigma, c[TALLY_HEAD:].copy(), flagged, np.asarray(failing_shots, dtype=np.int64), bool(failures_truncated),
                   int(seed), str(sampler), int(batch), float(seconds), shots / seconds if seconds > 0 else 0.0)


def _as_circuit(circuit):
    from .dem import Circuit
    return circuit if isinstance(circuit, Circuit) else Circuit(str(circuit))


def _check_sampler(sampler):
    if sampler not in ("circuit", "dem"):
        raise ValueError("sampler must be 'circuit' or 'dem'")


def _make_sampler(circ, sampler):
    from .decoder.device import CircuitSampler, DemSampler
    _check_sampler(sampler)
    if sampler == "circuit":
        return CircuitSampler(circ)
    from .decoder.base import detector_error_model_to_matrix
    H, L, priors = detector_error_model_to_matrix(circ.detector_error_model())
    return DemSampler(H, L, priors)


def _mask_to_indices(words, shot0, limit):
    """Ascending global indices of the set bits of a fail mask (uint64 words, bit l of word w = shot shot0 + 64 w + l): at most `limit`, and
    whether there were more.  Only the non-zero words are unpacked."""
    nz = np.flatnonzero(words)
    bits = np.unpackbits(words[nz].astype("<u8").view(np.uint8).reshape(-1, 8), axis=1, bitorder="little").astype(bool)
    idx = (np.int64(shot0) + nz.astype(np.int64)[:, None] * 64 + np.arange(64, dtype=np.int64)[None, :])[bits]
    return idx[:limit], idx.shape[0] > limit


def _default_batch(plan):
    """As many of the plan's chunks as the two-stream driver has lanes (at least two, so that it runs)."""
    return max(2, int(plan.lanes) if plan.pipeline else 2) * int(plan.chunk)


@dataclasses.dataclass
class _Setup:
    """What `_experiment_setup` hands a driver: the Circuit, the sampler (None where the driver asked for none), the model H, L, priors of the
    DEM-column drivers (else None), the strata [(k, N_k), ...] (else None), the cached plan, `batch` (the caller's, or the default), `step`
    (`batch` rounded up to a word of the fail mask, the result's `batch` field) and `words` = ceil(plan.nfaults / 32) of a correction row."""
    circ: object
    sampler: object
    H: object
    L: object
    priors: object
    strata: object
    plan: object
    batch: int
    step: int
    words: int

    def decode_tally(self, tally, det, obs, soft_fields=0):
        """One batch decoded with its correction in view and tallied: allocates the correction rows, the soft records where `soft_fields` says
        how many, and the fail mask (written by the tally, so not zeroed).  Returns (correction, fail mask, soft records or None)."""
        import torch
        n = det.shape[0]
        corr = torch.empty((n, self.words), dtype=torch.int32, device="cuda")
        rec = torch.empty((n, soft_fields), dtype=torch.int64, device="cuda") if soft_fields else None
        pred = self.plan.decode(det, None, corr, rec)
        mask = torch.empty(((n + 63) // 64,), dtype=torch.int64, device="cuda")
        tally.add(pred, obs, None, mask)
        return corr, mask, rec

    def decode_stats(self, Hdev, tally, fstats, det, obs, faults, shot0):
        """`decode_tally`, then `det` -- the batch's own rows -- becomes the residual H C xor det in place and `fstats` bins the batch by its
        faults, its correction and that residual.  Hdev: the model's H as a decoder.device.GF2Matrix.  Nothing is read back."""
        corr, mask, _ = self.decode_tally(tally, det, obs)
        Hdev.xor_apply(corr, det, accumulate=True)
        fstats.add(faults, corr, self.plan.nfaults, det, mask, shot0)


def _experiment_setup(circuit, hz, lz, W, F, decoder, opts, needs, *, sampler=None, columns=False, strata=None, batch=None, on_device=None):
    """What every driver below does before its loop, in this order -- a new driver is this call and a loop body:

      arguments  F != 0, `sampler` 'circuit', 'dem' or, with `columns` only, None (no sampler), `strata` a good k -> N_k mapping (_strata_plan): ValueError,
                 whether or not there is a device.  A driver's further checks of its own arguments go in front of this call.
      device     _lib.require_gpu and the entry-point groups named by `needs` (_lib.require_<name>, in that order; 'strata' is added where
                 `strata` is given): RuntimeError, there is no CPU fallback.  Then `on_device()`, if given, before anything is put on the device.
      model      the Circuit; with `columns` (the drivers that work on DEM columns) H, L, priors of its detector error model and from them the
                 sampler -- StratifiedDemSampler up to the largest k where `strata` is given, else DemSampler for 'dem', none for None; without `columns`
                 _make_sampler(circ, sampler), and the detector and observable counts are the sampler's (nothing extracts the model here).
      plan       the number of rounds from the detector count and hz, the whole-history warning, the cached plan of (`decoder`, `opts`), its
                 observable count against the circuit's and lz's, with `columns` its committed faults against the model's columns.

    Returns a _Setup."""
    import warnings
    from . import _lib
    if F == 0:
        raise ValueError("Input parameter F cannot be zero.")
    if sampler is not None:
        _check_sampler(sampler)
    todo = None if strata is None else _strata_plan(strata)
    lib = _lib.require_gpu()                                # no GPU or no library: RuntimeError, there is no CPU fallback
    for name in tuple(needs) + (("strata",) if todo is not None else ()):
        getattr(_lib, "require_" + name)(lib)
    if on_device is not None:
        on_device()
    from .decoder.base import detector_error_model_to_matrix, window_count
    from .decoder.plan import cached_circuit_plan
    circ = _as_circuit(circuit)
    H = L = priors = None
    if columns:
        from . import strata as st
        from .decoder.device import DemSampler, StratifiedDemSampler
        H, L, priors = detector_error_model_to_matrix(circ.detector_error_model())
        if todo is not None:
            smp = StratifiedDemSampler(H, L, priors, max([k for k, _ in todo], default=0))
            if todo:
                st.check_ks(np.array([k for k, _ in todo]), len(todo), priors, smp.kmax)
        else:
            smp = DemSampler(H, L, priors) if sampler == "dem" else None
        ndet, nobs = H.shape[0], L.shape[0]
    else:
        smp = _make_sampler(circ, sampler)
        ndet, nobs = smp.m, smp.nobs
    num_rounds = ndet // hz.shape[0] - 2
    if window_count(num_rounds, W, F)[2]:
        warnings.warn("Window size larger than the syndrome extraction rounds: Doing whole history correction")
    plan = cached_circuit_plan(circ, hz, W, F, num_rounds, decoder, decoder, opts, opts)
    if nobs != plan.nobs or np.asarray(lz.shape)[0] != plan.nobs:
        raise ValueError("the circuit has %d observables, lz %d rows, the window plan commits %d" % (nobs, lz.shape[0], plan.nobs))
    if columns and plan.nfaults != H.shape[1]:
        raise ValueError("the windows commit %d faults, the detector error model has %d" % (plan.nfaults, H.shape[1]))
    if batch is None:
        batch = _default_batch(plan)
    return _Setup(circ, smp, H, L, priors, todo, plan, batch, _batch_step(batch), (plan.nfaults + 31) // 32)


def get_circuit_mem_pL(circuit, hz, lz, W, F, num_trials, max_iter=2, osd_order=0, bp_method='product_sum', schedule='serial',
                       osd_method='osd_cs', *, seed=0, sampler='circuit', batch=None, max_errors=None, keep_failures=4096,
                       shard=None, distributed=False):
    """A logical-memory experiment of `num_trials` shots, entirely on the device: every batch is sampled (shots shot0 .. shot0 + n - 1 of the
    stream of `seed`), decoded by the sliding-window BP-OSD decoder and tallied there; the host receives the counters and the failing
    shots' indices at the end.  The decoder keywords are `sliding_window_bposd_circuit_mem`'s (same names, order, defaults; same cached
    plan), the number of rounds follows from the circuit's detector count as it does there from the sample width.

    sampler: 'circuit' (decoder.device.CircuitSampler: the circuit itself, what `get_circuit_mem_result` draws) or 'dem'
        (DemSampler on the circuit's detector error model, what `get_stim_mem_result` draws for circuit text).  A 'dem' batch is not
        asynchronous: every qd_sample_dem call uploads its threshold table (an allocation, a blocking copy, a stream synchronisation),
        so the host waits for each batch's sampling and the batches do not overlap; 'circuit' queues everything.
    batch: shots per batch, rounded up to a multiple of 64; default: as many of the plan's chunks as the two-stream driver has lanes
        (at least two, so that it runs).  The result does not depend on it, except through `max_errors`.
    max_errors: stop early.  Batches are issued in order; before batch i >= 2 is issued, the number of failing shots of batches
        0 .. i - 2 is read (it is two batches old, so the read does not wait for the batch in flight), and if it is >= max_errors no
        further batch is issued.  Every issued batch is counted, so `shots` and `errors` are a function of (num_trials, batch,
        max_errors, shard) and the seed alone -- not of timing.  `shots_before_stop` states the rule as arithmetic.
    keep_failures: how many failing shots' global indices to return (the smallest); 0 keeps no fail mask at all.
    shard: (rank, world): run this rank's contiguous slice of the shots (parallel.shard_range); indices stay global.
    distributed: take (rank, world) from RANK / WORLD_SIZE (parallel.init_distributed) and sum the counters over the ranks in one
        all-reduce; failing_shots stay this rank's.  With max_errors each rank stops on ceil(max_errors / world) of its own.

    Returns a MemExperimentResult.  `replay_shots(circuit, result.failing_shots, seed, sampler)` regenerates the failing shots."""
    from .decoder.bposd import BpOsdDecoder
    opts = {'bp_method': bp_method, 'max_iter': max_iter, 'schedule': schedule, 'osd_method': osd_method, 'osd_order': osd_order}
    return _mem_experiment(circuit, hz, lz, W, F, num_trials, BpOsdDecoder, opts, seed=seed, sampler=sampler, batch=batch, max_errors=max_errors,
                           keep_failures=keep_failures, shard=shard, distributed=distributed)


def get_relay_mem_pL(circuit, hz, lz, W, F, num_trials, relay=None, osd_method='osd_off', osd_order=0, *, seed=0, sampler='circuit', batch=None,
                     max_errors=None, keep_failures=4096, shard=None, distributed=False):
    """`get_circuit_mem_pL` with the sliding-window Relay-BP decoder (decoder.sliding_window_relaybp_circuit_mem: same cached plan): `relay` is a
    quits_amd.relay.RelayConfig (default RelayConfig()), `osd_method` / `osd_order` the post-processor of the shots no leg solves
    ('osd_off': they keep their last hard decision).  Every other argument, the early-stop rule and the result are that function's; the
    'post' flag counts the shots some window of which went to the post-processor."""
    from .decoder.relaybp import RelayBpDecoder, relay_options
    opts = relay_options(relay, osd_method, osd_order)
    return _mem_experiment(circuit, hz, lz, W, F, num_trials, RelayBpDecoder, opts, seed=seed, sampler=sampler, batch=batch, max_errors=max_errors,
                           keep_failures=keep_failures, shard=shard, distributed=distributed)


def _mem_experiment(circuit, hz, lz, W, F, num_trials, decoder, opts, *, seed, sampler, batch, max_errors, keep_failures, shard, distributed):
    """The experiment loop of get_circuit_mem_pL and get_relay_mem_pL: `decoder` is the plug-in class of both window kinds, `opts` its
    keyword dict (the cached plan's key)."""
    import time
    import torch
    from .decoder.device import Tally, shot_flags_fold
    from .parallel import env_rank_world, init_distributed, reduce_vector
    dist = None
    rank, world = (0, 1) if shard is None else (int(shard[0]), int(shard[1]))

    def join_ranks():
        nonlocal dist, rank, world
        env_rank, env_world, local = env_rank_world()
        if env_world > 1:
            torch.cuda.set_device(local % torch.cuda.device_count())    # one process per GPU; the plan, the samplers and RCCL follow the current device
        dist = init_distributed()
        if shard is None:
            rank, world = env_rank, env_world
    su = _experiment_setup(circuit, hz, lz, W, F, decoder, opts, ("experiment",), sampler=sampler, batch=batch,
                           on_device=join_ranks if distributed else None)
    smp, plan, k, step = su.sampler, su.plan, su.plan.nobs, su.step
    batches = experiment_batches(num_trials, su.batch, rank, world)
    limit = None if max_errors is None else -(-int(max_errors) // world)
    first = batches[0][0] if batches else 0
    nwin = len(plan.windows)
    with plan.in_use():
        tally = Tally(k)
        mask = torch.zeros((sum((n + 63) // 64 for _, n in batches),), dtype=torch.int64, device="cuda") if keep_failures else None
        seen = torch.zeros((3,), dtype=torch.int64).pin_memory()       # failing shots so far, as of the last three batches
        done = []
        issued = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, (shot0, n) in enumerate(batches):
            if i >= 2:
                # at most two batches are in flight; the count behind this event is two batches old and has long arrived
                done[i - 2].synchronize()
                if limit is not None and int(seen[(i - 2) % 3]) >= limit:
                    break
            det, obs = smp.sample(n, seed, shot0)
            stats = []
            pred = plan.decode(det, stats)
            # `stats` holds (window, status words) pairs.  Both drivers append a window's pairs in shot order: the single-stream one chunk by
            # chunk, each pair a tensor of its own; the two-stream one as views st_all[k, c0:c0 + B] of one tensor, c0 ascending within a
            # window.  So the pairs of window k, laid end to end, are the batch's shots 0 .. n - 1.  Checked: the lengths add up to n, and a
            # pair that is a view into the storage of its window's first pair starts where the pairs before it end.
            flags = torch.zeros((n,), dtype=torch.uint8, device="cuda")
            at = [0] * nwin
            origin = [None] * nwin
            for kw, st in stats:
                where = (st.untyped_storage().data_ptr(), st.storage_offset())
                if origin[kw] is None:
                    origin[kw] = where
                elif where[0] == origin[kw][0] and where[1] != origin[kw][1] + at[kw]:
                    raise RuntimeError("the decoder's status words of window %d are not in shot order (offset %d after %d shots)"
                                       % (kw, where[1] - origin[kw][1], at[kw]))
                shot_flags_fold(st, flags[at[kw]:at[kw] + st.shape[0]])
                at[kw] += st.shape[0]
            if any(a != n for a in at):
                raise RuntimeError("the decoder reported status words for %s shots per window, the batch has %d" % (at, n))
            w0 = (shot0 - first) // 64
            tally.add(pred, obs, flags, None if mask is None else mask[w0:w0 + (n + 63) // 64])
            seen[i % 3:i % 3 + 1].copy_(tally.data[1:2], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            done.append(ev)
            issued += 1
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        counts = tally.counts()
        failing, truncated = np.zeros((0,), np.int64), False
        if mask is not None and issued:
            nwords = (batches[issued - 1][0] + batches[issued - 1][1] - first + 63) // 64
            failing, truncated = _mask_to_indices(mask[:nwords].cpu().numpy().view(np.uint64), first, int(keep_failures))
    if dist is not None:
        counts = reduce_vector(dist, counts, device="cuda")
    return MemExperimentResult.from_counts(counts, failing, truncated, seed, sampler, step, seconds)


def replay_shots(circuit, shot_indices, seed, sampler='circuit'):
    """The samples of the given shots of `seed`'s stream again: numpy bool (det [n, ndet], obs [n, nobs]) like `get_circuit_mem_result`,
    row i being shot shot_indices[i] -- e.g. `result.failing_shots` of `get_circuit_mem_pL`, to decode them with other settings.  Both
    samplers draw shot s from (seed, s, site) alone, so nothing but the index is needed."""
    from . import _lib
    _check_sampler(sampler)
    _lib.require_experiment(_lib.require_gpu())
    det, obs = _make_sampler(_as_circuit(circuit), sampler).sample_shots(shot_indices, int(seed))
    return det.cpu().numpy().astype(bool), obs.cpu().numpy().astype(bool)


# ---- the same experiment with the decoder's confidence in view ----------------------------------------------------------------------------
@dataclasses.dataclass
class PostSelectionResult:
    """What `get_postselected_pL` returns.  shots, errors, pL, sigma as in MemExperimentResult.  hist: int64 [6, 2, 1024], per field of
    quits_amd.soft.FIELDS the shots (plane 0) and the failing shots (plane 1) by bin of width 2^shifts[field] (soft.bin_of: negative values in
    bin 0, everything past the last bin in it).  `curve` and `at_rejection` read the acceptance curve of a field off it: the shots are
    accepted in ascending order of the field, a whole bin at a time."""
    shots: int
    errors: int
    pL: float
    sigma: float
    shifts: np.ndarray
    hist: np.ndarray
    seed: int = 0
    sampler: str = "circuit"
    batch: int = 0
    seconds: float = 0.0

    @classmethod
    def from_counts(cls, counts, shifts, hist, seed=0, sampler="circuit", batch=0, seconds=0.0):
        """From decoder.device.Tally's counters and decoder.device.SoftTally's histogram; every plane must add up to the counters."""
        from .soft import BINS, FIELDS
        c = np.asarray(counts, dtype=np.int64)
        h = np.asarray(hist, dtype=np.int64)
        shots, errors = int(c[0]), int(c[1])
        if h.shape != (len(FIELDS), 2, BINS):
            raise ValueError("the histogram must be [%d, 2, %d]" % (len(FIELDS), BINS))
        if not (np.all(h[:, 0].sum(axis=1) == shots) and np.all(h[:, 1].sum(axis=1) == errors)):
            raise ValueError("soft histograms and counters disagree: %s / %s shots in the planes, counters %d / %d"
                             % (h[:, 0].sum(axis=1).tolist(), h[:, 1].sum(axis=1).tolist(), shots, errors))
        pL, sigma = _rate(shots, errors)
        return cls(shots, errors, pL, sigma, np.asarray(shifts, dtype=np.int32).copy(), h.copy(), int(seed), str(sampler), int(batch), float(seconds))

    def _field(self, field):
        from .soft import FIELDS
        if isinstance(field, str):
            if field not in FIELDS:
                raise ValueError("field must be one of %s" % (FIELDS,))
            return FIELDS.index(field)
        return int(field)

    def curve(self, field):
        """(edge, kept, errors, pL, sigma), arrays of 1024 entries: accepting the shots whose `field` is at most edge[t] = (t + 1) * 2^shift - 1
        keeps kept[t] shots of which errors[t] fail (soft.selection_curve).  The last bin also holds every larger value, so the last entry is
        (shots, errors) whatever edge says."""
        from .soft import BINS, selection_curve
        i = self._field(field)
        edge = (np.arange(1, BINS + 1, dtype=np.int64) << np.int64(self.shifts[i])) - 1
        return (edge,) + selection_curve(self.hist[i])

    def at_rejection(self, field, fraction):
        """The loosest threshold of `field` that discards at least `fraction` of the shots: a dict with threshold (accept value <= threshold; None
        if even the first bin keeps too many, so that nothing is kept), kept, errors, pL, sigma and the fraction actually rejected -- whole bins
        are kept or dropped, so that is `fraction` or more."""
        if not 0.0 <= float(fraction) <= 1.0:
            raise ValueError("fraction must lie in [0, 1]")
        edge, kept, errors, pL, sigma = self.curve(field)
        ok = np.flatnonzero((self.shots - kept) >= float(fraction) * self.shots)
        if ok.size == 0:
            return {"threshold": None, "kept": 0, "errors": 0, "pL": float("nan"), "sigma": float("nan"), "rejected": 1.0 if self.shots else float("nan")}
        t = int(ok[-1])
        return {"threshold": int(edge[t]), "kept": int(kept[t]), "errors": int(errors[t]), "pL": float(pL[t]), "sigma": float(sigma[t]),
                "rejected": (self.shots - int(kept[t])) / self.shots if self.shots else float("nan")}


def get_postselected_pL(circuit, hz, lz, W, F, num_trials, max_iter=2, osd_order=0, bp_method='product_sum', schedule='serial',
                        osd_method=None, *, relay=None, seed=0, sampler='circuit', batch=None, shifts=None):
    """`get_circuit_mem_pL` with the decoder's confidence in view: every batch (experiment_batches') is sampled, decoded with its space-time
    correction and a soft record per shot (plan.decode(det, None, correction, soft); quits_amd/soft.py), tallied (Tally, whose fail mask
    says which shots failed) and binned (SoftTally: qd_soft_tally).  Nothing per shot reaches the host; it reads the counters and the
    [6, 2, 1024] histogram once at the end.  Same shots, same decoder, same cached plan as `get_circuit_mem_pL`: `shots`, `errors`, `pL`
    and `sigma` are its numbers.

    The decoder keywords are get_circuit_mem_pL's (osd_method None = its 'osd_cs'); relay: a quits_amd.relay.RelayConfig selects the
    sliding-window Relay-BP decoder as in get_relay_mem_pL (osd_method None = 'osd_off', and `osd_order` its post-processor's).
    sampler, seed, batch: as there.  shifts: six bin-width exponents (soft.FIELDS' order); default soft.default_shifts of the plan's committed
    weights and priors, the detector count, the window count and max_iter (Relay-BP: the configuration's total_iter).

    Returns a PostSelectionResult: `result.curve('weight')`, `result.at_rejection('iters', 0.05)`."""
    import time
    import torch
    from . import soft as _soft
    from .decoder.device import SoftTally, Tally
    decoder, opts = _decoder_choice(relay, max_iter, osd_order, bp_method, schedule, osd_method)
    su = _experiment_setup(circuit, hz, lz, W, F, decoder, opts, ("experiment", "faults", "soft"), sampler=sampler, batch=batch)
    smp, plan = su.sampler, su.plan
    batches = experiment_batches(num_trials, su.batch)
    if shifts is None:
        iters = relay.total_iter if relay is not None else (int(max_iter) if int(max_iter) > 0 else max(w["graph"].n for w in plan.windows))
        shifts = _soft.default_shifts(plan.commit_weights().cpu().numpy(), plan.commit_priors(), smp.m, len(plan.windows), iters)
    with plan.in_use():
        tally, stally = Tally(plan.nobs), SoftTally(shifts)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for shot0, n in batches:
            det, obs = smp.sample(n, seed, shot0)
            _, mask, rec = su.decode_tally(tally, det, obs, len(_soft.FIELDS))
            stally.add(rec, mask)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        counts, hist = tally.counts(), stally.result()
    return PostSelectionResult.from_counts(counts, stally.shifts, hist, seed, sampler, su.step, seconds)


# ---- the same experiment with the faults in view --------------------------------------------------------------------------------------
@dataclasses.dataclass
class FaultSpectrumResult(_ByFaults):
    """What `get_fault_spectrum` returns.  shots, errors, pL as in MemExperimentResult.  shots_by_faults[w], errors_by_faults[w]: shots /
    failing shots in which w faults of the detector error model fired (bin 255 collects w >= 255).  residual_shots: shots whose correction C
    does not reproduce the syndrome (H C != det; some window reported an inconsistent syndrome), failing_residual_shots: the failing ones
    among them.  residual_weight_hist[w]: failing shots with H C = det whose residual E xor C -- then an undetectable logical fault -- has
    weight w (bin 255: >= 255).  lightest: (weight, global shot index) of the lightest such residual, ties to the smaller index, or None: an
    explicit upper bound on the circuit-level distance; `replay_faults(circuit, [shot], seed)` regenerates its fault set."""
    shots: int
    errors: int
    pL: float
    shots_by_faults: np.ndarray
    errors_by_faults: np.ndarray
    residual_weight_hist: np.ndarray
    residual_shots: int
    failing_residual_shots: int
    lightest: object
    seed: int = 0
    batch: int = 0
    seconds: float = 0.0

    @classmethod
    def from_counts(cls, hist, counts, lightest, seed=0, batch=0, seconds=0.0):
        """From decoder.device.FaultStats.result(): hist int64 [3, 256], counts = (shots, failing, shots with H C != det, failing ones of those)."""
        h = np.asarray(hist, dtype=np.int64)
        c = np.asarray(counts, dtype=np.int64)
        shots, errors = int(c[0]), int(c[1])
        if int(h[0].sum()) != shots or int(h[1].sum()) != errors or int(h[2].sum()) != errors - int(c[3]):
            raise ValueError("fault histograms and counters disagree: %d / %d / %d shots in the histograms, counters %s"
                             % (h[0].sum(), h[1].sum(), h[2].sum(), c.tolist()))
        return cls(shots, errors, _rate(shots, errors)[0], h[0].copy(), h[1].copy(), h[2].copy(), int(c[2]), int(c[3]),
                   None if lightest is None else (int(lightest[0]), int(lightest[1])), int(seed), int(batch), float(seconds))


def get_fault_spectrum(circuit, hz, lz, W, F, num_trials, max_iter=2, osd_order=0, bp_method='product_sum', schedule='serial',
                       osd_method='osd_cs', *, seed=0, batch=None, shard=None):
    """`get_circuit_mem_pL(..., sampler='dem')` with the faults in view: every batch (experiment_batches') is sampled with its fault set E
    (DemSampler.sample_faults), decoded with its space-time correction C (plan.decode(..., correction=...)), tallied (Tally), and
    qd_fault_stats_batch bins the shots by |E|, the failing ones too, and the failing shots with H C = det by |E xor C|.  Nothing per shot
    reaches the host.  Same shots, same decoder, same cached plan as that call: `shots` and `errors` are its numbers.

    The shots always come from the circuit's detector error model: its columns (merged faults, detector_error_model_to_matrix) are what the
    decoder's correction is written in.  The noise sites of the circuit-level frame sampler are not DEM columns -- one site is several
    columns, several sites one column -- so there is no `sampler` argument here.

    Returns a FaultSpectrumResult; `replay_faults(circuit, [result.lightest[1]], seed)` regenerates the lightest residual's fault set."""
    import time
    import torch
    from .decoder.device import FaultStats, GF2Matrix, Tally
    decoder, opts = _decoder_choice(None, max_iter, osd_order, bp_method, schedule, osd_method)
    rank, world = (0, 1) if shard is None else (int(shard[0]), int(shard[1]))
    su = _experiment_setup(circuit, hz, lz, W, F, decoder, opts, ("experiment", "faults"), sampler="dem", columns=True, batch=batch)
    smp, plan = su.sampler, su.plan
    batches = experiment_batches(num_trials, su.batch, rank, world)
    if batches and batches[-1][0] + batches[-1][1] > 1 << 40:
        raise ValueError("shot indices must stay below 2^40")
    Hdev = GF2Matrix(su.H)
    with plan.in_use():
        tally, fstats = Tally(plan.nobs), FaultStats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for shot0, n in batches:
            det, obs, faults = smp.sample_faults(n, seed, shot0)
            su.decode_stats(Hdev, tally, fstats, det, obs, faults, shot0)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        hist, counts, lightest = fstats.result()
        tc = tally.counts()
    if int(tc[0]) != int(counts[0]) or int(tc[1]) != int(counts[1]):
        raise RuntimeError("the tally counted %d shots and %d failures, the fault statistics %d and %d" % (tc[0], tc[1], counts[0], counts[1]))
    return FaultSpectrumResult.from_counts(hist, counts, lightest, seed, su.step, seconds)


def replay_faults(circuit, shot_indices, seed):
    """Which faults of the circuit's detector error model fired in the given shots of `seed`'s DEM-sampled stream (get_fault_spectrum's, and
    get_circuit_mem_pL's with sampler='dem'): numpy bool [len(shot_indices), nfaults], column j = column j of
    detector_error_model_to_matrix(circuit)."""
    from . import _lib
    _lib.require_faults(_lib.require_experiment(_lib.require_gpu()))
    smp = _make_sampler(_as_circuit(circuit), "dem")
    return _fault_rows(smp.sample_shots_faults(shot_indices, int(seed))[2], smp.nfaults)


# ---- the same experiment, stratified by the number of faults -----------------------------------------------------------------------------
@dataclasses.dataclass
class StratifiedResult(_ByFaults):
    """What `get_stratified_pL` returns.  shots_by_faults[k], errors_by_faults[k] (int64 [256]): shots drawn with exactly k faults and the
    failing ones among them; pmf[k] = P(|E| = k) under the detector error model (float64 [256]), tail = P(|E| > 255).
    pL = sum over the sampled k of pmf_k f_k, f_k = errors_k / shots_k; sigma = sqrt(sum pmf_k^2 f_k (1 - f_k) / shots_k);
    unsampled_mass = the pmf of the strata without shots + tail, so that pL <= truth <= pL + unsampled_mass (up to sigma).
    sigma adds the strata's variances, as for independent strata.  The strata of one seed share their Philox words -- shot s of stratum k and
    of stratum k + 1 make the same draws against neighbouring thresholds -- so their f are positively correlated and sigma understates the spread
    of a pL summed over many strata; sigma_max = sum pmf_k sqrt(f_k (1 - f_k) / shots_k) bounds it whatever the correlation.
    residual_weight_hist, residual_shots, failing_residual_shots: as in FaultSpectrumResult.  lightest: (weight, k, shot) of the lightest
    undetectable residual E xor C seen -- ties to the smaller k, then the smaller shot -- or None;
    `replay_strata_faults(circuit, k, [shot], seed)` regenerates its fault set."""
    shots_by_faults: np.ndarray
    errors_by_faults: np.ndarray
    pmf: np.ndarray
    tail: float
    pL: float
    sigma: float
    unsampled_mass: float
    residual_weight_hist: np.ndarray
    residual_shots: int
    failing_residual_shots: int
    lightest: object
    seed: int = 0
    batch: int = 0
    seconds: float = 0.0
    sigma_max: float = 0.0

    @classmethod
    def from_counts(cls, shots_by_faults, errors_by_faults, pmf, tail, residual_weight_hist=None, residual_shots=0, failing_residual_shots=0,
                    lightest=None, seed=0, batch=0, seconds=0.0):
        from .strata import estimate
        s = np.asarray(shots_by_faults, dtype=np.int64).copy()
        e = np.asarray(errors_by_faults, dtype=np.int64).copy()
        pmf = np.asarray(pmf, dtype=np.float64).copy()
        pL, sigma, unsampled = estimate(s, e, pmf, tail)
        rw = np.zeros(s.shape, np.int64) if residual_weight_hist is None else np.asarray(residual_weight_hist, dtype=np.int64).copy()
        on = s[:pmf.shape[0]] > 0
        f = e[:pmf.shape[0]][on] / s[:pmf.shape[0]][on]
        sigma_max = float(np.sum(pmf[on] * np.sqrt(f * (1.0 - f) / s[:pmf.shape[0]][on])))
        return cls(s, e, pmf, float(tail), pL, sigma, unsampled, rw, int(residual_shots), int(failing_residual_shots),
                   None if lightest is None else tuple(int(x) for x in lightest), int(seed), int(batch), float(seconds), sigma_max)


def _strata_plan(shots_per_weight):
    """[(k, N_k), ...] ascending in k, the strata with N_k > 0 of a mapping k -> N_k; ValueError on a k outside 0 .. 255 or a negative count."""
    from .strata import KMAX_LIMIT
    out = []
    for k, nk in sorted((int(k), int(nk)) for k, nk in dict(shots_per_weight).items()):
        if k < 0 or k > KMAX_LIMIT:
            raise ValueError("stratum %d outside 0 .. %d (the last bin of the fault histograms)" % (k, KMAX_LIMIT))
        if nk < 0:
            raise ValueError("stratum %d: negative shot count" % k)
        if nk > 1 << 40:
            raise ValueError("shot indices must stay below 2^40")
        if nk:
            out.append((k, nk))
    return out


def get_stratified_pL(circuit, hz, lz, W, F, shots_per_weight, max_iter=2, osd_order=0, bp_method='product_sum', schedule='serial',
                      osd_method='osd_cs', *, seed=0, batch=None):
    """`get_fault_spectrum` on shots that hold a prescribed number of faults: for every k of the mapping `shots_per_weight` (k -> N_k),
    shots 0 .. N_k - 1 of stratum k's stream are drawn from the detector error model conditioned on |E| = k
    (decoder.device.StratifiedDemSampler), decoded with their space-time correction, tallied and binned exactly as there -- same cached
    plan, same decoder keywords, nothing per shot on the host.  f(k) is thereby measured where independent faults put no mass (the light
    sets that bound the distance, the heavy tail at low p), and pL = sum_k P(|E| = k) f(k) follows with the bound of StratifiedResult.
    A row depends on (seed, shot, k) alone: the result does not depend on `batch`.

    Returns a StratifiedResult."""
    import time
    import torch
    from . import _lib
    from . import strata as st
    from .decoder.device import FaultStats, GF2Matrix, Tally
    decoder, opts = _decoder_choice(None, max_iter, osd_order, bp_method, schedule, osd_method)
    su = _experiment_setup(circuit, hz, lz, W, F, decoder, opts, ("experiment", "faults"), columns=True, strata=shots_per_weight, batch=batch)
    smp, plan, todo = su.sampler, su.plan, su.strata
    pmf, tail = st.fault_count_pmf(su.priors, st.KMAX_LIMIT)
    Hdev = GF2Matrix(su.H)
    shots_by = np.zeros(_lib.FAULT_HIST, np.int64)
    errors_by = np.zeros(_lib.FAULT_HIST, np.int64)
    rw = np.zeros(_lib.FAULT_HIST, np.int64)
    res_shots = fail_res_shots = 0
    lightest = None
    with plan.in_use():
        strata_stats = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k, nk in todo:
            tally, fstats = Tally(plan.nobs), FaultStats()             # per stratum: the lightest residual is then known with its k
            for shot0, n in experiment_batches(nk, su.batch):
                det, obs, faults = smp.sample_faults(k, seed, shot0, shots=n)
                su.decode_stats(Hdev, tally, fstats, det, obs, faults, shot0)
            strata_stats.append((k, nk, tally, fstats))
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        for k, nk, tally, fstats in strata_stats:
            hist, counts, best = fstats.result()
            tc = tally.counts()
            if int(tc[0]) != nk or int(counts[0]) != nk or int(tc[1]) != int(counts[1]):
                raise RuntimeError("stratum %d: %d shots asked for, the tally counted %d (%d failing), the fault statistics %d (%d failing)"
                                   % (k, nk, tc[0], tc[1], counts[0], counts[1]))
            if int(hist[0][k]) != nk or int(hist[1][k]) != int(counts[1]):
                raise RuntimeError("stratum %d: the sampled rows do not all hold %d faults (histogram %s)" % (k, k, np.flatnonzero(hist[0]).tolist()))
            shots_by[k], errors_by[k] = nk, int(counts[1])
            rw += hist[2]
            res_shots += int(counts[2])
            fail_res_shots += int(counts[3])
            if best is not None and (lightest is None or best[0] < lightest[0]):
                lightest = (int(best[0]), k, int(best[1]))
    return StratifiedResult.from_counts(shots_by, errors_by, pmf, tail, rw, res_shots, fail_res_shots, lightest, seed, su.step, seconds)


def replay_strata_faults(circuit, k, shot_indices, seed):
    """The fault sets of the given shots of stratum k of `seed`'s stream (get_stratified_pL's): numpy bool [len(shot_indices), nfaults] with
    exactly k ones per row, column j = column j of detector_error_model_to_matrix(circuit)."""
    from . import _lib
    from .decoder.base import detector_error_model_to_matrix
    from .decoder.device import StratifiedDemSampler
    _lib.require_strata(_lib.require_faults(_lib.require_gpu()))
    H, L, priors = detector_error_model_to_matrix(_as_circuit(circuit).detector_error_model())
    smp = StratifiedDemSampler(H, L, priors, int(k))
    return _fault_rows(smp.sample_shots_faults(shot_indices, int(k), int(seed))[2], smp.nfaults)


# ---- failing fault sets shrunk to 1-minimal ones ------------------------------------------------------------------------------------------
@dataclasses.dataclass
class MinimalFailuresResult:
    """What `get_minimal_failures` returns.  shots, errors: decoded shots and failing ones, `get_fault_spectrum`'s numbers (with
    shots_per_weight: `get_stratified_pL`'s, summed over the strata).  parents: failing shots that were shrunk -- the first `max_parents` in
    shot order -- and parents_truncated: failing shots beyond them, counted only.  Per parent, in that order: parent_shots (global shot
    index; with strata the index inside the stratum parent_strata[i]), start_weights = |E|, weights = |S| of the 1-minimal set S it ended on,
    minimal (the walk of quits_amd/shrink.py ended: True for every parent of a finished run), trials (decodes spent on it).
    start_weight_hist[w], weight_hist[w] (int64 [256], bin 255: >= 255): parents by |E| and by |S|.  lightest: (|S|, shot) of the lightest final
    set, ties to the earlier parent, or None: the decoder fails on a set of that many faults, so pL falls no faster than p^|S|.
    sets, set_shots, set_weights (set_strata): the `keep_sets` lightest final sets, packed int32 [., ceil(nfaults / 32)] words (bit j & 31 of
    word j >> 5 = column j of detector_error_model_to_matrix), lightest first.  residual_weight_hist[w]: final sets whose correction C
    reproduces the syndrome, by the weight of S xor C -- an undetectable logical fault; lightest_residual: (weight, shot) of the lightest, or
    None: an upper bound on the circuit-level distance.  rounds: decode rounds of the shrink (the longest walk), decodes: trial rows it
    decoded; seconds: the whole call, timing: its parts -- "find" (sample, decode, gather), "shrink", "final" (the final sets decoded once with
    their corrections), and with profile=True "shrink_decode", the part of "shrink" inside plan.decode (a device synchronise around every
    call: a profiling mode, it slows the run)."""
    shots: int
    errors: int
    parents: int
    parents_truncated: int
    start_weight_hist: np.ndarray
    weight_hist: np.ndarray
    lightest: object
    sets: np.ndarray
    set_shots: np.ndarray
    set_weights: np.ndarray
    residual_weight_hist: np.ndarray
    lightest_residual: object
    rounds: int
    decodes: int
    seconds: float
    parent_shots: np.ndarray = None
    start_weights: np.ndarray = None
    weights: np.ndarray = None
    minimal: np.ndarray = None
    trials: np.ndarray = None
    parent_strata: object = None
    set_strata: object = None
    seed: int = 0
    batch: int = 0
    timing: dict = dataclasses.field(default_factory=dict)


def _decoder_choice(relay, max_iter, osd_order, bp_method, schedule, osd_method):
    """(plug-in class, its keyword dict -- the cached plan's key) of the BP + OSD / LSD keywords, or of Relay-BP where `relay` is a RelayConfig."""
    if relay is None:
        from .decoder.bposd import BpOsdDecoder
        return BpOsdDecoder, {'bp_method': bp_method, 'max_iter': max_iter, 'schedule': schedule,
                              'osd_method': 'osd_cs' if osd_method is None else osd_method, 'osd_order': osd_order}
    from .decoder.relaybp import RelayBpDecoder, relay_options
    return RelayBpDecoder, relay_options(relay, 'osd_off' if osd_method is None else osd_method, osd_order)


def _shrink_on_plan(plan, shr, sets, batch, timing=None):
    """The one loop of shrink_fault_sets and get_minimal_failures (inside plan.in_use()): `shr`, a decoder.device.FaultShrinker, walks the packed
    `sets`; every round's trial rows are decoded by `plan` in pieces of `batch` rows and tallied, and the fail mask goes back to the shrinker.
    Per round the host learns the number of live parents, nothing else.  Returns the number of trial rows decoded.  timing: a dict that
    receives "shrink_decode", the seconds inside plan.decode, measured with a device synchronise on either side of every call, and what the
    status words say of the trial rows: "trial_mean_iterations" (BP iterations per row and window), "trial_unconverged_share" (rows of a
    window BP did not solve: the post-processor's, or with 'osd_off' returned as they were) and "trial_later_leg_share" (rows whose status
    word has a bit of the Relay-BP leg field set: with Relay-BP the rows whose output came from a leg after the first; other decoders do not
    define the field)."""
    import time
    import torch
    from . import _lib
    from .decoder.device import Tally
    step = _batch_step(batch)
    tally = Tally(plan.nobs)
    decodes = 0
    inside = 0.0
    seen = torch.zeros((4,), dtype=torch.int64, device="cuda") if timing is not None else None      # status words, iterations, converged, leg >= 1
    shr.begin(sets)
    while not shr.done:
        det, obs, _, _ = shr.trials()
        A = det.shape[0]
        mask = torch.empty(((A + 63) // 64,), dtype=torch.int64, device=det.device)
        for c0 in range(0, A, step):
            n = min(step, A - c0)
            if timing is not None:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            stats = None if timing is None else []
            pred = plan.decode(det[c0:c0 + n], stats)
            if timing is not None:
                torch.cuda.synchronize()
                inside += time.perf_counter() - t0
                for _, st in stats:
                    seen += torch.stack([torch.tensor(st.numel(), device=st.device), (st & _lib.STATUS_ITER_MASK).sum(),
                                         ((st & _lib.STATUS_CONVERGED) != 0).sum(), ((st & _lib.STATUS_RELAY_LEG_MASK) != 0).sum()])
            tally.add(pred, obs[c0:c0 + n], None, mask[c0 // 64:c0 // 64 + (n + 63) // 64])
        shr.commit(mask)
        decodes += A
    if timing is not None:
        timing["shrink_decode"] = inside
        words, iters, conv, later = (int(x) for x in seen.cpu())
        if words:
            timing.update(trial_mean_iterations=iters / words, trial_unconverged_share=1.0 - conv / words, trial_later_leg_share=later / words)
    return decodes


def shrink_fault_sets(circuit, hz, lz, W, F, fault_sets, max_iter=2, osd_order=0, bp_method='product_sum', schedule='serial', osd_method=None,
                      *, relay=None, batch=None):
    """Shrink fault sets of the circuit's detector error model to 1-minimal failing ones (quits_amd/shrink.py states the walk): a set S fails
    iff the sliding-window decoder's prediction for the detector bits H S differs from L S.  The decoder keywords are
    `sliding_window_bposd_circuit_mem`'s (same cached plan); relay=RelayConfig switches to the Relay-BP plan of
    `sliding_window_relaybp_circuit_mem`.  osd_method None: 'osd_cs', with `relay` 'osd_off'.  The trial rows are made, decoded and judged on
    the device (decoder.device.FaultShrinker); the host reads one count per round.

    fault_sets: bool [P, nfaults] (column j = column j of detector_error_model_to_matrix), or packed int32 [P, ceil(nfaults / 32)] words (numpy
    or a cuda tensor; bit j & 31 of word j >> 5).  batch: rows per decode call (default: as in get_fault_spectrum); no result depends on it.

    Returns a quits_amd.shrink.ShrinkResult: sets in the form they came in (packed ones as numpy), fails, minimal, start_weight, weight,
    trials per parent.  A parent that does not fail comes back unchanged with fails = False."""
    import torch
    from . import shrink as sk
    from .decoder.device import FaultShrinker
    decoder, opts = _decoder_choice(relay, max_iter, osd_order, bp_method, schedule, osd_method)
    su = _experiment_setup(circuit, hz, lz, W, F, decoder, opts, ("experiment", "faults", "shrink"), columns=True, batch=batch)
    plan, n, words = su.plan, su.plan.nfaults, su.words
    packed_in = isinstance(fault_sets, torch.Tensor) or (np.asarray(fault_sets).dtype != np.bool_ and np.asarray(fault_sets).ndim == 2
                                                         and np.asarray(fault_sets).shape[1] != n)
    if packed_in:
        sets = fault_sets if isinstance(fault_sets, torch.Tensor) else np.ascontiguousarray(fault_sets, dtype=np.int32)
        if sets.ndim != 2 or sets.shape[1] < words:
            raise ValueError("packed fault sets must be int32 [parents, >= %d] words" % words)
    else:
        bits = np.asarray(fault_sets)
        if bits.ndim != 2 or bits.shape[1] != n:
            raise ValueError("fault_sets must be a [parents, %d] array, one column per fault of the detector error model" % n)
        sets = sk.pack_sets(bits != 0)
    shr = FaultShrinker(su.H, su.L)
    with plan.in_use():
        _shrink_on_plan(plan, shr, sets, su.batch)
        res = shr.result()
    if not packed_in:
        res.sets = sk.unpack_sets(res.sets, n)
    return res


def _failing_rows(mask, n):
    """Ascending row indices (cuda int64) of the set bits of a fail mask over n rows."""
    import torch
    bits = (mask[:(n + 63) // 64, None] >> torch.arange(64, device=mask.device, dtype=torch.int64)[None, :]) & 1
    return torch.nonzero(bits.reshape(-1)[:n], as_tuple=False).reshape(-1)


def get_minimal_failures(circuit, hz, lz, W, F, num_trials, max_iter=2, osd_order=0, bp_method='product_sum', schedule='serial',
                         osd_method='osd_cs', *, seed=0, batch=None, shots_per_weight=None, max_parents=1 << 16, keep_sets=256, profile=False):
    """`get_fault_spectrum`, and then every failing shot's fault set shrunk to a 1-minimal failing set: the same `num_trials` DEM-sampled shots
    of `seed` (same rows, same decoder keywords, same cached plan, so `shots` and `errors` are that function's), the failing rows gathered on
    the device, shrunk there in one run (quits_amd/shrink.py; decoder.device.FaultShrinker; a trial is one decode), and the final sets decoded
    once more with their space-time corrections for the residuals S xor C.  With shots_per_weight (k -> N_k) the shots are
    `get_stratified_pL`'s instead -- N_k rows of exactly k faults per stratum, same rows for the same seed -- and `num_trials` is ignored.

    max_parents: failing shots beyond the first `max_parents` are counted (parents_truncated), not shrunk.  keep_sets: how many of the
    lightest final sets to return.  batch: as in get_fault_spectrum; the result does not depend on it.  profile: see MinimalFailuresResult.

    Returns a MinimalFailuresResult.  `replay_faults(circuit, [shot], seed)` (`replay_strata_faults` with strata) regenerates the parent of a
    set; `shrink_fault_sets` shrinks given sets."""
    decoder, opts = _decoder_choice(None, max_iter, osd_order, bp_method, schedule, osd_method)
    return _minimal_failures(circuit, hz, lz, W, F, num_trials, decoder, opts, seed=seed, batch=batch, shots_per_weight=shots_per_weight,
                             max_parents=max_parents, keep_sets=keep_sets, profile=profile)


def get_relay_minimal_failures(circuit, hz, lz, W, F, num_trials, relay=None, osd_method='osd_off', osd_order=0, *, seed=0, batch=None,
                               shots_per_weight=None, max_parents=1 << 16, keep_sets=256, profile=False):
    """`get_minimal_failures` with the sliding-window Relay-BP decoder (the plan of `get_relay_mem_pL`): `relay` is a quits_amd.relay.RelayConfig
    (default RelayConfig()), `osd_method` / `osd_order` the post-processor of the shots no leg solves.  Every other argument and the result are
    that function's."""
    from .relay import RelayConfig
    decoder, opts = _decoder_choice(RelayConfig() if relay is None else relay, 0, osd_order, None, None, osd_method)
    return _minimal_failures(circuit, hz, lz, W, F, num_trials, decoder, opts, seed=seed, batch=batch, shots_per_weight=shots_per_weight,
                             max_parents=max_parents, keep_sets=keep_sets, profile=profile)


def _minimal_failures(circuit, hz, lz, W, F, num_trials, decoder, opts, *, seed, batch, shots_per_weight, max_parents, keep_sets, profile):
    """The loop of get_minimal_failures and get_relay_minimal_failures: `decoder` is the plug-in class of both window kinds, `opts` its keyword
    dict (the cached plan's key)."""
    import time
    import torch
    from . import _lib
    from .decoder.device import FaultShrinker, FaultStats, Tally
    t_start = time.perf_counter()
    if int(max_parents) < 0 or int(keep_sets) < 0:
        raise ValueError("max_parents and keep_sets must not be negative")
    su = _experiment_setup(circuit, hz, lz, W, F, decoder, opts, ("experiment", "faults", "shrink"), sampler="dem", columns=True,
                           strata=shots_per_weight, batch=batch)
    smp, plan, todo, batch, step, words = su.sampler, su.plan, su.strata, su.batch, su.step, su.words
    nobs = plan.nobs
    if todo is None:
        work = [(None, shot0, n) for shot0, n in experiment_batches(num_trials, batch)]
    else:
        work = [(k, shot0, n) for k, nk in todo for shot0, n in experiment_batches(nk, batch)]
    if work and max(shot0 + n for _, shot0, n in work) > 1 << 40:
        raise ValueError("shot indices must stay below 2^40")
    shr = FaultShrinker(su.H, su.L)
    timing = {}
    with plan.in_use():
        tally = Tally(nobs)
        got_sets, got_shots, got_strata = [], [], []
        kept = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k, shot0, n in work:
            det, obs, faults = smp.sample_faults(n, seed, shot0) if k is None else smp.sample_faults(k, seed, shot0, shots=n)
            pred = plan.decode(det)
            mask = torch.empty(((n + 63) // 64,), dtype=torch.int64, device="cuda")
            tally.add(pred, obs, None, mask)
            if kept < max_parents:
                rows = _failing_rows(mask, n)[:max_parents - kept]
                if rows.numel():
                    got_sets.append(faults[:, :words].index_select(0, rows))
                    got_shots.append(rows + shot0)
                    got_strata.append(torch.full_like(rows, -1 if k is None else k))
                    kept += int(rows.numel())
        sets = torch.cat(got_sets) if got_sets else torch.zeros((0, words), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        decodes = _shrink_on_plan(plan, shr, sets, batch, timing if profile else None)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        P = int(sets.shape[0])
        fstats, final = FaultStats(), Tally(nobs)
        for c0 in range(0, P, step):
            n = min(step, P - c0)
            det = shr.kept_det[c0:c0 + n].clone()                  # a copy: the step turns it into the residual H C xor H S
            su.decode_stats(shr.H, final, fstats, det, shr.kept_obs[c0:c0 + n], shr.sets[c0:c0 + n], c0)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        tc = tally.counts()
        res = shr.result()
        hist, counts, best = fstats.result()
        parent_shots = torch.cat(got_shots).cpu().numpy() if got_shots else np.zeros((0,), np.int64)
        parent_strata = torch.cat(got_strata).cpu().numpy() if got_strata else np.zeros((0,), np.int64)
    timing.update(find=t1 - t0, shrink=t2 - t1, final=t3 - t2)
    shots, errors = int(tc[0]), int(tc[1])
    if not res.fails.all() or P != min(errors, int(max_parents)):
        raise RuntimeError("%d failing shots, %d parents gathered, %d of them fail when decoded again: the decoder does not return the same "
                           "bits for a row whatever batch it sits in" % (errors, P, int(res.fails.sum())))
    if int(counts[1]) != P:
        raise RuntimeError("%d final sets, %d of them fail when decoded with their corrections" % (P, int(counts[1])))
    clip = lambda w: np.bincount(np.minimum(w, _lib.FAULT_HIST - 1), minlength=_lib.FAULT_HIST).astype(np.int64)
    weight_hist = clip(res.weight)
    if not np.array_equal(weight_hist, hist[1]):
        raise RuntimeError("the final sets' weights disagree: the shrinker's state %s, the sets %s" % (np.flatnonzero(weight_hist).tolist(), np.flatnonzero(hist[1]).tolist()))
    order = np.lexsort((np.arange(P), res.weight))                 # lightest first, ties to the earlier parent
    top = order[:int(keep_sets)]
    strata_of = (lambda a: None) if todo is None else (lambda a: a.copy())
    return MinimalFailuresResult(
        shots, errors, P, errors - P, clip(res.start_weight), weight_hist,
        (int(res.weight[order[0]]), int(parent_shots[order[0]])) if P else None,
        res.sets[top].copy(), parent_shots[top].copy(), res.weight[top].copy(), hist[2].copy(),
        None if best is None else (int(best[0]), int(parent_shots[int(best[1])])),
        int(shr.rounds), int(decodes), time.perf_counter() - t_start, parent_shots, res.start_weight, res.weight, res.minimal, res.trials,
        strata_of(parent_strata), strata_of(parent_strata[top]), int(seed), step, timing)
