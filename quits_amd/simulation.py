"""Monte-Carlo drivers around the decoder, mirroring `/root/reference/src/quits/simulation.py`.

  get_codecap_pL       <- simulation.py:31-61   code-capacity logical error rate of a decoder plug-in
  get_stim_mem_result  <- simulation.py:8-28    detector / observable samples of a memory circuit
  get_circuit_mem_result                        the same samples from the circuit itself on the device (Pauli-frame simulation)
  get_circuit_mem_pL                            a whole memory experiment on the device: sampler -> sliding-window BP-OSD -> tallies; what
                                                the reference's users write around the two calls above (tests/test_sliding_window.py:72-83),
                                                without a host array per shot
  get_relay_mem_pL                              the same experiment with the sliding-window Relay-BP decoder
  replay_shots                                  the samples of given shot indices again (both samplers are counter-based)
  get_fault_spectrum                            the same experiment on DEM-sampled shots with the faults in view: shots and failures by the
                                                number of sampled faults, the residual E xor C of the failing shots, the lightest one seen
  replay_faults                                 which faults fired in given shots of the DEM sampler
  get_stratified_pL                             the same experiment on shots with a prescribed number of faults (subset sampling): f(k) where
                                                independent faults put no mass, pL = sum_k P(|E| = k) f(k) with an explicit truncation bound
  replay_strata_faults                          the fault sets of given shots of a stratum

`get_codecap_pL` keeps the reference's signature and its random stream (`np.random.seed(seed)` followed by one
`np.random.binomial(1, p, n)` per trial), so a given seed produces the same noise vectors as the reference.  With a plug-in
that decodes batches (`quits_amd.decoder.BpOsdDecoder`: it has `decode_batch`) all trials go through the device decoder in
one call; any other plug-in class runs the reference's per-trial loop on the host.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np


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
        pL = errors / shots if shots else float("nan")
        sigma = math.sqrt(pL * (1.0 - pL) / shots) if shots else float("nan")
        flagged = {name: (int(c[2 + 2 * j]), int(c[3 + 2 * j])) for j, name in enumerate(SHOT_FLAG_NAMES)}
        return cls(shots, errors, pL, sigma, c[TALLY_HEAD:].copy(), flagged, np.asarray(failing_shots, dtype=np.int64), bool(failures_truncated),
                   int(seed), str(sampler), int(batch), float(seconds), shots / seconds if seconds > 0 else 0.0)


def _as_circuit(circuit):
    from .dem import Circuit
    return circuit if isinstance(circuit, Circuit) else Circuit(str(circuit))


def _make_sampler(circ, sampler):
    from .decoder.device import CircuitSampler, DemSampler
    if sampler == "circuit":
        return CircuitSampler(circ)
    if sampler == "dem":
        from .decoder.base import detector_error_model_to_matrix
        H, L, priors = detector_error_model_to_matrix(circ.detector_error_model())
        return DemSampler(H, L, priors)
    raise ValueError("sampler must be 'circuit' or 'dem'")


def _mask_to_indices(words, shot0, limit):
    """Ascending global indices of the set bits of a fail mask (uint64 words, bit l of word w = shot shot0 + 64 w + l): at most `limit`, and
    whether there were more.  Only the non-zero words are unpacked."""
    nz = np.flatnonzero(words)
    bits = np.unpackbits(words[nz].astype("<u8").view(np.uint8).reshape(-1, 8), axis=1, bitorder="little").astype(bool)
    idx = (np.int64(shot0) + nz.astype(np.int64)[:, None] * 64 + np.arange(64, dtype=np.int64)[None, :])[bits]
    return idx[:limit], idx.shape[0] > limit


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
    import warnings
    from . import _lib
    from .decoder.base import window_count
    from .decoder.plan import cached_circuit_plan
    if F == 0:
        raise ValueError("Input parameter F cannot be zero.")
    if sampler not in ("circuit", "dem"):
        raise ValueError("sampler must be 'circuit' or 'dem'")
    _lib.require_experiment(_lib.require_gpu())           # no GPU or no library: RuntimeError, there is no CPU fallback
    import torch
    from .decoder.device import Tally, shot_flags_fold
    from .parallel import env_rank_world, init_distributed, reduce_vector
    dist = None
    rank, world = (0, 1) if shard is None else (int(shard[0]), int(shard[1]))
    if distributed:
        env_rank, env_world, local = env_rank_world()
        if env_world > 1:
            torch.cuda.set_device(local % torch.cuda.device_count())    # one process per GPU; the plan, the samplers and RCCL follow the current device
        dist = init_distributed()
        if shard is None:
            rank, world = env_rank, env_world
    circ = _as_circuit(circuit)
    smp = _make_sampler(circ, sampler)
    nz = hz.shape[0]
    num_rounds = smp.m // nz - 2
    if window_count(num_rounds, W, F)[2]:
        warnings.warn("Window size larger than the syndrome extraction rounds: Doing whole history correction")
    plan = cached_circuit_plan(circ, hz, W, F, num_rounds, decoder, decoder, opts, opts)
    k = plan.nobs
    if smp.nobs != k or np.asarray(lz.shape)[0] != k:
        raise ValueError("the circuit has %d observables, lz %d rows, the window plan commits %d" % (smp.nobs, lz.shape[0], k))
    if batch is None:
        batch = max(2, int(plan.lanes) if plan.pipeline else 2) * int(plan.chunk)
    batches = experiment_batches(num_trials, batch, rank, world)
    step = _batch_step(batch)
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
    _lib.require_experiment(_lib.require_gpu())
    det, obs = _make_sampler(_as_circuit(circuit), sampler).sample_shots(shot_indices, int(seed))
    return det.cpu().numpy().astype(bool), obs.cpu().numpy().astype(bool)


# ---- the same experiment with the faults in view --------------------------------------------------------------------------------------
@dataclasses.dataclass
class FaultSpectrumResult:
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

    def failure_fraction(self):
        """f(w) = errors_by_faults[w] / shots_by_faults[w], float64 [256]; NaN where no shot had w faults."""
        s = self.shots_by_faults.astype(np.float64)
        return np.divide(self.errors_by_faults.astype(np.float64), s, out=np.full(s.shape, np.nan), where=s > 0)

    @classmethod
    def from_counts(cls, hist, counts, lightest, seed=0, batch=0, seconds=0.0):
        """From decoder.device.FaultStats.result(): hist int64 [3, 256], counts = (shots, failing, shots with H C != det, failing ones of those)."""
        h = np.asarray(hist, dtype=np.int64)
        c = np.asarray(counts, dtype=np.int64)
        shots, errors = int(c[0]), int(c[1])
        if int(h[0].sum()) != shots or int(h[1].sum()) != errors or int(h[2].sum()) != errors - int(c[3]):
            raise ValueError("fault histograms and counters disagree: %d / %d / %d shots in the histograms, counters %s"
                             % (h[0].sum(), h[1].sum(), h[2].sum(), c.tolist()))
        return cls(shots, errors, errors / shots if shots else float("nan"), h[0].copy(), h[1].copy(), h[2].copy(), int(c[2]), int(c[3]),
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
    import warnings
    from . import _lib
    from .decoder.base import detector_error_model_to_matrix, window_count
    from .decoder.bposd import BpOsdDecoder
    from .decoder.plan import cached_circuit_plan
    if F == 0:
        raise ValueError("Input parameter F cannot be zero.")
    _lib.require_faults(_lib.require_experiment(_lib.require_gpu()))
    import torch
    from .decoder.device import DemSampler, FaultStats, GF2Matrix, Tally
    rank, world = (0, 1) if shard is None else (int(shard[0]), int(shard[1]))
    circ = _as_circuit(circuit)
    H, L, priors = detector_error_model_to_matrix(circ.detector_error_model())
    smp = DemSampler(H, L, priors)
    nz = hz.shape[0]
    num_rounds = smp.m // nz - 2
    if window_count(num_rounds, W, F)[2]:
        warnings.warn("Window size larger than the syndrome extraction rounds: Doing whole history correction")
    opts = {'bp_method': bp_method, 'max_iter': max_iter, 'schedule': schedule, 'osd_method': osd_method, 'osd_order': osd_order}
    plan = cached_circuit_plan(circ, hz, W, F, num_rounds, BpOsdDecoder, BpOsdDecoder, opts, opts)
    k = plan.nobs
    if smp.nobs != k or np.asarray(lz.shape)[0] != k:
        raise ValueError("the circuit has %d observables, lz %d rows, the window plan commits %d" % (smp.nobs, lz.shape[0], k))
    if plan.nfaults != smp.nfaults:
        raise ValueError("the windows commit %d faults, the detector error model has %d" % (plan.nfaults, smp.nfaults))
    if batch is None:
        batch = max(2, int(plan.lanes) if plan.pipeline else 2) * int(plan.chunk)
    batches = experiment_batches(num_trials, batch, rank, world)
    if batches and batches[-1][0] + batches[-1][1] > 1 << 40:
        raise ValueError("shot indices must stay below 2^40")
    Hdev = GF2Matrix(H)
    words = (plan.nfaults + 31) // 32
    with plan.in_use():
        tally, fstats = Tally(k), FaultStats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for shot0, n in batches:
            det, obs, faults = smp.sample_faults(n, seed, shot0)
            corr = torch.empty((n, words), dtype=torch.int32, device="cuda")
            pred = plan.decode(det, None, corr)
            mask = torch.empty(((n + 63) // 64,), dtype=torch.int64, device="cuda")
            tally.add(pred, obs, None, mask)
            Hdev.xor_apply(corr, det, accumulate=True)         # det is this batch's own: it becomes the residual H C xor det in place
            fstats.add(faults, corr, plan.nfaults, det, mask, shot0)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        hist, counts, lightest = fstats.result()
        tc = tally.counts()
    if int(tc[0]) != int(counts[0]) or int(tc[1]) != int(counts[1]):
        raise RuntimeError("the tally counted %d shots and %d failures, the fault statistics %d and %d" % (tc[0], tc[1], counts[0], counts[1]))
    return FaultSpectrumResult.from_counts(hist, counts, lightest, seed, _batch_step(batch), seconds)


def replay_faults(circuit, shot_indices, seed):
    """Which faults of the circuit's detector error model fired in the given shots of `seed`'s DEM-sampled stream (get_fault_spectrum's, and
    get_circuit_mem_pL's with sampler='dem'): numpy bool [len(shot_indices), nfaults], column j = column j of
    detector_error_model_to_matrix(circuit)."""
    from . import _lib
    _lib.require_faults(_lib.require_experiment(_lib.require_gpu()))
    smp = _make_sampler(_as_circuit(circuit), "dem")
    bits = smp.sample_shots_faults(shot_indices, int(seed))[2].cpu().numpy()
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, :smp.nfaults].astype(bool)


# ---- the same experiment, stratified by the number of faults -----------------------------------------------------------------------------
@dataclasses.dataclass
class StratifiedResult:
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

    def failure_fraction(self):
        """f(k) = errors_by_faults[k] / shots_by_faults[k], float64 [256]; NaN where stratum k has no shots."""
        s = self.shots_by_faults.astype(np.float64)
        return np.divide(self.errors_by_faults.astype(np.float64), s, out=np.full(s.shape, np.nan), where=s > 0)

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
    import warnings
    from . import _lib
    from . import strata as st
    from .decoder.base import detector_error_model_to_matrix, window_count
    from .decoder.bposd import BpOsdDecoder
    from .decoder.plan import cached_circuit_plan
    if F == 0:
        raise ValueError("Input parameter F cannot be zero.")
    todo = _strata_plan(shots_per_weight)
    _lib.require_strata(_lib.require_faults(_lib.require_experiment(_lib.require_gpu())))
    import torch
    from .decoder.device import FaultStats, GF2Matrix, StratifiedDemSampler, Tally
    circ = _as_circuit(circuit)
    H, L, priors = detector_error_model_to_matrix(circ.detector_error_model())
    pmf, tail = st.fault_count_pmf(priors, st.KMAX_LIMIT)
    smp = StratifiedDemSampler(H, L, priors, max([k for k, _ in todo], default=0))
    if todo:
        st.check_ks(np.array([k for k, _ in todo]), len(todo), priors, smp.kmax)
    nz = hz.shape[0]
    num_rounds = smp.m // nz - 2
    if window_count(num_rounds, W, F)[2]:
        warnings.warn("Window size larger than the syndrome extraction rounds: Doing whole history correction")
    opts = {'bp_method': bp_method, 'max_iter': max_iter, 'schedule': schedule, 'osd_method': osd_method, 'osd_order': osd_order}
    plan = cached_circuit_plan(circ, hz, W, F, num_rounds, BpOsdDecoder, BpOsdDecoder, opts, opts)
    nobs = plan.nobs
    if smp.nobs != nobs or np.asarray(lz.shape)[0] != nobs:
        raise ValueError("the circuit has %d observables, lz %d rows, the window plan commits %d" % (smp.nobs, lz.shape[0], nobs))
    if plan.nfaults != smp.nfaults:
        raise ValueError("the windows commit %d faults, the detector error model has %d" % (plan.nfaults, smp.nfaults))
    if batch is None:
        batch = max(2, int(plan.lanes) if plan.pipeline else 2) * int(plan.chunk)
    Hdev = GF2Matrix(H)
    words = (plan.nfaults + 31) // 32
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
            tally, fstats = Tally(nobs), FaultStats()                  # per stratum: the lightest residual is then known with its k
            for shot0, n in experiment_batches(nk, batch):
                det, obs, faults = smp.sample_faults(k, seed, shot0, shots=n)
                corr = torch.empty((n, words), dtype=torch.int32, device="cuda")
                pred = plan.decode(det, None, corr)
                mask = torch.empty(((n + 63) // 64,), dtype=torch.int64, device="cuda")
                tally.add(pred, obs, None, mask)
                Hdev.xor_apply(corr, det, accumulate=True)             # det becomes the residual H C xor det in place
                fstats.add(faults, corr, plan.nfaults, det, mask, shot0)
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
    return StratifiedResult.from_counts(shots_by, errors_by, pmf, tail, rw, res_shots, fail_res_shots, lightest, seed, _batch_step(batch), seconds)


def replay_strata_faults(circuit, k, shot_indices, seed):
    """The fault sets of the given shots of stratum k of `seed`'s stream (get_stratified_pL's): numpy bool [len(shot_indices), nfaults] with
    exactly k ones per row, column j = column j of detector_error_model_to_matrix(circuit)."""
    from . import _lib
    from .decoder.base import detector_error_model_to_matrix
    from .decoder.device import StratifiedDemSampler
    _lib.require_strata(_lib.require_faults(_lib.require_gpu()))
    H, L, priors = detector_error_model_to_matrix(_as_circuit(circuit).detector_error_model())
    smp = StratifiedDemSampler(H, L, priors, int(k))
    bits = smp.sample_shots_faults(shot_indices, int(k), int(seed))[2].cpu().numpy()
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, :smp.nfaults].astype(bool)
