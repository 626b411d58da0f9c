"""The decoders' soft outputs per shot, next to their logical predictions.

The reference returns predictions only.  A soft record (quits_amd/soft.py: FIELDS = weight, faults, events, iters, post, tail) says how sure
the decoder was of a shot: how unlikely the committed space-time correction is under the model's priors, how large it and the syndrome are,
how long BP ran, how many windows went to the post-processor and how many pivots (or which Relay-BP legs) those took.  The functions here
return the records through the same cached plans as `sliding_window_bposd_circuit_mem` / `sliding_window_bplsd_circuit_mem` / `decode_dem`:
the predictions are those calls', bit for bit.  `quits_amd.simulation.get_postselected_pL` turns the records into acceptance curves without
bringing them to the host.
"""
from __future__ import annotations

import warnings

import numpy as np

from .base import window_count
from .plan import cached_circuit_plan
from .whole_history import _dem_options, cached_dem_plan


def plan_soft_outputs(plan, zcheck_samples, corrections=False):
    """(logical_pred int64 [N, k], soft int64 [N, 6]) of any DeviceWindowPlan -- and, with corrections=True, the corrections as host
    PackedSamples behind them, as `plan.decode_host(..., corrections=True)` returns them.  Samples: what decode_host takes.  Pieces of
    `plan.host_piece` shots go to the device, through `plan.decode(det, None, correction, soft)`, and back."""
    from .. import _lib
    from . import pipeline
    _lib.require_soft(_lib.require_faults(_lib.require_gpu()))
    import torch
    from ..samples import PackedSamples
    if len(zcheck_samples.shape) != 2:
        raise ValueError("zcheck_samples must be a [shots, detectors] array")
    N = int(zcheck_samples.shape[0])
    words = (plan.nfaults + 31) // 32
    pred = np.zeros((N, plan.nobs), dtype=np.int64)
    soft = np.zeros((N, 6), dtype=np.int64)
    corr_words = np.zeros((N, words), dtype=np.int32) if corrections else None
    piece = max(int(plan.host_piece), 1)
    packed = isinstance(zcheck_samples, PackedSamples)
    with plan.in_use():
        dev = torch.device("cuda", plan.device) if plan.device >= 0 else torch.device("cuda")
        for lo in range(0, N, piece):
            hi = min(N, lo + piece)
            rows = zcheck_samples[lo:hi]
            det = pipeline._to_device_samples(rows if packed or isinstance(rows, torch.Tensor) else np.asarray(rows))
            if det.device != dev:
                raise RuntimeError("samples live on %s, the plan on %s" % (det.device, dev))
            corr = torch.empty((hi - lo, words), dtype=torch.int32, device=dev)
            rec = torch.empty((hi - lo, 6), dtype=torch.int64, device=dev)
            p = plan.decode(det, None, corr, rec)
            pred[lo:hi] = p.cpu().numpy()
            soft[lo:hi] = rec.cpu().numpy()
            if corrections:
                corr_words[lo:hi] = corr.cpu().numpy()
    if corrections:
        return pred, soft, pipeline.correction_words_to_packed(corr_words, plan.nfaults)
    return pred, soft


def sliding_window_soft_outputs(zcheck_samples, circuit, hz, lz, W, F, max_iter=2, osd_order=0, bp_method='product_sum', schedule='serial',
                                osd_method='osd_cs', lsd_method=None, lsd_order=None, *, corrections=False):
    """(logical_pred int64 [N, k], soft int64 [N, 6]) of the circuit-level sliding-window decoder: `sliding_window_corrections`' arguments,
    keywords and cached plan -- BP-OSD, or BP-LSD when `lsd_method` (or `lsd_order`) is given.  soft[:, i] is field quits_amd.soft.FIELDS[i];
    the weights of field 0 are `fault_weights` of the priors of detector_error_model_to_matrix(circuit)'s columns.  corrections=True appends
    `sliding_window_corrections`' PackedSamples as a third value."""
    from .bplsd import BpLsdDecoder
    from .bposd import BpOsdDecoder
    if F == 0:
        raise ValueError("Input parameter F cannot be zero.")
    from .. import _lib
    _lib.require_gpu()                                   # no GPU or no library: RuntimeError before anything is built
    nz = hz.shape[0]
    num_rounds = zcheck_samples.shape[1] // nz - 2
    if window_count(num_rounds, W, F)[2]:
        warnings.warn("Window size larger than the syndrome extraction rounds: Doing whole history correction")
    if lsd_method is not None or lsd_order is not None:
        cls = BpLsdDecoder
        opts = {'bp_method': bp_method, 'max_iter': max_iter, 'schedule': schedule, 'lsd_method': 'lsd_cs' if lsd_method is None else lsd_method,
                'lsd_order': 0 if lsd_order is None else lsd_order}
    else:
        cls = BpOsdDecoder
        opts = {'bp_method': bp_method, 'max_iter': max_iter, 'schedule': schedule, 'osd_method': osd_method, 'osd_order': osd_order}
    plan = cached_circuit_plan(circuit, hz, W, F, num_rounds, cls, cls, dict(opts), dict(opts))
    if np.asarray(lz).shape[0] != plan.nobs:
        raise ValueError("lz has %d rows, the window plan commits %d observables" % (np.asarray(lz).shape[0], plan.nobs))
    return plan_soft_outputs(plan, zcheck_samples, corrections=corrections)


def decode_dem_soft_outputs(dem_or_circuit, samples, max_iter=2, osd_order=0, bp_method='product_sum', schedule='serial', osd_method='osd_cs',
                            lsd_method=None, lsd_order=None, *, corrections=False):
    """(logical_pred int64 [N, observables], soft int64 [N, 6]) of `decode_dem` (same arguments, same cached plan): one window, so `iters`,
    `post` and `tail` are that window's.  corrections=True appends `decode_dem_corrections`' PackedSamples as a third value."""
    from .. import _lib
    _lib.require_gpu()
    cls, opts = _dem_options(max_iter, osd_order, bp_method, schedule, osd_method, lsd_method, lsd_order)
    dem, plan = cached_dem_plan(dem_or_circuit, samples, cls, opts)
    if plan is None:
        out = (np.zeros((0, dem.num_observables), dtype=np.int64), np.zeros((0, 6), dtype=np.int64))
        if corrections:
            from ..samples import PackedSamples
            from .base import detector_error_model_to_matrix
            n = detector_error_model_to_matrix(dem)[0].shape[1]
            out += (PackedSamples(np.zeros((0, (n + 7) // 8), np.uint8), n),)
        return out
    return plan_soft_outputs(plan, samples, corrections=corrections)


__all__ = ["sliding_window_soft_outputs", "decode_dem_soft_outputs", "plan_soft_outputs"]
