"""The decoders' space-time corrections, not only their logical predictions.

The reference's sliding-window loop computes a correction per window, keeps `window_observable_set[k] @ e` and `window_update[k] @ e` of it
and drops it (decoder/sliding_window.py:171-183).  The committed columns of the windows partition the faults of the detector error model
(base.commit_ranges), so laid end to end they are ONE correction C of the whole history: L C is the logical prediction, and H C = det
wherever no window reported an inconsistent syndrome.  The functions here return that C next to the predictions, through the same cached
plans as `sliding_window_bposd_circuit_mem` / `sliding_window_bplsd_circuit_mem` / `decode_dem`: the predictions are those calls', bit for
bit.  The columns are those of `detector_error_model_to_matrix` (merged faults).
"""
from __future__ import annotations

import warnings

import numpy as np

from .base import window_count
from .plan import cached_circuit_plan
from .whole_history import _dem_options, cached_dem_plan


def sliding_window_corrections(zcheck_samples, circuit, hz, lz, W, F, max_iter=2, osd_order=0, bp_method='product_sum', schedule='serial',
                               osd_method='osd_cs', lsd_method=None, lsd_order=None):
    """(logical_pred int64 [N, k], corrections) of the circuit-level sliding-window decoder: BP-OSD with
    sliding_window_bposd_circuit_mem's keywords and defaults, or BP-LSD with sliding_window_bplsd_circuit_mem's when `lsd_method` (or
    `lsd_order`) is given (the other then takes that wrapper's default: 'lsd_cs', 0).

    corrections: host quits_amd.samples.PackedSamples of `nfaults` bits per shot, bit j = fault j (column j of
    detector_error_model_to_matrix(circuit)) is in the shot's correction; `np.asarray(corrections)` unpacks them and
    `write_shots(path, corrections, 'b8')` writes them as they are."""
    from .bplsd import BpLsdDecoder
    from .bposd import BpOsdDecoder
    if F == 0:
        raise ValueError("Input parameter F cannot be zero.")
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
    return plan.decode_host(zcheck_samples, corrections=True)


def decode_dem_corrections(dem_or_circuit, samples, max_iter=2, osd_order=0, bp_method='product_sum', schedule='serial', osd_method='osd_cs',
                           lsd_method=None, lsd_order=None):
    """(logical_pred int64 [N, observables], corrections) of `decode_dem` (same arguments, same cached plan): the whole-history correction of
    every shot, as host PackedSamples of one bit per fault of the model."""
    cls, opts = _dem_options(max_iter, osd_order, bp_method, schedule, osd_method, lsd_method, lsd_order)
    dem, plan = cached_dem_plan(dem_or_circuit, samples, cls, opts)
    if plan is None:
        from ..samples import PackedSamples
        from .base import detector_error_model_to_matrix
        n = detector_error_model_to_matrix(dem)[0].shape[1]
        return np.zeros((0, dem.num_observables), dtype=np.int64), PackedSamples(np.zeros((0, (n + 7) // 8), np.uint8), n)
    return plan.decode_host(samples, corrections=True)


__all__ = ["sliding_window_corrections", "decode_dem_corrections"]
