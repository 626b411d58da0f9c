"""Whole-history decoding of any detector error model: no `hz`, no windows.

The reference decodes through windows cut along the rounds of a memory experiment (sliding_window.py:104-188) and needs the code's `hz`
for the cut; a detector error model that is not such an experiment -- or one that comes from a .dem file -- has no rounds to cut along.
`decode_dem` is the one-window case of the same driver: detector_error_model_to_matrix -> one window graph and decoder -> L e.
"""
from __future__ import annotations

import numpy as np

from ..dem import as_dem
from .base import detector_error_model_to_matrix
from .plan import DeviceWindowPlan, _kwargs_for_device
from .plan_cache import _circuit_fingerprint, _current_device, _freeze, cached_plan


def build_dem_plan(dem, cls, opts):
    """A DeviceWindowPlan of one window that spans every detector and every fault of `dem`."""
    check, observable, priors = detector_error_model_to_matrix(dem)
    kw = _kwargs_for_device(opts, cls)
    return DeviceWindowPlan([check], [observable], [priors], [], [0], check.shape[0], observable.shape[0], kw, kw)


def _dem_options(max_iter, osd_order, bp_method, schedule, osd_method, lsd_method, lsd_order):
    """(plug-in class, its keyword dict) for decode_dem's keywords: BP-LSD when `lsd_method` or `lsd_order` is given."""
    from .bplsd import BpLsdDecoder
    from .bposd import BpOsdDecoder
    opts = {'bp_method': bp_method, 'max_iter': max_iter, 'schedule': schedule}
    if lsd_method is not None or lsd_order is not None:
        opts.update(lsd_method='lsd_cs' if lsd_method is None else lsd_method, lsd_order=0 if lsd_order is None else lsd_order)
        return BpLsdDecoder, opts
    opts.update(osd_method=osd_method, osd_order=osd_order)
    return BpOsdDecoder, opts


def cached_dem_plan(dem_or_circuit, samples, cls, opts):
    """(dem, the process-wide cache's one-window plan for it and these options -- None for an empty batch, which needs no device); checks
    the samples' width against the model."""
    dem = as_dem(dem_or_circuit)
    if len(samples.shape) != 2 or samples.shape[1] != dem.num_detectors:
        raise ValueError("samples must have shape [shots, %d], the model's detectors; got %s" % (dem.num_detectors, tuple(samples.shape)))
    if samples.shape[0] == 0:
        return dem, None
    key = ("dem", ("device", _current_device()), _circuit_fingerprint(dem_or_circuit if isinstance(dem_or_circuit, str) else dem),
           int(dem.num_detectors), int(dem.num_observables), cls.__qualname__, _freeze(opts))
    return dem, cached_plan(key, lambda: build_dem_plan(dem, cls, opts))


def decode_dem(dem_or_circuit, samples, max_iter=2, osd_order=0, bp_method='product_sum', schedule='serial', osd_method='osd_cs',
               lsd_method=None, lsd_order=None):
    """Logical predictions, int64 [N, observables], for detector samples [N, detectors] of any detector error model, decoded over its
    whole history by BP-OSD -- or by BP-LSD when `lsd_method` (or `lsd_order`) is given, with sliding_window_bplsd_circuit_mem's defaults
    for the other.  Keywords and defaults are those of sliding_window_bposd_circuit_mem.

    dem_or_circuit: a stim.Circuit or stim.DetectorErrorModel, circuit text, a quits_amd.dem.Circuit, the text of a .dem file, or a
    quits_amd.dem.DetectorErrorModel.  samples: a numpy array or tensor (any integer dtype or bool), or quits_amd.samples.PackedSamples.
    The graph limits of the device decoder apply to the whole model (include/quits_amd.h: qd_graph_create)."""
    cls, opts = _dem_options(max_iter, osd_order, bp_method, schedule, osd_method, lsd_method, lsd_order)
    dem, plan = cached_dem_plan(dem_or_circuit, samples, cls, opts)
    if plan is None:
        return np.zeros((0, dem.num_observables), dtype=np.int64)
    return plan.decode_host(samples)


__all__ = ["decode_dem"]
