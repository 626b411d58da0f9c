"""Relay-BP bindings of the sliding-window decoders, and the plug-in decoder class.

No reference counterpart (the reference plugs in ldpc's BP-OSD and BP-LSD): `RelayBpDecoder` stands where `BpOsdDecoder` stands in bposd.py,
`sliding_window_relaybp_phenom_mem` / `sliding_window_relaybp_circuit_mem` where its two entry points stand, with the same samples and circuits
(bool / integer / bit-packed samples, a stim.Circuit, circuit text, `.dem` text).  The decoder is quits_amd/relay.py's, on the device
(csrc/bp_relay.hip); shots that no leg solves go to `osd_method`'s post-processor, 'osd_off' returns their last hard decision.
"""
from __future__ import annotations

import dataclasses

from ..relay import RelayConfig
from .bposd import BpOsdDecoder
from .sliding_window import sliding_window_circuit_mem, sliding_window_phenom_mem

RELAY_FIELDS = tuple(f.name for f in dataclasses.fields(RelayConfig))
_RATES = ("error_rate", "channel_probs", "error_channel")
_OWN = ("osd_method", "osd_order", "ms_scaling_factor")


def relay_device_kwargs(d):
    """The keyword dict of a RelayBpDecoder -> what DeviceWindowPlan builds its RelayBatchDecoder from: {"relay": RelayConfig, osd_method,
    osd_order, ms_scaling_factor}.  Unknown names raise TypeError, values RelayConfig refuses ValueError / TypeError: before any device call."""
    d = dict(d)
    extra = [k for k in d if k not in RELAY_FIELDS + _RATES + _OWN]
    if extra:
        raise TypeError("RelayBpDecoder does not take the keyword argument(s): %s" % ", ".join(sorted(extra)))
    out = {"relay": RelayConfig(**{k: d[k] for k in RELAY_FIELDS if k in d})}
    out.update({k: d[k] for k in _OWN if k in d})
    return out


def relay_options(relay=None, osd_method="osd_off", osd_order=0):
    """The keyword dict of the entry points below (and the plan cache's key) for a configuration."""
    relay = RelayConfig() if relay is None else relay
    if not isinstance(relay, RelayConfig):
        raise TypeError("relay must be a quits_amd.relay.RelayConfig, not %r" % type(relay).__name__)
    return dict(dataclasses.asdict(relay), osd_method=osd_method, osd_order=osd_order)


class RelayBpDecoder(BpOsdDecoder):
    """Plug-in decoder with BpOsdDecoder's `decode` / `decode_batch` surface, running Relay-BP.  The generic sliding-window functions
    recognise it as a device decoder and build one batched plan; `decode(syndrome)` is one launch per call, for drop-in use and tests."""

    def __init__(self, pcm, error_rate=None, channel_probs=None, osd_method="osd_off", osd_order=0, ms_scaling_factor=1.0, error_channel=None,
                 **relay_fields):
        from .device import RelayBatchDecoder, WindowGraph
        kw = relay_device_kwargs(dict(relay_fields, osd_method=osd_method, osd_order=osd_order, ms_scaling_factor=ms_scaling_factor))
        if channel_probs is not None:
            error_channel = channel_probs
        if error_channel is None:
            if error_rate is None:
                raise ValueError("Please specify the error channel. Either: 1) error_rate: float or "
                                 "2) channel_probs: list of floats of length equal to the block length of the code.")
            error_channel = float(error_rate)
        self.graph = WindowGraph(pcm, error_channel)
        self._dec = RelayBatchDecoder(self.graph, kw["relay"], osd_method=osd_method, osd_order=osd_order, ms_scaling_factor=ms_scaling_factor)
        self.m, self.n = self.graph.m, self.graph.n
        self.converge = False
        self.iter = 0
        self.last_status = None


def sliding_window_relaybp_phenom_mem(zcheck_samples, hz, lz, W, F, eff_error_rate_per_fault: float = None, relay=None, osd_method="osd_off",
                                      osd_order=0, tqdm_on=False):
    """Phenomenological sliding-window Relay-BP: sliding_window_bposd_phenom_mem's samples, windows and hand-off with the Relay-BP decoder.
    `relay`: a RelayConfig (default RelayConfig()).

    :return logical_z_pred: int64 (# trials, # logical qubits)
    """
    if eff_error_rate_per_fault is None:
        raise ValueError("eff_error_rate_per_fault must be provided.")
    opts = dict(relay_options(relay, osd_method, osd_order), error_rate=float(eff_error_rate_per_fault))
    return sliding_window_phenom_mem(zcheck_samples, hz, lz, W, F, RelayBpDecoder, RelayBpDecoder, dict(opts), dict(opts), 'decode', 'decode',
                                     tqdm_on=tqdm_on)


def sliding_window_relaybp_circuit_mem(zcheck_samples, circuit, hz, lz, W, F, relay=None, osd_method="osd_off", osd_order=0, tqdm_on=False):
    """Circuit-level sliding-window Relay-BP on the space-time detector error model: sliding_window_bposd_circuit_mem's samples, circuit, windows
    and hand-off with the Relay-BP decoder.  `relay`: a RelayConfig (default RelayConfig()).

    :return logical_z_pred: int64 (# trials, # logical qubits)
    """
    opts = relay_options(relay, osd_method, osd_order)
    return sliding_window_circuit_mem(zcheck_samples, circuit, hz, lz, W, F, RelayBpDecoder, RelayBpDecoder, dict(opts), dict(opts),
                                      'channel_probs', 'channel_probs', 'decode', 'decode', tqdm_on=tqdm_on)


__all__ = ["RelayBpDecoder", "sliding_window_relaybp_phenom_mem", "sliding_window_relaybp_circuit_mem"]
