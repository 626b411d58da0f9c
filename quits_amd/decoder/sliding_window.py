"""Sliding-window decoders (S. Huang and S. Puri, PRA 110, 012453) with the `quits.decoder` call surface.

Mirrors `/root/reference/src/quits/decoder/sliding_window.py`:
  sliding_window_phenom_mem   <- :14-101
  sliding_window_circuit_mem  <- :104-188
Same positional order, keyword names, return type (int64 [shots, logicals]) and errors.

Two execution paths, chosen by the plug-in decoder class, never silently by availability:
  * decoder classes are `quits_amd.decoder.BpOsdDecoder` (the HIP decoder): the loops are inverted -- windows outer,
    the whole shot batch inner -- and everything between the detector record and the logical prediction stays on
    the MI355X (the reference's per-shot Python loop tops out at a few thousand shots/s on its own);
  * any other class (e.g. ldpc's, or the CPU oracle in the tests): the reference's per-shot loop, restated, so
    third-party plug-ins keep working exactly as upstream.
"""
from __future__ import annotations

import warnings

import numpy as np
from scipy.sparse import csc_matrix

from .base import spacetime, window_count
# the device path lives in plan.py (DeviceWindowPlan, its builders), pipeline.py (the two-stream driver, host staging) and plan_cache.py;
# their public names stay importable from here
from .pipeline import lane_groups                                                                    # noqa: F401
from .plan import (DeviceWindowPlan, build_circuit_plan, build_phenom_plan, cached_circuit_plan,     # noqa: F401
                   cached_phenom_plan, fit_lanes_and_chunk, phenom_window_set)
from .plan_cache import cached_plan, plan_cache_clear, plan_cache_info, plan_key                     # noqa: F401


def _progress(it, on):
    if on:
        try:
            from tqdm import tqdm
            return tqdm(it)
        except ImportError:  # pragma: no cover
            return it
    return it


def phenom_window_matrices(hz, W, F, W_last):
    """Analytic window matrices of the phenomenological variant (reference sliding_window.py:56-68) plus the
    commit/hand-off selectors the reference applies by slicing (:86,:88,:96): for window matrix
    H_w = [ I_W (x) hz | B (x) I_nz ],  data block f of the decoded vector is e[f*nq:(f+1)*nq] and the syndrome update
    is the measurement block F-1."""
    hz = np.asarray(hz) % 2
    nz, nq = hz.shape
    B = np.eye(W, dtype=int)
    for i in range(1, W):
        B[i, i - 1] = 1
    h_mid = np.column_stack((np.kron(np.eye(W, dtype=int), hz), np.kron(B, np.eye(nz, dtype=int))))
    B_last = np.eye(W_last, dtype=int)
    for i in range(1, W_last):
        B_last[i, i - 1] = 1
    B_last = B_last[:, :W_last - 1]
    h_last = np.column_stack((np.kron(np.eye(W_last, dtype=int), hz), np.kron(B_last, np.eye(nz, dtype=int))))
    return csc_matrix(h_mid), csc_matrix(h_last)


def _is_device_decoder(cls) -> bool:
    from .bposd import BpOsdDecoder
    return isinstance(cls, type) and issubclass(cls, BpOsdDecoder)


def sliding_window_phenom_mem(zcheck_samples, hz, lz, W, F, decoder1, decoder2, dict1: dict, dict2: dict,
                              function_name1: str, function_name2: str, tqdm_on=False):
    """Phenomenological sliding-window decoder with plug-in inner decoders (reference sliding_window.py:14-101).

    :return logical_z_pred: int64 array (# trials, # logical qubits)
    """
    if F == 0:
        raise ValueError("Input parameter F cannot be zero.")
    nz, nq = hz.shape
    num_trials = zcheck_samples.shape[0]
    num_rounds = zcheck_samples.shape[1] // nz - 2
    num_cor_rounds, W_last, whole = window_count(num_rounds, W, F)
    if whole:
        warnings.warn("Window size larger than the syndrome extraction rounds: Doing whole history correction")

    if _is_device_decoder(decoder1) and _is_device_decoder(decoder2) and function_name1 == function_name2 == "decode":
        return cached_phenom_plan(hz, lz, W, F, num_rounds, decoder1, decoder2, dict1, dict2).decode_host(zcheck_samples)

    h_mid, h_last = phenom_window_matrices(hz, W, F, W_last)
    dec_mid = decoder1(h_mid, **dict1)
    dec_last = decoder2(h_last, **dict2)
    samples = np.asarray(zcheck_samples)
    out = np.zeros((num_trials, lz.shape[0]), dtype=int)
    for i in _progress(range(num_trials), tqdm_on):
        total = np.zeros(nq, dtype=int)
        carry = np.zeros(nz, dtype=int)
        for k in range(num_cor_rounds):
            s = samples[i, F * k * nz:(F * k + W) * nz].copy() % 2
            s[:nz] = (s[:nz] + carry) % 2
            e = getattr(dec_mid, function_name1)(s)
            total = (total + np.sum(e[:F * nq].reshape(F, nq), axis=0)) % 2
            carry = e[W * nq + (F - 1) * nz:W * nq + F * nz].copy()
        s = samples[i, F * num_cor_rounds * nz:].copy() % 2
        s[:nz] = (s[:nz] + carry) % 2
        e = getattr(dec_last, function_name2)(s)
        total = (total + np.sum(e[:W_last * nq].reshape(W_last, nq), axis=0)) % 2
        out[i, :] = (lz @ total) % 2
    return out


def sliding_window_circuit_mem(zcheck_samples, circuit, hz, lz, W, F, decoder1, decoder2, dict1: dict, dict2: dict,
                               error_rate_name1: str, error_rate_name2: str,
                               function_name1: str, function_name2: str, tqdm_on=False):
    """Circuit-level (space-time detector error model) sliding-window decoder with plug-in inner decoders
    (reference sliding_window.py:104-188).  `circuit`: a stim.Circuit, circuit text, or quits_amd.dem.Circuit.

    :return logical_z_pred: int64 array (# trials, # logical qubits)
    """
    if F == 0:
        # the reference only reaches this message through spacetime() (base.py:149-150) and, when R + 2 >= W, dies
        # earlier on the integer division at sliding_window.py:135; one ValueError up front covers both
        raise ValueError("Input parameter F cannot be zero.")
    nz = hz.shape[0]
    num_trials = zcheck_samples.shape[0]
    num_rounds = zcheck_samples.shape[1] // nz - 2
    num_cor_rounds, _, whole = window_count(num_rounds, W, F)
    if whole:
        warnings.warn("Window size larger than the syndrome extraction rounds: Doing whole history correction")

    if _is_device_decoder(decoder1) and _is_device_decoder(decoder2) and function_name1 == function_name2 == "decode":
        return cached_circuit_plan(circuit, hz, W, F, num_rounds, decoder1, decoder2, dict1, dict2).decode_host(zcheck_samples)

    checks, commits, priors, updates = spacetime(circuit, hz, W, F, num_cor_rounds)
    decoders = []
    for k in range(len(checks)):
        last = k == len(checks) - 1
        kw = dict(dict2 if last else dict1)          # the reference writes into the caller's dicts (:148,:151); we don't
        kw[error_rate_name2 if last else error_rate_name1] = priors[k]
        decoders.append((decoder2 if last else decoder1)(checks[k], **kw))
    samples = np.asarray(zcheck_samples)
    out = np.zeros((num_trials, lz.shape[0]), dtype=int)
    for i in _progress(range(num_trials), tqdm_on):
        acc = np.zeros(commits[0].shape[0], dtype=int)
        carry = np.zeros(nz, dtype=int)
        for k in range(num_cor_rounds):
            s = samples[i, F * k * nz:(F * k + W) * nz].copy() % 2
            s[:nz] = (s[:nz] + carry) % 2
            e = getattr(decoders[k], function_name1)(s)
            ncommit = commits[k].shape[1]
            acc = (acc + commits[k] @ e[:ncommit] % 2) % 2
            carry = updates[k] @ e[:ncommit] % 2
        s = samples[i, F * num_cor_rounds * nz:].copy() % 2
        s[:nz] = (s[:nz] + carry) % 2
        e = getattr(decoders[num_cor_rounds], function_name2)(s)
        acc = (acc + commits[num_cor_rounds] @ e % 2) % 2
        out[i, :] = acc
    return out


__all__ = ["sliding_window_phenom_mem", "sliding_window_circuit_mem", "plan_cache_info", "plan_cache_clear"]