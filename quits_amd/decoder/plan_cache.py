"""The process-wide cache of window plans behind the reference-shaped entry points.

The reference entry points are called once per experiment point with host arrays (bposd.py:54-86; doc/06B_end_to_end_demo_bb.ipynb
cell 5 loops over p), and every call used to rebuild everything: DEM extraction + spacetime() + one qd_graph_create per window
(0.4 s for the headline window, 15 s for the QLP [[1020,136]] circuit).  Plans are kept, least recently used first out, keyed on
everything they depend on: the circuit (hash of its text), hz, W, F, the number of rounds, both plug-in classes and both option
dicts -- and the CUDA device that is current, because graphs, decoders and workspaces are bound to the device they were built on.
QD_PLAN_CACHE = number of plans kept (default 8, 0 = off), read at every lookup.  ONE cache per process (the per-thread caches
of round 5 rebuilt the plan and kept a second set of graphs, decoders and workspaces per calling thread), guarded by a module lock; a plan
carries mutable state (staging buffers, side streams, decoder workspaces), so its USE is serialised by the plan's own re-entrant lock
(DeviceWindowPlan.decode_host): two threads calling with the same arguments share one plan and take turns, threads with different
arguments run different plans side by side.  Only plans that are in use keep device workspaces: a lookup releases the workspaces of
every other cached plan whose lock is free (whatever thread used it last); a plan that another thread is decoding with is left alone.
The cache stores whatever build() returns; the workspace rule applies to objects that have `release_workspaces`."""
from __future__ import annotations

import hashlib
import threading
from collections import OrderedDict

import numpy as np

_CACHE = OrderedDict()
_CACHE_LOCK = threading.RLock()
_CACHE_STATS = {"hits": 0, "misses": 0}


def _current_device():
    """Index of the current CUDA device (-1 without a GPU): plans, graphs, decoders and workspaces are bound to it."""
    try:
        import torch
        return int(torch.cuda.current_device()) if torch.cuda.is_available() else -1
    except Exception:            # pragma: no cover
        return -1


def _freeze(v):
    """Hashable fingerprint of an option value: arrays by content, floats by repr."""
    if isinstance(v, dict):
        return tuple(sorted((str(k), _freeze(x)) for k, x in v.items()))
    if isinstance(v, (list, tuple)):
        return tuple(_freeze(x) for x in v)
    if isinstance(v, np.ndarray) or hasattr(v, "__array__"):
        a = np.ascontiguousarray(np.asarray(v))
        return ("ndarray", a.dtype.str, a.shape, hashlib.sha1(a.tobytes()).hexdigest())
    if isinstance(v, float):
        return ("float", repr(float(v)))
    return (type(v).__name__, repr(v))


def _circuit_fingerprint(circuit):
    """sha1 of the circuit text (stim.Circuit, quits_amd.dem.Circuit and plain text all print as Stim text); an object that is
    already a detector error model goes by its printed form as well.  A quits_amd.dem.Circuit that carries
    `approximate_disjoint_errors` gives another detector error model than its bare text (which has none, if the circuit holds a
    Pauli channel), so the setting is part of the fingerprint."""
    h = hashlib.sha1(str(circuit).encode())
    setting = getattr(circuit, "approximate_disjoint_errors", False)
    if isinstance(setting, (bool, int, float)):
        setting = float(setting)                             # True and 1.0 are the same threshold
    if setting:                                              # (some other object's attribute of that name goes by its printed form)
        h.update(("\0approximate_disjoint_errors=%r" % (setting,)).encode())
    return h.hexdigest()


def _matrix_fingerprint(mat):
    if hasattr(mat, "tocsr"):
        c = mat.tocsr()
        c.sort_indices()
        h = hashlib.sha1(np.asarray(c.indptr, np.int64).tobytes())
        h.update(np.asarray(c.indices, np.int64).tobytes())
        h.update((np.asarray(c.data) % 2).astype(np.uint8).tobytes())
        return ("sparse", c.shape, h.hexdigest())
    a = np.ascontiguousarray(np.asarray(mat) % 2).astype(np.uint8)
    return ("dense", a.shape, hashlib.sha1(a.tobytes()).hexdigest())


def plan_key(kind, circuit, hz, lz, W, F, num_rounds, decoder1, decoder2, dict1, dict2):
    """Everything a DeviceWindowPlan depends on.  kind: 'circuit' (circuit is the circuit) or 'phenom' (circuit is None; lz enters
    because the phenomenological commit matrices are built from it)."""
    return (kind, ("device", _current_device()), None if circuit is None else _circuit_fingerprint(circuit), _matrix_fingerprint(hz),
            None if lz is None else _matrix_fingerprint(lz), int(W), int(F), int(num_rounds),
            getattr(decoder1, "__qualname__", repr(decoder1)), getattr(decoder2, "__qualname__", repr(decoder2)),
            _freeze(dict1), _freeze(dict2))


def _plan_cache_size():
    import os
    try:
        return max(0, int(os.environ.get("QD_PLAN_CACHE", "8")))
    except ValueError:
        return 8


def _release_if_idle(plan):
    """Only plans in use keep device workspaces (the per-edge BP kernel sizes its message planes for tens of GB): the others keep
    their graphs and decoders and size their workspaces again when they are used next."""
    if not hasattr(plan, "release_workspaces") or not getattr(plan, "_ws_live", True):
        return
    lock = getattr(plan, "_lock", None)
    if lock is not None and not lock.acquire(blocking=False):        # (busy in another thread: leave it)
        return
    try:
        plan.release_workspaces()
        plan._ws_live = False
    finally:
        if lock is not None:
            lock.release()


def cached_plan(key, build):
    """The plan stored under `key` in the process-wide cache, built with build() on a miss (under the cache lock: two threads asking for
    the same new plan build it once)."""
    cap = _plan_cache_size()
    with _CACHE_LOCK:
        if cap == 0:
            _CACHE_STATS["misses"] += 1
            return build()
        plan = _CACHE.get(key)
        for k, other in _CACHE.items():
            if k != key:
                _release_if_idle(other)
        if plan is not None:
            _CACHE.move_to_end(key)
            _CACHE_STATS["hits"] += 1
        else:
            _CACHE_STATS["misses"] += 1
            plan = build()
            _CACHE[key] = plan
            while len(_CACHE) > cap:
                _CACHE.popitem(last=False)
        try:
            plan._ws_live = True
        except AttributeError:
            pass
        return plan


def plan_cache_info():
    with _CACHE_LOCK:
        return {"size": len(_CACHE), "capacity": _plan_cache_size(), **_CACHE_STATS}


def plan_cache_clear():
    with _CACHE_LOCK:
        _CACHE.clear()
        _CACHE_STATS.update(hits=0, misses=0)
