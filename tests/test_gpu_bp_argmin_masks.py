"""The gather pass of the several-checks-per-lane min-sum kernel (bp_scatter_wide.hip) decides "is this the edge my check's last
minimum came from" with lane masks kept in scalar registers: four masks per check and pass for the position inside a group of four
edges, one per group for the group, ANDed on the scalar unit (bp_scatter_wide_walk.inc, QS_MAG_MASK).  A wrong mask sends min1 where
min2 belongs (or the reverse) on one edge of one check, which moves posteriors, iteration counts and hard decisions.  So three paths
are compared bit for bit -- the default path (first-pass table made by the same walk with "no argmin yet"), the gather kernel
(QD_NO_SCATTER=1), and the double-precision oracle on the device's LLR grid -- plus QD_BP_NO_FAST_START=1, where the "no argmin yet"
pass runs inside the kernel, on one window per instantiation and argmin-position range:

  bb72 W=3 F=1 (108 checks)      <128,8,2,2>
  bb72 single window (288)       <256,8,2,2>
  bb144 headline window (1008)   <512,8,2,2>  rows of 16..35: second sign word, mixed-degree rounds (the tail forms of the walk)
  hgp225 W=3 (324)               <256,8,2,2>  rows of 22..52
  qlp1020 W=3 (1350)             <512,4,3,3>  rows of 25..78: third sign word, argmin positions >= 64

Compared: hard decisions (stage 1), OSD-0 outputs (stage 3), status words (iteration count and flags), and the posteriors the kernel
exports for shots that did not converge."""
import functools

import numpy as np
import pytest

import helpers
import oracle as orc

pytestmark = pytest.mark.gpu

SWITCHES = ("QD_NO_SCATTER", "QD_BP_NO_FAST_START", "QD_SCATTER_M2_LIMIT")
PATHS = (("default", {}), ("generic", {"QD_BP_NO_FAST_START": "1"}), ("gather", {"QD_NO_SCATTER": "1"}))
WINDOWS = {            # name: (fixture, (W, F, index) or None for the whole history as one window, shots, largest row, (lanes, checks per lane, sign words) of the instantiation)
    "bb72_w3": ("bb72_custom_r6_p0.003", (3, 1, 0), 128, 35, (128, 2, 2)),
    "bb72": ("bb72_custom_r6_p0.003", None, 128, 35, (256, 2, 2)),
    "bb144": ("bb144_custom_r12_p0.003", None, 96, 35, (512, 2, 2)),
    "hgp225_w3": ("hgp225_cardinal_r3_p0.01", (3, 1, 0), 64, 52, (256, 2, 2)),
    "qlp1020_w3": ("qlp1020_cardinal_r20_p0.003", (3, 1, 0), 32, 78, (512, 3, 3)),
}
NLLR = 6               # posteriors are read back one shot at a time (a synchronising call each): the first NLLR shots that did not converge


@functools.lru_cache(maxsize=None)
def _window(which):
    name, wf, shots, max_row, _ = WINDOWS[which]
    if wf is None:
        H, _, pri = helpers.dem_matrices(name)
    else:
        w = helpers.window_set(name, wf[0], wf[1])[wf[2]]
        H, pri = w["H"], w["priors"]
    pri = np.asarray(pri, dtype=np.float64)
    assert int(np.diff(H.tocsr().indptr).max()) == max_row
    s = np.ascontiguousarray(orc.sample_dem(H, H[:1], pri, seed=31, shot0=0, B=shots)[0]).astype(np.uint8)
    s.setflags(write=False)
    return H, pri, s


@functools.lru_cache(maxsize=None)
def _reference(which, max_iter):
    """The oracle in double precision on the device's grid: (OSD-0 outputs, flags, {shot: (hard decisions, posteriors)} of the first NLLR
    shots BP leaves unconverged)."""
    H, pri, s = _window(which)
    g, form = orc.device_arithmetic(H, pri, "minimum_sum", "parallel", max_iter, 1.0)
    prm = orc.make_params("minimum_sum", "parallel", max_iter, "osd_0", 0, 1.0, form)
    ref, flags = g.decode_batch(s, prm)
    soft = {}
    for b in np.flatnonzero(flags[:, 0] == 0)[:NLLR]:
        conv, dec, llr, it = g.bp(s[b], prm)
        assert not conv and it == flags[b, 1]
        soft[int(b)] = (dec, llr)
    return ref, flags, soft


def _run(monkeypatch, which, env, max_iter):
    import torch
    from quits_amd.decoder.device import BatchDecoder, WindowGraph, unpack_bits
    H, pri, s = _window(which)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wg = WindowGraph(H, pri)
    dec = BatchDecoder(wg, max_iter=max_iter, osd_method="osd_0")
    det = torch.from_numpy(np.array(s)).cuda()
    out = {}
    bits, status = dec.decode(det, stage=1)
    out[1] = (unpack_bits(bits, wg.n).cpu().numpy(), status.cpu().numpy())
    failed = np.flatnonzero(((out[1][1] >> 16) & 1) == 0)[:NLLR]
    out["llr"] = {int(b): dec.failed_llr(int(b)).cpu().numpy() for b in failed}
    bits, status = dec.decode(det, stage=3)
    out[3] = (unpack_bits(bits, wg.n).cpu().numpy(), status.cpu().numpy())
    # which instantiation ran: entries 12 and 13 of qd_graph_info_ex are the wide kernel's lanes and checks per lane; rows of more than 64 faults take
    # three sign words
    import ctypes
    arr = (ctypes.c_int32 * 14)()
    assert wg._L.qd_graph_info_ex(wg._h, arr, 14) == 0
    if "QD_NO_SCATTER" not in env:
        assert (int(arr[12]), int(arr[13]), 3 if wg.info()["max_row_weight"] > 64 else 2) == WINDOWS[which][4], (which, list(arr))
    return out, dec.info()


def _same(a, b, what):
    for stage in (1, 3):
        bad = np.flatnonzero((a[stage][0] != b[stage][0]).any(axis=1) | (a[stage][1] != b[stage][1]))
        assert bad.size == 0, "%s, stage %d: %d shots differ, first %s" % (what, stage, bad.size, bad[:8])
    assert sorted(a["llr"]) == sorted(b["llr"]), what
    for k in a["llr"]:
        assert np.array_equal(a["llr"][k], b["llr"][k]), "%s: posteriors of shot %d differ" % (what, k)


def _against_oracle(which, max_iter, out, tag):
    ref, flags, soft = _reference(which, max_iter)
    bits, status = out[3]
    assert np.array_equal((status >> 16) & 1, flags[:, 0]), tag
    assert np.array_equal(status & 0x3FFF, flags[:, 1]), tag
    assert np.array_equal(bits, ref), tag
    assert sorted(out["llr"]) == sorted(soft), tag
    for b, (dec, llr) in soft.items():
        assert np.array_equal(out[1][0][b], dec), (tag, b)
        assert np.array_equal(out["llr"][b].astype(np.float64), llr), (tag, b)      # exact: the grid's posteriors fit a float


def _paths(monkeypatch, which, max_iter, extra_env=None):
    outs = {}
    for tag, env in PATHS:
        outs[tag], info = _run(monkeypatch, which, dict(env, **(extra_env or {})), max_iter)
        assert info["scatter_wide_kernel"] == (tag != "gather"), (tag, info)
        assert info["bp_fast_start"] == (tag == "default"), (tag, info)
    _same(outs["default"], outs["gather"], "default path against the gather kernel")
    _same(outs["generic"], outs["gather"], "QD_BP_NO_FAST_START=1 against the gather kernel")
    for tag in ("default", "generic", "gather"):
        _against_oracle(which, max_iter, outs[tag], tag)
    return outs


@pytest.mark.parametrize("max_iter", [1, 2, 3, 50])
@pytest.mark.parametrize("which", list(WINDOWS))
def test_argmin_masks_change_nothing(gpu, monkeypatch, which, max_iter):
    """max_iter 1: only the table's pass and the thin last pass run (no mask is consulted in the kernel on the default path, every one
    is "none" on the generic path); 2 and 3: the first passes whose masks name real edges; 50: the headline's limit, where each check
    has moved its argmin many times."""
    outs = _paths(monkeypatch, which, max_iter)
    st = outs["default"][1][1]
    run = st[(st >> 19) & 1 == 0]
    assert run.size and (run & 0x3FFF).min() >= 1 and (run & 0x3FFF).max() <= max_iter
    if max_iter == 50 and which == "bb144":
        conv = ((st >> 16) & 1).mean()
        assert 0.05 < conv < 0.95, conv            # some shots leave through the convergence test, some run all 50 iterations


@pytest.mark.parametrize("which,max_iter,limit", [("bb144", 50, "40000"), ("bb144", 3, "1"), ("qlp1020_w3", 3, "1"), ("bb72_w3", 3, "1")])
def test_argmin_masks_through_the_recheck_pass(gpu, monkeypatch, which, max_iter, limit):
    """QD_SCATTER_M2_LIMIT low enough that the kernel's exactness bound parks shots for the gather kernel's recheck pass (limit 1:
    every shot with a defect): parked or not, every output stays what it was."""
    _paths(monkeypatch, which, max_iter, extra_env={"QD_SCATTER_M2_LIMIT": limit})
