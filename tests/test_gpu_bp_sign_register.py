"""The gather pass of the several-checks-per-lane min-sum kernel (bp_scatter_wide.hip) keeps the signs a check sent last time and the
signs it collects now in ONE register per sign word (bp_scatter_wide_walk.inc): the word starts as the sent word shifted left by
32 - kend (kend = the word's edge positions, a multiple of 4), every edge reads its sent sign at bit 31 (QS_SIGN_TOP) and the
v_alignbit that enters the edge's new sign at bit 0 moves the next edge's sent sign up.  What can go wrong is the alignment: a wrong
pre-shift (the & 31 of a full word, a short last word), a position of the walk that does not shift (pads, lanes past their degree),
or bits of the sent word above kend - 1 leaking into the result -- `flip` sets all of them for a check whose syndrome bit differs
from the parity of its incoming signs.  Each of these sends a wrong sign on some edge or leaves a stray bit in the sign word, which
moves posteriors, iteration counts and hard decisions.

So, as in test_gpu_bp_argmin_masks.py, three paths are compared bit for bit -- the default path (first-pass table, walked with
"nothing sent": O = 0), QD_BP_NO_FAST_START=1 (every pass in the kernel) and the gather kernel (QD_NO_SCATTER=1) -- and each of them
with the double-precision oracle on the device's LLR grid: hard decisions, status words, OSD-0 outputs, exported posteriors.

The fixture windows are covered by the files that exist.  This one walks small synthetic windows (<= 128 checks: the <128,8,2,2>
instantiation; column weights 2..6; seeded) whose row weights put the word boundaries where the shared register can go wrong:

  w4      all rows of weight 4      one group per word, pre-shift 28
  w32     all of weight 32          a full word: pre-shift 32 & 31 = 0
  w33     all of weight 33          the second word is one group of which one position is real and three are pads (pre-shift 28)
  w36     all of weight 36          the second word is one full group
  w64     all of weight 64          two full words, a partial second wavefront (72 checks)
  w29_36  64 checks, 8 each of weight 29..36: one degree-sorted round whose lanes run past their degree in both words
  pads    64 checks of weight 33..35 and 64 of 26..30: two rounds whose largest degree is no multiple of 4 -- pad positions in the
          second word of one round and in the first (and only) word of the other, beside lanes past their degree

each with sampled syndromes (64 shots) and with the all-ones syndrome, which makes `flip` all ones on every check with even
incoming parity from the first pass on; max_iter 1 (table + thin last pass on the default path), 3 and 50.  qlp1020_w3 (rows of
25..78, <512,4,3,3>) at max_iter 3 adds the third sign word."""
import ctypes
import functools

import numpy as np
import pytest
from scipy.sparse import csc_matrix

import helpers
import oracle as orc

pytestmark = pytest.mark.gpu

SWITCHES = ("QD_NO_SCATTER", "QD_BP_NO_FAST_START", "QD_SCATTER_M2_LIMIT", "QD_SCATTER_CPL1")
PATHS = (("default", {}), ("generic", {"QD_BP_NO_FAST_START": "1"}), ("gather", {"QD_NO_SCATTER": "1"}))
SHOTS = 64
ONES_SHOTS = 4         # the all-ones syndrome is one syndrome: a few copies, so that more than one workgroup runs it
NLLR = 6               # posteriors are read back one shot at a time: the first NLLR shots that did not converge
SYNTH = {              # name: row weights, heaviest first (the library sorts check slots by degree; the rows are shuffled)
    "w4": [4] * 128,
    "w32": [32] * 96,
    "w33": [33] * 96,
    "w36": [36] * 96,
    "w64": [64] * 72,
    "w29_36": [w for w in range(36, 28, -1) for _ in range(8)],
    "pads": [35] * 20 + [34] * 24 + [33] * 20 + [30] * 12 + [29] * 13 + [28] * 13 + [27] * 13 + [26] * 13,
}
SHAPES = {name: (128, 2, 2) for name in SYNTH}
SHAPES["qlp1020_w3"] = (512, 3, 3)


def _synthetic(name):
    """A seeded random parity-check matrix with the row weights of SYNTH[name] and column weights 2..6, and its priors.
    Every row has exactly two faults of column weight 2 (as many such columns as rows); its other faults have weight 3..6 (4 each, then
    seeded +1 / -1 moves that keep the sum).  The two light faults keep min-sum's magnitudes from growing geometrically on a syndrome
    BP cannot meet (the all-ones one): a light fault passes on its prior plus ONE message, and every message a check sends is the
    minimum over edges that include a light fault, so the largest message grows by at most the largest prior per iteration and the
    posteriors stay where the device's integer and float sums are exact (checked in _reference)."""
    rows = SYNTH[name]
    rng = np.random.default_rng(20260 + sorted(SYNTH).index(name))
    m = len(rows)
    light = helpers._place(rng, [2] * m, np.full(m, 2, dtype=np.int64))
    total = sum(rows) - 2 * m
    n = max(total // 4, max(rows) - 2)
    cdeg = np.full(n, total // n, dtype=np.int64)
    cdeg[:total - cdeg.sum()] += 1
    for _ in range(2 * n):
        a, b = rng.integers(0, n, size=2)
        if a != b and cdeg[a] < 6 and cdeg[b] > 3:
            cdeg[a] += 1
            cdeg[b] -= 1
    assert cdeg.sum() == total and cdeg.min() >= 3 and cdeg.max() == 6, (name, cdeg.min(), cdeg.max())
    H = np.concatenate([light, helpers._place(rng, [w - 2 for w in rows], cdeg)], axis=1)
    H = H[:, rng.permutation(H.shape[1])]
    assert sorted(H.sum(axis=1).tolist(), reverse=True) == rows
    assert H.sum(axis=0).min() == 2 and H.sum(axis=0).max() == 6
    # three to four faults per shot, spread over three decades: with near-equal priors the all-ones syndrome of an odd row weight is met
    # by the first iteration's hard decisions (every fault set) and nothing is left to iterate
    pri = np.minimum(0.08, 10.0 ** rng.uniform(-2.5, 0.5, size=H.shape[1]) * 8.0 / H.shape[1])
    return csc_matrix(H), pri


@functools.lru_cache(maxsize=None)
def _window(which, synd):
    if which in SYNTH:
        H, pri = _synthetic(which)
    else:
        w = helpers.window_set("qlp1020_cardinal_r20_p0.003", 3, 1)[0]
        H, pri = w["H"], np.asarray(w["priors"], dtype=np.float64)
        assert int(np.diff(H.tocsr().indptr).max()) == 78
    if synd == "ones":
        s = np.ones((ONES_SHOTS, H.shape[0]), dtype=np.uint8)
    else:
        s = np.ascontiguousarray(orc.sample_dem(H, H[:1], pri, seed=47, shot0=0, B=SHOTS)[0]).astype(np.uint8)
    s.setflags(write=False)
    return H, pri, s


@functools.lru_cache(maxsize=None)
def _reference(which, synd, max_iter):
    """The oracle in double precision on the device's grid, on the CPU: (OSD-0 outputs, flags, {shot: (hard decisions, posteriors)} of
    the first NLLR shots BP leaves unconverged).  Checked here: with max_iter > 1 some shot runs more than one iteration."""
    H, pri, s = _window(which, synd)
    g, form = orc.device_arithmetic(H, pri, "minimum_sum", "parallel", max_iter, 1.0)
    prm = orc.make_params("minimum_sum", "parallel", max_iter, "osd_0", 0, 1.0, form)
    ref, flags = g.decode_batch(s, prm)
    print("%s / %s / max_iter %d: oracle iterations min %d max %d, converged %d of %d" % (
        which, synd, max_iter, flags[:, 1].min(), flags[:, 1].max(), int(flags[:, 0].sum()), len(flags)))
    assert max_iter == 1 or int(flags[:, 1].max()) > 1, (which, synd, max_iter)
    soft = {}
    for b in np.flatnonzero(flags[:, 0] == 0)[:NLLR]:
        conv, dec, llr, it = g.bp(s[b], prm)
        assert not conv and it == flags[b, 1]
        # the device adds grid units in int32 and float: exact, and so comparable bit for bit, below 2^23 units
        assert float(np.abs(llr).max()) * 2.0 ** orc.grid_bits(pri, max_iter)[0] < 2.0 ** 23, (which, synd, max_iter, float(np.abs(llr).max()))
        soft[int(b)] = (dec, llr)
    return ref, flags, soft


def _run(monkeypatch, which, synd, env, max_iter):
    import torch
    from quits_amd.decoder.device import BatchDecoder, WindowGraph, unpack_bits
    H, pri, s = _window(which, synd)
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
    # which instantiation ran: entries 12 and 13 of qd_graph_info_ex are the wide kernel's lanes and checks per lane; rows of more than
    # 64 faults take three sign words
    arr = (ctypes.c_int32 * 14)()
    assert wg._L.qd_graph_info_ex(wg._h, arr, 14) == 0
    if "QD_NO_SCATTER" not in env:
        assert (int(arr[12]), int(arr[13]), 3 if wg.info()["max_row_weight"] > 64 else 2) == SHAPES[which], (which, list(arr))
    return out, dec.info()


def _same(a, b, what):
    for stage in (1, 3):
        bad = np.flatnonzero((a[stage][0] != b[stage][0]).any(axis=1) | (a[stage][1] != b[stage][1]))
        assert bad.size == 0, "%s, stage %d: %d shots differ, first %s" % (what, stage, bad.size, bad[:8])
    assert sorted(a["llr"]) == sorted(b["llr"]), what
    for k in a["llr"]:
        assert np.array_equal(a["llr"][k], b["llr"][k]), "%s: posteriors of shot %d differ" % (what, k)


def _against_oracle(ref3, out, tag):
    ref, flags, soft = ref3
    bits, status = out[3]
    assert np.array_equal((status >> 16) & 1, flags[:, 0]), tag
    assert np.array_equal(status & 0x3FFF, flags[:, 1]), tag
    assert np.array_equal(bits, ref), tag
    assert sorted(out["llr"]) == sorted(soft), tag
    for b, (dec, llr) in soft.items():
        assert np.array_equal(out[1][0][b], dec), (tag, b)
        assert np.array_equal(out["llr"][b].astype(np.float64), llr), (tag, b)      # exact: the grid's posteriors fit a float


def _paths(monkeypatch, which, synd, max_iter):
    ref3 = _reference(which, synd, max_iter)
    outs = {}
    for tag, env in PATHS:
        outs[tag], info = _run(monkeypatch, which, synd, env, max_iter)
        assert info["scatter_wide_kernel"] == (tag != "gather"), (tag, info)       # the wide scatter kernel really ran
        assert info["bp_fast_start"] == (tag == "default"), (tag, info)
    _same(outs["default"], outs["gather"], "default path against the gather kernel")
    _same(outs["generic"], outs["gather"], "QD_BP_NO_FAST_START=1 against the gather kernel")
    for tag in ("default", "generic", "gather"):
        _against_oracle(ref3, outs[tag], tag)
    st = outs["default"][1][1]
    run = st[(st >> 19) & 1 == 0]
    assert run.size and (run & 0x3FFF).min() >= 1 and (run & 0x3FFF).max() <= max_iter
    return outs


@pytest.mark.parametrize("max_iter", [1, 3, 50])
@pytest.mark.parametrize("synd", ["sampled", "ones"])
@pytest.mark.parametrize("which", list(SYNTH))
def test_shared_sign_register_on_synthetic_rows(gpu, monkeypatch, which, synd, max_iter):
    """Every row-weight pattern of the module's table, with sampled syndromes and with the all-ones syndrome (sent words with every bit
    above kend - 1 set)."""
    _paths(monkeypatch, which, synd, max_iter)


@pytest.mark.parametrize("synd", ["sampled", "ones"])
def test_shared_sign_register_third_word(gpu, monkeypatch, synd):
    """qlp1020 W = 3: rows of up to 78 faults, three sign words per check, the last one short."""
    _paths(monkeypatch, "qlp1020_w3", synd, 3)
