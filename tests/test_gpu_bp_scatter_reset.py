"""The scatter pass of the several-checks-per-lane min-sum kernel (bp_scatter_wide.hip) no longer works in place: behind the vote's
barrier the accumulator region goes back to the priors (qs_reset_to_priors, bp_scatter_edge.h: global_load_lds_dwordx4, 1 KB per
wavefront instruction, the pieces dealt over the workgroup's wavefronts), a second barrier follows, and every edge adds its whole new
message, +-min1; the new argmin edge is corrected by +-(min2 - min1) behind the loop.  What the new text can get wrong:

  * the copy: a piece that is missed or doubled, a last piece that stops short (trash slots left non-zero flip a parity in the next
    gather pass: they are read every pass) or runs on (the output words lie behind the region: hard decisions of shots that converge
    late), wavefronts with no piece at all, a region beyond the first 64 KB of LDS;
  * the order: an add issued before every wavefront's copy has landed, a copy issued before the last read of the pass;
  * the message: the sign of min1 per edge, lanes past their degree (they must add 0), the argmin correction where min1 = min2.

So, as in test_gpu_bp_sign_register.py, three paths are compared bit for bit -- the default path (first-pass table; the first scatter
pass finds the prologue's fill), QD_BP_NO_FAST_START=1 (every pass in the kernel: gather pass 0, then a reset of what is already there)
and the gather kernel (QD_NO_SCATTER=1) -- and each of them with the double-precision oracle on the device's LLR grid: hard decisions,
status words, OSD-0 outputs, exported posteriors of the first few shots that do not converge.

The windows (seeded, <= 128 checks: the <128,8,2,2> instantiation, two wavefronts).  An accumulator region has nslots = 32 * (fullest
bank + 1) slots with ceil(n / 32) <= fullest bank <= ceil(n / 32) + 1 (graph_layout.hip: scatter_banks' cap), so it is always a multiple
of 32 slots -- a slot count that is no multiple of 4 does not exist, and a 16-byte unit is never partial; what varies is whether the
last 1 KB piece is partial and whether every wavefront has a piece.  From the number of faults alone (test_case_table_properties):

  small    48 rows of weight 8, 120 faults: 160 or 192 slots, less than one piece -- the second wavefront copies nothing
  w2_4     40 rows of weight 4 and 88 of weight 2, every fault in two checks, 168 faults: 224 or 256 slots, at most one piece; the
           argmin changes edge nearly every iteration (on a row of weight 2 whenever the two incoming magnitudes swap order), and
           the first round mixes both weights: lanes past their degree
  w2_4eq   the same matrix with all priors equal: min1 = min2 wherever nothing has been told apart yet, the correction adds 0
  w29_36   64 rows, 8 each of weight 29..36 (552 faults: 608 or 640 slots, a multiple of 4 and not of 256: the last piece is partial):
           one degree-sorted round whose lanes run past their degree in both sign words
  pads     64 rows of weight 33..35 and 64 of 26..30 (1055 faults: 1088 or 1120 slots): two rounds whose largest degree is no multiple
           of 4, five pieces over two wavefronts

each with sampled syndromes (64 shots) and the all-ones syndrome at max_iter 1 (table + thin last pass: no reset at all on the default
path), 2 (one reset), 3 and 50.  Beside them: qlp1020_w3 at max_iter 3 (<512,4,3,3>, three sign words, a region of 76 KB), one window
under QD_SCATTER_CPL1=1, one with QD_SCATTER_M2_LIMIT forced low (every shot goes through the recheck pass), and `small` with 4096
sampled shots, so that several workgroups per CU reset at once (all three paths on all shots, the oracle on a seeded 64 of them)."""
import ctypes
import functools

import numpy as np
import pytest
from scipy.sparse import csc_matrix

import helpers
import oracle as orc

SWITCHES = ("QD_NO_SCATTER", "QD_BP_NO_FAST_START", "QD_SCATTER_M2_LIMIT", "QD_SCATTER_CPL1")
PATHS = (("default", {}), ("generic", {"QD_BP_NO_FAST_START": "1"}), ("gather", {"QD_NO_SCATTER": "1"}))
SHOTS = 64
ONES_SHOTS = 4         # the all-ones syndrome is one syndrome: a few copies, so that more than one workgroup runs it
MANY_SHOTS = 4096
NLLR = 6               # posteriors are read back one shot at a time: the first NLLR shots that did not converge
SYNTH = {              # name: (row weights, heaviest first; lightest and heaviest of the heavy columns, None: every column of weight 2; seed)
    "small": ([8] * 48, (3, 5), 30101),
    "w2_4": ([4] * 40 + [2] * 88, None, 30102),
    "w2_4eq": ([4] * 40 + [2] * 88, None, 30102),
    "w29_36": ([w for w in range(36, 28, -1) for _ in range(8)], (3, 6), 30103),
    "pads": ([35] * 20 + [34] * 24 + [33] * 20 + [30] * 12 + [29] * 13 + [28] * 13 + [27] * 13 + [26] * 13, (3, 6), 30104),
}
# name: (faults, the two slot counts the layout can give, fewer slots than one 1 KB piece, a multiple of 256 slots possible, lanes past their degree)
CLAIMS = {
    "small": (120, (160, 192), True, False, False),
    "w2_4": (168, (224, 256), True, True, True),
    "w2_4eq": (168, (224, 256), True, True, True),
    "w29_36": (552, (608, 640), False, False, True),
    "pads": (1055, (1088, 1120), False, False, True),
}
SHAPES = {name: (128, 2, 2) for name in SYNTH}
SHAPES["qlp1020_w3"] = (512, 3, 3)


@functools.lru_cache(maxsize=None)
def _matrix(which):
    rows, heavy, seed = SYNTH[which]
    if heavy is not None:
        return helpers.synthetic_window(rows, heavy[0], heavy[1], seed)
    # rows of weight 2 and 4 over faults of weight 2 (a fault passes on its prior plus ONE message: magnitudes grow by at most the largest
    # prior per iteration, as with synthetic_window's light faults)
    rng = np.random.default_rng(seed)
    H = helpers._place(rng, rows, np.full(sum(rows) // 2, 2, dtype=np.int64))
    H = H[:, rng.permutation(H.shape[1])]
    if which == "w2_4eq":
        pri = np.full(H.shape[1], 0.02)
    else:
        pri = np.minimum(0.08, 10.0 ** rng.uniform(-2.5, 0.5, size=H.shape[1]) * 8.0 / H.shape[1])
    return csc_matrix(H), pri


@functools.lru_cache(maxsize=None)
def _window(which, synd):
    if which in SYNTH:
        H, pri = _matrix(which)
    else:
        w = helpers.window_set("qlp1020_cardinal_r20_p0.003", 3, 1)[0]
        H, pri = w["H"], np.asarray(w["priors"], dtype=np.float64)
        assert int(np.diff(H.tocsr().indptr).max()) == 78
    if synd == "ones":
        s = np.ones((ONES_SHOTS, H.shape[0]), dtype=np.uint8)
    else:
        B = MANY_SHOTS if synd == "many" else SHOTS
        s = np.ascontiguousarray(orc.sample_dem(H, H[:1], pri, seed=53, shot0=0, B=B)[0]).astype(np.uint8)
    s.setflags(write=False)
    return H, pri, s


@functools.lru_cache(maxsize=None)
def _reference(which, synd, max_iter):
    """The oracle in double precision on the device's grid, on the CPU: (shots it decoded, OSD-0 outputs, flags, {shot: (hard decisions,
    posteriors)} of the first NLLR of them that BP leaves unconverged)."""
    H, pri, s = _window(which, synd)
    shots = np.arange(len(s)) if synd != "many" else np.sort(np.random.default_rng(7).choice(len(s), size=SHOTS, replace=False))
    g, form = orc.device_arithmetic(H, pri, "minimum_sum", "parallel", max_iter, 1.0)
    prm = orc.make_params("minimum_sum", "parallel", max_iter, "osd_0", 0, 1.0, form)
    ref, flags = g.decode_batch(np.ascontiguousarray(s[shots]), prm)
    print("%s / %s / max_iter %d: oracle iterations min %d max %d, converged %d of %d" % (
        which, synd, max_iter, flags[:, 1].min(), flags[:, 1].max(), int(flags[:, 0].sum()), len(flags)))
    assert max_iter == 1 or int(flags[:, 1].max()) > 1, (which, synd, max_iter)      # some shot meets a reset
    soft = {}
    if synd != "many":
        for b in np.flatnonzero(flags[:, 0] == 0)[:NLLR]:
            conv, dec, llr, it = g.bp(s[b], prm)
            assert not conv and it == flags[b, 1]
            # the device adds grid units in int32 and float: exact, and so comparable bit for bit, below 2^23 units
            assert float(np.abs(llr).max()) * 2.0 ** orc.grid_bits(pri, max_iter)[0] < 2.0 ** 23, (which, synd, max_iter, float(np.abs(llr).max()))
            soft[int(b)] = (dec, llr)
    return shots, ref, flags, soft


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
    shape = (int(arr[12]), int(arr[13]), 3 if wg.info()["max_row_weight"] > 64 else 2)
    return out, dec.info(), shape


def _same(a, b, what):
    for stage in (1, 3):
        bad = np.flatnonzero((a[stage][0] != b[stage][0]).any(axis=1) | (a[stage][1] != b[stage][1]))
        assert bad.size == 0, "%s, stage %d: %d shots differ, first %s" % (what, stage, bad.size, bad[:8])
    assert sorted(a["llr"]) == sorted(b["llr"]), what
    for k in a["llr"]:
        assert np.array_equal(a["llr"][k], b["llr"][k]), "%s: posteriors of shot %d differ" % (what, k)


def _against_oracle(ref4, out, tag, whole):
    shots, ref, flags, soft = ref4
    bits, status = out[3][0][shots], out[3][1][shots]
    assert np.array_equal((status >> 16) & 1, flags[:, 0]), tag
    assert np.array_equal(status & 0x3FFF, flags[:, 1]), tag
    assert np.array_equal(bits, ref), tag
    if whole:                                                   # the oracle saw every shot: the same shots fail first
        assert sorted(out["llr"]) == sorted(soft), tag
    for b, (dec, llr) in soft.items():
        assert np.array_equal(out[1][0][b], dec), (tag, b)
        assert np.array_equal(out["llr"][b].astype(np.float64), llr), (tag, b)      # exact: the grid's posteriors fit a float


def _paths(monkeypatch, which, synd, max_iter, extra_env=None, shape=None):
    ref4 = _reference(which, synd, max_iter)
    outs = {}
    for tag, env in PATHS:
        outs[tag], info, ran = _run(monkeypatch, which, synd, dict(env, **(extra_env or {})), max_iter)
        # the scatter kernel really ran (with one check per lane the decoder reports it under the old one-check-per-lane kernel's label)
        cpl1 = "QD_SCATTER_CPL1" in (extra_env or {})
        assert info["scatter_kernel"] == (tag != "gather") and info["scatter_wide_kernel"] == (tag != "gather" and not cpl1), (tag, info)
        assert info["bp_fast_start"] == (tag == "default"), (tag, info)
        if tag != "gather":
            want = shape or SHAPES[which]
            assert ran[1:] == want[1:] and want[0] in (None, ran[0]), (which, tag, ran)
    _same(outs["default"], outs["gather"], "default path against the gather kernel")
    _same(outs["generic"], outs["gather"], "QD_BP_NO_FAST_START=1 against the gather kernel")
    for tag in ("default", "generic", "gather"):
        _against_oracle(ref4, outs[tag], tag, synd != "many")
    st = outs["default"][1][1]
    run = st[(st >> 19) & 1 == 0]
    assert run.size and (run & 0x3FFF).min() >= 1 and (run & 0x3FFF).max() <= max_iter
    return outs


def test_case_table_properties():
    """What the module's table claims about its windows, from the matrices alone (no GPU): the number of faults and with it the two slot
    counts the layout can give (see the module's text), on which side of one 1 KB piece and of a multiple of 256 slots they lie, the
    row weights, and whether a degree-sorted group of 64 checks mixes degrees (lanes past their degree, adds of 0 to trash slots)."""
    for which, (n, slots, below_piece, may_be_whole, mixed) in CLAIMS.items():
        H, pri = _matrix(which)
        rows = SYNTH[which][0]
        assert H.shape == (len(rows), n) and len(rows) <= 128, which
        deg = sorted(np.diff(H.tocsr().indptr).tolist(), reverse=True)
        assert deg == rows, which
        full = -(-n // 32)
        assert slots == (32 * (full + 1), 32 * (full + 2)), which
        assert all(c % 32 == 0 and c % 4 == 0 for c in slots), which          # whole 16-byte units, always
        assert below_piece == all(c <= 256 for c in slots), which
        assert may_be_whole == any(c % 256 == 0 for c in slots), which
        groups = [deg[k:k + 64] for k in range(0, len(deg), 64)]
        assert mixed == any(len(set(grp)) > 1 for grp in groups), which
        if which == "pads":
            assert all(grp[0] % 4 for grp in groups), which                    # largest degrees that are no multiple of 4: pad positions too
        if which == "w29_36":
            assert groups[0][0] > 32 and groups[0][-1] < 32, which             # lanes past their degree in both sign words
    assert set(np.diff(_matrix("w2_4")[0].tocsr().indptr).tolist()) == {2, 4}
    assert np.array_equal(_matrix("w2_4")[0].toarray(), _matrix("w2_4eq")[0].toarray())
    assert np.unique(_matrix("w2_4eq")[1]).size == 1 and np.unique(_matrix("w2_4")[1]).size > 100


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [1, 2, 3, 50])
@pytest.mark.parametrize("synd", ["sampled", "ones"])
@pytest.mark.parametrize("which", list(SYNTH))
def test_reset_and_whole_messages_on_synthetic_windows(gpu, monkeypatch, which, synd, max_iter):
    """Every window of the module's table, with sampled syndromes and with the all-ones syndrome."""
    _paths(monkeypatch, which, synd, max_iter)


@pytest.mark.gpu
def test_reset_third_sign_word_and_region_beyond_64k(gpu, monkeypatch):
    """qlp1020 W = 3: rows of up to 78 faults, three checks per lane, an accumulator region of more than 64 KB."""
    _paths(monkeypatch, "qlp1020_w3", "sampled", 3)


@pytest.mark.gpu
def test_reset_one_check_per_lane(gpu, monkeypatch):
    """QD_SCATTER_CPL1=1: the same text with one check per lane (twice the wavefronts deal the pieces)."""
    _paths(monkeypatch, "pads", "sampled", 50, extra_env={"QD_SCATTER_CPL1": "1"}, shape=(None, 1, 2))      # (as many lanes as the gather kernel takes for 128 checks)


@pytest.mark.gpu
def test_reset_with_recheck_pass(gpu, monkeypatch):
    """QD_SCATTER_M2_LIMIT = 1: every shot with a defect is parked and decoded again by the gather kernel; every output stays."""
    _paths(monkeypatch, "w29_36", "sampled", 50, extra_env={"QD_SCATTER_M2_LIMIT": "1"})


@pytest.mark.gpu
def test_reset_with_co_resident_workgroups(gpu, monkeypatch):
    """4096 shots of the smallest window: sixteen workgroups per CU reset their regions at once."""
    _paths(monkeypatch, "small", "many", 50)
