"""The fast start of the several-checks-per-lane min-sum kernel (bp_scatter_wide.hip): gather pass 0 taken from the decoder's
first-pass table, and the last gather pass folded down to the hard-decision parity.  Neither may change a bit: the default build
path, the same library with QD_BP_NO_FAST_START=1 (generic start, full last pass), the gather kernel (QD_NO_SCATTER=1) and the
double-precision oracle on the same LLR grid return the same hard decisions, status words and OSD-0 outputs (the OSD-0 outputs are
computed from the exported posteriors, so they cover those)."""
import numpy as np
import pytest

import helpers
import oracle as orc

pytestmark = pytest.mark.gpu

BB144 = "bb144_custom_r12_p0.003"
SWITCHES = ("QD_NO_SCATTER", "QD_BP_NO_FAST_START", "QD_SCATTER_M2_LIMIT")
PATHS = (("fast", {}), ("generic", {"QD_BP_NO_FAST_START": "1"}), ("gather", {"QD_NO_SCATTER": "1"}))


def _window(which):
    if which == "bb144_w3":                    # W = 3, F = 1, window 1: 216 checks, the 128-lane shape
        w = helpers.window_set(BB144, 3, 1)[1]
        return w["H"], np.asarray(w["priors"], dtype=np.float64)
    H, L, pri = helpers.dem_matrices({"bb144": BB144, "bb72": "bb72_custom_r6_p0.003", "hgp225": "hgp225_cardinal_r3_p0.01"}[which])
    return H, np.asarray(pri, dtype=np.float64)


def _shots(H, pri, B, seed):
    """B sampled syndromes; shot 0 all zero, shot 1 a single defect, shot 2 every detector set."""
    s = np.ascontiguousarray(orc.sample_dem(H, H[:1], pri, seed=seed, shot0=0, B=B)[0]).astype(np.uint8)
    s[0] = 0
    s[1] = 0
    s[1, H.shape[0] // 2] = 1
    s[2] = 1
    return s


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(monkeypatch, H, pri, env, max_iter, det, det_offset=0, upd=None):
    """{stage: (hard decisions / OSD-0 outputs [B, n], status words [B])} of a fresh graph + decoder under the switches `env`, and its info()."""
    from quits_amd.decoder.device import BatchDecoder, WindowGraph, unpack_bits
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wg = WindowGraph(H, pri)
    dec = BatchDecoder(wg, max_iter=max_iter, osd_method="osd_0")
    out = {}
    for stage in (1, 3):
        bits, status = dec.decode(det, det_offset=det_offset, upd=upd, stage=stage)
        out[stage] = (unpack_bits(bits, wg.n).cpu().numpy(), status.cpu().numpy())
    return out, dec.info()


def _same(a, b, what):
    for stage in (1, 3):
        bad = np.flatnonzero((a[stage][0] != b[stage][0]).any(axis=1) | (a[stage][1] != b[stage][1]))
        assert bad.size == 0, "%s, stage %d: %d shots differ, first %s" % (what, stage, bad.size, bad[:8])


def _oracle_bits(H, pri, max_iter, synd):
    g, form = orc.device_arithmetic(H, pri, "minimum_sum", "parallel", max_iter, 1.0)
    ref, flags = g.decode_batch(np.ascontiguousarray(synd), orc.make_params("minimum_sum", "parallel", max_iter, "osd_0", 0, 1.0, form))
    return ref, flags


def _three_paths(monkeypatch, H, pri, max_iter, s, nref, extra_env=None, det=None, det_offset=0, upd=None):
    det = _dev(s) if det is None else det
    outs = {}
    for tag, env in PATHS:
        env = dict(env, **(extra_env or {}))
        outs[tag], info = _run(monkeypatch, H, pri, env, max_iter, det, det_offset, upd)
        assert info["scatter_wide_kernel"] == (tag != "gather"), (tag, info)
        assert info["bp_fast_start"] == (tag == "fast"), (tag, info)
    _same(outs["fast"], outs["generic"], "fast start against QD_BP_NO_FAST_START=1")
    _same(outs["fast"], outs["gather"], "fast start against the gather kernel")
    _same(outs["generic"], outs["gather"], "generic start against the gather kernel")
    ref, flags = _oracle_bits(H, pri, max_iter, s[:nref])
    for tag in ("fast", "generic"):
        bits, status = outs[tag][3]
        assert np.array_equal(bits[:nref], ref), tag
        assert np.array_equal((status[:nref] >> 16) & 1, flags[:, 0]) and np.array_equal(status[:nref] & 0x3FFF, flags[:, 1]), tag
    return outs


@pytest.mark.parametrize("max_iter", [1, 2, 3, 50])
@pytest.mark.parametrize("which", ["bb144", "bb72", "hgp225", "bb144_w3"])
def test_fast_start_changes_nothing(gpu, monkeypatch, which, max_iter):
    """Single windows of three codes and the 128-lane W = 3 window, at the iteration limits where the start and the last pass meet
    (max_iter 1: scatter pass 0 is followed directly by the thin pass; 2, 3) and at the headline's 50."""
    H, pri = _window(which)
    s = _shots(H, pri, 384, seed=21)
    outs = _three_paths(monkeypatch, H, pri, max_iter, s, nref=48)
    st = outs["fast"][1][1]
    assert st[0] == (1 << 16) | (1 << 19)                      # the all-zero syndrome: converged, zero vector, no BP
    assert (st[1:] & 0x3FFF).min() >= 1 and (st[1:] & 0x3FFF).max() <= max_iter   # iterations are counted from the same origin
    if max_iter == 50 and which == "bb144":
        conv = ((st >> 16) & 1).mean()
        assert 0.05 < conv < 0.95, conv                        # some shots leave through the convergence test, some through the last pass


def test_fast_start_honours_slice_and_carry(gpu, monkeypatch):
    """The table holds what does not depend on the shot; the syndrome bit that flips the signs must still come through det_offset,
    the row strides and the carry: a record with an odd offset, noise around the slice and a carry XORed in decodes like the
    contiguous syndromes, on all three paths."""
    H, pri = _window("bb144_w3")
    m = H.shape[0]
    s = _shots(H, pri, 256, seed=22)
    base = _three_paths(monkeypatch, H, pri, 8, s, nref=48)
    rng = np.random.default_rng(5)
    off, rows = 37, 36
    rec = rng.integers(0, 2, size=(s.shape[0], off + m + 3), dtype=np.uint8)
    u = rng.integers(0, 2, size=(s.shape[0], rows), dtype=np.uint8)
    upd = rng.integers(0, 2, size=(s.shape[0], rows + 5), dtype=np.uint8)
    upd[:, :rows] = u
    sl = s.copy()
    sl[:, :rows] ^= u
    rec[:, off:off + m] = sl
    got = _three_paths(monkeypatch, H, pri, 8, s, nref=48, det=_dev(rec), det_offset=off, upd=_dev(upd)[:, :rows])
    _same(got["fast"], base["fast"], "record with det_offset / carry against the contiguous syndromes")


@pytest.mark.parametrize("max_iter", [3, 30])
def test_fast_start_through_the_recheck_pass(gpu, monkeypatch, max_iter):
    """QD_SCATTER_M2_LIMIT low enough to park shots for the gather kernel's recheck pass.  The set of parked shots is not visible
    through the API, and the thin last pass may legitimately shrink it: the second minima of the gather pass at t = max_iter are
    magnitudes of messages nobody sends, so a shot whose only second minimum above the limit sits in that pass is certified now
    where it was parked before.  Parked or not, a shot's answer is the same -- the recheck kernel computes the same arithmetic
    exactly -- so all outputs must equal the switch-off path, the gather kernel and the oracle."""
    H, pri = _window("bb72")
    s = _shots(H, pri, 384, seed=23)
    _three_paths(monkeypatch, H, pri, max_iter, s, nref=48, extra_env={"QD_SCATTER_M2_LIMIT": "40000"})
    _three_paths(monkeypatch, H, pri, max_iter, s, nref=48, extra_env={"QD_SCATTER_M2_LIMIT": "1"})      # every shot with a defect is parked


def test_fast_start_with_priors_above_one_half(gpu, monkeypatch):
    """Faults with p > 0.5 have L < 0 before anything is sent: pass 0 meets negative accumulators (sign bits set in the table, hard
    decision 1 at the start)."""
    H, pri = _window("bb72")
    pri = pri.copy()
    pri[[3, 500, 1001, 2000]] = (0.55, 0.6, 0.75, 0.9)
    s = _shots(H, pri, 256, seed=24)
    _three_paths(monkeypatch, H, pri, 20, s, nref=48)
