"""Fault-level outputs on the device: which faults the DEM sampler fired (qd_sample_dem_faults), the space-time correction a sliding-window
decode commits (qd_commit_bits, DeviceWindowPlan.decode(..., correction=...)), and the tallies by fault weight (qd_fault_stats_batch,
simulation.get_fault_spectrum).

1. the sampler's fault bits: same det / obs as `sample`, H E = det, L E = obs, the oracle's fault counts, a numpy Philox mirror; a partial
   last word; the path without an LDS bitmap; shot lists;
2. qd_commit_bits against numpy;
3. the plan's corrections against the per-window oracle, L C against the wrappers, H C = det, both drivers;
4. decode_dem_corrections against BatchDecoder;
5. qd_fault_stats_batch against numpy;
6. get_fault_spectrum against get_circuit_mem_pL, and its lightest residual on the host.

The oracle is orc.device_arithmetic's form for the options (tests/test_gpu_large_window.py)."""
import functools

import numpy as np
import pytest

import helpers
import oracle as orc
from frame_mirror import philox, threshold

pytestmark = pytest.mark.gpu

BB72 = "bb72_custom_r6_p0.003"
HGP = "hgp225_cardinal_r3_p0.01"
MINSUM = dict(bp_method="minimum_sum", schedule="parallel", max_iter=20, osd_method="osd_0", osd_order=0)
INCONSISTENT = 1 << 18


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _unpack(words, n):
    """int32 / uint32 [B, words] -> uint8 [B, n]."""
    w = np.ascontiguousarray(words)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :n]


def _pack(bits, words):
    """uint8 [B, n] -> int32 [B, words]."""
    pad = np.zeros((bits.shape[0], 32 * words), np.uint8)
    pad[:, :bits.shape[1]] = bits
    return np.packbits(pad, axis=1, bitorder="little").view("<i4").reshape(bits.shape[0], words)


def _mirror_faults(pri, seed, shots):
    """What the sampler must fire: fault j of shot s fires iff word j & 3 of Philox4x32-10(key = seed, counter = (s lo, s hi, j >> 2, 0)) is
    below floor(p_j 2^32)."""
    n = len(pri)
    s = np.asarray(shots, dtype=np.uint64)
    groups = np.arange((n + 3) // 4, dtype=np.uint64)
    r = philox((s & np.uint64(0xFFFFFFFF))[:, None], (s >> np.uint64(32))[:, None], groups[None, :], 0, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    words = np.stack(r, axis=2).reshape(len(s), -1)[:, :n]
    thr = np.array([threshold(p) for p in pri], dtype=np.uint64)
    return (words < thr[None, :]).astype(np.uint8)


def _check_sampler(H, L, pri, B, seed, shot0, oracle_counts=True):
    """sample_faults on (H, L, pri): everything test 1 asks of one model.  The fault rows are one word wider than needed and pre-filled: the
    extra word must survive.  Returns (sampler, E)."""
    import torch
    from scipy.sparse import csr_matrix
    from quits_amd.decoder.device import DemSampler
    n = H.shape[1]
    words = (n + 31) // 32
    smp = DemSampler(H, L, pri)
    assert smp.nfaults == n
    buf = torch.full((B, words + 1), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    det, obs, fb = smp.sample_faults(B, seed, shot0, fault_bits=buf)
    det0, obs0 = smp.sample(B, seed, shot0)
    assert torch.equal(det, det0) and torch.equal(obs, obs0), "det / obs differ from sample()'s"
    raw = fb.cpu().numpy()
    assert (raw[:, words] == 0x5A5A5A5A).all(), "the word past ceil(n / 32) was written"
    if n % 32:
        assert not (raw[:, words - 1].view(np.uint32) >> np.uint32(n % 32)).any(), "padding bits of the last word are set"
    E = _unpack(raw[:, :words], n)
    det, obs = det.cpu().numpy(), obs.cpu().numpy()
    assert np.array_equal((csr_matrix(H) @ E.T.astype(np.int64)).T % 2, det), "H E != det"
    assert np.array_equal((csr_matrix(L) @ E.T.astype(np.int64)).T % 2, obs), "L E != obs"
    shots = np.uint64(shot0) + np.arange(B, dtype=np.uint64)
    assert np.array_equal(E, _mirror_faults(pri, seed, shots)), "fault bits differ from the Philox mirror"
    if oracle_counts:
        d, o, nf = orc.sample_dem(H, L, pri, seed=seed, shot0=shot0, B=B)
        assert np.array_equal(d, det) and np.array_equal(o, obs)
        assert np.array_equal(E.sum(axis=1), nf), "row popcounts differ from the oracle's fault counts"
    tight = smp.sample_faults(B, seed, shot0)[2]                # rows of exactly ceil(n / 32) words
    assert tight.shape == (B, words) and np.array_equal(tight.cpu().numpy(), raw[:, :words])
    return smp, E


# ---- 1. the sampler ------------------------------------------------------------------------------------------------------------------
def test_sampler_fault_bits_bb72_across_the_32_bit_shot_counter(gpu):
    """BB72 r6 (288 x 2592: 81 whole words), 200 shots from 2^32 - 100 on: the shot counter crosses its low word."""
    H, L, pri = helpers.dem_matrices(BB72)
    assert H.shape == (288, 2592)
    shot0 = 2 ** 32 - 100
    smp, E = _check_sampler(H, L, pri, 200, 7, shot0)
    assert 5 < E.sum(axis=1).mean() < 30
    # a permuted shot list with a repeat equals the matching rows of the range
    rng = np.random.default_rng(0)
    pick = np.concatenate([rng.permutation(200)[:50], [17, 17]])
    det, obs, fb = smp.sample_shots_faults((shot0 + pick).tolist(), 7)
    d0, o0 = smp.sample_shots((shot0 + pick).tolist(), 7)
    assert np.array_equal(det.cpu().numpy(), d0.cpu().numpy()) and np.array_equal(obs.cpu().numpy(), o0.cpu().numpy())
    assert np.array_equal(_unpack(fb.cpu().numpy(), 2592), E[pick])


def test_sampler_fault_bits_hgp_partial_last_word(gpu):
    """HGP r3: n = 5409 = 169 words + 1 bit."""
    H, L, pri = helpers.dem_matrices(HGP)
    assert H.shape[1] == 5409
    _check_sampler(H, L, pri, 64, 7, 3)


@pytest.mark.parametrize("n", [3, 33, 2 ** 19 + 5])
def test_sampler_fault_bits_synthetic(gpu, n):
    """Three shots of synthetic models: fewer faults than a Philox group, one word and a bit, and 2^19 + 5 faults -- 65 540 bytes of bitmap,
    more than the kernel's 64 KiB of LDS: the global row with atomics."""
    from scipy.sparse import csc_matrix
    rng = np.random.default_rng(n)
    m, nobs = 40, 2
    rows = np.stack([rng.permutation(m)[:2] for _ in range(min(n, 4096))])
    rows = rows[rng.integers(0, len(rows), size=n)].reshape(-1)
    H = csc_matrix((np.ones(2 * n, np.uint8), (rows, np.repeat(np.arange(n), 2))), shape=(m, n))
    L = csc_matrix((np.ones(n, np.uint8), (rng.integers(0, nobs, size=n), np.arange(n))), shape=(nobs, n))
    pri = rng.uniform(0.2, 0.6, size=n) if n < 100 else rng.uniform(0.0005, 0.002, size=n)
    smp, E = _check_sampler(H, L, pri, 3, 11, 2 ** 32 - 1)
    assert E.any()
    if n > 100:
        idx = [2 ** 32 + 1, 2 ** 32 - 1]
        assert np.array_equal(_unpack(smp.sample_shots_faults(idx, 11)[2].cpu().numpy(), n), E[[2, 0]])


# ---- 2. qd_commit_bits ---------------------------------------------------------------------------------------------------------------
def _commit_ref(out_bits, src_bits, nbits, bit0):
    ref = out_bits.copy()
    ref[:, bit0:bit0 + nbits] = src_bits[:, :nbits]
    return ref


def test_commit_bits_against_numpy(gpu):
    """Every (nbits, out_bit0) of the grid, 70 rows, strides wider than needed, random bits everywhere: the range takes the source's bits
    (whatever lies in the source past nbits), every other bit of the output survives."""
    from quits_amd.decoder.device import commit_bits
    rng = np.random.default_rng(1)
    B = 70
    for nbits in (0, 1, 31, 32, 33, 64, 1000):
        for bit0 in (0, 1, 31, 32, 37, 63):
            sw, ow = (nbits + 31) // 32 + 2, (bit0 + nbits + 31) // 32 + 2
            src = rng.integers(-2 ** 31, 2 ** 31, size=(B, sw + 3), dtype=np.int64).astype(np.int32)
            out = rng.integers(-2 ** 31, 2 ** 31, size=(B, ow + 1), dtype=np.int64).astype(np.int32)
            d_src, d_out = _dev(src)[:, :sw], _dev(out)[:, :ow]
            commit_bits(d_src, nbits, d_out, bit0)
            got = d_out.cpu().numpy()
            ref = _commit_ref(_unpack(out[:, :ow], 32 * ow), _unpack(src[:, :sw], 32 * sw), nbits, bit0)
            assert np.array_equal(_unpack(got, 32 * ow), ref), "nbits = %d, out_bit0 = %d" % (nbits, bit0)


def test_commit_bits_chain_of_adjacent_ranges(gpu):
    """324, 360, 360, 828 bits one after the other (the first, two middle and the last window of BB72 (3, 1)): stream-ordered calls whose
    ranges share words equal one concatenation; the bits past the last range survive."""
    from quits_amd.decoder.device import commit_bits
    rng = np.random.default_rng(2)
    B, widths = 70, (324, 360, 360, 828)
    total = sum(widths)
    ow = (total + 31) // 32 + 1
    out = rng.integers(-2 ** 31, 2 ** 31, size=(B, ow), dtype=np.int64).astype(np.int32)
    d_out = _dev(out)
    parts, at = [], 0
    for nb in widths:
        src = rng.integers(-2 ** 31, 2 ** 31, size=(B, (nb + 31) // 32), dtype=np.int64).astype(np.int32)
        commit_bits(_dev(src), nb, d_out, at)
        parts.append(_unpack(src, nb))
        at += nb
    ref = _unpack(out, 32 * ow)
    ref[:, :total] = np.concatenate(parts, axis=1)
    assert np.array_equal(_unpack(d_out.cpu().numpy(), 32 * ow), ref)


# ---- 3. the plan's corrections -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(name):
    from quits_amd.dem import Circuit
    code = {BB72: "bb72", HGP: "hgp225"}[name]
    cd = helpers.code(code)
    H, L, pri = helpers.dem_matrices(name)
    wins = helpers.window_set(name, 3, 1)
    nz = cd["hz"].shape[0]
    for k, w in enumerate(wins):
        w["row0"] = k * nz
    return Circuit(helpers.circuit_text(name)), cd, H, L, np.asarray(pri, np.float64), wins, H.shape[0] // nz - 2


@functools.lru_cache(maxsize=None)
def _shots(name, B=300, seed=5):
    """300 DEM-sampled shots of seed 5 with their fault sets: (det, obs, E) on the host, and the device's packed fault words."""
    from quits_amd.decoder.device import DemSampler
    circ, cd, H, L, pri, wins, R = _model(name)
    det, obs, fb = DemSampler(H, L, pri).sample_faults(B, seed)
    return det.cpu().numpy(), obs.cpu().numpy(), _unpack(fb.cpu().numpy(), H.shape[1]), fb.cpu().numpy()


def _oracle_correction(name, det, prm):
    """The concatenation of the per-window oracle results: window k decodes its detector rows xor the carry U_{k-1} e_{k-1} and commits its
    first ncommit columns.  prm: orc.make_params' argument tuple without the form; flooding min-sum goes on the device's LLR grid."""
    circ, cd, H, L, pri, wins, R = _model(name)
    nz = cd["hz"].shape[0]
    C_ref = np.zeros((det.shape[0], H.shape[1]), np.uint8)
    carry = np.zeros((det.shape[0], nz), np.uint8)
    col0 = 0
    for w in wins:
        Hk, pk = w["H"], np.asarray(w["priors"], np.float64)
        g, form = orc.device_arithmetic(Hk, pk, prm[0], prm[1], prm[2], 1.0)
        s = det[:, w["row0"]:w["row0"] + Hk.shape[0]].copy()
        s[:, :nz] ^= carry
        err, _ = helpers.oracle_decode_batch_parallel(Hk, pk, s, prm + (1.0, form), prm[2] if form == orc.FORM_LDPC_F64 else None)
        nc = w["L"].shape[1]
        C_ref[:, col0:col0 + nc] = err[:, :nc]
        if w["U"] is not None:
            carry = ((w["U"] @ err[:, :nc].T.astype(np.int64)).T % 2).astype(np.uint8)
        col0 += nc
    assert col0 == H.shape[1]
    return C_ref


def _plan_corrections(plan, det, chunk, pipelined):
    """plan.decode with `correction` through one of the two drivers: (pred, C words, inconsistent-in-any-window per shot)."""
    import torch
    words = (plan.nfaults + 31) // 32
    saved = plan.chunk, plan.pipeline
    try:
        plan.chunk, plan.pipeline = chunk, pipelined
        with plan.in_use():
            corr = torch.full((det.shape[0], words + 1), 0x33333333, dtype=torch.int32, device="cuda")      # (pre-filled: the call zero-fills)
            stats = []
            pred = plan.decode(_dev(det), stats, corr)
            torch.cuda.synchronize()
            bad = np.zeros(det.shape[0], bool)
            at = [0] * len(plan.windows)
            for k, st in stats:
                bad[at[k]:at[k] + st.shape[0]] |= (st.cpu().numpy() & INCONSISTENT) != 0
                at[k] += st.shape[0]
            assert all(a == det.shape[0] for a in at)
            return pred.cpu().numpy(), corr.cpu().numpy(), bad
    finally:
        plan.chunk, plan.pipeline = saved


CORRECTION_CASES = {
    "bb72-minsum-osd0": (BB72, "osd", MINSUM, ("minimum_sum", "parallel", 20, "osd_0", 0)),
    "bb72-wrapper-defaults": (BB72, "osd", {}, ("product_sum", "serial", 2, "osd_cs", 0)),
    "bb72-lsd_cs-0": (BB72, "lsd", dict(bp_method="minimum_sum", schedule="parallel", max_iter=20, lsd_method="lsd_cs", lsd_order=0),
                      ("minimum_sum", "parallel", 20, "lsd_0", 0)),
    "hgp-minsum-osd0": (HGP, "osd", MINSUM, ("minimum_sum", "parallel", 20, "osd_0", 0)),
}


@pytest.mark.parametrize("case", sorted(CORRECTION_CASES))
def test_plan_corrections_equal_the_windows_oracle(gpu, case):
    """300 shots through plan.decode(..., correction=...): C equals the concatenation of the per-window oracle results, L C the wrapper's
    predictions, H C = det on every shot no window of which was inconsistent (at least 290 of the 300), and the single-stream driver and the
    pipelined one (chunks of 64: five chunks, the last of 44 shots) give the same words.  HGP's commit offsets 1188 and 2484 are off the
    word grid."""
    from scipy.sparse import csr_matrix
    from quits_amd.decoder import (BpLsdDecoder, BpOsdDecoder, sliding_window_bplsd_circuit_mem, sliding_window_bposd_circuit_mem,
                                   sliding_window_corrections)
    from quits_amd.decoder.plan import cached_circuit_plan
    name, kind, kw, prm = CORRECTION_CASES[case]
    circ, cd, H, L, pri, wins, R = _model(name)
    det, obs, E, _ = _shots(name)
    n = H.shape[1]
    words = (n + 31) // 32
    wrapper, cls = (sliding_window_bplsd_circuit_mem, BpLsdDecoder) if kind == "lsd" else (sliding_window_bposd_circuit_mem, BpOsdDecoder)
    pred_w = wrapper(det, circ, cd["hz"], cd["lz"], 3, 1, **kw)
    # the wrapper's own plan (same dict, same cache key)
    if kind == "lsd":
        opts = {'bp_method': prm[0], 'max_iter': prm[2], 'schedule': prm[1], 'lsd_method': kw["lsd_method"], 'lsd_order': kw["lsd_order"]}
    else:
        opts = {'bp_method': prm[0], 'max_iter': prm[2], 'schedule': prm[1], 'osd_method': prm[3], 'osd_order': prm[4]}
    from quits_amd.decoder.plan_cache import plan_cache_info
    hits = plan_cache_info()["hits"]
    plan = cached_circuit_plan(circ, cd["hz"], 3, 1, R, cls, cls, dict(opts), dict(opts))
    assert plan_cache_info()["hits"] == hits + 1, "the test's plan is not the wrapper's cached plan"
    assert plan.nfaults == n and plan.commit_ranges == [(sum(w["L"].shape[1] for w in wins[:k]), wins[k]["L"].shape[1]) for k in range(len(wins))]
    pred_s, raw_s, bad = _plan_corrections(plan, det, 64, False)
    pred_p, raw_p, bad_p = _plan_corrections(plan, det, 64, True)
    for raw in (raw_s, raw_p):
        assert not raw[:, words].any(), "the call zero-fills the whole tensor"
        if n % 32:
            assert not (raw[:, words - 1].view(np.uint32) >> np.uint32(n % 32)).any()
    assert np.array_equal(raw_s, raw_p), "single-stream and pipelined corrections differ"
    assert np.array_equal(pred_s, pred_p) and np.array_equal(bad, bad_p)
    Cd = _unpack(raw_s[:, :words], n)
    C_ref = _oracle_correction(name, det, prm)
    diff = np.flatnonzero((Cd != C_ref).any(axis=1))
    assert diff.size == 0, "corrections differ from the per-window oracle on shots %s" % diff[:10]
    LC = ((csr_matrix(L) @ Cd.T.astype(np.int64)).T % 2).astype(np.int64)
    assert np.array_equal(LC, pred_w) and np.array_equal(pred_s.astype(np.int64), pred_w)
    good = ~bad
    print("%s: %d of %d shots without an inconsistent window, mean |C| = %.2f, mean |E| = %.2f" % (case, good.sum(), len(good), Cd.sum(axis=1).mean(),
                                                                                              E.sum(axis=1).mean()))
    assert good.sum() >= 290
    HC = (csr_matrix(H) @ Cd.T.astype(np.int64)).T % 2
    assert np.array_equal(HC[good], det[good]), "H C != det on a shot without an inconsistent window"
    # the public function: the same predictions and corrections from host samples, through the staged path
    pred_f, packed = sliding_window_corrections(det, circ, cd["hz"], cd["lz"], 3, 1, **kw)
    assert packed.num_bits == n and not packed.is_cuda and len(packed) == len(det)
    assert np.array_equal(pred_f, pred_w) and np.array_equal(np.asarray(packed), Cd)


def test_host_corrections_through_the_chained_pieces(gpu):
    """sliding_window_corrections on host samples with chunks of 64 and pieces of three chunks: the staged, chained path (two pieces in
    flight, a ragged last one) returns what the device-resident call returns."""
    from quits_amd.decoder import BpOsdDecoder
    from quits_amd.decoder.plan import cached_circuit_plan
    circ, cd, H, L, pri, wins, R = _model(BB72)
    det = _shots(BB72)[0]
    opts = {'bp_method': "minimum_sum", 'max_iter': 20, 'schedule': "parallel", 'osd_method': "osd_0", 'osd_order': 0}
    plan = cached_circuit_plan(circ, cd["hz"], 3, 1, R, BpOsdDecoder, BpOsdDecoder, dict(opts), dict(opts))
    pred0, raw0, _ = _plan_corrections(plan, det, 1 << 16, False)
    saved = plan.chunk, plan.pipeline, plan.host_piece
    try:
        plan.chunk, plan.pipeline, plan.host_piece = 64, True, 128
        plan._staging = None
        pred, packed = plan.decode_host(det, corrections=True)
    finally:
        plan.chunk, plan.pipeline, plan.host_piece = saved
        plan._staging = None
    n = H.shape[1]
    assert np.array_equal(pred, pred0.astype(np.int64))
    assert np.array_equal(np.asarray(packed), _unpack(raw0[:, :(n + 31) // 32], n))


def test_phenomenological_plan_corrections_at_plan_level(gpu):
    """A phenomenological plan fills `correction` through the same code: window k's whole vector (its commit matrix spans the window) at
    commit_ranges[k], and the sum of L_k applied to the pieces is the call's prediction; both drivers agree."""
    from quits_amd.decoder import BpOsdDecoder, sliding_window_bposd_phenom_mem
    from quits_amd.decoder.plan import cached_phenom_plan, phenom_window_set
    circ, cd, H, L, pri, wins, R = _model(BB72)
    det = _shots(BB72)[0]
    hz, lz = cd["hz"], cd["lz"]
    opts = {'bp_method': "minimum_sum", 'max_iter': 10, 'schedule': "parallel", 'osd_method': "osd_0", 'osd_order': 0, 'error_rate': 0.03}
    pred_w = sliding_window_bposd_phenom_mem(det, hz, lz, 3, 1, eff_error_rate_per_fault=0.03, max_iter=10, bp_method="minimum_sum",
                                             schedule="parallel", osd_method="osd_0")
    plan = cached_phenom_plan(hz, lz, 3, 1, R, BpOsdDecoder, BpOsdDecoder, dict(opts), dict(opts))
    checks, commits, priors, updates = phenom_window_set(hz, lz, 3, 1, R, 0.03, 0.03)
    assert plan.commit_ranges == [(sum(c.shape[1] for c in checks[:k]), checks[k].shape[1]) for k in range(len(checks))]
    pred, raw, _ = _plan_corrections(plan, det, 64, False)
    pred_p, raw_p, _ = _plan_corrections(plan, det, 64, True)
    assert np.array_equal(raw, raw_p) and np.array_equal(pred, pred_p) and np.array_equal(pred.astype(np.int64), pred_w)
    Cd = _unpack(raw, plan.nfaults)
    acc = np.zeros_like(pred_w)
    for (col0, nc), Lk in zip(plan.commit_ranges, commits):
        acc ^= (Lk @ Cd[:, col0:col0 + nc].T.astype(np.int64)).T % 2
    assert Cd.any() and np.array_equal(acc, pred_w)


# ---- 4. the whole history ------------------------------------------------------------------------------------------------------------
def test_decode_dem_corrections_equal_batch_decoder(gpu):
    from quits_amd.decoder import decode_dem, decode_dem_corrections
    from quits_amd.decoder.device import BatchDecoder, WindowGraph, unpack_bits
    from quits_amd.samples import PackedSamples
    circ, cd, H, L, pri, wins, R = _model(BB72)
    det = _shots(BB72)[0][:128]
    pred, packed = decode_dem_corrections(circ, det, **MINSUM)
    assert np.array_equal(pred, decode_dem(circ, det, **MINSUM))
    wg = WindowGraph(H, pri)
    bits, _ = BatchDecoder(wg, **MINSUM).decode(_dev(det))
    ref = unpack_bits(bits, wg.n).cpu().numpy()
    assert isinstance(packed, PackedSamples) and packed.num_bits == H.shape[1] and np.array_equal(np.asarray(packed), ref)
    pred_p, packed_p = decode_dem_corrections(circ, PackedSamples.pack(det), **MINSUM)
    assert np.array_equal(pred_p, pred) and np.array_equal(np.asarray(packed_p), ref)
    empty = decode_dem_corrections(circ, det[:0], **MINSUM)
    assert empty[0].shape == (0, L.shape[0]) and empty[1].shape == (0, H.shape[1])


def test_predict_writes_corrections(gpu, tmp_path):
    """python -m quits_amd predict --corrections_out: the b8 file holds decode_dem_corrections' words as they are; predictions unchanged."""
    from quits_amd.__main__ import main
    from quits_amd.decoder import decode_dem_corrections
    from quits_amd.samples import read_shots, write_shots
    circ, cd, H, L, pri, wins, R = _model(BB72)
    det = _shots(BB72)[0][:64]
    (tmp_path / "c.stim").write_text(str(circ))
    write_shots(str(tmp_path / "s.b8"), det, "b8")
    base = ["predict", "--circuit", str(tmp_path / "c.stim"), "--in", str(tmp_path / "s.b8"), "--in_format", "b8", "--out_format", "01",
            "--bp_method", "minimum_sum", "--schedule", "parallel", "--max_iter", "20", "--osd_method", "osd_0"]
    assert main(base + ["--out", str(tmp_path / "p0.01")]) == 0
    assert main(base + ["--out", str(tmp_path / "p1.01"), "--corrections_out", str(tmp_path / "c.b8")]) == 0
    assert main(base + ["--out", str(tmp_path / "p2.01"), "--corrections_out", str(tmp_path / "c.hits"), "--corrections_format", "hits",
                        "--checks_per_round", str(cd["hz"].shape[0]), "--window", "3", "--commit", "1"]) == 0
    assert (tmp_path / "p0.01").read_text() == (tmp_path / "p1.01").read_text()
    pred, packed = decode_dem_corrections(circ, det, **MINSUM)
    n = H.shape[1]
    assert np.array_equal(np.asarray(read_shots(str(tmp_path / "c.b8"), "b8", n)), np.asarray(packed))
    assert read_shots(str(tmp_path / "c.hits"), "hits", n).shape == (64, n)


# ---- 5. qd_fault_stats_batch ---------------------------------------------------------------------------------------------------------
def _stats_ref(E, Cm, res_nonzero, failed, shot0):
    hist = np.zeros((3, 256), np.int64)
    we = np.minimum(E.sum(axis=1), 255)
    wx = np.minimum((E ^ Cm).sum(axis=1), 255)
    np.add.at(hist[0], we, 1)
    np.add.at(hist[1], we[failed], 1)
    sel = failed & ~res_nonzero
    np.add.at(hist[2], wx[sel], 1)
    counts = [len(E), int(failed.sum()), int(res_nonzero.sum()), int((failed & res_nonzero).sum())]
    full = (E ^ Cm).sum(axis=1).astype(np.int64)
    best = min(((int(full[b]) << 40) | (shot0 + b) for b in np.flatnonzero(sel)), default=None)
    return hist, np.array(counts, np.int64), None if best is None else (best >> 40, best & ((1 << 40) - 1))


def test_fault_stats_against_numpy(gpu):
    """The 300 shots of test 3 with their corrections, tallied in two calls (200 + 100, so the counters accumulate and the second call's
    shot0 counts), plus hand-made rows: a fault set of weight 300 (last bin), a row with a non-zero residual that fails and one that does
    not, and a failing row whose residual is lighter than any decoded one."""
    import torch
    from scipy.sparse import csr_matrix
    from quits_amd.decoder import BpOsdDecoder
    from quits_amd.decoder.device import FaultStats, GF2Matrix, Tally
    from quits_amd.decoder.plan import cached_circuit_plan
    circ, cd, H, L, pri, wins, R = _model(BB72)
    det, obs, E, fwords = _shots(BB72)
    n, m = H.shape[1], H.shape[0]
    words = (n + 31) // 32
    opts = {'bp_method': "minimum_sum", 'max_iter': 20, 'schedule': "parallel", 'osd_method': "osd_0", 'osd_order': 0}
    plan = cached_circuit_plan(circ, cd["hz"], 3, 1, R, BpOsdDecoder, BpOsdDecoder, dict(opts), dict(opts))
    pred, raw, _ = _plan_corrections(plan, det, 1 << 16, False)
    Cm = _unpack(raw[:, :words], n)
    # hand-made rows appended to the batch
    rng = np.random.default_rng(3)
    extra_E = np.zeros((4, n), np.uint8)
    extra_C = np.zeros((4, n), np.uint8)
    extra_E[0, rng.permutation(n)[:300]] = 1                      # weight 300: the last bin; decoded "perfectly"
    extra_C[0] = extra_E[0]
    extra_E[1, [5, 77]] = 1                                        # fails with a non-zero residual
    extra_E[2, [9]] = 1                                            # does not fail, non-zero residual
    extra_E[3, [1, 2, n - 1]] = 1                                  # fails, zero residual, |E xor C| = 2: the lightest
    extra_C[3, [1]] = 1
    E_all, C_all = np.concatenate([E, extra_E]), np.concatenate([Cm, extra_C])
    B = len(E_all)
    res = np.zeros((B, m), np.uint8)
    res[:300] = ((csr_matrix(H) @ Cm.T.astype(np.int64)).T % 2).astype(np.uint8) ^ det
    res[301, m - 1] = 1
    res[302, 0] = 3
    failed = np.zeros(B, bool)
    failed[:300] = (pred != obs).any(axis=1)
    failed[[301, 303]] = True
    assert failed[:300].sum() >= 8
    # the device's own residual on the decoded rows: H applied to the corrections onto a copy of det
    d_res = _dev(det.copy())
    GF2Matrix(H).xor_apply(_dev(raw), d_res, accumulate=True)
    assert np.array_equal(d_res.cpu().numpy(), res[:300])
    stride = words + 1
    d_E, d_C, d_r = _dev(_pack(E_all, stride)), _dev(_pack(C_all, stride)), _dev(res)
    # padding bits of the last word and the extra word must not count
    d_E[:, words:] = -1
    shot0 = 2 ** 33
    fs = FaultStats()
    for lo, hi in ((0, 200), (200, B)):
        mask = np.zeros(((hi - lo + 63) // 64,), np.uint64)
        for b in np.flatnonzero(failed[lo:hi]):
            mask[b >> 6] |= np.uint64(1) << np.uint64(b & 63)
        fs.add(d_E[lo:hi], d_C[lo:hi], n, d_r[lo:hi], _dev(mask.view(np.int64)), shot0 + lo)
    hist, counts, lightest = fs.result()
    rh, rc, rl = _stats_ref(E_all, C_all, res.any(axis=1), failed, shot0)
    assert np.array_equal(counts, rc), (counts, rc)
    for i, what in enumerate(("shots by |E|", "failing shots by |E|", "failing shots with a zero residual by |E xor C|")):
        assert np.array_equal(hist[i], rh[i]), what
    assert hist[0, 255] == 1 and counts[2] >= 2 and counts[3] >= 1
    assert lightest == rl == (2, shot0 + 303)
    # the fail mask of Tally.add is the mask this kernel reads
    t = Tally(obs.shape[1])
    tm = torch.zeros((5,), dtype=torch.int64, device="cuda")
    t.add(_dev(pred), _dev(obs), None, tm)
    fs2 = FaultStats()
    fs2.add(_dev(_pack(E, words)), _dev(raw[:, :words].copy()), n, d_res, tm, 0)
    h2, c2, l2 = fs2.result()
    r2 = _stats_ref(E, Cm, res[:300].any(axis=1), failed[:300], 0)
    assert np.array_equal(h2, r2[0]) and np.array_equal(c2, r2[1]) and l2 == r2[2]
    assert FaultStats().result()[2] is None


# ---- 6. the experiment ---------------------------------------------------------------------------------------------------------------
def test_fault_spectrum_equals_the_memory_experiment(gpu):
    """4096 shots in batches of 1024: shots and errors are get_circuit_mem_pL's (sampler 'dem', same seed and batch), the histograms sum to
    them, no shot has a non-zero residual, and the lightest residual is what its shot says: replay_faults xor the shot's correction has that
    weight, lies in the kernel of H and flips an observable."""
    from scipy.sparse import csr_matrix
    from quits_amd.decoder import sliding_window_corrections
    from quits_amd.simulation import get_circuit_mem_pL, get_fault_spectrum, replay_faults, replay_shots
    circ, cd, H, L, pri, wins, R = _model(BB72)
    args = (circ, cd["hz"], cd["lz"], 3, 1, 4096)
    r = get_fault_spectrum(*args, seed=5, batch=1024, **MINSUM)
    ref = get_circuit_mem_pL(*args, sampler="dem", seed=5, batch=1024, **MINSUM)
    print("fault spectrum: %d shots, %d errors, lightest %s, residual shots %d" % (r.shots, r.errors, r.lightest, r.residual_shots))
    assert (r.shots, r.errors) == (ref.shots, ref.errors) == (4096, ref.errors) and r.pL == ref.pL
    assert r.errors >= 8
    assert r.shots_by_faults.sum() == r.shots and r.errors_by_faults.sum() == r.errors
    assert r.residual_shots == 0 and r.failing_residual_shots == 0 and r.residual_weight_hist.sum() == r.errors
    assert (r.errors_by_faults <= r.shots_by_faults).all()
    f = r.failure_fraction()
    assert np.nanmax(f) <= 1.0 and np.isnan(f[r.shots_by_faults == 0]).all()
    w, s = r.lightest
    assert 0 < w and r.residual_weight_hist[:w].sum() == 0 and r.residual_weight_hist[min(w, 255)] >= 1
    assert s in set(ref.failing_shots.tolist())
    Es = replay_faults(circ, [s], 5)
    det, obs = replay_shots(circ, [s], 5, sampler="dem")
    assert np.array_equal((csr_matrix(H) @ Es.T.astype(np.int64)).T % 2, det.astype(np.int64))
    pred, packed = sliding_window_corrections(det, circ, cd["hz"], cd["lz"], 3, 1, **MINSUM)
    resid = Es[0].astype(np.uint8) ^ np.asarray(packed)[0]
    assert resid.sum() == w
    assert not ((csr_matrix(H) @ resid.astype(np.int64)) % 2).any(), "the lightest residual is detectable"
    assert ((csr_matrix(L) @ resid.astype(np.int64)) % 2).any(), "the lightest residual flips no observable"
    # a shard of the shots is the matching slice of the experiment
    half = get_fault_spectrum(*args, seed=5, batch=1024, shard=(1, 2), **MINSUM)
    assert half.shots == 2048 and half.errors == int(((ref.failing_shots >= 2048)).sum())
