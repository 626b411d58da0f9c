"""Soft outputs on the device: every result equals quits_amd/soft.py, the definition.

1. qd_soft_weigh against numpy: bit counts around the word grid, wider rows, padding garbage, weights of +-(2^31 - 1), detector bytes of which
   only the low bit counts;
2. qd_soft_fold: every field at its maximum, bits 14 .. 19 leaking nowhere, three folds, two row strides;
3. qd_soft_tally: bin edges, negative and overflowing values, four shifts, accumulation, the NULL mask;
4. the public calls on BB72 r6, W = 3 / F = 1: records = soft_mirror of the corrections, the samples and the status words; BP-OSD, BP-LSD and
   Relay-BP;
5. the pipelined driver equals the single-stream one;
6. get_postselected_pL against get_circuit_mem_pL and against the records of the replayed shots."""
import functools

import numpy as np
import pytest

import helpers
from quits_amd import soft

pytestmark = pytest.mark.gpu

BB72 = "bb72_custom_r6_p0.003"
MINSUM = dict(bp_method="minimum_sum", schedule="parallel", max_iter=20, osd_method="osd_0", osd_order=0)
SMALL = dict(pre_iter=20, num_sets=4, set_max_iter=15)          # the relay tests' settings (test_gpu_relay.py)
W_MAX = 2 ** 31 - 1
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _unpack(words, n):
    w = np.ascontiguousarray(words)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :n]


# ---- 1. qd_soft_weigh ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", [1, 32, 33, 2592, 4097])
def test_soft_weigh_against_numpy(gpu, nbits):
    """Rows: empty, all ones, only bit nbits - 1, random ones; every padding bit of the last word and every word past it holds garbage.  With
    the table of all 2^31 - 1 an all-ones row of 4097 bits sums to 4097 (2^31 - 1) > 2^43."""
    import torch
    from quits_amd.decoder.device import soft_weigh
    rng = np.random.default_rng(nbits)
    need = (nbits + 31) // 32
    mixed = rng.integers(-W_MAX, W_MAX + 1, size=nbits, dtype=np.int64)
    mixed[rng.integers(0, nbits, size=max(1, nbits // 7))] = W_MAX
    mixed[rng.integers(0, nbits, size=max(1, nbits // 7))] = -W_MAX
    mixed[nbits - 1] = -W_MAX if nbits > 1 else W_MAX
    tables = {"mixed": mixed, "max": np.full(nbits, W_MAX, dtype=np.int64)}
    det_bytes = np.array([0x00, 0x01, 0xFE, 0xFF], dtype=np.uint8)
    ms = [1, 3, 4, 108, 1009]
    case = 0
    for extra in (0, 3):
        for B in (0, 1, 63, 64, 65, 257):
            for tname, table in tables.items():
                m = ms[case % len(ms)]
                case += 1
                bits = (rng.random((B, nbits)) < 0.3).astype(np.uint8)
                bits[0::5] = 0
                bits[1::5] = 1
                bits[2::5] = 0
                bits[2::5, nbits - 1] = 1
                raw = rng.integers(0, 256, size=(B, 4 * (need + extra)), dtype=np.uint8)      # garbage everywhere ...
                rowbits = np.unpackbits(raw, axis=1, bitorder="little")
                rowbits[:, :nbits] = bits                                                     # ... but in the nbits bits that count
                if nbits % 32 and B:
                    rowbits[:, nbits:32 * need] = 1                                           # the padding bits of the last word: all set
                corr = np.packbits(rowbits, axis=1, bitorder="little").view("<i4").reshape(B, need + extra)
                det = np.full((B, m + 5), 0xFF, dtype=np.uint8)                               # non-zero bytes past m
                det[:, :m] = det_bytes[rng.integers(0, 4, size=(B, m))]
                rec = torch.full((B, 8), SENTINEL, dtype=torch.int64, device="cuda")
                soft_weigh(_dev(corr), nbits, _dev(table.astype(np.int32)), _dev(det)[:, :m], rec)
                got = rec.cpu().numpy()
                want = soft.soft_mirror(bits, det[:, :m], [], table)
                tag = "nbits %d, %d extra words, B %d, m %d, %s weights" % (nbits, extra, B, m, tname)
                assert np.array_equal(got[:, :3], want[:, :3]), tag
                assert (got[:, 3:] == SENTINEL).all(), tag + ": fields 3 .. 5 or the spare columns were written"
                if B > 1 and tname == "max":
                    assert got[1, 0] == nbits * W_MAX and got[1, 1] == nbits
    assert 4097 * W_MAX > 2 ** 43


def test_soft_weigh_every_m(gpu):
    """Every detector count of the list with one correction shape, rows of six int64 (no spare columns)."""
    import torch
    from quits_amd.decoder.device import soft_weigh
    rng = np.random.default_rng(3)
    nbits, B = 33, 65
    bits = (rng.random((B, nbits)) < 0.5).astype(np.uint8)
    pad = np.zeros((B, 64), np.uint8)
    pad[:, :nbits] = bits
    corr = np.packbits(pad, axis=1, bitorder="little").view("<i4").reshape(B, 2)
    table = rng.integers(-W_MAX, W_MAX + 1, size=nbits, dtype=np.int64)
    for m in (1, 3, 4, 108, 1009):
        det = np.full((B, m + 5), 0x01, dtype=np.uint8)
        det[:, :m] = np.array([0x00, 0x01, 0xFE, 0xFF], dtype=np.uint8)[rng.integers(0, 4, size=(B, m))]
        rec = torch.full((B, 6), SENTINEL, dtype=torch.int64, device="cuda")
        soft_weigh(_dev(corr), nbits, _dev(table.astype(np.int32)), _dev(det)[:, :m], rec)
        got = rec.cpu().numpy()
        assert np.array_equal(got[:, :3], soft.soft_mirror(bits, det[:, :m], [], table)[:, :3]), "m = %d" % m
        assert (got[:, 3:] == SENTINEL).all()


# ---- 2. qd_soft_fold -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [6, 8])
def test_soft_fold_against_the_mirror(gpu, stride):
    import torch
    from quits_amd.decoder.device import soft_fold
    rng = np.random.default_rng(stride)
    crafted = [0, 0x3FFF, 0xFFF << 20, 0x3FFF | (0xFFF << 20) | (1 << 17), 0x3F << 14, (0x3F << 14) & ~(1 << 17), 0xFFFFFFFF, 1 << 31]
    crafted += [1 << b for b in range(14, 20)] + [(1 << b) | 7 | (5 << 20) for b in range(14, 20)]
    B = 300
    folds = []
    for i in range(3):
        s = rng.integers(0, 2 ** 32, size=B, dtype=np.uint64)
        s[:len(crafted)] = np.roll(np.array(crafted, dtype=np.uint64), i)
        folds.append(s.astype(np.uint32).view(np.int32))
    rec = torch.full((B, stride), SENTINEL, dtype=torch.int64, device="cuda")
    rec[:, 3:6] = 0
    want = np.zeros((B, 3), dtype=np.int64)
    for i, s in enumerate(folds):
        soft_fold(_dev(s), rec)
        it, post, tail = soft.status_fields(s)
        want += np.stack([it, post, tail], axis=1)
        got = rec.cpu().numpy()
        assert np.array_equal(got[:, 3:6], want), "after fold %d" % (i + 1)
        assert (got[:, :3] == SENTINEL).all() and (got[:, 6:] == SENTINEL).all(), "fields 0 .. 2 or the spare columns were written"
    # bits 14 .. 19 alone: only bit 17 shows, and only in `post`
    for b in range(14, 20):
        one = torch.zeros((1, stride), dtype=torch.int64, device="cuda")
        soft_fold(_dev(np.array([1 << b], dtype=np.int32)), one)
        assert one.cpu().numpy()[0].tolist() == [0, 0, 0, 0, 1 if b == 17 else 0, 0] + [0] * (stride - 6)
    every = torch.zeros((1, stride), dtype=torch.int64, device="cuda")
    soft_fold(_dev(np.array([0x3F << 14], dtype=np.int32)), every)
    assert every.cpu().numpy()[0, :6].tolist() == [0, 0, 0, 0, 1, 0]
    top = torch.zeros((1, stride), dtype=torch.int64, device="cuda")
    soft_fold(_dev(np.array([0x3FFF | (0xFFF << 20)], dtype=np.uint32).view(np.int32)), top)
    assert top.cpu().numpy()[0, :6].tolist() == [0, 0, 0, 0x3FFF, 0, 0xFFF]
    soft_fold(_dev(np.zeros((0,), np.int32)), torch.zeros((0, stride), dtype=torch.int64, device="cuda"))       # B = 0


# ---- 3. qd_soft_tally ------------------------------------------------------------------------------------------------------------------
def _edge_values(shift):
    vals = [0, -1, -2 ** 62, 2 ** 62, 1024 * 2 ** shift, 1024 * 2 ** shift - 1, 1023 * 2 ** shift]
    for k in (1, 2, 3, 511, 1023):
        vals += [k * 2 ** shift - 1, k * 2 ** shift]
    return np.array(vals, dtype=np.int64)


@pytest.mark.parametrize("shifts", [(0, 1, 15, 40, 0, 15), (40, 15, 1, 0, 1, 40)])
def test_soft_tally_against_the_mirror(gpu, shifts):
    import torch
    from quits_amd.decoder.device import SoftTally, soft_tally
    rng = np.random.default_rng(sum(shifts))
    st = SoftTally(shifts)
    want = np.zeros((6, 2, 1024), dtype=np.int64)
    for B in (0, 1, 64, 100, 100):                      # (the two calls of 100 shots accumulate, like everything before them)
        rec = np.zeros((B, 6), dtype=np.int64)
        for f in range(6):
            pool = _edge_values(shifts[f])
            rec[:, f] = pool[rng.integers(0, len(pool), size=B)]
            rec[:min(B, len(pool)), f] = pool[:min(B, len(pool))]
        fail = rng.random(B) < 0.4
        pad = np.zeros(((B + 63) // 64) * 64, np.uint8)
        pad[:B] = fail                                  # bits past B are zero
        mask = np.packbits(pad, bitorder="little").view("<i8").copy() if B else np.zeros((0,), np.int64)
        st.add(_dev(rec), _dev(mask))
        want += soft.histogram(rec, shifts, fail)
        assert np.array_equal(st.result(), want), "after B = %d" % B
    assert want[:, 0].sum(axis=1).tolist() == [265] * 6
    # no mask: plane 1 stays as it was -- zeros, and garbage
    rec = np.stack([_edge_values(s)[:17] for s in shifts], axis=1)
    for fill in (0, 12345):
        hist = torch.full((6, 2, 1024), fill, dtype=torch.int64, device="cuda")
        soft_tally(_dev(rec), shifts, None, hist)
        got = hist.cpu().numpy()
        assert (got[:, 1] == fill).all(), "plane 1 was touched without a mask"
        assert np.array_equal(got[:, 0] - fill, soft.histogram(rec, shifts)[:, 0])
    # rows of eight int64: the spare columns are not read as fields
    wide = np.full((17, 8), 7 << 50, dtype=np.int64)
    wide[:, :6] = rec
    hist = torch.zeros((6, 2, 1024), dtype=torch.int64, device="cuda")
    soft_tally(_dev(wide), shifts, None, hist)
    assert np.array_equal(hist.cpu().numpy(), soft.histogram(rec, shifts))
    with pytest.raises(ValueError):
        SoftTally((0, 0, 0, 0, 0, 63))


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model():
    from quits_amd.dem import Circuit
    cd = helpers.code("bb72")
    H, L, pri = helpers.dem_matrices(BB72)
    return Circuit(helpers.circuit_text(BB72)), cd, H, L, np.asarray(pri, np.float64), H.shape[0] // cd["hz"].shape[0] - 2


@functools.lru_cache(maxsize=None)
def _shots(B=512, seed=1):
    from quits_amd.decoder.device import DemSampler
    circ, cd, H, L, pri, R = _model()
    det, obs = DemSampler(H, L, pri).sample(B, seed)
    return det.cpu().numpy(), obs.cpu().numpy()


def _statuses(plan, det):
    """(window, status words on the host) pairs of plan.decode(stats=...)."""
    import torch
    with plan.in_use():
        stats = []
        pred = plan.decode(_dev(det), stats)
        torch.cuda.synchronize()
        return pred.cpu().numpy().astype(np.int64), [(k, st.cpu().numpy()) for k, st in stats]


def _check_against_mirror(plan, det, pred, rec, packed, pred_wrapper, pri):
    n = len(pri)
    assert rec.dtype == np.int64 and rec.shape == (len(det), 6) and packed.num_bits == n
    pred_s, statuses = _statuses(plan, det)
    want = soft.soft_mirror(packed, det, statuses, soft.fault_weights(pri))
    bad = np.flatnonzero((rec != want).any(axis=1))
    assert bad.size == 0, "soft records differ from the mirror on shots %s: %s vs %s" % (bad[:5], rec[bad[:5]], want[bad[:5]])
    assert np.array_equal(pred, pred_wrapper) and np.array_equal(pred_s, pred_wrapper), "predictions differ from the wrapper's"
    assert np.array_equal(plan.commit_weights().cpu().numpy(), soft.fault_weights(pri)), "the plan's weights are not the model's"
    return want


def test_soft_outputs_bposd_equal_the_mirror(gpu):
    from quits_amd.decoder import BpOsdDecoder, sliding_window_bposd_circuit_mem, sliding_window_corrections, sliding_window_soft_outputs
    from quits_amd.decoder.plan import cached_circuit_plan
    circ, cd, H, L, pri, R = _model()
    det, obs = _shots()
    assert H.shape == (288, 2592) and R == 6
    pred, rec = sliding_window_soft_outputs(det, circ, cd["hz"], cd["lz"], 3, 1, **MINSUM)
    pred_c, packed = sliding_window_corrections(det, circ, cd["hz"], cd["lz"], 3, 1, **MINSUM)
    opts = {'bp_method': "minimum_sum", 'max_iter': 20, 'schedule': "parallel", 'osd_method': "osd_0", 'osd_order': 0}
    plan = cached_circuit_plan(circ, cd["hz"], 3, 1, R, BpOsdDecoder, BpOsdDecoder, dict(opts), dict(opts))
    assert len(plan.windows) == 6 and plan.nfaults == 2592
    want = _check_against_mirror(plan, det, pred, rec, packed, sliding_window_bposd_circuit_mem(det, circ, cd["hz"], cd["lz"], 3, 1, **MINSUM), pri)
    assert np.array_equal(pred_c, pred)
    assert want[:, 4].any() and want[:, 5].any()                                         # post-processed windows, and their pivots
    assert (want[:, 3] <= 6 * 20).all() and (want[:, 4] <= 6).all() and (want[:, 0] > 0)[want[:, 1] > 0].all()
    # three values on request, the third being the corrections
    p3, r3, c3 = sliding_window_soft_outputs(det[:70], circ, cd["hz"], cd["lz"], 3, 1, corrections=True, **MINSUM)
    assert np.array_equal(p3, pred[:70]) and np.array_equal(r3, rec[:70]) and np.array_equal(np.asarray(c3), np.asarray(packed)[:70])


def test_soft_outputs_bplsd_equal_the_mirror(gpu):
    from quits_amd.decoder import BpLsdDecoder, sliding_window_bplsd_circuit_mem, sliding_window_corrections, sliding_window_soft_outputs
    from quits_amd.decoder.plan import cached_circuit_plan
    circ, cd, H, L, pri, R = _model()
    det, obs = _shots()
    kw = dict(bp_method="minimum_sum", schedule="parallel", max_iter=20, lsd_method="lsd_0")
    pred, rec = sliding_window_soft_outputs(det, circ, cd["hz"], cd["lz"], 3, 1, **kw)
    pred_c, packed = sliding_window_corrections(det, circ, cd["hz"], cd["lz"], 3, 1, **kw)
    opts = {'bp_method': "minimum_sum", 'max_iter': 20, 'schedule': "parallel", 'lsd_method': "lsd_0", 'lsd_order': 0}
    plan = cached_circuit_plan(circ, cd["hz"], 3, 1, R, BpLsdDecoder, BpLsdDecoder, dict(opts), dict(opts))
    want = _check_against_mirror(plan, det, pred, rec, packed,
                                 sliding_window_bplsd_circuit_mem(det, circ, cd["hz"], cd["lz"], 3, 1, lsd_order=0, **kw), pri)
    assert np.array_equal(pred_c, pred) and want[:, 4].any()


def test_soft_outputs_relay_equal_the_mirror(gpu):
    from quits_amd.decoder import RelayBpDecoder, sliding_window_relaybp_circuit_mem
    from quits_amd.decoder.plan import cached_circuit_plan
    from quits_amd.decoder.relaybp import relay_options
    from quits_amd.decoder.soft_outputs import plan_soft_outputs
    from quits_amd.relay import RelayConfig
    circ, cd, H, L, pri, R = _model()
    det, obs = _shots()
    cfg = RelayConfig(**SMALL)
    pred_w = sliding_window_relaybp_circuit_mem(det, circ, cd["hz"], cd["lz"], 3, 1, relay=cfg)
    opts = relay_options(cfg, "osd_off", 0)
    from quits_amd.decoder.plan_cache import plan_cache_info
    hits = plan_cache_info()["hits"]
    plan = cached_circuit_plan(circ, cd["hz"], 3, 1, R, RelayBpDecoder, RelayBpDecoder, dict(opts), dict(opts))
    assert plan_cache_info()["hits"] == hits + 1, "the test's plan is not the wrapper's cached plan"
    pred, rec, packed = plan_soft_outputs(plan, det, corrections=True)
    want = _check_against_mirror(plan, det, pred, rec, packed, pred_w, pri)
    assert (want[:, 4] == 0).all(), "osd_off: no window is post-processed"
    assert (want[:, 3] <= 6 * cfg.total_iter).all() and (want[:, 5] <= 6 * cfg.num_sets).all()
    print("relay: %d of %d shots with a leg past the first, mean iterations %.1f" % ((want[:, 5] > 0).sum(), len(want), want[:, 3].mean()))


def test_decode_dem_soft_outputs_one_window(gpu):
    from quits_amd.decoder import decode_dem, decode_dem_corrections, decode_dem_soft_outputs
    circ, cd, H, L, pri, R = _model()
    det = _shots()[0][:128]
    pred, rec = decode_dem_soft_outputs(circ, det, **MINSUM)
    pred_c, packed = decode_dem_corrections(circ, det, **MINSUM)
    assert np.array_equal(pred, decode_dem(circ, det, **MINSUM)) and np.array_equal(pred, pred_c)
    want = soft.soft_mirror(packed, det, [], soft.fault_weights(pri))
    assert np.array_equal(rec[:, :3], want[:, :3])
    assert (rec[:, 3] <= 20).all() and (rec[:, 4] <= 1).all()
    p0, r0 = decode_dem_soft_outputs(circ, det[:0], **MINSUM)
    assert p0.shape == (0, 12) and r0.shape == (0, 6) and r0.dtype == np.int64


def test_predict_writes_soft_records(gpu, tmp_path):
    """python -m quits_amd predict --soft_out: six decimal integers per shot, decode_dem_soft_outputs' records; predictions and corrections
    as without it."""
    from quits_amd.__main__ import main
    from quits_amd.decoder import decode_dem_soft_outputs
    from quits_amd.samples import write_shots
    circ, cd, H, L, pri, R = _model()
    det = _shots()[0][:64]
    (tmp_path / "c.stim").write_text(str(circ))
    write_shots(str(tmp_path / "s.b8"), det, "b8")
    base = ["predict", "--circuit", str(tmp_path / "c.stim"), "--in", str(tmp_path / "s.b8"), "--in_format", "b8", "--out_format", "01",
            "--bp_method", "minimum_sum", "--schedule", "parallel", "--max_iter", "20", "--osd_method", "osd_0"]
    assert main(base + ["--out", str(tmp_path / "p0.01"), "--corrections_out", str(tmp_path / "c0.b8")]) == 0
    assert main(base + ["--out", str(tmp_path / "p1.01"), "--soft_out", str(tmp_path / "s1.txt")]) == 0
    assert main(base + ["--out", str(tmp_path / "p2.01"), "--soft_out", str(tmp_path / "s2.txt"), "--corrections_out", str(tmp_path / "c2.b8")]) == 0
    assert (tmp_path / "p0.01").read_text() == (tmp_path / "p1.01").read_text() == (tmp_path / "p2.01").read_text()
    assert (tmp_path / "c0.b8").read_bytes() == (tmp_path / "c2.b8").read_bytes()
    pred, rec = decode_dem_soft_outputs(circ, det, **MINSUM)
    text = (tmp_path / "s1.txt").read_text()
    assert text == (tmp_path / "s2.txt").read_text()
    assert np.array_equal(np.array([[int(v) for v in line.split()] for line in text.splitlines()], dtype=np.int64), rec)
    sw = ["--checks_per_round", str(cd["hz"].shape[0]), "--window", "3", "--commit", "1"]
    assert main(base + sw + ["--out", str(tmp_path / "p3.01"), "--soft_out", str(tmp_path / "s3.txt")]) == 0
    assert len((tmp_path / "s3.txt").read_text().splitlines()) == 64


# ---- 5. both drivers -------------------------------------------------------------------------------------------------------------------
def test_pipelined_driver_equals_the_single_stream_one(gpu):
    """Three chunks (of 64 shots) and a ragged fourth through plan.decode(det, stats, correction, soft), `plan.pipeline` on and off: the same
    records, corrections, predictions and status words.  The records come pre-filled: the call zero-fills them."""
    import torch
    from quits_amd.decoder import BpOsdDecoder
    from quits_amd.decoder.plan import cached_circuit_plan
    circ, cd, H, L, pri, R = _model()
    opts = {'bp_method': "minimum_sum", 'max_iter': 20, 'schedule': "parallel", 'osd_method': "osd_0", 'osd_order': 0}
    plan = cached_circuit_plan(circ, cd["hz"], 3, 1, R, BpOsdDecoder, BpOsdDecoder, dict(opts), dict(opts))
    words = (plan.nfaults + 31) // 32
    saved = plan.chunk, plan.pipeline
    out = {}
    try:
        for N in (3 * 64, 3 * 64 + 20):
            det = _dev(_shots()[0][:N])
            for pipelined in (False, True):
                plan.chunk, plan.pipeline = 64, pipelined
                with plan.in_use():
                    corr = torch.full((N, words), 0x33333333, dtype=torch.int32, device="cuda")
                    rec = torch.full((N, 6), SENTINEL, dtype=torch.int64, device="cuda")
                    stats = []
                    pred = plan.decode(det, stats, corr, rec)
                    torch.cuda.synchronize()
                    out[N, pipelined] = (pred.cpu().numpy(), corr.cpu().numpy(), rec.cpu().numpy(), [(k, st.cpu().numpy()) for k, st in stats])
                    with pytest.raises(ValueError, match="correction"):
                        plan.decode(det, None, None, rec)
                    with pytest.raises(ValueError):
                        plan.decode(det, None, corr, rec[:, :5])
            s, p = out[N, False], out[N, True]
            assert np.array_equal(s[0], p[0]) and np.array_equal(s[1], p[1]), "predictions or corrections differ between the drivers"
            assert np.array_equal(s[2], p[2]), "soft records differ between the drivers"
            want = soft.soft_mirror(_unpack(s[1], plan.nfaults), det.cpu().numpy(), p[3], soft.fault_weights(pri))
            assert np.array_equal(p[2], want) and np.array_equal(want, soft.soft_mirror(_unpack(s[1], plan.nfaults), det.cpu().numpy(), s[3],
                                                                                      soft.fault_weights(pri)))
    finally:
        plan.chunk, plan.pipeline = saved


# ---- 6. the experiment -----------------------------------------------------------------------------------------------------------------
def test_postselected_pL_equals_the_memory_experiment_and_the_replayed_records(gpu):
    """4096 DEM-sampled shots of seed 1.  The CPU oracle fails on 508 of them (and on 60 of the shots whose event count is at most the 0.33
    quantile), so: at least 100 failing shots, and the `events` curve at about one-third acceptance lies below the whole set's pL.  No
    finer shape is asserted."""
    from quits_amd.decoder import sliding_window_soft_outputs
    from quits_amd.simulation import get_circuit_mem_pL, get_postselected_pL, replay_shots
    circ, cd, H, L, pri, R = _model()
    N = 4096
    res = get_postselected_pL(circ, cd["hz"], cd["lz"], 3, 1, N, sampler="dem", seed=1, **MINSUM)
    ref = get_circuit_mem_pL(circ, cd["hz"], cd["lz"], 3, 1, N, sampler="dem", seed=1, **MINSUM)
    print("postselected: %d shots, %d errors; the memory experiment: %d, %d" % (res.shots, res.errors, ref.shots, ref.errors))
    assert (res.shots, res.errors) == (ref.shots, ref.errors) == (N, ref.errors) and res.pL == ref.pL and res.sigma == ref.sigma
    assert res.errors >= 100
    assert res.hist.shape == (6, 2, 1024) and res.hist.dtype == np.int64
    assert (res.hist[:, 0].sum(axis=1) == res.shots).all() and (res.hist[:, 1].sum(axis=1) == res.errors).all()
    for f in soft.FIELDS:
        edge, kept, errors, pL, sigma = res.curve(f)
        assert (kept[-1], errors[-1]) == (res.shots, res.errors) and kept.dtype == np.int64 and len(edge) == 1024
    det, obs = replay_shots(circ, np.arange(N), 1, sampler="dem")
    pred, rec = sliding_window_soft_outputs(det, circ, cd["hz"], cd["lz"], 3, 1, **MINSUM)
    fail = (pred != obs).any(axis=1)
    assert fail.sum() == res.errors and np.array_equal(np.flatnonzero(fail), ref.failing_shots)
    assert np.array_equal(res.hist, soft.histogram(rec, res.shifts, fail)), "the device histogram is not bin_of of the replayed records"
    assert np.array_equal(res.shifts, soft.default_shifts(soft.fault_weights(pri), pri, 288, 6, 20))
    third = res.at_rejection("events", 2.0 / 3.0)
    print("events <= %s: %d kept, %d errors, pL %.4f (all: %.4f)" % (third["threshold"], third["kept"], third["errors"], third["pL"], res.pL))
    assert third["kept"] > 0 and third["rejected"] >= 2.0 / 3.0 and third["pL"] < res.pL
    # explicit shifts are used as given; the relay decoder goes through the same loop
    res2 = get_postselected_pL(circ, cd["hz"], cd["lz"], 3, 1, 256, sampler="dem", seed=1, shifts=[20, 0, 0, 0, 0, 0], batch=100, **MINSUM)
    assert res2.shifts.tolist() == [20, 0, 0, 0, 0, 0] and res2.shots == 256 and res2.batch == 128
    assert np.array_equal(res2.hist, soft.histogram(rec[:256], res2.shifts, fail[:256]))


def test_postselected_pL_with_relay(gpu):
    from quits_amd.relay import RelayConfig
    from quits_amd.simulation import get_postselected_pL, get_relay_mem_pL
    circ, cd, H, L, pri, R = _model()
    cfg = RelayConfig(**SMALL)
    res = get_postselected_pL(circ, cd["hz"], cd["lz"], 3, 1, 1024, relay=cfg, sampler="dem", seed=1)
    ref = get_relay_mem_pL(circ, cd["hz"], cd["lz"], 3, 1, 1024, relay=cfg, sampler="dem", seed=1)
    assert (res.shots, res.errors) == (ref.shots, ref.errors) and res.shots == 1024
    assert (res.hist[:, 0].sum(axis=1) == 1024).all() and (res.hist[:, 1].sum(axis=1) == res.errors).all()
    assert res.hist[4, 0, 0] == 1024, "osd_off: no window is post-processed"
    assert np.array_equal(res.shifts, soft.default_shifts(soft.fault_weights(pri), pri, 288, 6, cfg.total_iter))
