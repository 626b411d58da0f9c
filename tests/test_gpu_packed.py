"""Bit-packed samples on the GPU: qd_unpack_b8 / qd_pack_b8 (csrc/bitpack.hip) against numpy, at offsets beyond 2^32, and PackedSamples /
DEM text through every entry point that takes samples or a circuit; decode_dem; the samplers' packed output; the command line."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBITS = (1, 7, 8, 9, 64, 65, 1008, 1009)
BIT0 = (0, 3, 8, 13)
SHOTS = (1, 65, 1000)
KW = dict(max_iter=20, osd_order=0, bp_method="minimum_sum", schedule="parallel", osd_method="osd_0")


def test_unpack_against_numpy(gpu):
    """Every width / bit offset / batch / row padding: inside the output's column slice the bits numpy unpacks, outside it nothing written."""
    import torch
    from quits_amd.samples import unpack_b8_into
    rng = np.random.default_rng(11)
    for nbits in NBITS:
        for bit0 in BIT0:
            need = (bit0 + nbits + 7) // 8
            for B in SHOTS:
                for pad in (0, 3):
                    packed = rng.integers(0, 256, (B, need + pad), dtype=np.uint8)
                    want = np.unpackbits(packed, axis=1, bitorder="little")[:, bit0:bit0 + nbits]
                    wide = torch.full((B, nbits + 11), 0xAA, dtype=torch.uint8, device=gpu)
                    unpack_b8_into(torch.from_numpy(packed).to(gpu), bit0, nbits, wide[:, 5:5 + nbits])
                    got = wide.cpu().numpy()
                    case = (nbits, bit0, B, pad)
                    assert np.array_equal(got[:, 5:5 + nbits], want), case
                    assert (got[:, :5] == 0xAA).all() and (got[:, 5 + nbits:] == 0xAA).all(), case


def test_pack_against_numpy(gpu):
    """The low bit of every input byte counts; padding bits of the last byte are zero; bytes of a row past ceil(nbits / 8) are not touched.
    Same shapes as the unpack test: the input is a column slice at offset bit0 of a wider array, so its rows start at every alignment."""
    import torch
    from quits_amd.samples import pack_b8_into
    rng = np.random.default_rng(12)
    values = np.array([0, 1, 2, 3, 255], np.uint8)
    for nbits in NBITS:
        nb = (nbits + 7) // 8
        for off in BIT0:
            for B in SHOTS:
                for pad in (0, 3):
                    src = values[rng.integers(0, 5, (B, off + nbits + pad))]
                    want = np.packbits(src[:, off:off + nbits] & 1, axis=1, bitorder="little")
                    packed = torch.full((B, nb + pad), 0x55, dtype=torch.uint8, device=gpu)
                    pack_b8_into(torch.from_numpy(src).to(gpu)[:, off:off + nbits], packed[:, :nb] if pad == 0 else packed)
                    got = packed.cpu().numpy()
                    case = (nbits, off, B, pad)
                    assert np.array_equal(got[:, :nb], want), case
                    if nbits % 8:
                        assert not (got[:, nb - 1] >> (nbits % 8)).any(), case
                    assert (got[:, nb:] == 0x55).all(), case


def test_offsets_beyond_4_gib(gpu):
    """2^22 + 1 rows of 1024 bytes: the last row starts at byte 2^32 of both buffers.  Unpack 16 bits per row, then pack them back."""
    import torch
    from quits_amd.samples import pack_b8_into, unpack_b8_into
    B, stride, nbits = (1 << 22) + 1, 1024, 16
    rows = [0, 1 << 21, 1 << 22]
    pat = torch.tensor([[0xA5, 0x0F], [0x3C, 0x81], [0xFF, 0x42]], dtype=torch.uint8, device=gpu)
    packed = torch.empty((B, stride), dtype=torch.uint8, device=gpu)         # two 4 GiB buffers, mostly untouched
    out = torch.empty((B, stride), dtype=torch.uint8, device=gpu)
    for r, p in zip(rows, pat):
        packed[r, :2] = p
        packed[r, 2:8] = 0x77
    sentinel = (1 << 21) + 1
    out[sentinel, nbits:64] = 0xAA
    out[rows[2], nbits:64] = 0xAA
    unpack_b8_into(packed, 0, nbits, out[:, :nbits])
    want = torch.from_numpy(np.unpackbits(pat.cpu().numpy(), axis=1, bitorder="little")).to(gpu)
    assert torch.equal(out[rows, :nbits], want)
    assert bool((out[sentinel, nbits:64] == 0xAA).all()) and bool((out[rows[2], nbits:64] == 0xAA).all())
    for r in rows:
        packed[r, :2] = 0
    pack_b8_into(out[:, :nbits], packed)
    assert torch.equal(packed[rows, :2], pat)
    assert bool((packed[rows, 2:8] == 0x77).all())
    del packed, out
    torch.cuda.empty_cache()


def _model(name):
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.dem import Circuit
    circ = Circuit(helpers.circuit_text(name))
    return circ, detector_error_model_to_matrix(circ)


@pytest.mark.parametrize("name,code,W,F", [("bb72_custom_r6_p0.003", "bb72", 3, 1), ("hgp225_cardinal_r3_p0.01", "hgp225", 6, 1)],
                         ids=["bb72-W3F1", "hgp225-one-window"])
def test_packed_and_dem_text_through_the_api(gpu, name, code, W, F, monkeypatch):
    """288 detectors (36 bytes) in W = 3 / F = 1 windows, 540 detectors (68 bytes, 4 padding bits) as one window: packed samples from the
    host and from the device, and DEM text in the circuit's place, give the bool array's predictions; so do several staged pieces."""
    import torch
    from quits_amd.decoder import plan_cache, sliding_window_bposd_circuit_mem
    from quits_amd.decoder import sliding_window as sw
    from quits_amd.decoder.device import DemSampler
    from quits_amd.dem import dem_to_text
    from quits_amd.samples import PackedSamples
    circ, (H, L, pri) = _model(name)
    cd = helpers.code(code)
    hz, lz = cd["hz"], cd["lz"]
    det, _ = DemSampler(H, L, pri).sample(3001, seed=77)
    det_h = det.cpu().numpy().astype(bool)
    sw.plan_cache_clear()
    monkeypatch.setenv("QD_PLAN_CACHE", "4")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                # (whole-history notice for the single window)
        ref = sliding_window_bposd_circuit_mem(det_h, circ, hz, lz, W, F, **KW)
        assert ref.shape == (3001, L.shape[0]) and ref.any()
        host = PackedSamples.pack(det_h)
        assert host.data.shape == (3001, (H.shape[0] + 7) // 8) and not host.is_cuda
        a = sliding_window_bposd_circuit_mem(host, circ, hz, lz, W, F, **KW)
        assert a.dtype == np.int64 and np.array_equal(a, ref)
        dev = PackedSamples.pack(det)
        assert dev.is_cuda and np.array_equal(dev.data.cpu().numpy(), host.data)
        assert np.array_equal(sliding_window_bposd_circuit_mem(dev, circ, hz, lz, W, F, **KW), ref)
        assert sw.plan_cache_info()["misses"] == 1
        text = dem_to_text(circ.detector_error_model())
        assert np.array_equal(sliding_window_bposd_circuit_mem(det_h, text, hz, lz, W, F, **KW), ref)
        assert np.array_equal(sliding_window_bposd_circuit_mem(host, text, hz, lz, W, F, **KW), ref)
        assert sw.plan_cache_info()["misses"] == 2                  # the text is another key, and one key
    # several staged pieces, chained and not: 3001 = 1024 + 1024 + 953 in chunks of 256; a field of a wider record, at a bit offset
    plan = next(iter(plan_cache._CACHE.values()))
    plan.chunk, plan.host_piece = 256, 1024
    assert np.array_equal(plan.decode_host(host), ref)
    assert np.array_equal(plan.decode_host(host[:10]), ref[:10]) and plan.decode_host(host[:0]).shape == (0, ref.shape[1])
    rec = PackedSamples.pack(np.concatenate([np.ones((3001, 5), bool), det_h, np.ones((3001, 3), bool)], axis=1))
    assert np.array_equal(plan.decode_host(rec.field(5, H.shape[0])), ref)
    plan.pipeline = False
    assert np.array_equal(plan.decode_host(host[:2900]), ref[:2900])
    plan.pipeline = True
    assert np.array_equal(plan.decode_host(det_h), ref)             # the unpacked path after the packed one: the staging buffers are refitted
    with pytest.raises(Exception, match="exceeds the row stride"):  # a wrong width: what the unpacked path says
        plan.decode_host(PackedSamples.pack(det_h[:16, :-8]))
    with pytest.raises(Exception, match="exceeds the row stride"):
        plan.decode_host(det_h[:16, :-8])
    sw.plan_cache_clear()


def test_decode_batch_takes_packed_syndromes(gpu):
    from quits_amd.decoder import BpOsdDecoder
    from quits_amd.decoder.device import DemSampler
    from quits_amd.samples import PackedSamples
    _, (H, L, pri) = _model("bb72_custom_r6_p0.003")
    det, _ = DemSampler(H, L, pri).sample(300, seed=3)
    dec = BpOsdDecoder(H, error_channel=pri, max_iter=20, bp_method="minimum_sum", schedule="parallel", osd_method="osd_0")
    ref = dec.decode_batch(det)
    assert ref.shape == (300, H.shape[1]) and ref.dtype == np.uint8
    assert np.array_equal(dec.decode_batch(PackedSamples.pack(det)), ref)
    assert np.array_equal(dec.decode_batch(PackedSamples.pack(det.cpu().numpy())), ref)
    with pytest.raises(ValueError, match=r"syndromes must have shape \[B, 288\]"):
        dec.decode_batch(PackedSamples.pack(det[:, :280]))


@pytest.mark.parametrize("opts", [dict(KW), {}, dict(lsd_method="lsd_cs", lsd_order=1)], ids=["minsum-osd0", "wrapper-defaults", "lsd_cs-1"])
def test_decode_dem_is_the_whole_history_window(gpu, opts):
    from quits_amd.decoder import decode_dem, sliding_window_bplsd_circuit_mem, sliding_window_bposd_circuit_mem
    from quits_amd.decoder import sliding_window as sw
    from quits_amd.decoder.device import DemSampler
    from quits_amd.dem import dem_to_text
    from quits_amd.samples import PackedSamples
    name = "bb72_custom_r6_p0.003"
    circ, (H, L, pri) = _model(name)
    cd = helpers.code("bb72")
    det, _ = DemSampler(H, L, pri).sample(512, seed=9)
    det_h = det.cpu().numpy()
    sw.plan_cache_clear()
    wrapper = sliding_window_bplsd_circuit_mem if "lsd_method" in opts else sliding_window_bposd_circuit_mem
    with pytest.warns(UserWarning, match="whole history"):
        ref = wrapper(det_h, circ, cd["hz"], cd["lz"], 9, 1, **opts)
    got = decode_dem(circ, det_h, **opts)
    assert got.dtype == np.int64 and got.shape == (512, 12) and np.array_equal(got, ref)
    text = dem_to_text(circ.detector_error_model())
    assert np.array_equal(decode_dem(text, PackedSamples.pack(det_h), **opts), ref)
    assert np.array_equal(decode_dem(circ.detector_error_model(), PackedSamples.pack(det), **opts), ref)
    assert decode_dem(text, det_h[:0], **opts).shape == (0, 12)
    with pytest.raises(ValueError, match="288"):
        decode_dem(text, det_h[:, :280], **opts)
    sw.plan_cache_clear()


def test_samplers_pack_on_the_device(gpu):
    import torch
    from quits_amd.decoder.device import CircuitSampler, DemSampler
    from quits_amd.samples import PackedSamples
    circ, (H, L, pri) = _model("bb72_custom_r6_p0.003")
    for sampler in (DemSampler(H, L, pri), CircuitSampler(circ)):
        det, obs = sampler.sample(1000, 2026, 77)
        pdet, pobs = sampler.sample_packed(1000, 2026, shot0=77)
        assert pdet.is_cuda and pobs.is_cuda and pdet.shape == (1000, 288) and pobs.shape == (1000, 12)
        assert pdet.data.shape == (1000, 36) and pobs.data.shape == (1000, 2)
        assert np.array_equal(pdet.data.cpu().numpy(), PackedSamples.pack(det.cpu().numpy()).data)
        assert np.array_equal(pobs.data.cpu().numpy(), PackedSamples.pack(obs.cpu().numpy()).data)
        assert torch.equal(pdet.unpack(), det) and torch.equal(pobs.unpack(), obs)
        assert det.any() and obs.any()


def test_cli_predict(gpu, tmp_path, capsys):
    """`python -m quits_amd predict` as a fresh process: whole history and sliding windows, b8 in, every format out, --obs_in tallies."""
    from quits_amd.decoder import decode_dem, sliding_window_bposd_circuit_mem
    from quits_amd.decoder.device import DemSampler
    from quits_amd.dem import dem_to_text
    from quits_amd.samples import read_shots, write_shots
    name = "bb72_custom_r6_p0.003"
    circ, (H, L, pri) = _model(name)
    cd = helpers.code("bb72")
    det, obs = DemSampler(H, L, pri).sample(700, seed=4)
    det_h, obs_h = det.cpu().numpy(), obs.cpu().numpy()
    dem, shots, obs_file = str(tmp_path / "m.dem"), str(tmp_path / "s.b8"), str(tmp_path / "o.01")
    open(dem, "w").write(dem_to_text(circ.detector_error_model()))
    write_shots(shots, det_h, "b8")
    write_shots(obs_file, obs_h, "01")
    opts = ["--bp_method", "minimum_sum", "--schedule", "parallel", "--max_iter", "20", "--osd_method", "osd_0", "--osd_order", "0"]
    want_whole = decode_dem(circ, det_h, **KW)
    want_win = sliding_window_bposd_circuit_mem(det_h, circ, cd["hz"], cd["lz"], 3, 1, **KW)
    for tag, extra, want, fmt in (("whole", [], want_whole, "dets"), ("win", ["--checks_per_round", "36", "--window", "3", "--commit", "1"], want_win, "b8")):
        out = str(tmp_path / (tag + "." + fmt))
        run = subprocess.run([sys.executable, "-m", "quits_amd", "predict", "--dem", dem, "--in", shots, "--in_format", "b8", "--out", out,
                              "--out_format", fmt, "--obs_in", obs_file, "--obs_in_format", "01"] + opts + extra,
                             capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        assert np.array_equal(np.asarray(read_shots(out, fmt, 0, 12)), want), tag
        assert json.loads(run.stdout.strip().split("\n")[-1]) == {"shots": 700, "errors": int((want != obs_h).any(axis=1).sum())}, tag
    # the circuit in the model's place, observables appended to the samples
    rec, cfile, out = str(tmp_path / "rec.hits"), str(tmp_path / "c.stim"), str(tmp_path / "c.01")
    write_shots(rec, np.concatenate([det_h, obs_h], axis=1), "hits")
    open(cfile, "w").write(str(circ))
    from quits_amd.__main__ import main                   # (in this process: the child processes above are what starts fresh)
    capsys.readouterr()
    assert main(["predict", "--circuit", cfile, "--in", rec, "--in_format", "hits", "--in_includes_appended_observables", "--out", out,
                 "--out_format", "01"] + opts) == 0
    assert np.array_equal(np.asarray(read_shots(out, "01", 0, 12)), want_whole)
    assert json.loads(capsys.readouterr().out.strip().split("\n")[-1]) == {"shots": 700, "errors": int((want_whole != obs_h).any(axis=1).sum())}
