"""The counting pass of the prior fit on the device (csrc/calibrate.hip) against the numpy mirror (quits_amd.calibrate): the bit planes at the
word edges, every counter on a crafted model with columns of every weight and on two circuit models, one result whatever form the samples
come in, the refusals and the command line."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from quits_amd import calibrate as qc
from test_calibrate import crafted_70, from_columns, model, z_conditions

pytestmark = pytest.mark.gpu


def device_planes(det, fill=-1):
    """qd_bit_planes of a cuda uint8 tensor (any row stride) into planes of one spare word, pre-filled: (planes [ndet, W], spare column)."""
    import torch
    from quits_amd import _lib
    from quits_amd.samples import _stream_ptr
    L = _lib.require_calibrate(_lib.require_gpu())
    B, ndet = det.shape
    W = (B + 63) // 64
    out = torch.full((ndet, W + 1), fill, dtype=torch.int64, device="cuda")
    _lib.check(L.qd_bit_planes(ctypes.c_void_p(det.data_ptr()), det.stride(0), ndet, B, ctypes.c_void_p(out.data_ptr()), W + 1, _stream_ptr()))
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint64)
    return host[:, :W], host[:, W]


@pytest.mark.parametrize("ndet", [1, 9, 70])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_planes(gpu, B, ndet):
    import torch
    rng = np.random.default_rng(1000 * B + ndet)
    bits = rng.random((B, ndet)) < 0.5
    for raw in (bits.astype(np.uint8), bits.astype(np.uint8) + 2):         # the second input holds bytes 2 and 3: the low bit counts
        wide = torch.full((B, ndet + 3), 1, dtype=torch.uint8, device="cuda")          # row stride ndet + 3; the bytes between rows are ones
        wide[:, :ndet] = torch.from_numpy(raw).to("cuda")
        planes, spare = device_planes(wide[:, :ndet])
        assert np.array_equal(planes, qc.bit_planes_mirror(bits))
        assert (spare == np.uint64(0xFFFFFFFFFFFFFFFF)).all()               # the word past the last one is not touched
        if B % 64:
            assert not (planes[:, -1] >> np.uint64(B % 64)).any()           # pad bits of the last word


def test_counts_on_the_crafted_model(gpu):
    import torch
    H, L = crafted_70()
    table = qc.hyperedge_table(H, L)
    assert sorted(set(table.weight.tolist())) == list(range(1, 11)) and table.total == int(((1 << table.weight) - 1).sum())
    rng = np.random.default_rng(70)
    first, second = rng.random((229, 70)) < 0.3, rng.random((64, 70)) < 0.3
    counter = qc.ParityCounter(table)
    try:
        assert counter.tasks == sum(1 << max(0, int(w) - 6) for w in table.weight)
        row = torch.zeros(table.total, dtype=torch.int64, device="cuda")
        counter.add(torch.from_numpy(first.view(np.uint8)).to("cuda"), row)
        ref1 = qc.parity_counts_mirror(first, table, blocks=1)[0][0]
        assert np.array_equal(row.cpu().numpy(), ref1)
        counter.add(torch.from_numpy(second.view(np.uint8)).to("cuda"), row)       # a second call goes into the same row
        ref2 = ref1 + qc.parity_counts_mirror(second, table, blocks=1)[0][0]
        assert np.array_equal(row.cpu().numpy(), ref2)
        counter.add(torch.zeros((0, 70), dtype=torch.uint8, device="cuda"), row)    # no shots: nothing changes
        assert np.array_equal(row.cpu().numpy(), ref2)
        assert np.array_equal(ref2, qc.parity_counts_mirror(np.concatenate([first, second]), table, blocks=1)[0][0])
    finally:
        counter.close()


def test_bb72_r6_counts_and_jackknife(gpu):
    from quits_amd.decoder.device import DemSampler
    H, L, p = model("bb72_custom_r6_p0.003")
    res = qc.estimate_priors((H, L, p), shots=1 << 18, seed=1, sampler="dem", blocks=16)
    det = DemSampler(H, L, p).sample(1 << 18, 1)[0].cpu().numpy()
    ref, shots = qc.parity_counts_mirror(det, res.table, blocks=16)
    assert res.shots == 1 << 18 and np.array_equal(res.block_shots, shots) and np.array_equal(res.counts, ref)
    z_conditions(res, p)


def test_alldet_counts(gpu):
    """216 x 5400, column weights 1 .. 9: the columns of several wavefronts on a real model."""
    from quits_amd.decoder.device import DemSampler
    H, L, p = model("bb72_custom_r2_alldet_p0.003")
    res = qc.estimate_priors((H, L, p), shots=1 << 16, seed=1, blocks=16)
    assert res.table.weight.max() == 9 and res.table.total == 544320
    det = DemSampler(H, L, p).sample(1 << 16, 1)[0].cpu().numpy()
    assert np.array_equal(res.counts, qc.parity_counts_mirror(det, res.table, blocks=16)[0])


def test_one_result_whatever_the_input_form(gpu):
    import torch
    from quits_amd.decoder.device import DemSampler
    from quits_amd.samples import PackedSamples
    H, L, p = model("bb72_custom_r6_p0.003")
    dev = DemSampler(H, L, p).sample(20000, 7)[0]
    host = dev.cpu().numpy()
    ref = qc.estimate_priors((H, L, p), dev).counts
    assert ref.shape[0] == 16 and ref.any()
    assert np.array_equal(qc.estimate_priors((H, L, p), host.astype(bool)).counts, ref)
    assert np.array_equal(qc.estimate_priors((H, L, p), PackedSamples.pack(host)).counts, ref)
    assert np.array_equal(qc.estimate_priors((H, L, p), PackedSamples.pack(dev)).counts, ref)
    rng = np.random.default_rng(9)
    wider = np.concatenate([rng.integers(0, 2, (20000, 5), dtype=np.uint8), host, rng.integers(0, 2, (20000, 12), dtype=np.uint8)], axis=1)
    assert np.array_equal(qc.estimate_priors((H, L, p), PackedSamples.pack(wider).field(5, 288)).counts, ref)
    assert np.array_equal(qc.estimate_priors((H, L, p), PackedSamples.pack(torch.from_numpy(wider).to("cuda")).field(5, 288)).counts, ref)
    assert np.array_equal(qc.estimate_priors((H, L, p), dev, batch=4096).counts, ref)
    assert np.array_equal(qc.estimate_priors((H, L, p), dev, batch=1000).counts, ref)
    assert np.array_equal(ref, qc.parity_counts_mirror(host, qc.hyperedge_table(H, L), blocks=16)[0])


def test_refusals_before_any_launch(gpu):
    H, L, p = model("bb72_custom_r6_p0.003")
    H11, L11 = from_columns([[0], list(range(11))], 12)
    with pytest.raises(NotImplementedError, match="column 1 has weight 11"):
        qc.estimate_priors((H11, L11, np.array([0.1, 0.1])), np.zeros((8, 12), np.uint8))
    with pytest.raises(ValueError, match="287 detectors wide, the model has 288"):
        qc.estimate_priors((H, L, p), np.zeros((8, 287), np.uint8))
    with pytest.raises(ValueError, match="no shots"):
        qc.estimate_priors((H, L, p), np.zeros((0, 288), np.uint8))
    with pytest.raises(ValueError, match="no shots"):
        qc.estimate_priors((H, L, p), shots=0)


def test_command_line(gpu, tmp_path):
    from quits_amd.decoder.base import detector_error_model_to_matrix
    from quits_amd.decoder.device import DemSampler
    from quits_amd.dem import Circuit, dem_to_text, parse_dem
    from quits_amd.samples import write_shots
    name = "bb72_custom_r6_p0.003"
    H, L, p = model(name)
    (tmp_path / "m.dem").write_text(dem_to_text(Circuit(helpers.circuit_text(name)).detector_error_model()))
    det = DemSampler(H, L, p).sample(1 << 15, 3)[0]
    write_shots(str(tmp_path / "s.b8"), det, "b8")
    out = subprocess.run([sys.executable, "-m", "quits_amd", "calibrate", "--dem", str(tmp_path / "m.dem"), "--in", str(tmp_path / "s.b8"), "--in_format", "b8",
                          "--out", str(tmp_path / "f.dem")], capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(helpers.GOLD)))
    assert out.returncode == 0, out.stderr[-2000:]
    info = json.loads(out.stdout)
    assert info["shots"] == 1 << 15 and info["columns"] == 2592
    res = qc.estimate_priors((tmp_path / "m.dem").read_text(), det)
    assert info["clipped"] == len(res.clipped) and info["unidentified"] == len(res.unidentified)
    H2, L2, p2 = detector_error_model_to_matrix(parse_dem((tmp_path / "f.dem").read_text()))
    assert helpers.same_sparse(H, H2) and helpers.same_sparse(L, L2) and np.array_equal(p2, res.priors)
