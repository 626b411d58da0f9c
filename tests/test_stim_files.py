"""Stim's files without a GPU: detector-error-model text (quits_amd.dem.parse_dem / dem_to_text / as_dem), the result formats b8, 01, hits
and dets (quits_amd.samples), PackedSamples on the host, the two C-ABI exports' argument checks, bitpack.hip's resource usage, the CLI."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers
from quits_amd.dem import Circuit, DemParseError, DetectorErrorModel, as_dem, dem_to_text, looks_like_dem_text, parse_dem
from quits_amd.samples import PackedSamples, ShotFileError, read_shots, write_shots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEM_TEXT = """# a hand-written model
error(0.125) D0 D1 ^ D2 L0        # '^' separators are dropped
ERROR(0.25) D0 D3 D0 L1 L1        # D0 and L1 cancel

repeat 2 {
    error(0.5) D0 L0
    shift_detectors(1, 0.5) 3
    Repeat 2 {
        error(0) D1
        shift_detectors 1
    }
    error(1e-3)
}
detector(7, 1) D2
logical_observable L2
"""
# shifts: block 1 starts at 0: D0; +3; inner D1 at 3 -> D4, +1, D1 at 4 -> D5, +1 (now 5); empty error; block 2 starts at 5: D5; +3 = 8;
# inner D9, D10, now 10; trailing detector D2 at shift 10 -> D12: 13 detectors
DEM_FLAT = [(0.125, (0, 1, 2), (0,)), (0.25, (3,), ()),
            (0.5, (0,), (0,)), (0.0, (4,), ()), (0.0, (5,), ()), (1e-3, (), ()),
            (0.5, (5,), (0,)), (0.0, (9,), ()), (0.0, (10,), ()), (1e-3, (), ())]


def test_parser_reads_the_grammar_by_hand():
    d = parse_dem(DEM_TEXT)
    assert d.errors == DEM_FLAT
    assert (d.num_detectors, d.num_observables) == (13, 3)
    assert d.structure_key is None and isinstance(d, DetectorErrorModel)
    assert parse_dem("").errors == [] and parse_dem("# nothing\n\n").num_detectors == 0
    assert parse_dem("error[tagged](0.5) D1").errors == [(0.5, (1,), ())]


@pytest.mark.parametrize("name", ["bb72_custom_r6_p0.003", "hgp225_cardinal_r3_p0.01"])
def test_text_round_trip_is_exact(name):
    d = Circuit(helpers.circuit_text(name)).detector_error_model()
    back = parse_dem(dem_to_text(d))
    assert back.errors == d.errors                                   # %.17g round-trips a double
    assert (back.num_detectors, back.num_observables) == (d.num_detectors, d.num_observables)
    assert str(d) == "\n".join(dem_to_text(d).split("\n")[:len(d.errors)])      # __str__ is what it was: the error lines alone
    # sizes survive when the last ids occur in no error
    e = DetectorErrorModel([(0.1, (0,), ())], 5, 2)
    text = dem_to_text(e, digits=3)
    assert text == "error(0.1) D0\ndetector D4\nlogical_observable L1\n"
    back = parse_dem(text)
    assert (back.errors, back.num_detectors, back.num_observables) == (e.errors, 5, 2)


@pytest.mark.parametrize("text,line,what", [
    ("error(0.1) D0\nerror(1.5) D1", 2, "probability"),
    ("error(-0.1) D0", 1, "probability"),
    ("error(nan) D0", 1, "probability"),
    ("error(0.1, 0.2) D0", 1, "probability"),
    ("error(abc) D0", 1, "bad probability"),
    ("error(0.1) D0\n\nmeasure D0", 3, "unknown instruction"),
    ("error(0.1) D0 Q3", 1, "bad target"),
    ("error(0.1) D-1", 1, "bad target"),
    ("detector L0", 1, "observable target"),
    ("logical_observable D0", 1, "detector target"),
    ("detector D0 ^ D1", 1, "'\\^'"),
    ("repeat 2 {\nerror(0.1) D0", 1, "never closed"),
    ("error(0.1) D0\n}", 2, "without a repeat"),
    ("repeat x {\n}", 1, "repeat count"),
    ("repeat 2\nerror(0.1) D0\n}", 1, "repeat N \\{"),
    ("shift_detectors 1 2", 1, "shift_detectors"),
    ("shift_detectors(1, z) 1", 1, "coordinate"),
])
def test_parser_refusals_name_the_line(text, line, what):
    with pytest.raises(DemParseError, match=r"line %d: .*%s" % (line, what)) as exc:
        parse_dem(text)
    assert isinstance(exc.value, ValueError)


def test_as_dem_takes_dem_text_and_leaves_circuits_alone(monkeypatch):
    d = as_dem(DEM_TEXT)
    assert d.errors == DEM_FLAT
    assert as_dem("  # comment first\n\n  Error(0.5) D0\n").errors == [(0.5, (0,), ())]
    assert as_dem("repeat 3 {\n  error(0.5) D0\n shift_detectors 1\n}").num_detectors == 3
    # circuit text takes the path it always took: Circuit(text).detector_error_model()
    name = "bb72_custom_r2_alldet_p0.003"
    text = helpers.circuit_text(name)
    assert not looks_like_dem_text(text)
    import quits_amd.dem as dem_mod
    calls = []
    real = dem_mod.circuit_to_dem
    monkeypatch.setattr(dem_mod, "circuit_to_dem", lambda t, a=False: calls.append(1) or real(t, a))
    monkeypatch.setattr(dem_mod, "parse_dem", lambda t: pytest.fail("circuit text went to the DEM parser"))
    got = as_dem(text)
    assert calls == [1] and got.errors == real(text).errors and got.structure_key is not None
    c = Circuit(text)
    assert as_dem(c) is c.detector_error_model()
    monkeypatch.undo()
    # a circuit's own DETECTOR / REPEAT lines do not look like a model
    assert not looks_like_dem_text("DETECTOR(1, 2) rec[-1]\n") and not looks_like_dem_text("REPEAT 2 {\n  H 0\n}\n") and not looks_like_dem_text("")
    assert looks_like_dem_text("detector(1) D0\n") and looks_like_dem_text("logical_observable L0") and looks_like_dem_text("shift_detectors 4")
    # the window slicer takes DEM text where it takes a circuit
    from quits_amd.decoder import detector_error_model_to_matrix
    H, L, pri = detector_error_model_to_matrix("error(0.25) D0 D1 L0\nerror(0.5) D1\n")
    assert H.toarray().tolist() == [[1, 0], [1, 1]] and L.toarray().tolist() == [[1, 0]] and pri.tolist() == [0.25, 0.5]


# ---- result formats ----------------------------------------------------------------------------------------------------------------------
BITS_9x2 = np.array([[1, 0, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 0, 0]], np.uint8)
BYTES = {"b8": bytes([0x01, 0x01, 0x00, 0x00]), "01": b"100000001\n000000000\n", "hits": b"0,8\n\n", "dets": b"shot D0 L0\nshot\n"}


@pytest.mark.parametrize("fmt", ["b8", "01", "hits", "dets"])
def test_formats_byte_for_byte(fmt, tmp_path):
    path = str(tmp_path / ("x." + fmt))
    write_shots(path, BITS_9x2, fmt, num_detectors=8)
    assert open(path, "rb").read() == BYTES[fmt]
    rec = read_shots(path, fmt, 8, 1)
    assert isinstance(rec, PackedSamples) and rec.shape == (2, 9)
    assert np.array_equal(rec.unpack(), BITS_9x2)
    assert np.array_equal(rec.field(0, 8).unpack(), BITS_9x2[:, :8]) and np.array_equal(rec.field(8, 1).unpack(), BITS_9x2[:, 8:])


@pytest.mark.parametrize("shots", [1, 65])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 1008, 1009])
def test_formats_round_trip(n, shots, tmp_path):
    rng = np.random.default_rng(1000 * n + shots)
    bits = (rng.random((shots, n)) < 0.3).astype(np.uint8)
    nobs = min(3, n - 1)
    for fmt in ("b8", "01", "hits", "dets"):
        path = str(tmp_path / ("r." + fmt))
        write_shots(path, PackedSamples.pack(bits) if fmt != "hits" else bits.astype(bool), fmt, num_detectors=n - nobs)
        rec = read_shots(path, fmt, n - nobs, nobs)
        assert len(rec) == shots and rec.num_bits == n
        assert np.array_equal(rec.unpack(), bits), fmt
        assert np.array_equal(rec.field(n - nobs, nobs).unpack(), bits[:, n - nobs:]), fmt
    assert os.path.getsize(str(tmp_path / "r.b8")) == shots * ((n + 7) // 8)


def test_malformed_files_are_refused(tmp_path):
    p = str(tmp_path / "t.b8")
    open(p, "wb").write(bytes(7))
    with pytest.raises(ShotFileError, match=r"7 bytes.*2-byte shots"):
        read_shots(p, "b8", 9)
    assert len(read_shots(p, "b8", 50, 6)) == 1
    for fmt, body, line in (("01", "101\n10\n", 2), ("01", "1x1\n", 1), ("hits", "0,2\n\n3\n", 3), ("hits", "0,a\n", 1),
                            ("dets", "shot D0\nshoot D1\n", 2), ("dets", "shot D0 L1\n", 1), ("dets", "shot D3\n", 1), ("dets", "shot M0\n", 1)):
        p = str(tmp_path / "t.txt")
        open(p, "w").write(body)
        with pytest.raises(ValueError, match="line %d" % line):
            read_shots(p, fmt, 3, 1 if fmt == "dets" else 0)
    with pytest.raises(ValueError, match="format"):
        read_shots(p, "r8", 3)


def test_packed_samples_on_the_host():
    rng = np.random.default_rng(5)
    bits = (rng.random((70, 45)) < 0.5).astype(np.uint8)
    for arr in (bits, bits.astype(bool), bits.astype(np.int64) * 3 - 2 * (bits == 0), bits.astype(np.int8) - 2):      # the low bit counts
        ps = PackedSamples.pack(arr)
        assert ps.data.dtype == np.uint8 and ps.data.shape == (70, 6) and ps.shape == (70, 45) and len(ps) == 70 and not ps.is_cuda
        assert np.array_equal(ps.data, np.packbits((np.asarray(arr).astype(np.int64) & 1).astype(np.uint8), axis=1, bitorder="little"))
        assert np.array_equal(ps.unpack(), bits) and ps.unpack().dtype == np.uint8
    ps = PackedSamples.pack(bits)
    assert not (ps.data[:, -1] >> 5).any()                                       # padding bits are zero
    assert np.array_equal(ps[10:33].unpack(), bits[10:33]) and len(ps[60:]) == 10 and len(ps[::2]) == 35
    assert np.array_equal(ps.field(3, 20).unpack(), bits[:, 3:23]) and np.array_equal(ps.field(13, 32).field(3, 9).unpack(), bits[:, 16:25])
    assert np.array_equal(ps.field(40, 5)[5:9].unpack(), bits[5:9, 40:]) and ps.field(45, 0).unpack().shape == (70, 0)
    assert np.array_equal(np.asarray(ps), bits)
    wide = PackedSamples(np.concatenate([ps.data, np.full((70, 2), 0xFF, np.uint8)], axis=1), 45)   # rows wider than the bits need
    assert np.array_equal(wide.unpack(), bits) and wide.dense().data.shape == (70, 6)
    dirty = PackedSamples(ps.data | np.uint8(0xE0) * (np.arange(6) == 5).astype(np.uint8), 45)      # set padding bits are not data
    assert np.array_equal(dirty.unpack(), bits) and np.array_equal(dirty.dense().data, ps.data)
    with pytest.raises(ValueError):
        PackedSamples(ps.data, 49)
    with pytest.raises(ValueError):
        ps.field(40, 6)
    with pytest.raises(TypeError):
        ps[3]
    with pytest.raises(ValueError):
        PackedSamples(ps.data.astype(np.int32), 45)


# ---- the library -------------------------------------------------------------------------------------------------------------------------
def test_exports_check_their_arguments_without_a_gpu():
    from quits_amd import _lib
    L = _lib.load()
    assert L.qd_version() >= 109
    assert "qd_unpack_b8" in _lib.EXPORTS and "qd_pack_b8" in _lib.EXPORTS
    buf = ctypes.create_string_buffer(64)          # never dereferenced: every call below is refused, or has no shots
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: L.qd_last_error().decode()
    # unpack(d_packed, packed_stride, bit0, nbits, B, d_out, out_stride, stream)
    assert L.qd_unpack_b8(None, 2, 0, 9, 1, p, 9, None) == -1 and "null" in err()
    assert L.qd_unpack_b8(p, 2, 0, 9, 1, None, 9, None) == -1 and "null" in err()
    assert L.qd_unpack_b8(p, 2, 0, -1, 1, p, 9, None) == -1 and "negative" in err()
    assert L.qd_unpack_b8(p, 2, 0, 9, -1, p, 9, None) == -1 and "negative" in err()
    assert L.qd_unpack_b8(p, 2, -1, 9, 1, p, 9, None) == -1 and "negative" in err()
    assert L.qd_unpack_b8(p, 1, 0, 9, 1, p, 9, None) == -1 and "packed_stride" in err()
    assert L.qd_unpack_b8(p, 2, 8, 9, 1, p, 9, None) == -1 and "packed_stride" in err()        # bits 8 .. 16 need a third byte
    assert L.qd_unpack_b8(p, 2, 7, 9, 1, p, 8, None) == -1 and "out_stride" in err()
    assert L.qd_unpack_b8(None, 2, 7, 9, 0, None, 9, None) == 0                                # B = 0: nothing to do
    # pack(d_in, in_stride, nbits, B, d_packed, packed_stride, stream)
    assert L.qd_pack_b8(None, 9, 9, 1, p, 2, None) == -1 and "null" in err()
    assert L.qd_pack_b8(p, 9, 9, 1, None, 2, None) == -1 and "null" in err()
    assert L.qd_pack_b8(p, 9, -1, 1, p, 2, None) == -1 and "negative" in err()
    assert L.qd_pack_b8(p, 9, 9, -1, p, 2, None) == -1 and "negative" in err()
    assert L.qd_pack_b8(p, 9, 9, 1, p, 1, None) == -1 and "packed_stride" in err()
    assert L.qd_pack_b8(p, 8, 9, 1, p, 2, None) == -1 and "in_stride" in err()
    assert L.qd_pack_b8(None, 9, 9, 0, None, 2, None) == 0


def test_bitpack_compiles_to_two_kernels_without_scratch(tmp_path):
    cs = os.path.join(ROOT, "quits_amd", "csrc")
    mk = open(os.path.join(cs, "Makefile")).read()
    assert re.search(r"^SRC := .*\bbitpack\.hip\b", mk, re.M)
    flags = [f for f in re.search(r"^FLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split() if f != "-shared"]
    out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o",
                          str(tmp_path / "bitpack.o"), os.path.join(cs, "bitpack.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out.stderr)]
    assert len(names) == 2 and any("qd_unpack_b8_kernel" in n for n in names) and any("qd_pack_b8_kernel" in n for n in names), names
    assert scratch == [0, 0] and lds == [0, 0]
    src = open(os.path.join(cs, "bitpack.hip")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", src, re.M)


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def test_cli_help_and_argument_errors(tmp_path, capsys):
    out = subprocess.run([sys.executable, "-m", "quits_amd", "predict", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0
    for word in ("--dem", "--circuit", "--in_format", "--in_includes_appended_observables", "--out_format", "--obs_in", "--bp_method", "--schedule",
                 "--max_iter", "--osd_method", "--osd_order", "--checks_per_round", "--window", "--commit"):
        assert word in out.stdout, word
    from quits_amd.__main__ import main
    dem = str(tmp_path / "m.dem")
    open(dem, "w").write("error(0.1) D0 L0\n")
    base = ["predict", "--in", "x", "--in_format", "b8", "--out", "y", "--out_format", "01"]
    for argv in ([], ["predict"], base, base + ["--dem", dem, "--circuit", dem], ["predict", "--dem", dem, "--in", "x", "--in_format", "r8", "--out", "y", "--out_format", "01"],
                 base + ["--dem", dem, "--window", "3"], base + ["--dem", dem, "--checks_per_round", "0", "--window", "3", "--commit", "1"]):
        with pytest.raises(SystemExit) as exc:
            main(argv)
        assert exc.value.code == 2, argv
    capsys.readouterr()
    assert main(base + ["--dem", dem]) == 1 and "x" in capsys.readouterr().err                      # the sample file does not exist
    open(str(tmp_path / "bad.dem"), "w").write("error(3) D0\n")
    assert main(base + ["--dem", str(tmp_path / "bad.dem")]) == 1 and "line 1" in capsys.readouterr().err
    import torch
    if not torch.cuda.is_available():                                                               # no GPU: the package's own text, status 2
        shots = str(tmp_path / "s.b8")
        open(shots, "wb").write(bytes(4))
        assert main(["predict", "--dem", dem, "--in", shots, "--in_format", "b8", "--out", str(tmp_path / "p.01"), "--out_format", "01"]) == 2
        assert "no HIP device" in capsys.readouterr().err
