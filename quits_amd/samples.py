"""Bit-packed samples and Stim's result files.

Stim's native sample format is `b8`: ceil(n / 8) bytes per shot, bit k of a shot in byte k >> 3 at bit k & 7 -- what
`compile_detector_sampler().sample(..., bit_packed=True)` returns and what `stim sample --out_format b8` writes.  `PackedSamples` holds such
rows, on the host (numpy) or on the GPU (a CUDA tensor), and is accepted wherever the decoders take `zcheck_samples` / `syndromes`
(the reference takes them unpacked, decoder/sliding_window.py:104-118): an eighth of the bytes on the host and over PCIe, widened on the
device by qd_unpack_b8 (csrc/bitpack.hip).  `read_shots` / `write_shots` read and write Stim's result formats `b8`, `01`, `hits` and `dets`.
"""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

FORMATS = ("b8", "01", "hits", "dets")


def _is_tensor(x) -> bool:
    try:
        import torch
    except ImportError:      # pragma: no cover
        return False
    return isinstance(x, torch.Tensor)


def _stream_ptr(stream=None):
    import torch
    return C.c_void_p((torch.cuda.current_stream() if stream is None else stream).cuda_stream)


def unpack_b8_into(packed, bit0: int, nbits: int, out, stream=None):
    """out[b, c] = bit (bit0 + c) of row b of `packed`, c < nbits (qd_unpack_b8): cuda uint8 tensors, rows of any stride (unit stride inside
    a row); `out` may be a column slice.  Asynchronous on `stream` (default: the current one)."""
    import torch
    from . import _lib
    L = _lib.require_bitpack(_lib.load())
    assert packed.is_cuda and out.is_cuda and packed.dtype == torch.uint8 and out.dtype == torch.uint8
    assert packed.dim() == 2 and out.dim() == 2 and packed.shape[0] == out.shape[0] and out.shape[1] == nbits
    assert (packed.shape[1] <= 1 or packed.stride(1) == 1) and (out.shape[1] <= 1 or out.stride(1) == 1)
    if 8 * packed.shape[1] < bit0 + nbits:
        raise ValueError("packed rows hold %d bits, bits %d .. %d are wanted" % (8 * packed.shape[1], bit0, bit0 + nbits - 1))
    B = packed.shape[0]
    ps = packed.stride(0) if B > 1 else max(packed.stride(0), packed.shape[1])
    os_ = out.stride(0) if B > 1 else max(out.stride(0), nbits)
    _lib.check(L.qd_unpack_b8(C.c_void_p(packed.data_ptr()), ps, int(bit0), int(nbits), B, C.c_void_p(out.data_ptr()), os_, _stream_ptr(stream)))
    return out


def pack_b8_into(bits, packed, stream=None):
    """packed[b, i] = bits 8 i .. 8 i + 7 of row b of `bits` (low bit of each byte; qd_pack_b8): cuda uint8 tensors."""
    import torch
    from . import _lib
    L = _lib.require_bitpack(_lib.load())
    assert bits.is_cuda and packed.is_cuda and bits.dtype == torch.uint8 and packed.dtype == torch.uint8
    assert bits.dim() == 2 and packed.dim() == 2 and bits.shape[0] == packed.shape[0] and 8 * packed.shape[1] >= bits.shape[1]
    assert (bits.shape[1] <= 1 or bits.stride(1) == 1) and (packed.shape[1] <= 1 or packed.stride(1) == 1)
    B, n = bits.shape
    bs = bits.stride(0) if B > 1 else max(bits.stride(0), n)
    ps = packed.stride(0) if B > 1 else max(packed.stride(0), packed.shape[1])
    _lib.check(L.qd_pack_b8(C.c_void_p(bits.data_ptr()), bs, int(n), B, C.c_void_p(packed.data_ptr()), ps, _stream_ptr(stream)))
    return packed


class PackedSamples:
    """N shots of `num_bits` bits each, bit-packed as Stim's b8: `data` is a numpy uint8 array [N, >= ceil(num_bits / 8)] or a CUDA uint8
    tensor of that shape.  Rows may be wider than the bits need (a record of several fields: see `field`)."""

    def __init__(self, data, num_bits: int, bit0: int = 0):
        num_bits, bit0 = int(num_bits), int(bit0)
        if num_bits < 0 or bit0 < 0:
            raise ValueError("num_bits and bit0 must not be negative")
        if _is_tensor(data):
            import torch
            if data.dtype != torch.uint8 or data.dim() != 2:
                raise ValueError("packed data must be a uint8 [shots, bytes] tensor")
            if not data.is_cuda:
                data = data.numpy()
            elif data.shape[1] > 1 and data.stride(1) != 1:
                data = data.contiguous()
        if not _is_tensor(data):
            data = np.asarray(data)
            if data.dtype != np.uint8 or data.ndim != 2:
                raise ValueError("packed data must be a uint8 [shots, bytes] array")
        if 8 * data.shape[1] < bit0 + num_bits:
            raise ValueError("rows of %d bytes cannot hold bits %d .. %d" % (data.shape[1], bit0, bit0 + num_bits - 1))
        self.data, self.num_bits, self.bit0 = data, num_bits, bit0

    # ---- what the decoders' entry points ask of their samples
    @property
    def is_cuda(self) -> bool:
        return _is_tensor(self.data)

    @property
    def shape(self):
        return (int(self.data.shape[0]), self.num_bits)

    @property
    def ndim(self) -> int:
        return 2

    @property
    def num_bytes(self) -> int:
        return (self.num_bits + 7) // 8

    def __len__(self) -> int:
        return int(self.data.shape[0])

    def __getitem__(self, key):
        if not isinstance(key, slice):
            raise TypeError("PackedSamples are sliced by shots: samples[a:b]")
        return PackedSamples(self.data[key], self.num_bits, self.bit0)

    def field(self, bit0: int, nbits: int) -> "PackedSamples":
        """Bits bit0 .. bit0 + nbits - 1 of every shot, as packed samples over the same rows: nothing is copied or unpacked until asked for
        (e.g. the observables Stim appends after the detectors: `rec.field(num_detectors, num_observables)`)."""
        if bit0 < 0 or nbits < 0 or bit0 + nbits > self.num_bits:
            raise ValueError("field [%d, %d) lies outside the %d bits of a shot" % (bit0, bit0 + nbits, self.num_bits))
        return PackedSamples(self.data, nbits, self.bit0 + bit0)

    def __array__(self, dtype=None, copy=None):
        a = self.unpack()
        a = a.cpu().numpy() if _is_tensor(a) else a
        return a if dtype is None else a.astype(dtype)

    # ---- packing and unpacking
    @classmethod
    def pack(cls, bits) -> "PackedSamples":
        """From [N, n] bits, one per element: a numpy array or a torch tensor of any integer dtype or bool; the low bit counts.  A CUDA tensor
        is packed on the device (qd_pack_b8) and stays there."""
        if _is_tensor(bits) and bits.is_cuda:
            import torch
            if bits.dim() != 2:
                raise ValueError("samples must be a [shots, bits] tensor")
            t = bits if bits.dtype == torch.uint8 else (bits.to(torch.uint8) if bits.dtype == torch.bool else torch.bitwise_and(bits, 1).to(torch.uint8))
            if t.shape[1] > 1 and t.stride(1) != 1:
                t = t.contiguous()
            packed = torch.empty((t.shape[0], (t.shape[1] + 7) // 8), dtype=torch.uint8, device=t.device)
            if packed.numel():
                pack_b8_into(t, packed)
            return cls(packed, t.shape[1])
        a = bits.numpy() if _is_tensor(bits) else np.asarray(bits)
        if a.ndim != 2:
            raise ValueError("samples must be a [shots, bits] array")
        if a.dtype == np.bool_:
            a = a.view(np.uint8)
        elif a.dtype.kind in "iu":
            a = (a & 1).astype(np.uint8) if a.dtype != np.uint8 else a & 1
        else:
            raise ValueError("samples must have an integer or bool dtype, not %s" % a.dtype)
        return cls(np.packbits(a, axis=1, bitorder="little"), a.shape[1])

    def unpack(self):
        """uint8 [N, num_bits] of zeros and ones, of the same kind as `data`: numpy, or a CUDA tensor (qd_unpack_b8)."""
        if self.is_cuda:
            import torch
            out = torch.empty(self.shape, dtype=torch.uint8, device=self.data.device)
            if out.numel():
                unpack_b8_into(self.data, self.bit0, self.num_bits, out)
            return out
        lo, hi = self.bit0 >> 3, (self.bit0 + self.num_bits + 7) >> 3
        sh = self.bit0 & 7
        return np.ascontiguousarray(np.unpackbits(self.data[:, lo:hi], axis=1, bitorder="little")[:, sh:sh + self.num_bits])

    def dense(self) -> "PackedSamples":
        """The same bits with bit0 = 0 and rows of exactly ceil(num_bits / 8) bytes whose padding bits are zero (what `b8` files hold)."""
        nb, rest = self.num_bytes, self.num_bits % 8
        if self.bit0 == 0 and self.data.shape[1] == nb and rest == 0:
            return self
        if self.bit0 == 0 and not self.is_cuda:
            d = np.array(self.data[:, :nb])                      # (a copy: the padding bits are cleared in it)
            if rest:
                d[:, -1] &= (1 << rest) - 1
            return PackedSamples(d, self.num_bits)
        return PackedSamples.pack(self.unpack())

    def cpu(self) -> "PackedSamples":
        return PackedSamples(self.data.cpu().numpy(), self.num_bits, self.bit0) if self.is_cuda else self

    def __repr__(self):
        return "PackedSamples(%d shots x %d bits, %s)" % (len(self), self.num_bits, "cuda" if self.is_cuda else "numpy")


# ---- Stim's result formats ---------------------------------------------------------------------------------------------------------------
class ShotFileError(ValueError):
    """A malformed result file; the message names the line, or for b8 the byte count."""


def _check_fmt(fmt):
    f = str(fmt).lower()
    if f not in FORMATS:
        raise ValueError("format must be one of %s, not %r (sparse formats r8 / ptb64 are not read here)" % (", ".join(FORMATS), fmt))
    return f


def _read_text_bits(path, fmt, ndet, nobs):
    n = ndet + nobs
    rows = []
    with open(path, "r") as fh:
        for no, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            row = np.zeros(n, dtype=np.uint8)
            if fmt == "01":
                if len(line) != n or line.strip("01"):
                    raise ShotFileError("%s line %d: expected %d characters 0 / 1, got %r" % (path, no, n, line[:40]))
                row[:] = np.frombuffer(line.encode(), dtype=np.uint8) - 48
            elif fmt == "hits":
                if line.strip():
                    for tok in line.split(","):
                        try:
                            k = int(tok)
                        except ValueError:
                            k = -1
                        if not 0 <= k < n:
                            raise ShotFileError("%s line %d: %r is not an index below %d" % (path, no, tok.strip()[:20], n))
                        row[k] ^= 1
            else:
                toks = line.split()
                if not toks:
                    continue                                    # (a blank line between shots)
                if toks[0].lower() != "shot":
                    raise ShotFileError("%s line %d: a dets line starts with 'shot', got %r" % (path, no, toks[0][:20]))
                for tok in toks[1:]:
                    m = re.fullmatch(r"([DdLl])(\d+)", tok)
                    if not m:
                        raise ShotFileError("%s line %d: %r is not a D# / L# token" % (path, no, tok[:20]))
                    k, obs = int(m.group(2)), m.group(1) in "Ll"
                    if k >= (nobs if obs else ndet):
                        raise ShotFileError("%s line %d: %s is beyond the %d %s of a shot" % (path, no, tok, nobs if obs else ndet,
                                                                                              "observables" if obs else "detectors"))
                    row[ndet + k if obs else k] ^= 1
            rows.append(row)
    return np.stack(rows) if rows else np.zeros((0, n), dtype=np.uint8)


def read_shots(path, fmt, num_detectors: int, num_observables: int = 0) -> PackedSamples:
    """The shots of a Stim result file as PackedSamples of num_detectors + num_observables bits (with num_observables > 0 the file was
    written with --append_observables: `.field(0, num_detectors)` and `.field(num_detectors, num_observables)` split the record).
    fmt: 'b8', '01', 'hits' or 'dets'."""
    fmt = _check_fmt(fmt)
    ndet, nobs = int(num_detectors), int(num_observables)
    if ndet < 0 or nobs < 0:
        raise ValueError("num_detectors and num_observables must not be negative")
    n = ndet + nobs
    if fmt == "b8":
        nb = (n + 7) // 8
        raw = np.fromfile(path, dtype=np.uint8)
        if nb == 0 or raw.size % nb:
            raise ShotFileError("%s holds %d bytes, not a whole number of %d-byte shots (%d bits each)" % (path, raw.size, nb, n))
        return PackedSamples(raw.reshape(-1, nb), n)
    return PackedSamples.pack(_read_text_bits(path, fmt, ndet, nobs))


def write_shots(path, samples, fmt, num_detectors=None) -> None:
    """Write shots in one of Stim's result formats.  samples: PackedSamples or a [N, n] array / tensor of bits.  num_detectors (format
    'dets' only): bits at and beyond it are observables, written as L#; default: every bit is a detector."""
    fmt = _check_fmt(fmt)
    ps = samples if isinstance(samples, PackedSamples) else PackedSamples.pack(samples)
    if fmt == "b8":
        np.ascontiguousarray(ps.dense().cpu().data).tofile(path)
        return
    bits = np.asarray(ps)
    n = bits.shape[1]
    ndet = n if num_detectors is None else int(num_detectors)
    if not 0 <= ndet <= n:
        raise ValueError("num_detectors = %d lies outside the %d bits of a shot" % (ndet, n))
    with open(path, "w", newline="\n") as fh:
        if fmt == "01":
            if n:
                chars = (bits + 48).astype(np.uint8)
                lines = np.concatenate([chars, np.full((bits.shape[0], 1), 10, np.uint8)], axis=1)
                fh.write(lines.tobytes().decode())
            else:
                fh.write("\n" * bits.shape[0])
            return
        for row in bits:
            idx = np.flatnonzero(row)
            if fmt == "hits":
                fh.write(",".join(str(int(k)) for k in idx) + "\n")
            else:
                fh.write(" ".join(["shot"] + [("D%d" % k) if k < ndet else ("L%d" % (k - ndet)) for k in idx]) + "\n")


__all__ = ["PackedSamples", "read_shots", "write_shots", "ShotFileError", "FORMATS"]
