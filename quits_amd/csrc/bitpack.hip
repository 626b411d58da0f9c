// bitpack.hip -- Stim's bit-packed sample format (b8: bit k of a shot is bit k & 7 of byte k >> 3 of its row) to and from the one byte per
// detector that every kernel of this library reads (qd_unpack_b8, qd_pack_b8).  The reference takes `zcheck_samples` unpacked
// (decoder/sliding_window.py:104-118); what Stim's sampler returns with bit_packed=True, or writes with --out_format b8, is eight times
// smaller on the host and over PCIe, and is widened here, on the device, in front of the decoder.
#include "../../include/quits_amd.h"
#include "qd_internal.h"
#include "qd_host.h"

#define QD_BITPACK_THREADS 256
#define QD_BITPACK_MAX_BLOCKS 16384     // the grid is bounded: every lane strides over the groups

// One lane per group of 8 output bytes; consecutive lanes take consecutive packed bytes of a row, then the next row.  Packed rows start at
// any byte address: byte loads.  The 8 bytes leave as one store only where that store is aligned and wholly inside the row's nbits columns.
__global__ void __launch_bounds__(QD_BITPACK_THREADS) qd_unpack_b8_kernel(const uint8_t *__restrict__ packed, int64_t packed_stride, int64_t bit0,
                                                                          int nbits, int64_t B, uint8_t *__restrict__ out, int64_t out_stride)
{
    const int64_t groups = ((int64_t)nbits + 7) >> 3, total = B * groups;
    const int64_t byte0 = bit0 >> 3;
    const int sh = (int)(bit0 & 7);
    const int64_t step = (int64_t)gridDim.x * QD_BITPACK_THREADS;
    for (int64_t idx = (int64_t)blockIdx.x * QD_BITPACK_THREADS + threadIdx.x; idx < total; idx += step) {
        const int64_t b = idx / groups, g = idx - b * groups;
        const int cnt = (int)(nbits - 8 * g < 8 ? nbits - 8 * g : 8);
        const uint8_t *p = packed + b * packed_stride + byte0 + g;
        uint32_t v = (uint32_t)p[0] >> sh;
        if (sh + cnt > 8) v |= (uint32_t)p[1] << (8 - sh);          // (the last bit wanted, bit0 + 8 g + cnt - 1, lies in that byte: inside the row)
        v &= 0xFFu >> (8 - cnt);
        // byte j of x = bit j of v: v in every byte, one bit kept per byte, then "non-zero" as 0 / 1
        uint64_t x = ((uint64_t)v * 0x0101010101010101ull) & 0x8040201008040201ull;
        x = ((x + 0x7F7F7F7F7F7F7F7Full) >> 7) & 0x0101010101010101ull;
        uint8_t *o = out + b * out_stride + 8 * g;
        if (cnt == 8 && (reinterpret_cast<uintptr_t>(o) & 7u) == 0)
            *reinterpret_cast<uint64_t *>(o) = x;
        else
#pragma clang loop vectorize(disable) unroll(disable)       // byte stores stay byte stores: the address is not aligned for anything wider
            for (int j = 0; j < cnt; ++j) o[j] = (uint8_t)(x >> (8 * j));
    }
}

// One lane per packed byte, in the same order.  The 8 input bytes come as one load only where it is aligned and wholly inside the row's
// nbits columns; the low bit of each counts.
__global__ void __launch_bounds__(QD_BITPACK_THREADS) qd_pack_b8_kernel(const uint8_t *__restrict__ in, int64_t in_stride, int nbits, int64_t B,
                                                                        uint8_t *__restrict__ packed, int64_t packed_stride)
{
    const int64_t groups = ((int64_t)nbits + 7) >> 3, total = B * groups;
    const int64_t step = (int64_t)gridDim.x * QD_BITPACK_THREADS;
    for (int64_t idx = (int64_t)blockIdx.x * QD_BITPACK_THREADS + threadIdx.x; idx < total; idx += step) {
        const int64_t b = idx / groups, g = idx - b * groups;
        const int cnt = (int)(nbits - 8 * g < 8 ? nbits - 8 * g : 8);
        const uint8_t *p = in + b * in_stride + 8 * g;
        uint32_t v = 0;
        if (cnt == 8 && (reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
            // bit 8 j of x -> bit 56 + j: the factor has a one at 56 - 7 j for every j, and no two products meet in one bit
            const uint64_t x = *reinterpret_cast<const uint64_t *>(p) & 0x0101010101010101ull;
            v = (uint32_t)((x * 0x0102040810204080ull) >> 56);
        } else {
#pragma clang loop vectorize(disable) unroll(disable)       // byte loads stay byte loads, as above
            for (int j = 0; j < cnt; ++j) v |= (uint32_t)(p[j] & 1u) << j;
        }
        packed[b * packed_stride + g] = (uint8_t)v;
    }
}

static unsigned bitpack_blocks(int64_t total)
{
    const int64_t blocks = (total + QD_BITPACK_THREADS - 1) / QD_BITPACK_THREADS;
    return (unsigned)(blocks < QD_BITPACK_MAX_BLOCKS ? blocks : QD_BITPACK_MAX_BLOCKS);
}

extern "C" int qd_unpack_b8(const uint8_t *d_packed, int64_t packed_stride, int64_t bit0, int32_t nbits, int64_t B, uint8_t *d_out,
                            int64_t out_stride, void *stream)
{
    if (B < 0 || nbits < 0 || bit0 < 0) return qd_fail(QD_EINVAL, "negative shot count, bit count or bit offset");
    if (bit0 > INT64_MAX - nbits - 7) return qd_fail(QD_EINVAL, "bit offset too large");
    if (packed_stride < (bit0 + nbits + 7) / 8)
        return qd_fail(QD_EINVAL, "packed_stride %lld is smaller than the %lld bytes that hold bits %lld .. %lld of a row", (long long)packed_stride,
                       (long long)((bit0 + nbits + 7) / 8), (long long)bit0, (long long)(bit0 + nbits - 1));
    if (out_stride < nbits) return qd_fail(QD_EINVAL, "out_stride %lld is smaller than nbits = %d", (long long)out_stride, nbits);
    if (B == 0) return QD_OK;
    if (!d_packed || !d_out) return qd_fail(QD_EINVAL, "null packed rows or output");
    if (nbits == 0) return QD_OK;
    const int64_t total = B * (((int64_t)nbits + 7) >> 3);
    hipLaunchKernelGGL(qd_unpack_b8_kernel, dim3(bitpack_blocks(total)), dim3(QD_BITPACK_THREADS), 0, reinterpret_cast<hipStream_t>(stream), d_packed,
                       packed_stride, bit0, nbits, B, d_out, out_stride);
    HIP_TRY(hipGetLastError());
    return QD_OK;
}

extern "C" int qd_pack_b8(const uint8_t *d_in, int64_t in_stride, int32_t nbits, int64_t B, uint8_t *d_packed, int64_t packed_stride, void *stream)
{
    if (B < 0 || nbits < 0) return qd_fail(QD_EINVAL, "negative shot count or bit count");
    if (packed_stride < ((int64_t)nbits + 7) / 8)
        return qd_fail(QD_EINVAL, "packed_stride %lld is smaller than the %lld bytes of %d bits", (long long)packed_stride, (long long)(((int64_t)nbits + 7) / 8), nbits);
    if (in_stride < nbits) return qd_fail(QD_EINVAL, "in_stride %lld is smaller than nbits = %d", (long long)in_stride, nbits);
    if (B == 0) return QD_OK;
    if (!d_in || !d_packed) return qd_fail(QD_EINVAL, "null input or packed rows");
    if (nbits == 0) return QD_OK;
    const int64_t total = B * (((int64_t)nbits + 7) >> 3);
    hipLaunchKernelGGL(qd_pack_b8_kernel, dim3(bitpack_blocks(total)), dim3(QD_BITPACK_THREADS), 0, reinterpret_cast<hipStream_t>(stream), d_in, in_stride,
                       nbits, B, d_packed, packed_stride);
    HIP_TRY(hipGetLastError());
    return QD_OK;
}
