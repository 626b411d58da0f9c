// soft.hip -- soft outputs per shot (qd_soft_fold, qd_soft_weigh, qd_soft_tally): a record of six 64-bit integers -- the weight of the committed
// correction under the priors' log-likelihood table, its size, the syndrome's weight, and the iterations, post-processed windows and pivot /
// leg counts folded from the windows' status words -- and a histogram of every field over all shots and over the failing ones, from which the
// host reads how the logical error rate falls when the least certain shots are discarded.  The definition, bit for bit, is quits_amd/soft.py
// (soft_mirror, bin_of).  The reference returns predictions only and drops the decoders' `converge` and iteration counts (sliding_window.py:171).
#include "../../include/quits_amd.h"
#include "qd_internal.h"
#include "qd_host.h"

#define QD_SOFT_THREADS 256
#define QD_SOFT_FOLD_MAX_BLOCKS 4096    // the grids are bounded: every lane (fold, tally) or wavefront (weigh) strides over the shots
#define QD_SOFT_WEIGH_MAX_BLOCKS 16384
#define QD_SOFT_TALLY_MAX_BLOCKS 256    // ... per field; a workgroup flushes its 2 * QD_SOFT_BINS sums once

struct SoftShifts {
    int s[QD_SOFT_FIELDS];
};

// soft[b][3 .. 5] += iterations, post-processed (0 / 1), bits 20 .. 31 of one window's status word.  One lane per shot.
__global__ void __launch_bounds__(QD_SOFT_THREADS) qd_soft_fold_kernel(const int32_t *__restrict__ status, int64_t B, long long *soft, int64_t soft_stride)
{
    const int64_t step = (int64_t)gridDim.x * QD_SOFT_THREADS;
    for (int64_t b = (int64_t)blockIdx.x * QD_SOFT_THREADS + threadIdx.x; b < B; b += step) {
        const uint32_t s = (uint32_t)status[b];
        long long *r = soft + b * soft_stride;
        r[3] += (long long)(s & QD_STATUS_ITER_MASK);
        r[4] += (long long)((s >> 17) & 1u);
        r[5] += (long long)((s >> 20) & 0xFFFu);
    }
}

// One wavefront per shot (qd_fault_stats_kernel's shape): its lanes stride over the words of C (coalesced) and gather a weight per set bit, then
// over the detector bytes; the three sums are added over the wavefront and lane 0 writes them.  The weight sum is 64-bit throughout: 4097
// faults of weight 2^31 - 1 need 44 bits.
__global__ void __launch_bounds__(QD_SOFT_THREADS) qd_soft_weigh_kernel(const uint32_t *__restrict__ corr, int64_t stride, int nbits,
                                                                        const int32_t *__restrict__ weights, const uint8_t *__restrict__ det,
                                                                        int64_t det_stride, int m, int64_t B, long long *soft, int64_t soft_stride)
{
    const int lane = threadIdx.x & (QD_WAVE - 1), wv = threadIdx.x >> 6;
    const int nwords = (nbits + 31) >> 5;
    const uint32_t last_mask = (nbits & 31) ? (1u << (nbits & 31)) - 1u : 0xFFFFFFFFu;
    const int64_t step = (int64_t)gridDim.x * (QD_SOFT_THREADS / QD_WAVE);
    for (int64_t b = (int64_t)blockIdx.x * (QD_SOFT_THREADS / QD_WAVE) + wv; b < B; b += step) {      // uniform in the wavefront
        const uint32_t *c = corr + b * stride;
        long long wsum = 0;
        uint32_t nf = 0, ne = 0;
        for (int w = lane; w < nwords; w += QD_WAVE) {
            uint32_t x = c[w] & (w == nwords - 1 ? last_mask : 0xFFFFFFFFu);
            nf += (uint32_t)__popc(x);
            while (x) {                                      // (every index is below nbits: the padding bits are masked off)
                const int j = __ffs((int)x) - 1;
                x &= x - 1u;
                wsum += (long long)weights[(w << 5) + j];
            }
        }
        const uint8_t *d = det + b * det_stride;
        for (int i = lane; i < m; i += QD_WAVE) ne += d[i] & 1u;
#pragma unroll
        for (int s = QD_WAVE / 2; s >= 1; s >>= 1) wsum += __shfl_xor(wsum, s);
        nf = qd_wave_add(nf);
        ne = qd_wave_add(ne);
        if (lane == 0) {
            long long *r = soft + b * soft_stride;
            r[0] = wsum;
            r[1] = (long long)nf;
            r[2] = (long long)ne;
        }
    }
}

// blockIdx.y = the field: a workgroup keeps that field's two planes (all shots, failing shots) in LDS, one lane per shot strides over the
// shots, and the workgroup flushes its non-zero bins once.  Global atomics: at most 2 * QD_SOFT_BINS per workgroup, whatever B is.  A
// wavefront whose live lanes all fall into one bin -- `post` and `tail` of the shots BP solved, most of them -- adds its count once.
__global__ void __launch_bounds__(QD_SOFT_THREADS) qd_soft_tally_kernel(const long long *__restrict__ soft, int64_t soft_stride, int64_t B, SoftShifts sh,
                                                                        const unsigned long long *__restrict__ fail_mask, unsigned long long *hist)
{
    __shared__ unsigned long long sm[2 * QD_SOFT_BINS];
    const int tid = threadIdx.x, lane = tid & (QD_WAVE - 1), f = blockIdx.y;
    for (int i = tid; i < 2 * QD_SOFT_BINS; i += QD_SOFT_THREADS) sm[i] = 0ull;
    __syncthreads();
    const int shift = sh.s[f];
    const int64_t step = (int64_t)gridDim.x * QD_SOFT_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * QD_SOFT_THREADS; base < B; base += step) {       // uniform in the workgroup
        const int64_t b = base + tid;
        const bool live = b < B;
        int bin = 0;
        bool failed = false;
        if (live) {
            const long long v = soft[b * soft_stride + f];
            const long long q = v < 0 ? 0ll : (v >> shift);
            bin = (int)(q < QD_SOFT_BINS - 1 ? q : QD_SOFT_BINS - 1);
            if (fail_mask) failed = (fail_mask[b >> 6] >> (b & 63)) & 1ull;
        }
        const unsigned long long lm = __ballot(live), fm = __ballot(failed);
        const int first = __builtin_amdgcn_readfirstlane(bin);          // (lane 0 of a wavefront is live whenever any lane of it is)
        if (__ballot(live && bin != first) == 0ull) {
            if (lane == 0 && lm) {
                atomicAdd(&sm[first], (unsigned long long)__popcll(lm));
                if (fm) atomicAdd(&sm[QD_SOFT_BINS + first], (unsigned long long)__popcll(fm));
            }
        } else if (live) {
            atomicAdd(&sm[bin], 1ull);
            if (failed) atomicAdd(&sm[QD_SOFT_BINS + bin], 1ull);
        }
    }
    __syncthreads();
    unsigned long long *h = hist + (size_t)f * 2 * QD_SOFT_BINS;
    for (int i = tid; i < (fail_mask ? 2 : 1) * QD_SOFT_BINS; i += QD_SOFT_THREADS)
        if (sm[i]) atomicAdd(&h[i], sm[i]);
}

static unsigned qd_soft_blocks(int64_t items, int per_block, int max_blocks)
{
    const int64_t blocks = (items + per_block - 1) / per_block;
    return (unsigned)(blocks < max_blocks ? blocks : max_blocks);
}

extern "C" int qd_soft_fold(const int32_t *d_status, int64_t B, int64_t *d_soft, int64_t soft_stride, void *stream)
{
    if (B == 0) return QD_OK;
    if (B < 0) return qd_fail(QD_EINVAL, "negative shot count");
    if (soft_stride < QD_SOFT_FIELDS) return qd_fail(QD_EINVAL, "soft_stride %lld is smaller than the %d fields of a record", (long long)soft_stride, QD_SOFT_FIELDS);
    if (!d_status || !d_soft) return qd_fail(QD_EINVAL, "null status or soft records");
    hipLaunchKernelGGL(qd_soft_fold_kernel, dim3(qd_soft_blocks(B, QD_SOFT_THREADS, QD_SOFT_FOLD_MAX_BLOCKS)), dim3(QD_SOFT_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), d_status, B, reinterpret_cast<long long *>(d_soft), soft_stride);
    HIP_TRY(hipGetLastError());
    return QD_OK;
}

extern "C" int qd_soft_weigh(const uint32_t *d_corr, int64_t stride_words, int32_t nbits, const int32_t *d_weights, const uint8_t *d_det,
                             int64_t det_stride, int32_t m, int64_t B, int64_t *d_soft, int64_t soft_stride, void *stream)
{
    if (B == 0) return QD_OK;
    if (B < 0 || nbits < 0 || m < 0) return qd_fail(QD_EINVAL, "negative shot count, bit count or detector count");
    if (nbits > INT32_MAX - 63) return qd_fail(QD_EINVAL, "too many bits in a row");
    if (soft_stride < QD_SOFT_FIELDS) return qd_fail(QD_EINVAL, "soft_stride %lld is smaller than the %d fields of a record", (long long)soft_stride, QD_SOFT_FIELDS);
    if (stride_words < ((int64_t)nbits + 31) / 32)
        return qd_fail(QD_EINVAL, "stride_words %lld is smaller than the %lld words of %d bits", (long long)stride_words, (long long)(((int64_t)nbits + 31) / 32), nbits);
    if (det_stride < m) return qd_fail(QD_EINVAL, "det_stride %lld is smaller than m = %d", (long long)det_stride, m);
    if (!d_soft) return qd_fail(QD_EINVAL, "null soft records");
    if (nbits > 0 && (!d_corr || !d_weights)) return qd_fail(QD_EINVAL, "null correction rows or weights");
    if (m > 0 && !d_det) return qd_fail(QD_EINVAL, "null detector rows");
    hipLaunchKernelGGL(qd_soft_weigh_kernel, dim3(qd_soft_blocks(B, QD_SOFT_THREADS / QD_WAVE, QD_SOFT_WEIGH_MAX_BLOCKS)), dim3(QD_SOFT_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), d_corr, stride_words, nbits, d_weights, d_det, det_stride, m, B,
                       reinterpret_cast<long long *>(d_soft), soft_stride);
    HIP_TRY(hipGetLastError());
    return QD_OK;
}

extern "C" int qd_soft_tally(const int64_t *d_soft, int64_t soft_stride, int64_t B, const int32_t *shifts6, const uint64_t *d_fail_mask,
                             int64_t *d_hist, void *stream)
{
    if (B == 0) return QD_OK;
    if (B < 0) return qd_fail(QD_EINVAL, "negative shot count");
    if (soft_stride < QD_SOFT_FIELDS) return qd_fail(QD_EINVAL, "soft_stride %lld is smaller than the %d fields of a record", (long long)soft_stride, QD_SOFT_FIELDS);
    if (!shifts6) return qd_fail(QD_EINVAL, "null shifts");
    SoftShifts sh;
    for (int f = 0; f < QD_SOFT_FIELDS; ++f) {
        if (shifts6[f] < 0 || shifts6[f] > 62) return qd_fail(QD_EINVAL, "shift %d of field %d outside 0 .. 62", shifts6[f], f);
        sh.s[f] = shifts6[f];
    }
    if (!d_soft || !d_hist) return qd_fail(QD_EINVAL, "null soft records or histogram");
    hipLaunchKernelGGL(qd_soft_tally_kernel, dim3(qd_soft_blocks(B, QD_SOFT_THREADS, QD_SOFT_TALLY_MAX_BLOCKS), QD_SOFT_FIELDS), dim3(QD_SOFT_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const long long *>(d_soft), soft_stride, B, sh,
                       reinterpret_cast<const unsigned long long *>(d_fail_mask), reinterpret_cast<unsigned long long *>(d_hist));
    HIP_TRY(hipGetLastError());
    return QD_OK;
}
