// faults.hip -- the decoder's fault-level outputs (qd_sample_dem_faults, qd_commit_bits, qd_fault_stats_batch): which faults the DEM sampler
// fired, the space-time correction the windows of a sliding-window decode commit (the reference computes it per window and keeps only
// `window_observable_set[k] @ e` and `window_update[k] @ e` of it, decoder/sliding_window.py:171-183), and what a memory experiment tallies
// of the two: shots and failures by the number of sampled faults, and the weight of the residual E xor C of the failing shots whose
// correction reproduces the syndrome -- undetectable logical faults, the lightest of which bounds the circuit-level distance from above.
#include "../../include/quits_amd.h"
#include "qd_internal.h"
#include "qd_host.h"
#include "sample_dem_kernel.h"

#define QD_COMMIT_THREADS 256
#define QD_COMMIT_MAX_BLOCKS 16384      // the grid is bounded: every lane strides over the output words
#define QD_FSTATS_THREADS 256
#define QD_FSTATS_MAX_BLOCKS 1024       // ... every wavefront over the shots; a workgroup flushes its sums once

// Bits [out_bit0, out_bit0 + nbits) of row b of `out` = bits [0, nbits) of row b of `err`.  One lane per output word that the range touches:
// output word w0 + q holds source bits 32 q - sh .. 32 q - sh + 31 (sh = out_bit0 & 31), i.e. source words q - 1 and q shifted as one 64-bit
// value.  A word wholly inside the range is stored; the first and the last one keep their bits outside it -- read, merged and written by the
// one lane that owns the word, so calls on one stream whose ranges share a word compose without atomics.
__global__ void __launch_bounds__(QD_COMMIT_THREADS) qd_commit_bits_kernel(const uint32_t *__restrict__ err, int64_t err_stride, int nbits, int64_t B,
                                                                           uint32_t *out, int64_t out_stride, int64_t out_bit0)
{
    const int64_t w0 = out_bit0 >> 5, end = out_bit0 + nbits;
    const int nw = (int)(((end + 31) >> 5) - w0);           // output words per row
    const int src_words = (nbits + 31) >> 5;
    const int sh = (int)(out_bit0 & 31);
    const int64_t total = B * nw;
    const int64_t step = (int64_t)gridDim.x * QD_COMMIT_THREADS;
    for (int64_t idx = (int64_t)blockIdx.x * QD_COMMIT_THREADS + threadIdx.x; idx < total; idx += step) {
        const int64_t b = idx / nw;
        const int q = (int)(idx - b * nw);
        const uint32_t *e = err + b * err_stride;
        const uint32_t lo = q >= 1 ? e[q - 1] : 0u, hi = q < src_words ? e[q] : 0u;      // (q - 1 < src_words: nw <= src_words + 1)
        const uint32_t v = sh ? (uint32_t)((((uint64_t)hi << 32) | lo) >> (32 - sh)) : hi;
        const int64_t bit_lo = (w0 + q) << 5;
        const int first = out_bit0 > bit_lo ? (int)(out_bit0 - bit_lo) : 0;              // the range's bits of this word: first .. last - 1
        const int last = end < bit_lo + 32 ? (int)(end - bit_lo) : 32;
        const uint32_t mask = (last == 32 ? 0xFFFFFFFFu : (1u << last) - 1u) & ~((1u << first) - 1u);
        uint32_t *o = out + b * out_stride + w0 + q;
        *o = mask == 0xFFFFFFFFu ? v : ((*o & ~mask) | (v & mask));
    }
}

// One wavefront per shot: its lanes stride over the words of E and C (coalesced) and over the residual bytes, |E| and |E xor C| are summed
// over the wavefront, and lane 0 adds the shot to the workgroup's histograms in LDS.  Global atomics: at most 3 * QD_FAULT_HIST + 5 per
// workgroup, once, whatever B is (qd_tally_kernel's pattern, experiment.hip).
__global__ void __launch_bounds__(QD_FSTATS_THREADS) qd_fault_stats_kernel(const uint32_t *__restrict__ faults, const uint32_t *__restrict__ corr,
                                                                           int64_t stride, int nbits, const uint8_t *__restrict__ residual,
                                                                           int64_t res_stride, int m, const unsigned long long *__restrict__ fail_mask,
                                                                           int64_t B, int64_t shot0, unsigned long long *hist,
                                                                           unsigned long long *counts, unsigned long long *best)
{
    __shared__ unsigned long long sm[3 * QD_FAULT_HIST + 5];      // the histograms, counts[1..3] at 3 H + 1 .., the best word at 3 H + 4
    const int tid = threadIdx.x, lane = tid & (QD_WAVE - 1), wv = tid >> 6;
    for (int i = tid; i < 3 * QD_FAULT_HIST + 4; i += QD_FSTATS_THREADS) sm[i] = 0ull;
    if (tid == 0) sm[3 * QD_FAULT_HIST + 4] = ~0ull;
    __syncthreads();
    const int nwords = (nbits + 31) >> 5;
    const uint32_t last_mask = (nbits & 31) ? (1u << (nbits & 31)) - 1u : 0xFFFFFFFFu;
    const int64_t step = (int64_t)gridDim.x * (QD_FSTATS_THREADS / QD_WAVE);
    for (int64_t b = (int64_t)blockIdx.x * (QD_FSTATS_THREADS / QD_WAVE) + wv; b < B; b += step) {      // uniform in the wavefront
        const uint32_t *e = faults + b * stride, *c = corr + b * stride;
        int we = 0, wx = 0;
        for (int w = lane; w < nwords; w += QD_WAVE) {
            const uint32_t mk = w == nwords - 1 ? last_mask : 0xFFFFFFFFu;
            const uint32_t x = e[w] & mk;
            we += __popc(x);
            wx += __popc(x ^ (c[w] & mk));
        }
        bool nz = false;
        const uint8_t *r = residual + b * res_stride;
        for (int i = lane; i < m; i += QD_WAVE) nz |= r[i] != 0;
#pragma unroll
        for (int d = QD_WAVE / 2; d >= 1; d >>= 1) {
            we += __shfl_xor(we, d);
            wx += __shfl_xor(wx, d);
        }
        const bool res = __ballot(nz) != 0ull;
        if (lane == 0) {
            const bool failed = (fail_mask[b >> 6] >> (b & 63)) & 1ull;
            atomicAdd(&sm[we < QD_FAULT_HIST - 1 ? we : QD_FAULT_HIST - 1], 1ull);
            if (res) atomicAdd(&sm[3 * QD_FAULT_HIST + 2], 1ull);
            if (failed) {
                atomicAdd(&sm[QD_FAULT_HIST + (we < QD_FAULT_HIST - 1 ? we : QD_FAULT_HIST - 1)], 1ull);
                atomicAdd(&sm[3 * QD_FAULT_HIST + 1], 1ull);
                if (res)
                    atomicAdd(&sm[3 * QD_FAULT_HIST + 3], 1ull);
                else {
                    atomicAdd(&sm[2 * QD_FAULT_HIST + (wx < QD_FAULT_HIST - 1 ? wx : QD_FAULT_HIST - 1)], 1ull);
                    atomicMin(&sm[3 * QD_FAULT_HIST + 4], ((unsigned long long)wx << 40) | (unsigned long long)(shot0 + b));
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < 3 * QD_FAULT_HIST; i += QD_FSTATS_THREADS)
        if (sm[i]) atomicAdd(&hist[i], sm[i]);
    if (tid < 4) {
        const unsigned long long v = tid == 0 ? (blockIdx.x == 0 ? (unsigned long long)B : 0ull) : sm[3 * QD_FAULT_HIST + tid];
        if (v) atomicAdd(&counts[tid], v);
    }
    if (tid == 4 && sm[3 * QD_FAULT_HIST + 4] != ~0ull) atomicMin(best, sm[3 * QD_FAULT_HIST + 4]);
}

// The bitmap of the n faults goes to LDS where it fits beside the detector and observable bits, else to the (zeroed) global row
hipError_t qd_launch_sample_faults(const SpmatDev &Ht, const SpmatDev &Lt, const uint32_t *thr, uint64_t seed, int64_t shot0,
                                   const int64_t *shot_list, int64_t B, int m, int nobs, uint8_t *det, int64_t det_stride, uint8_t *obs,
                                   int64_t obs_stride, uint32_t *fault_bits, int64_t fault_stride, hipStream_t s)
{
    if (B == 0) return hipSuccess;
    const size_t lds = sizeof(uint32_t) * (size_t)(((m + 31) >> 5) + ((nobs + 31) >> 5));
    const size_t lds_faults = lds + sizeof(uint32_t) * (size_t)((Ht.nrows + 31) >> 5);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (lds_faults <= QD_SAMPLE_LDS_MAX)
        hipLaunchKernelGGL(qd_sample_dem_kernel<1>, dim3((unsigned)B), dim3(256), lds_faults, s, Ht, Lt, thr, k0, k1, shot0, shot_list, m, nobs,
                           det, det_stride, obs, obs_stride, fault_bits, fault_stride);
    else
        hipLaunchKernelGGL(qd_sample_dem_kernel<2>, dim3((unsigned)B), dim3(256), lds, s, Ht, Lt, thr, k0, k1, shot0, shot_list, m, nobs, det,
                           det_stride, obs, obs_stride, fault_bits, fault_stride);
    return hipGetLastError();
}

hipError_t qd_launch_commit_bits(const uint32_t *err, int64_t err_stride, int nbits, int64_t B, uint32_t *out, int64_t out_stride, int64_t out_bit0,
                                 hipStream_t s)
{
    if (B <= 0 || nbits <= 0) return hipSuccess;
    const int64_t total = B * (((out_bit0 + nbits + 31) >> 5) - (out_bit0 >> 5));
    const int64_t blocks = (total + QD_COMMIT_THREADS - 1) / QD_COMMIT_THREADS;
    hipLaunchKernelGGL(qd_commit_bits_kernel, dim3((unsigned)(blocks < QD_COMMIT_MAX_BLOCKS ? blocks : QD_COMMIT_MAX_BLOCKS)), dim3(QD_COMMIT_THREADS), 0, s,
                       err, err_stride, nbits, B, out, out_stride, out_bit0);
    return hipGetLastError();
}

hipError_t qd_launch_fault_stats(const uint32_t *faults, const uint32_t *corr, int64_t stride, int nbits, const uint8_t *residual, int64_t res_stride,
                                 int m, const uint64_t *fail_mask, int64_t B, int64_t shot0, int64_t *hist, int64_t *counts, uint64_t *best, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    const int64_t blocks = (B + QD_FSTATS_THREADS / QD_WAVE - 1) / (QD_FSTATS_THREADS / QD_WAVE);
    hipLaunchKernelGGL(qd_fault_stats_kernel, dim3((unsigned)(blocks < QD_FSTATS_MAX_BLOCKS ? blocks : QD_FSTATS_MAX_BLOCKS)), dim3(QD_FSTATS_THREADS), 0, s,
                       faults, corr, stride, nbits, residual, res_stride, m, reinterpret_cast<const unsigned long long *>(fail_mask), B, shot0,
                       reinterpret_cast<unsigned long long *>(hist), reinterpret_cast<unsigned long long *>(counts),
                       reinterpret_cast<unsigned long long *>(best));
    return hipGetLastError();
}

extern "C" int qd_sample_dem_faults(const qd_spmat *Ht, const qd_spmat *Lt, const double *priors, uint64_t seed, int64_t shot0, const int64_t *d_shots,
                                    int64_t B, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride, uint32_t *d_fault_bits,
                                    int64_t fault_stride_words, void *stream)
{
    if (B == 0) return QD_OK;
    if (B < 0 || B > INT32_MAX) return qd_fail(QD_EINVAL, "bad shot count (one workgroup per shot: at most 2^31 - 1 in one call)");
    if (!d_shots && shot0 < 0) return qd_fail(QD_EINVAL, "negative shot0");
    if (!d_fault_bits) return qd_fail(QD_EINVAL, "null fault rows");
    return qd_sample_dem_impl(Ht, Lt, priors, seed, d_shots ? 0 : shot0, d_shots, B, d_det, det_stride, d_obs, obs_stride, d_fault_bits,
                              fault_stride_words, stream);
}

extern "C" int qd_commit_bits(const uint32_t *d_err_bits, int64_t err_stride_words, int32_t nbits, int64_t B, uint32_t *d_out,
                              int64_t out_stride_words, int64_t out_bit0, void *stream)
{
    if (B < 0 || nbits < 0 || out_bit0 < 0) return qd_fail(QD_EINVAL, "negative shot count, bit count or bit offset");
    if (out_bit0 > INT64_MAX / 2) return qd_fail(QD_EINVAL, "bit offset too large");
    if (err_stride_words < ((int64_t)nbits + 31) / 32)
        return qd_fail(QD_EINVAL, "err_stride_words %lld is smaller than the %lld words of %d bits", (long long)err_stride_words,
                       (long long)(((int64_t)nbits + 31) / 32), nbits);
    if (out_stride_words < (out_bit0 + nbits + 31) / 32)
        return qd_fail(QD_EINVAL, "out_stride_words %lld is smaller than the %lld words that hold bits %lld .. %lld of a row", (long long)out_stride_words,
                       (long long)((out_bit0 + nbits + 31) / 32), (long long)out_bit0, (long long)(out_bit0 + nbits - 1));
    if (B == 0 || nbits == 0) return QD_OK;
    if (!d_err_bits || !d_out) return qd_fail(QD_EINVAL, "null error bits or output");
    HIP_TRY(qd_launch_commit_bits(d_err_bits, err_stride_words, nbits, B, d_out, out_stride_words, out_bit0, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

extern "C" int qd_fault_stats_batch(const uint32_t *d_faults, const uint32_t *d_corr, int64_t stride_words, int32_t nbits, const uint8_t *d_residual,
                                    int64_t res_stride, int32_t m, const uint64_t *d_fail_mask, int64_t B, int64_t shot0, int64_t *d_hist,
                                    int64_t *d_counts, uint64_t *d_best, void *stream)
{
    if (B == 0) return QD_OK;
    if (B < 0 || nbits < 0 || m < 0 || shot0 < 0) return qd_fail(QD_EINVAL, "negative shot count, bit count, detector count or shot0");
    if (shot0 > (1ll << 40) - B) return qd_fail(QD_EINVAL, "shot indices must stay below 2^40 (the low bits of the best word)");
    if (!d_faults || !d_corr || !d_fail_mask || !d_hist || !d_counts || !d_best) return qd_fail(QD_EINVAL, "null argument");
    if (m > 0 && !d_residual) return qd_fail(QD_EINVAL, "null residual");
    if (stride_words < ((int64_t)nbits + 31) / 32)
        return qd_fail(QD_EINVAL, "stride_words %lld is smaller than the %lld words of %d bits", (long long)stride_words, (long long)(((int64_t)nbits + 31) / 32), nbits);
    if (res_stride < m) return qd_fail(QD_EINVAL, "res_stride %lld is smaller than m = %d", (long long)res_stride, m);
    HIP_TRY(qd_launch_fault_stats(d_faults, d_corr, stride_words, nbits, d_residual, res_stride, m, d_fail_mask, B, shot0, d_hist, d_counts, d_best,
                                  reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}
