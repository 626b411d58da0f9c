// experiment.hip -- what a memory experiment keeps of a decoded batch (qd_shot_flags_fold, qd_tally_batch): a flag byte per shot folded
// from the windows' status words, and the tallies -- shots, failing shots, the same per flag, mismatches per observable -- plus one fail
// bit per shot.  Stands in for the host side of tests/test_sliding_window.py:83 of the reference (`pL = np.sum((pred != obs).any(axis=1)) / n`)
// and for what a user would compute from the status words with torch; nothing of a batch but these counters has to leave the device.
#include "../../include/quits_amd.h"
#include "qd_internal.h"
#include "qd_host.h"

#define QD_TALLY_THREADS 256
#define QD_TALLY_MAX_BLOCKS 1024        // the grid is bounded: every workgroup strides over the shots and flushes its sums once

// flags[b] |= the four facts of a window decode that a tally is broken down by.  One lane per shot.
__global__ void __launch_bounds__(256) qd_shot_flags_kernel(const int32_t *__restrict__ status, int64_t B, uint8_t *flags)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int32_t s = status[b];
    const uint32_t f = ((s & QD_STATUS_OSD) ? QD_SHOT_POST : 0u) | ((s & QD_STATUS_INCONSISTENT) ? QD_SHOT_INCONSISTENT : 0u) |
                       ((s & QD_STATUS_INEXACT) ? QD_SHOT_INEXACT : 0u) | ((s & QD_STATUS_COARSE_GRID) ? QD_SHOT_COARSE : 0u);
    if (f) flags[b] = (uint8_t)(flags[b] | f);
}

// One lane per shot, a wavefront = 64 consecutive shots = one word of the fail mask.  Every predicate is turned into a count by
// __ballot + popcount, i.e. per wavefront and in scalar registers; the head counters stay there over the whole stride loop, the k
// per-observable sums go to the workgroup's LDS (one ds_add by lane 0, and only for an observable that some shot of the wave missed).
// Global atomics: at most QD_TALLY_HEAD + k per workgroup, once, whatever B is.
__global__ void __launch_bounds__(QD_TALLY_THREADS) qd_tally_kernel(const uint8_t *__restrict__ pred, int64_t pred_stride,
                                                                    const uint8_t *__restrict__ obs, int64_t obs_stride, int k, int64_t B,
                                                                    const uint8_t *__restrict__ flags, unsigned long long *counts,
                                                                    unsigned long long *fail_mask)
{
    extern __shared__ __align__(16) unsigned long long tsm[];      // [QD_TALLY_HEAD + k]
    const int tid = threadIdx.x, lane = tid & (QD_WAVE - 1);
    for (int i = tid; i < QD_TALLY_HEAD + k; i += QD_TALLY_THREADS) tsm[i] = 0ull;
    __syncthreads();
    unsigned long long head[QD_TALLY_HEAD] = {};                    // wave-uniform; [0] (shots) is added by workgroup 0 at the end
    const int64_t step = (int64_t)gridDim.x * QD_TALLY_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * QD_TALLY_THREADS; base < B; base += step) {       // uniform in the workgroup
        const int64_t b = base + tid;
        const bool live = b < B;
        const uint8_t *p = pred + (live ? b : 0) * pred_stride, *o = obs + (live ? b : 0) * obs_stride;
        bool bad = false;
        for (int i = 0; i < k; ++i) {
            const bool x = live && ((p[i] ^ o[i]) & 1u);
            bad |= x;
            const unsigned long long m = __ballot(x);
            if (m && lane == 0) atomicAdd(&tsm[QD_TALLY_HEAD + i], (unsigned long long)__popcll(m));
        }
        const unsigned long long fm = __ballot(bad);
        head[1] += (unsigned long long)__popcll(fm);
        if (flags) {
            const uint32_t f = live ? flags[b] : 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long sm = __ballot((f >> j) & 1u);
                head[2 + 2 * j] += (unsigned long long)__popcll(sm);
                head[3 + 2 * j] += (unsigned long long)__popcll(sm & fm);
            }
        }
        if (fail_mask && lane == 0 && live) fail_mask[b >> 6] = fm;   // (base is a multiple of 64.)  Bits past B are zero: those lanes are not live
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 1; j < QD_TALLY_HEAD; ++j)
            if (head[j]) atomicAdd(&tsm[j], head[j]);
    }
    __syncthreads();
    for (int i = tid; i < QD_TALLY_HEAD + k; i += QD_TALLY_THREADS) {
        const unsigned long long v = i == 0 ? (blockIdx.x == 0 ? (unsigned long long)B : 0ull) : tsm[i];
        if (v) atomicAdd(&counts[i], v);
    }
}

hipError_t qd_launch_shot_flags(const int32_t *status, int64_t B, uint8_t *flags, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(qd_shot_flags_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, status, B, flags);
    return hipGetLastError();
}

hipError_t qd_launch_tally(const uint8_t *pred, int64_t pred_stride, const uint8_t *obs, int64_t obs_stride, int k, int64_t B,
                           const uint8_t *flags, int64_t *counts, uint64_t *fail_mask, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    const int64_t blocks = (B + QD_TALLY_THREADS - 1) / QD_TALLY_THREADS;
    const size_t lds = sizeof(unsigned long long) * (size_t)(QD_TALLY_HEAD + k);
    hipLaunchKernelGGL(qd_tally_kernel, dim3((unsigned)(blocks < QD_TALLY_MAX_BLOCKS ? blocks : QD_TALLY_MAX_BLOCKS)), dim3(QD_TALLY_THREADS), lds, s,
                       pred, pred_stride, obs, obs_stride, k, B, flags, reinterpret_cast<unsigned long long *>(counts),
                       reinterpret_cast<unsigned long long *>(fail_mask));
    return hipGetLastError();
}
