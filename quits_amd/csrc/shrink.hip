// shrink.hip -- the step of the fault-set shrinker between two decodes (qd_shrink_begin, qd_shrink_step; the definition and its numpy mirror are
// quits_amd/shrink.py).  A parent is a failing fault set S that loses one fault per accepted trial; a trial is the detector row H (S \ {j}) and the
// observable row L (S \ {j}), which the caller decodes like any sampled shot and answers with one verdict bit (qd_tally_batch's fail mask over the
// live list).  Everything per parent stays in caller-owned device memory: the packed set, H S and L S as bytes (a trial row is that row with the
// bytes of column j flipped -- column j is row j of the CSR of H^T / L^T that the DEM sampler uses -- never a fresh product over the set), and
// QD_SHRINK_STATE words of state.  One wavefront per live parent; no scratch, 16 words of LDS in the compaction and none elsewhere.
#include "../../include/quits_amd.h"
#include "qd_internal.h"
#include "qd_host.h"

#define QD_SHRINK_THREADS 256                          // four wavefronts = four parents per workgroup
#define QD_SHRINK_WAVES (QD_SHRINK_THREADS / QD_WAVE)
#define QD_SHRINK_COMPACT_THREADS 1024

enum { ST_LAST = 0, ST_QUIET = 1, ST_W = 2, ST_TRIALS = 3, ST_FLAGS = 4, ST_CUR = 5, ST_W0 = 6 };

// The first member of the packed set S at or above bit `from`, or -1: lanes stride over the row's words (coalesced), the first word masked below
// `from`, the last one above n; a ballot picks the first lane that holds a set bit, then its lowest bit.  `cleared` (or -1) is a bit this
// wavefront has just cleared in memory: it is cleared in the register too, so the answer does not depend on whether the load sees the store.
__device__ __forceinline__ int shrink_first_member(const uint32_t *__restrict__ S, int n, int from, int cleared, int lane)
{
    const int nwords = (n + 31) >> 5;
    const uint32_t last_mask = (n & 31) ? (1u << (n & 31)) - 1u : 0xFFFFFFFFu;
    const int w0 = from >> 5;
    for (int base = w0; base < nwords; base += QD_WAVE) {          // uniform in the wavefront
        const int wi = base + lane;
        uint32_t v = 0u;
        if (wi < nwords) {
            v = S[wi];
            if (wi == nwords - 1) v &= last_mask;
            if (wi == w0) v &= 0xFFFFFFFFu << (from & 31);
            if (cleared >= 0 && wi == (cleared >> 5)) v &= ~(1u << (cleared & 31));
        }
        const unsigned long long bal = __ballot(v != 0u);
        if (bal) {
            const int src = __ffsll((long long)bal) - 1;
            const uint32_t vv = (uint32_t)__shfl((int)v, src);
            return 32 * (base + src) + __ffs((int)vv) - 1;
        }
    }
    return -1;
}

// Start-up, one wavefront per parent: the padding bits of the set's last word are cleared, w = |E| is counted, the state is that of the
// definition before trial 0 (pending fault -1) and the live list is 0 .. P - 1.
__global__ void __launch_bounds__(QD_SHRINK_THREADS) qd_shrink_init_kernel(uint32_t *sets, int64_t set_stride, int n, int64_t P, int32_t *state,
                                                                           int32_t *live, int32_t *count)
{
    const int lane = threadIdx.x & (QD_WAVE - 1);
    const int64_t p = (int64_t)blockIdx.x * QD_SHRINK_WAVES + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = (int32_t)P;
    if (p >= P) return;
    uint32_t *S = sets + p * set_stride;
    const int nwords = (n + 31) >> 5;
    int w = 0;
    for (int wi = lane; wi < nwords; wi += QD_WAVE) {
        uint32_t v = S[wi];
        if (wi == nwords - 1 && (n & 31)) {
            const uint32_t kept = v & ((1u << (n & 31)) - 1u);
            if (kept != v) S[wi] = kept;
            v = kept;
        }
        w += __popc(v);
    }
#pragma unroll
    for (int d = QD_WAVE / 2; d >= 1; d >>= 1) w += __shfl_xor(w, d);
    if (lane < QD_SHRINK_STATE) {
        const int32_t v = lane == ST_LAST || lane == ST_CUR ? -1 : (lane == ST_W || lane == ST_W0 ? w : 0);
        state[p * QD_SHRINK_STATE + lane] = v;
    }
    if (lane == 0) live[p] = (int32_t)p;
}

// Apply, one wavefront per row i of the previous round's live list: read the verdict bit, update the parent as the definition says (an accepted
// trial clears bit j of the set and flips the bytes of column j in the kept H S and L S -- the indices of a CSR row are distinct, so no two lanes
// touch one byte), end the parent or find its next fault.  The pending fault goes to the state; the emit kernel reads it from there.
__global__ void __launch_bounds__(QD_SHRINK_THREADS) qd_shrink_apply_kernel(SpmatDev Ht, SpmatDev Lt, uint32_t *sets, int64_t set_stride, int64_t P,
                                                                            int32_t *state, const int32_t *__restrict__ live, int64_t A,
                                                                            const unsigned long long *__restrict__ fail_mask, uint8_t *hs,
                                                                            int64_t hs_stride, uint8_t *ls, int64_t ls_stride)
{
    const int lane = threadIdx.x & (QD_WAVE - 1);
    const int64_t i = (int64_t)blockIdx.x * QD_SHRINK_WAVES + (threadIdx.x >> 6);
    if (i >= A) return;
    const int p = __builtin_amdgcn_readfirstlane(live[i]);
    if (p < 0 || p >= P) return;
    const bool verdict = (fail_mask[i >> 6] >> (i & 63)) & 1ull;
    int32_t *st = state + (int64_t)p * QD_SHRINK_STATE;
    const int n = Ht.nrows;
    int last = __builtin_amdgcn_readfirstlane(st[ST_LAST]), quiet = __builtin_amdgcn_readfirstlane(st[ST_QUIET]);
    int w = __builtin_amdgcn_readfirstlane(st[ST_W]), flags = __builtin_amdgcn_readfirstlane(st[ST_FLAGS]);
    int cur = __builtin_amdgcn_readfirstlane(st[ST_CUR]);
    const int trials = __builtin_amdgcn_readfirstlane(st[ST_TRIALS]) + 1;
    if ((flags & QD_SHRINK_ENDED) || cur >= n) return;                 // (not on the live list of a consistent state)
    uint32_t *S = sets + (int64_t)p * set_stride;
    int cleared = -1;
    if (cur < 0) {                                                     // trial 0: the parent itself
        if (verdict) flags |= QD_SHRINK_FAILS;
        else flags |= QD_SHRINK_ENDED;
    } else {
        if (verdict) {
            cleared = cur;
            w -= 1;
            quiet = 0;
            if (lane == 0) S[cur >> 5] &= ~(1u << (cur & 31));
            uint8_t *h = hs + (int64_t)p * hs_stride, *l = ls + (int64_t)p * ls_stride;
            for (uint32_t x = Ht.row_ptr[cur] + lane; x < Ht.row_ptr[cur + 1]; x += QD_WAVE) h[Ht.col_idx[x]] ^= 1u;
            for (uint32_t x = Lt.row_ptr[cur] + lane; x < Lt.row_ptr[cur + 1]; x += QD_WAVE) l[Lt.col_idx[x]] ^= 1u;
        } else
            quiet += 1;
        last = cur;
    }
    if (!(flags & QD_SHRINK_ENDED)) {
        if (quiet >= w)
            flags |= QD_SHRINK_MINIMAL | QD_SHRINK_ENDED;
        else {
            int j = last + 1 < n ? shrink_first_member(S, n, last + 1, cleared, lane) : -1;
            if (j < 0) j = shrink_first_member(S, n, 0, cleared, lane);            // wrap: the smallest member
            if (j < 0) flags |= QD_SHRINK_ENDED;                       // (w > 0 says the set has a member: not reached)
            else cur = j;
        }
    }
    if (lane == 0) {
        st[ST_LAST] = last;
        st[ST_QUIET] = quiet;
        st[ST_W] = w;
        st[ST_TRIALS] = trials;
        st[ST_FLAGS] = flags;
        st[ST_CUR] = cur;
    }
}

// Compaction, one workgroup: the rows of `live` whose parent has not ended, in the same (ascending parent) order, and their number.  Every
// thread owns a contiguous piece of the list; the pieces' counts are scanned with shuffles inside a wavefront and 16 words of LDS across them.
__global__ void __launch_bounds__(QD_SHRINK_COMPACT_THREADS) qd_shrink_compact_kernel(const int32_t *__restrict__ state, int64_t P,
                                                                                      const int32_t *__restrict__ live, int64_t A,
                                                                                      int32_t *__restrict__ live_next, int32_t *count)
{
    __shared__ int wsum[QD_SHRINK_COMPACT_THREADS / QD_WAVE];
    const int tid = threadIdx.x, lane = tid & (QD_WAVE - 1), wv = tid >> 6;
    const int64_t per = (A + QD_SHRINK_COMPACT_THREADS - 1) / QD_SHRINK_COMPACT_THREADS;
    const int64_t lo = tid * per < A ? tid * per : A, hi = lo + per < A ? lo + per : A;
    int c = 0;
    for (int64_t i = lo; i < hi; ++i) {
        const int p = live[i];
        c += p >= 0 && p < P && !(state[(int64_t)p * QD_SHRINK_STATE + ST_FLAGS] & QD_SHRINK_ENDED);
    }
    int incl = c;
#pragma unroll
    for (int d = 1; d < QD_WAVE; d <<= 1) {
        const int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    if (lane == QD_WAVE - 1) wsum[wv] = incl;
    __syncthreads();
    int offset = 0, total = 0;
    for (int k = 0; k < QD_SHRINK_COMPACT_THREADS / QD_WAVE; ++k) {
        if (k < wv) offset += wsum[k];
        total += wsum[k];
    }
    int64_t pos = offset + incl - c;
    for (int64_t i = lo; i < hi; ++i) {
        const int p = live[i];
        if (p >= 0 && p < P && !(state[(int64_t)p * QD_SHRINK_STATE + ST_FLAGS] & QD_SHRINK_ENDED)) live_next[pos++] = p;
    }
    if (tid == 0) *count = total;
}

// Emit, one wavefront per row i of the new live list (the launch covers the old one; rows past *count return): the trial's detector and observable
// rows, each byte written once and complete by the lane that owns it -- the kept byte, flipped if the pending fault's column holds that row --
// and the trial's fault and parent.  A fault whose column is empty leaves the kept rows as they are.
__global__ void __launch_bounds__(QD_SHRINK_THREADS) qd_shrink_emit_kernel(SpmatDev Ht, SpmatDev Lt, int64_t P, const int32_t *__restrict__ state,
                                                                           const int32_t *__restrict__ live, const int32_t *__restrict__ count,
                                                                           const uint8_t *__restrict__ hs, int64_t hs_stride,
                                                                           const uint8_t *__restrict__ ls, int64_t ls_stride, uint8_t *det,
                                                                           int64_t det_stride, uint8_t *obs, int64_t obs_stride, int32_t *fault,
                                                                           int32_t *parent)
{
    const int lane = threadIdx.x & (QD_WAVE - 1);
    const int64_t i = (int64_t)blockIdx.x * QD_SHRINK_WAVES + (threadIdx.x >> 6);
    if (i >= *count) return;
    const int p = __builtin_amdgcn_readfirstlane(live[i]);
    if (p < 0 || p >= P) return;
    int j = __builtin_amdgcn_readfirstlane(state[(int64_t)p * QD_SHRINK_STATE + ST_CUR]);
    if (j >= Ht.nrows) j = -1;
    const int m = Ht.ncols, k = Lt.ncols;
    const uint32_t h0 = j >= 0 ? Ht.row_ptr[j] : 0u, h1 = j >= 0 ? Ht.row_ptr[j + 1] : 0u;
    const uint32_t l0 = j >= 0 ? Lt.row_ptr[j] : 0u, l1 = j >= 0 ? Lt.row_ptr[j + 1] : 0u;
    const uint8_t *h = hs + (int64_t)p * hs_stride, *l = ls + (int64_t)p * ls_stride;
    uint8_t *d = det + i * det_stride, *o = obs + i * obs_stride;
    for (int r = lane; r < m; r += QD_WAVE) {
        uint32_t v = h[r];
        for (uint32_t x = h0; x < h1; ++x) v ^= Ht.col_idx[x] == (uint32_t)r ? 1u : 0u;
        d[r] = (uint8_t)v;
    }
    for (int r = lane; r < k; r += QD_WAVE) {
        uint32_t v = l[r];
        for (uint32_t x = l0; x < l1; ++x) v ^= Lt.col_idx[x] == (uint32_t)r ? 1u : 0u;
        o[r] = (uint8_t)v;
    }
    if (lane == 0) {
        fault[i] = j;
        parent[i] = p;
    }
}

static unsigned shrink_blocks(int64_t rows) { return (unsigned)((rows + QD_SHRINK_WAVES - 1) / QD_SHRINK_WAVES); }

static int shrink_check(const qd_spmat *Ht, const qd_spmat *Lt, const void *d_sets, int64_t set_stride_words, int64_t P, const void *d_state,
                        const void *d_count, const void *d_hs, int64_t hs_stride, const void *d_ls, int64_t ls_stride, const void *d_det,
                        int64_t det_stride, const void *d_obs, int64_t obs_stride, const void *d_fault, const void *d_parent)
{
    if (!Ht || !Lt) return qd_fail(QD_EINVAL, "null matrix");
    if (Ht->d.nrows != Lt->d.nrows) return qd_fail(QD_EINVAL, "Ht has %d rows and Lt %d: both must have one row per fault", Ht->d.nrows, Lt->d.nrows);
    if (Ht->device != Lt->device) return qd_fail(QD_EINVAL, "Ht and Lt live on different devices");
    if (P < 0 || P > INT32_MAX) return qd_fail(QD_EINVAL, "bad parent count %lld (at most 2^31 - 1)", (long long)P);
    const int n = Ht->d.nrows, m = Ht->d.ncols, k = Lt->d.ncols;
    if (set_stride_words < ((int64_t)n + 31) / 32)
        return qd_fail(QD_EINVAL, "set_stride_words %lld is smaller than the %lld words of %d faults", (long long)set_stride_words, (long long)(((int64_t)n + 31) / 32), n);
    if (hs_stride < m || det_stride < m)
        return qd_fail(QD_EINVAL, "detector row strides %lld (kept) and %lld (trial) must be at least m = %d", (long long)hs_stride, (long long)det_stride, m);
    if (ls_stride < k || obs_stride < k)
        return qd_fail(QD_EINVAL, "observable row strides %lld (kept) and %lld (trial) must be at least k = %d", (long long)ls_stride, (long long)obs_stride, k);
    if (P == 0) return QD_OK;
    if (!d_sets || !d_state || !d_count || !d_fault || !d_parent || (m > 0 && (!d_hs || !d_det)) || (k > 0 && (!d_ls || !d_obs)))
        return qd_fail(QD_EINVAL, "null argument");
    return QD_OK;
}

extern "C" int qd_shrink_begin(const qd_spmat *Ht, const qd_spmat *Lt, uint32_t *d_sets, int64_t set_stride_words, int64_t P, int32_t *d_state,
                               int32_t *d_live, int32_t *d_count, const uint8_t *d_hs, int64_t hs_stride, const uint8_t *d_ls, int64_t ls_stride,
                               uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride, int32_t *d_fault, int32_t *d_parent,
                               void *stream)
{
    const int rc = shrink_check(Ht, Lt, d_sets, set_stride_words, P, d_state, d_count, d_hs, hs_stride, d_ls, ls_stride, d_det, det_stride, d_obs,
                                obs_stride, d_fault, d_parent);
    if (rc) return rc;
    if (!d_count) return qd_fail(QD_EINVAL, "null live count");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(Ht->device));
    if (P == 0) {
        HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(int32_t), s));
        return QD_OK;
    }
    if (!d_live) return qd_fail(QD_EINVAL, "null live list");
    hipLaunchKernelGGL(qd_shrink_init_kernel, dim3(shrink_blocks(P)), dim3(QD_SHRINK_THREADS), 0, s, d_sets, set_stride_words, Ht->d.nrows, P, d_state,
                       d_live, d_count);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(qd_shrink_emit_kernel, dim3(shrink_blocks(P)), dim3(QD_SHRINK_THREADS), 0, s, Ht->d, Lt->d, P, d_state, d_live, d_count, d_hs,
                       hs_stride, d_ls, ls_stride, d_det, det_stride, d_obs, obs_stride, d_fault, d_parent);
    HIP_TRY(hipGetLastError());
    return QD_OK;
}

extern "C" int qd_shrink_step(const qd_spmat *Ht, const qd_spmat *Lt, uint32_t *d_sets, int64_t set_stride_words, int64_t P, int32_t *d_state,
                              const int32_t *d_live, int64_t A, const uint64_t *d_fail_mask, int32_t *d_live_next, int32_t *d_count, uint8_t *d_hs,
                              int64_t hs_stride, uint8_t *d_ls, int64_t ls_stride, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs,
                              int64_t obs_stride, int32_t *d_fault, int32_t *d_parent, void *stream)
{
    const int rc = shrink_check(Ht, Lt, d_sets, set_stride_words, P, d_state, d_count, d_hs, hs_stride, d_ls, ls_stride, d_det, det_stride, d_obs,
                                obs_stride, d_fault, d_parent);
    if (rc) return rc;
    if (A < 0 || A > P) return qd_fail(QD_EINVAL, "%lld live rows of %lld parents", (long long)A, (long long)P);
    if (!d_count) return qd_fail(QD_EINVAL, "null live count");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(Ht->device));
    if (A == 0) {
        HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(int32_t), s));
        return QD_OK;
    }
    if (!d_live || !d_live_next || !d_fail_mask) return qd_fail(QD_EINVAL, "null live list or fail mask");
    if (d_live == d_live_next) return qd_fail(QD_EINVAL, "the live list is compacted out of place: d_live_next must not be d_live");
    hipLaunchKernelGGL(qd_shrink_apply_kernel, dim3(shrink_blocks(A)), dim3(QD_SHRINK_THREADS), 0, s, Ht->d, Lt->d, d_sets, set_stride_words, P, d_state,
                       d_live, A, reinterpret_cast<const unsigned long long *>(d_fail_mask), d_hs, hs_stride, d_ls, ls_stride);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(qd_shrink_compact_kernel, dim3(1), dim3(QD_SHRINK_COMPACT_THREADS), 0, s, d_state, P, d_live, A, d_live_next, d_count);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(qd_shrink_emit_kernel, dim3(shrink_blocks(A)), dim3(QD_SHRINK_THREADS), 0, s, Ht->d, Lt->d, P, d_state, d_live_next, d_count, d_hs,
                       hs_stride, d_ls, ls_stride, d_det, det_stride, d_obs, obs_stride, d_fault, d_parent);
    HIP_TRY(hipGetLastError());
    return QD_OK;
}
