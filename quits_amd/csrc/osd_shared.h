// osd_shared.h -- pieces shared by the OSD kernels (osd_kernels.hip: row-form / column-form kernels; osd_sr.hip: the
// OSD-0 kernel with simultaneous singleton pivots): key order, workgroup sums, the lazily drawn column order.
#pragma once
#include "qd_internal.h"

#define QD_NOKEY 0xFFFFFFFFu

#ifdef QD_OSD_TIMING
// phase timers accumulate in registers and are flushed once per shot (a global atomic per tick would stall every
// following barrier on vmcnt(0) and measure itself)
#define QD_TICK(slot)                                                                   \
    {                                                                                   \
        const unsigned long long now_ = wall_clock64();                                 \
        acc_[slot] += now_ - tick_;                                                     \
        tick_ = now_;                                                                   \
    }
#else
#define QD_TICK(slot)
#endif

__device__ __forceinline__ uint64_t &qd_qword(uint64_t *q_lds, uint64_t *q_glb, int kw_lds, int m_pad, int w, int r)
{
    return (w < kw_lds) ? q_lds[(size_t)w * m_pad + r] : q_glb[(size_t)(w - kw_lds) * m_pad + r];
}

__device__ __forceinline__ uint32_t qd_mono_key(float llr)
{
    const float f = llr + 0.0f;                    // -0 -> +0, so that +-0 tie on the index like the oracle's '<'
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // monotone float -> unsigned
}

template <int T>
__device__ __forceinline__ void qd_bitonic_u64(uint64_t *buf, int P, int tid)
{
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int pi = tid; pi < (P >> 1); pi += T) {
                const int i = ((pi & ~(j - 1)) << 1) | (pi & (j - 1));
                const int l = i | j;
                const uint64_t x = buf[i], y = buf[l];
                const bool up = ((i & k) == 0);
                if ((x > y) == up) { buf[i] = y; buf[l] = x; }
            }
            __syncthreads();
        }
}

// One kernel, no restarts: the column order is produced lazily in TIERS of <= QD_OSD_TIER columns (the next-smallest keys,
// found by bisecting on the key value), each tier is bitonic-sorted and eliminated before the next one is drawn; the
// elimination state survives between tiers.  A thread owns RPT rows and keeps their batch image, syndrome bit, pivot flag
// and the first QD_OSD_KWR Q planes in registers; LDS holds a write-through mirror that other threads read when one of
// those rows becomes the pivot row.  Q planes beyond the LDS budget spill to HBM (rare: > 64 * f_kw pivots).
#define QD_OSD_TIER 1024
#define QD_OSD_TIER_FIRST 256
#define QD_OSD_KWR 6
#define QD_OSD_KWR0 2
#define QD_OSD_KPT 1      // monotone keys a thread keeps in registers while a tier is drawn (windows with n <= KPT * T; else re-read).
                          // (20, i.e. every key of the headline window held in registers, was the round-1 choice: see qd_osd_draw_tier)

// Sum of v over the workgroup; one barrier; `buf` = 2 x 64 words alternating with `phase` (entries beyond the wave count must be zero).
template <int T>
__device__ __forceinline__ uint32_t qd_block_sum(uint32_t v, uint32_t *buf, int &phase)
{
    constexpr int NW = T / 64;
    v = qd_wave_add(v);
    if ((threadIdx.x & 63) == 0) buf[phase * 64 + (threadIdx.x >> 6)] = v;     // 64-word stride: the 3-way counter of the tier search shares these buffers
    __syncthreads();
    const uint4 *p4 = reinterpret_cast<const uint4 *>(buf + phase * 64);
    uint32_t tot = 0;
#pragma unroll
    for (int w = 0; w < (NW + 3) / 4; ++w) { const uint4 x = p4[w]; tot += x.x + x.y + x.z + x.w; }
    phase ^= 1;
    return tot;
}

// Only what this kernel needs, so the scalar registers are not flooded with three full descriptor structs.
struct OsdRegArgs {
    int m, n, m_pad, n_pad, max_cdeg, mw, f_kw, out_words, upd_rows;
    int off[10], off_sort, off_order, off_pivmask, off_npl;
    int osd_w;                  // 0 = OSD-0 (early stop), 1 = combination sweep, 2 = exhaustive
    int osd_order, rank;
    const uint32_t *wfix;       // [n] round(log(1/p_j) * 2^18): candidate cost per fault
    const uint32_t *bit_slot_of;// [n] fault -> bit slot (row of llr_ws)
    const uint32_t *csc_ptr;
    const uint16_t *csc_row;
    const uint32_t *bit_orig;
    const uint8_t *det, *upd;
    int64_t det_stride, det_offset, upd_stride;
    const float *llr_ws;
    const int32_t *fail_list, *fail_count;
    const int32_t *slot_list, *slot_count;      // when set: only these fail-list slots (a subset handed over by an earlier pass)
    uint64_t *q_spill_fast;
    uint64_t *mt_ws;
    uint32_t *err_bits;
    int32_t *status;
    unsigned long long *dbg;
};

struct TierState {
    uint32_t lo_key, lo_idx; int sphase, exhausted, limit;    // limit: tier size wanted (<= QD_OSD_TIER)
    // guess (in, 0: none): an upper key bound to try first -- every key in [lo_key, guess) is gathered in ONE pass over the posteriors; if that is between
    // 1 and `limit` columns it IS the tier (any cut gives a valid tier: the elimination depends on the column order, not on where tiers end), otherwise the
    // radix selection below runs as before.  A tier's cut moves little from shot to shot, so the caller carries it (cut / count, out).
    uint32_t guess = 0u, cut = 0u, count = 0u;
};

// Draws the next tier: the <= QD_OSD_TIER not yet consumed columns with the smallest (key, fault index), sorted, as fault
// indices in order[0..cnt).  State: every column with (key, index) < (lo_key, lo_idx) has been consumed.
// KPT = monotone keys a thread keeps in registers while the tier is drawn (used when n <= KPT * T; otherwise, and always with
// KPT = 1 on windows of more than T faults, every radix level and the gather re-read the posteriors, which sit in L2).
template <int T, int KPT = QD_OSD_KPT, class ARGS = OsdRegArgs, int SCAN = 0>     // ARGS: anything with n and bit_orig; SCAN: 16-byte loads in flight per pass over the posteriors (0: one float at a time)
__device__ __forceinline__ int qd_osd_draw_tier(const ARGS &a, const float *llr, uint64_t *sortbuf, uint16_t *order,
                                             uint32_t *red, uint32_t *sumbuf, TierState &ts)
{
    const int tid = threadIdx.x;
    const int n = a.n;
    const bool in_regs = n <= KPT * T;
    uint32_t lo_key = ts.lo_key, lo_idx = ts.lo_idx;
    int sphase = ts.sphase;
    const uint32_t lim = (uint32_t)ts.limit;
    bool exhausted = false;
    int cnt = 0;
    {
            uint32_t kreg[KPT];
            if (in_regs) {
#pragma unroll
                for (int i = 0; i < KPT; ++i) {
                    const int b = tid + i * T;
                    kreg[i] = (b < n) ? qd_mono_key(llr[b]) : 0xFFFFFFFFu;
                }
            }
            // One pass over the posteriors (L2).  SCAN > 0: 16-byte loads, SCAN of them in flight per thread before the first is used -- a
            // plain loop waits for every load in turn (~19 L2 round trips per pass at the headline window: most of what a tier used to
            // cost).  The register kernels of osd_kernels.hip keep the plain loop: they are at their register budget already.
            auto scan_keys = [&](auto fn) {                                    // fn(monotone key, bit slot)
                if constexpr (SCAN == 0) {
                    for (int b = tid; b < n; b += T) fn(qd_mono_key(llr[b]), b);
                } else {
                    const float4 *l4 = reinterpret_cast<const float4 *>(llr);  // rows of llr_ws start on 256-byte boundaries (n_pad = 64 k)
                    const int n4 = n >> 2;
                    for (int b0 = 0; b0 < n4; b0 += SCAN * T) {
                        float4 v[SCAN > 0 ? SCAN : 1];
#pragma unroll
                        for (int u = 0; u < SCAN; ++u) {
                            const int b4 = b0 + u * T + tid;
                            v[u] = l4[b4 < n4 ? b4 : 0];
                        }
#pragma unroll
                        for (int u = 0; u < SCAN; ++u) {
                            const int b4 = b0 + u * T + tid;
                            if (b4 < n4) {
                                fn(qd_mono_key(v[u].x), 4 * b4); fn(qd_mono_key(v[u].y), 4 * b4 + 1);
                                fn(qd_mono_key(v[u].z), 4 * b4 + 2); fn(qd_mono_key(v[u].w), 4 * b4 + 3);
                            }
                        }
                    }
                    for (int b = (n4 << 2) + tid; b < n; b += T) fn(qd_mono_key(llr[b]), b);
                }
            };
            // tie group at key == lo_key that is only partly consumed (or too big for one tier): ordered by fault index;
            // rare, so it simply re-reads the LLRs and fault indices
            auto count_ties = [&](uint32_t key, uint32_t ilo, uint32_t ihi) -> uint32_t {
                uint32_t c = 0;
                for (int b = tid; b < n; b += T)
                    if (qd_mono_key(llr[b]) == key) { const uint32_t j = a.bit_orig[b]; c += (j >= ilo && j < ihi) ? 1u : 0u; }
                return qd_block_sum<T>(c, sumbuf, sphase);
            };
            bool by_index = false;
            uint32_t t_lo = lo_key, t_hi = lo_key, i_lo = 0, i_hi = 0;
            if (lo_idx > 0) {
                if (count_ties(lo_key, lo_idx, 0xFFFFFFFFu) > 0) by_index = true;
                else { lo_key += 1; lo_idx = 0; }
            }
            // the guess first (TierState::guess): the gather below runs with [lo_key, guess) as the cut; if that is not 1..lim columns the selection runs and
            // the gather is repeated (one instance of the pass over the posteriors serves both)
            bool spec = !by_index && !in_regs && ts.guess > lo_key;
            for (;;) {
            if (spec) { t_lo = lo_key; t_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)ts.guess); }
            else {
            if (!by_index) {
                // largest bin boundary t_hi with  #{lo_key <= key < t_hi} <= lim   (key 0xFFFFFFFF is reserved for "no
                // column").  Radix selection: a histogram of the keys over 2048 bins of 2^21 (one LDS atomic per key), a scan
                // for the bin where the running count passes `lim`; when the cut in front of that bin would leave a thin tier,
                // the bin itself is resolved with 2048 bins of 2^10, then 1024 bins of 1.
                uint32_t *hist = reinterpret_cast<uint32_t *>(sortbuf);            // 8 KB, free until the gather
                uint32_t base = 0u, cur_lo = lo_key, cum = 0u;
                uint64_t thi64 = 0;
                for (int level = 0; level < 3; ++level) {
                    const int shift = level == 0 ? 21 : (level == 1 ? 10 : 0);
                    const int nb = level == 2 ? 1024 : 2048;
                    for (int i = tid; i < nb; i += T) hist[i] = 0u;
                    __syncthreads();
                    auto tally = [&](uint32_t u) {
                        if (u != 0xFFFFFFFFu && u >= cur_lo) {
                            const uint32_t bin = (u - base) >> shift;              // cur_lo >= base
                            if (bin < (uint32_t)nb) atomicAdd(&hist[bin], 1u);
                        }
                    };
                    if (in_regs) {
#pragma unroll
                        for (int i = 0; i < KPT; ++i) tally(kreg[i]);
                    } else {
                        scan_keys([&](uint32_t u, int) { tally(u); });
                    }
                    __syncthreads();
                    // every thread owns nb / T consecutive bins; exclusive prefix over the workgroup
                    const int per = nb / T;                                        // 2..8
                    uint32_t h[8], mysum = 0u;
#pragma unroll
                    for (int q = 0; q < 8; ++q) { h[q] = (q < per) ? hist[tid * per + q] : 0u; mysum += h[q]; }
                    uint32_t incl = mysum;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d); if ((tid & 63) >= d) incl += o; }
                    uint32_t *buf = sumbuf + sphase * 64;
                    if ((tid & 63) == 63) buf[tid >> 6] = incl;
                    if (tid == 0) { buf[32] = 0xFFFFFFFFu; }                       // first overflowing bin (minimum over threads)
                    __syncthreads();
                    uint32_t before = cum;
                    for (int w = 0; w < (tid >> 6); ++w) before += buf[w];
                    uint32_t run = before + incl - mysum;                          // keys in [lo_key, first key of my first bin)
                    int kk = -1;
                    uint32_t run_at = 0u;
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (q < per && kk < 0) { if (run + h[q] > lim) { kk = tid * per + q; run_at = run; } else run += h[q]; }
                    if (kk >= 0) atomicMin(&buf[32], (uint32_t)kk);
                    __syncthreads();
                    const uint32_t kmin = buf[32];
                    if (kk >= 0 && (uint32_t)kk == kmin) buf[33] = run_at;         // exactly one thread owns that bin
                    if (kmin == 0xFFFFFFFFu && tid == T - 1) buf[33] = run;        // nothing overflows: everything fits
                    __syncthreads();
                    const uint32_t k = (kmin == 0xFFFFFFFFu) ? (uint32_t)nb : kmin;
                    const uint32_t cnt_here = buf[33];
                    sphase ^= 1;
                    thi64 = (uint64_t)base + ((uint64_t)k << shift);
                    cnt = (int)cnt_here;
                    if (k == (uint32_t)nb || cnt_here >= lim / 4u || level == 2) break;
                    // descend into the overflowing bin
                    base = (uint32_t)thi64; cum = cnt_here; cur_lo = max(cur_lo, base);
                }
                __syncthreads();                                                   // hist (= sortbuf) is reused by the gather
                t_lo = lo_key; t_hi = thi64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)thi64;
                if (cnt > 0) { ts.cut = t_hi; ts.count = (uint32_t)cnt; }
                if (cnt == 0) {
                    if (t_hi == 0xFFFFFFFFu) exhausted = true;                 // nothing at or above lo_key
                    else { lo_key = t_hi; lo_idx = 0; by_index = true; }       // more than `lim` columns share the next key value
                } else lo_key = t_hi;
            }
            if (by_index) {
                uint64_t L = lo_idx, H = (uint64_t)n;
                uint32_t cntL = 0;
                while (L < H) {
                    const uint64_t mid = (L + H + 1) >> 1;
                    const uint32_t c = count_ties(lo_key, lo_idx, (uint32_t)mid);
                    if (c <= lim) { L = mid; cntL = c; } else H = mid - 1;
                }
                i_lo = lo_idx; i_hi = (uint32_t)L;
                cnt = (int)cntL;
                t_lo = lo_key;
                if (i_hi >= (uint32_t)n) { lo_key += 1; lo_idx = 0; } else lo_idx = i_hi;
            }
            if (exhausted) { ts.lo_key = lo_key; ts.lo_idx = lo_idx; ts.sphase = sphase; ts.exhausted = 1; return 0; }
            }
            // gather and sort the tier
            if (tid == 0) red[80] = 0u;
            __syncthreads();
            if (in_regs && !by_index) {
                // keys are in registers: count the takes, one workgroup scan for the write offsets (order inside the tier
                // buffer is irrelevant, it is sorted next)
                uint32_t mask = 0u;
#pragma unroll
                for (int i = 0; i < KPT; ++i) mask |= (kreg[i] >= t_lo && kreg[i] < t_hi) ? (1u << i) : 0u;
                const uint32_t mine = (uint32_t)__popc(mask);
                uint32_t incl = mine;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d); if ((tid & 63) >= d) incl += o; }
                uint32_t *buf = sumbuf + sphase * 64;
                if ((tid & 63) == 63) buf[tid >> 6] = incl;
                __syncthreads();
                uint32_t at = incl - mine;
                for (int w = 0; w < (tid >> 6); ++w) at += buf[w];
                sphase ^= 1;
#pragma unroll
                for (int i = 0; i < KPT; ++i)
                    if ((mask >> i) & 1u) sortbuf[at++] = ((uint64_t)kreg[i] << 32) | a.bit_orig[tid + i * T];
            } else
            scan_keys([&](uint32_t u, int b) {
                // (one LDS counter bump per taken column: a tier takes a few hundred of the n columns)
                bool take = false;
                uint32_t j = 0;
                if (by_index) { if (u == t_lo) { j = a.bit_orig[b]; take = (j >= i_lo && j < i_hi); } }
                else if (u >= t_lo && u < t_hi) { j = a.bit_orig[b]; take = true; }
                if (take) {
                    const uint32_t at = atomicAdd(&red[80], 1u);
                    if (at < (uint32_t)QD_OSD_TIER) sortbuf[at] = ((uint64_t)u << 32) | j;      // (a guess may overflow the buffer; a selected cut never does)
                }
            });
            __syncthreads();
            if (!spec) break;
            {
                const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)red[80]);
                ts.count = c;
                if (c > 0u && c <= lim) { cnt = (int)c; lo_key = t_hi; ts.cut = t_hi; break; }
                spec = false;                                                      // no column or too many: select, gather again
                __syncthreads();
            }
            }
            int P = 64;
            while (P < cnt) P <<= 1;
            for (int i = cnt + tid; i < P; i += T) sortbuf[i] = ~0ull;
            __syncthreads();
            if (cnt <= 256 && cnt <= T) {
                // small tier: rank by counting (the keys are distinct), one pass of broadcast reads instead of 36 barrier stages
                if ((tid & ~63) < cnt) {
                    const uint64_t mine = tid < cnt ? sortbuf[tid] : ~0ull;
                    const uint4 *sb4 = reinterpret_cast<const uint4 *>(sortbuf);
                    int rank = 0;
                    for (int i = 0; i < (cnt + 1) / 2; ++i) {                 // sortbuf[cnt] is padding (~0) when cnt is odd
                        const uint4 v = sb4[i];
                        const uint64_t k0 = (uint64_t)v.x | ((uint64_t)v.y << 32), k1 = (uint64_t)v.z | ((uint64_t)v.w << 32);
                        rank += (k0 < mine ? 1 : 0) + (k1 < mine ? 1 : 0);
                    }
                    if (tid < cnt) order[rank] = (uint16_t)(mine & 0xFFFFu);
                }
            } else {
                qd_bitonic_u64<T>(sortbuf, P, tid);
                for (int i = tid; i < cnt; i += T) order[i] = (uint16_t)(sortbuf[i] & 0xFFFFu);
            }
            __syncthreads();
    }
    ts.lo_key = lo_key; ts.lo_idx = lo_idx; ts.sphase = sphase; ts.exhausted = 0;
    return cnt;
}

// ---- the elimination shared by qd_osd0_full_kernel (osd_kernels.hip) and qd_osd0_offchip_kernel (osd_offchip.hip): state in LDS, Q planes beyond
// the LDS budget in a per-workgroup HBM buffer
struct OsdLds {
    uint64_t *q;          // Q planes resident in LDS
    uint64_t *tb;         // [m_pad] image of the 64 batch columns
    uint8_t *sp;          // [m_pad] transformed syndrome
    int16_t *rowpiv;      // [m_pad] row -> pivot order or -1
    uint16_t *prow;       // [m_pad] pivot order -> row
    uint32_t *pcol;       // [m_pad] pivot order -> fault
    uint32_t *pairs;      // [64 * max_cdeg] column-in-batch | pivot order << 8
    uint32_t *bcols;      // [64]
    uint32_t *red;        // [0..15] keys A, [16..31] keys B, [32..47] flags A, [48..63] flags B, [64..] counters
    uint32_t *outw;       // packed solution
};

template <bool SPILL>
__device__ __forceinline__ uint64_t qd_q_load(const OsdLds &S, uint64_t *qglb, int kw_lds, int m_pad, int w, int r)
{
    if (SPILL && w >= kw_lds) return qglb[(size_t)(w - kw_lds) * m_pad + r];
    return S.q[(size_t)w * m_pad + r];
}
template <bool SPILL>
__device__ __forceinline__ void qd_q_store(const OsdLds &S, uint64_t *qglb, int kw_lds, int m_pad, int w, int r, uint64_t v)
{
    if (SPILL && w >= kw_lds) qglb[(size_t)(w - kw_lds) * m_pad + r] = v;
    else S.q[(size_t)w * m_pad + r] = v;
}

// Elimination over order[0..ncols).  kcap = number of pivots the Q storage can hold.
// Returns 0 when finished (early stop, rank exhausted or every column consumed with ncols == n), 1 when it ran out of
// sorted columns (ncols < n) or of Q capacity before finishing -- the caller must then redo the shot with more.
//
// One barrier per pivot: a round is  [own rows -> candidate key] -> wave min -> LDS -> BARRIER -> every thread reads the
// 16 partials -> every thread updates its own rows from row p (which its owner leaves alone this round).  The barrier
// of round i+1 also separates the updates of round i from those of round i+1, and the two reduction buffers alternate.
//
// TIERED (qd_osd0_offchip_kernel): the order arrives in tiers.  The call with first != 0 resets the state, every later call goes on from the
// state in LDS / qglb and from *npiv_out pivots; a call with last == 0 that runs out of columns unfinished returns 1 with the state kept
// and *npiv_out updated -- the caller draws the next tier -- and the call with last != 0 is the one whose order[] ends the column order.
template <int T, bool SPILL, bool TIERED = false>
__device__ int qd_osd_eliminate(const OsdGraphDev &g, const OsdLds &S, uint64_t *qglb, int kw_lds, int kcap,
                                const uint16_t *order, int ncols, const uint8_t *det, const uint8_t *upd,
                                int upd_rows, int out_words, int *npiv_out, int *inconsistent_out,
                                unsigned long long *a_dbg = nullptr, int first = 1, int last = 1)
{
    const int tid = threadIdx.x;
    constexpr int NW = T / 64;
    uint32_t *red = S.red;
    if (!TIERED || first) {
        for (int r = tid; r < g.m_pad; r += T) {
            uint8_t s = 0;
            if (r < g.m) {
                s = det[r] & 1u;
                if (upd && r < upd_rows) s ^= upd[r] & 1u;
            }
            S.sp[r] = s;
            S.rowpiv[r] = -1;
        }
        for (int i = tid; i < kw_lds * g.m_pad; i += T) S.q[i] = 0ull;
        if (SPILL && qglb)
            for (int i = tid; i < (g.mw - kw_lds) * g.m_pad; i += T) qglb[i] = 0ull;
        for (int w = tid; w < out_words; w += T) S.outw[w] = 0u;
    }
    if (tid < 32) red[tid] = QD_NOKEY;
    else if (tid < 64) red[tid] = 0u;
    __syncthreads();

    int npiv = (TIERED && !first) ? *npiv_out : 0, done = 0, hard = 0, phase = 0;
    for (int base = 0; base < ncols && !done && !hard; base += 64) {
        // ---- transform the next 64 columns: tb[r] bit c = (T * column_c)[r]
        for (int r = tid; r < g.m_pad; r += T) S.tb[r] = 0ull;
        if (tid == 0) red[64] = 0u;
        if (tid < 64) S.bcols[tid] = (base + tid < ncols) ? (uint32_t)order[base + tid] : 0xFFFFFFFFu;
        __syncthreads();
        for (int x = tid; x < 64 * g.max_cdeg; x += T) {
            const int c = x / g.max_cdeg, q = x - c * g.max_cdeg;
            const uint32_t col = S.bcols[c];
            if (col != 0xFFFFFFFFu) {
                const uint32_t e0 = g.csc_ptr[col], e1 = g.csc_ptr[col + 1];
                if (e0 + q < e1) {
                    const int r = g.csc_row[e0 + q];
                    atomicXor(reinterpret_cast<unsigned long long *>(&S.tb[r]), 1ull << c);
                    const int k = S.rowpiv[r];
                    if (k >= 0) S.pairs[atomicAdd(&red[64], 1u)] = (uint32_t)c | ((uint32_t)k << 8);
                }
            }
        }
        __syncthreads();
        const int np = (int)red[64];
        if (np)
            for (int r = tid; r < g.m; r += T) {
                uint64_t x = S.tb[r];
                for (int i = 0; i < np; ++i) {
                    const uint32_t pr = S.pairs[i];
                    const int k = (int)(pr >> 8);
                    const uint64_t qw = qd_q_load<SPILL>(S, qglb, kw_lds, g.m_pad, k >> 6, r);
                    x ^= ((qw >> (k & 63)) & 1ull) << (pr & 63u);
                }
                S.tb[r] = x;
            }
        // ---- take pivots out of the batch, in column order
        for (;;) {
            uint32_t key = QD_NOKEY;
            int resid = 0;
            for (int r = tid; r < g.m; r += T)
                if (S.rowpiv[r] < 0) {
                    const uint64_t x = S.tb[r];
                    if (x) key = min(key, ((uint32_t)__builtin_ctzll(x) << 16) | (uint32_t)r);
                    resid |= S.sp[r];
                }
            key = qd_wave_umin(key);
            const unsigned long long bal = __ballot(resid);
            if ((tid & 63) == 0) { red[phase * 16 + (tid >> 6)] = key; red[32 + phase * 16 + (tid >> 6)] = (bal != 0ull); }
            __syncthreads();
            key = QD_NOKEY;
            int anyres = 0;
            {
                const uint4 *kv = reinterpret_cast<const uint4 *>(red + phase * 16);
                const uint4 *fv = reinterpret_cast<const uint4 *>(red + 32 + phase * 16);
#pragma unroll
                for (int w = 0; w < (NW + 3) / 4; ++w) {       // entries beyond NW hold NOKEY / 0 (set once per call)
                    const uint4 k4 = kv[w], f4 = fv[w];
                    key = min(key, min(min(k4.x, k4.y), min(k4.z, k4.w)));
                    anyres |= (int)(f4.x | f4.y | f4.z | f4.w);
                }
            }
            phase ^= 1;
            if (!anyres) { done = 1; break; }            // syndrome already in the span of the pivots found
            if (key == QD_NOKEY) break;                   // rest of the batch depends on earlier pivots
            if (npiv >= kcap) { hard = 1; break; }        // no room for another pivot in this kernel's Q storage
            const int c = (int)(key >> 16), p = (int)(key & 0xFFFFu);
            const int K = npiv, kw = K >> 6;
            const uint64_t kb = 1ull << (K & 63);
            const uint64_t tp = S.tb[p];
            const uint8_t spp = S.sp[p];
            for (int r = tid; r < g.m; r += T) {
                if (r == p) { S.rowpiv[r] = (int16_t)K; S.prow[K] = (uint16_t)p; S.pcol[K] = S.bcols[c]; }   // the owner records the pivot
                else if ((S.tb[r] >> c) & 1ull) {
                    S.tb[r] ^= tp;
                    S.sp[r] ^= spp;
                    for (int w = 0; w <= kw; ++w) {
                        uint64_t v = qd_q_load<SPILL>(S, qglb, kw_lds, g.m_pad, w, r) ^ qd_q_load<SPILL>(S, qglb, kw_lds, g.m_pad, w, p);
                        if (w == kw) v ^= kb;
                        qd_q_store<SPILL>(S, qglb, kw_lds, g.m_pad, w, r, v);
                    }
                }
            }
            npiv = K + 1;
        }
        __syncthreads();                                  // last round's updates, before the next batch re-uses tb / reads rowpiv
    }
    if (!done && !hard && (TIERED ? !last : ncols < g.n)) {
        // out of sorted columns: finished only if the syndrome happens to be resolved already or no row is left
        int resid = 0;
        for (int r = tid; r < g.m; r += T)
            if (S.rowpiv[r] < 0) resid |= S.sp[r];
        const unsigned long long bal = __ballot(resid);
        if ((tid & 63) == 0) red[32 + phase * 16 + (tid >> 6)] = (bal != 0ull);
        __syncthreads();
        int anyres = 0;
        for (int w = 0; w < NW; ++w) anyres |= (int)red[32 + phase * 16 + w];
        if (anyres && npiv < g.m) hard = 1;
        phase ^= 1;
        __syncthreads();
    }
    if (hard) {
        if (TIERED) *npiv_out = npiv;
        return 1;
    }
    // residual left on a non-pivot row <=> syndrome outside the column space
    int inconsistent = 0;
    {
        int resid = 0;
        for (int r = tid; r < g.m; r += T)
            if (S.rowpiv[r] < 0) resid |= S.sp[r];
        const unsigned long long bal = __ballot(resid);
        if ((tid & 63) == 0) red[32 + phase * 16 + (tid >> 6)] = (bal != 0ull);
        __syncthreads();
        for (int w = 0; w < NW; ++w) inconsistent |= (int)red[32 + phase * 16 + w];
    }
    // OSD-0 solution
    for (int k = tid; k < npiv; k += T)
        if (S.sp[S.prow[k]]) {
            const uint32_t j = S.pcol[k];
            atomicOr(&S.outw[j >> 5], 1u << (j & 31u));
        }
    __syncthreads();
    *npiv_out = npiv;
    *inconsistent_out = inconsistent;
    return 0;
}

__device__ __forceinline__ void qd_osd_carve(unsigned char *smem, const int *off, OsdLds &S)
{
    S.q = reinterpret_cast<uint64_t *>(smem + off[0]);
    S.tb = reinterpret_cast<uint64_t *>(smem + off[1]);
    S.sp = smem + off[2];
    S.rowpiv = reinterpret_cast<int16_t *>(smem + off[3]);
    S.prow = reinterpret_cast<uint16_t *>(smem + off[4]);
    S.pcol = reinterpret_cast<uint32_t *>(smem + off[5]);
    S.pairs = reinterpret_cast<uint32_t *>(smem + off[6]);
    S.bcols = reinterpret_cast<uint32_t *>(smem + off[7]);
    S.red = reinterpret_cast<uint32_t *>(smem + off[8]);
    S.outw = reinterpret_cast<uint32_t *>(smem + off[9]);
}
