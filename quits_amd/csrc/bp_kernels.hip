// bp_kernels.hip -- flooding min-sum belief propagation, one workgroup per shot, all message state in LDS.
//
// Replaces ldpc.BpOsdDecoder.decode -> BpDecoder::bp_decode_parallel (MINIMUM_SUM) as the reference calls it at
// quits/decoder/sliding_window.py:171,182.  CPU restatement with the same arithmetic: oracle/bp_core.inc,
// bp_minsum_compressed (REAL=float) -- the two agree bit for bit (tests/test_gpu_parity.py).
//
// Design (gfx950):
//   * A check keeps only (min1, min2, argmin, parity, per-edge sign bits) of its incoming messages: 16 bytes instead
//     of one float per edge; a fault keeps its posterior LLR and one sign bit per edge.  For the [[144,12,12]] R=12
//     window (1008 x 9504, 33192 edges) that is 68 KB of LDS per shot, so two shots are resident per CU and the
//     message traffic never leaves the CU.  HBM only sees the syndrome bytes in and the packed decision bits out.
//   * lane = node.  Check pass: lane owns a check, walks its faults (ELL-transposed adjacency -> coalesced index
//     loads, LDS gathers of the posteriors).  Bit pass: lane owns a fault, gathers the <= 16 checks' 16-byte states
//     with one ds_read_b128 each.  Nodes are degree-sorted so a wavefront's lanes share a trip count.
//   * The syndrome test of iteration t rides on check pass t+1 (it needs the same gathers), so an iteration costs
//     one check pass + one bit pass + two barriers.
//   * No atomics on floats, fixed summation order (ascending detector index) -> bit-reproducible.
#include "bp_gather_common.h"
#include "qd_host.h"

#ifdef QD_BP_TIMING   // phase cycle counters of wavefront 0 (tools/bp_timing.py); slots: 0 check pass, 1 block-OR, 2 bit pass, 3 barrier, 4 prologue, 5 epilogue
#define QD_BP_TICK(slot) { const unsigned long long now_ = clock64(); acc_[slot] += now_ - tick_; tick_ = now_; }
#else
#define QD_BP_TICK(slot)
#endif

// Bit pass, one edge: the check->fault message of record `rec` from its gathered check state `st_`, onto the posterior and onto S_j
#define QD_BIT_USE(rec, st_)                                                                                 \
    {                                                                                                        \
        uint32_t mag_, sg_;                                                                                  \
        qd_msg_decode<SM>(rec, st_, mylabel, csgn_hi, m_pad, mag_, sg_);                                     \
        acc += __uint_as_float(sg_ << 31 | mag_);                                                            \
        sabs += __uint_as_float(mag_);                                                                       \
    }

// The check-state layout, the check pass, the gathers of the bit pass, prologue and epilogue: bp_gather_common.h.  Here: the grid form of
// the check pass (with the early gathers in sign mode 2), the bit pass with its exactness bound, and the redo / park logic around them.
template <int T, int NCH, int SM, int MW>
__global__ void __launch_bounds__(T, MW) qd_bp_minsum_kernel(BpGraphDev g, DecodeArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    qd_require_lds_at_zero(smem);
    float4 *chk = reinterpret_cast<float4 *>(smem + g.off_chk);
    uint32_t *csgn_hi = reinterpret_cast<uint32_t *>(smem + g.off_cneg);
    float *llr = reinterpret_cast<float *>(smem + g.off_llr);
    uint32_t *outw = reinterpret_cast<uint32_t *>(smem + g.off_out);
    int *misc = reinterpret_cast<int *>(smem + g.off_misc);   // [0..31] OR flags, [32] fail slot
    constexpr int NW = T / 64;

    const int tid = threadIdx.x;
    const int wave0 = __builtin_amdgcn_readfirstlane(tid & ~63);   // first thread of this wavefront
    int64_t shot = blockIdx.x;
    if (a.shot_list) {                                             // redo pass: one workgroup per parked shot
        if ((int)blockIdx.x >= *a.shot_count) return;
        shot = a.shot_list[blockIdx.x];
    }
    const int m_pad = g.m_pad, n_pad = g.n_pad;
    const __amdgpu_buffer_rsrc_t rec_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)g.bit_rec, 0, g.rec_words * n_pad * 4, 0x00020000);
    const int rec_voff = tid * 16;

#ifdef QD_BP_TIMING
    unsigned long long acc_[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long tick_ = clock64();
#endif
    // ---- the window's syndrome, posteriors = priors, no message yet; records beyond a fault's degree read the message +0
    if (SM == 2)
        for (int c = tid; c < g.m; c += T)
            for (int w = 1; w < g.neg_words; ++w) csgn_hi[(w - 1) * m_pad + c] = 0u;
    if (!qd_gather_prologue<T>(g, a, shot, chk, llr, llr, outw, misc, qd_chk_reset(0u), a.status_or)) return;

    // Exactness bound of the grid arithmetic.  The channel LLRs are multiples of q = 2^-k and ms_scaling is 1, so every
    // message is a multiple of q; a float sum or difference of such values is exact while its magnitude stays below
    // 2^24 q.  S_j = |llr0_j| + sum_k |c2b_k| bounds every partial sum of fault j's posterior, and a bit->check message
    // |L_j - c2b| <= S_j as well; S_j itself is a sum of non-negative terms (monotone: exact whenever the total is).  So
    // max_j S_j < 2^23 q over the whole run (a.s_limit) certifies that no operation rounded: the result is then what
    // ldpc's double-precision arithmetic returns for the same LLRs.  One extra add per edge, one compare per fault.
    bool trip = false;             // a lane mask in scalar registers: costs no vector register
    const float s_lim = a.s_limit > 0.f ? a.s_limit : __builtin_inff();
    int t = 0, converged = 0, phase = 1;
    QD_BP_TICK(4)
    for (;;) {
        const float alpha = (a.ms_scale == 0.f) ? (1.0f - ldexpf(1.0f, -(t + 1))) : a.ms_scale;
        // ---- check pass t+1 in its grid form, early gathers on wide checks; its parity test is the convergence test of iteration t
        const bool unsat = qd_check_pass<T, SM, /* FLOAT_SIGN */ false, /* PREGATHER */ SM == 2>(g, chk, csgn_hi, alpha);
        QD_BP_TICK(0)
        const int anyun = qd_block_or(unsat ? 1 : 0, misc, NW, phase);
        QD_BP_TICK(1)
        phase ^= 1;
        if (t >= 1 && !anyun) { converged = 1; break; }
        if (t == a.max_iter) break;
        // ---- bit pass t+1: posterior = prior + sum of check->bit messages, in ascending detector order.
        // Records beyond a fault's degree point at the dummy check (message +0), so edges are handled in fixed groups
        // (3 | 2 | 2 | 4 | 4 | 1) with one wave-uniform test per group instead of one per edge.
        // (the trip count and everything derived from it stay in scalar registers; only the last trip is partial)
        for (int base = 0; base < g.n; base += T) {
            const int b = base + tid;
            if (base + T > g.n && b >= g.n) break;
            const int b0 = base + wave0;                                // first slot of this wavefront
            const uint16_t mylabel = (uint16_t)b;                       // my slot; the check keeps its argmin slot in the low 16 bits of w
            // records through buffer loads: per-lane offset tid * 16 fixed, everything that moves is a scalar offset
            const qd_u32x4 r0 = __builtin_amdgcn_raw_buffer_load_b128(rec_rsrc, rec_voff, base * 16, 0);
            qd_u32x4 r1, r2, r3, r4;
            if (NCH > 1 && b0 < g.bit_thr[3]) r1 = __builtin_amdgcn_raw_buffer_load_b128(rec_rsrc, rec_voff, (n_pad + base) * 16, 0);
            if (NCH > 2 && b0 < g.bit_thr[7]) r2 = __builtin_amdgcn_raw_buffer_load_b128(rec_rsrc, rec_voff, (2 * n_pad + base) * 16, 0);
            if (NCH > 3 && b0 < g.bit_thr[11]) r3 = __builtin_amdgcn_raw_buffer_load_b128(rec_rsrc, rec_voff, (3 * n_pad + base) * 16, 0);
            if (NCH > 4 && b0 < g.bit_thr[15]) r4 = __builtin_amdgcn_raw_buffer_load_b128(rec_rsrc, rec_voff, (4 * n_pad + base) * 16, 0);
            float acc = __uint_as_float(r0.x);
            float sabs = fabsf(acc);
            {
                qd_u32x4 s0 = qd_lds_gather16(r0.y), s1 = qd_lds_gather16(r0.z), s2 = qd_lds_gather16(r0.w);
                qd_lds_wait(s0, s1, s2);
                QD_BIT_USE(r0.y, s0) QD_BIT_USE(r0.z, s1)
                if (b0 < g.bit_thr[2]) QD_BIT_USE(r0.w, s2)          // (a wavefront of weight-2 faults gathers the dummy but skips its arithmetic)
            }
            if (NCH > 1 && b0 < g.bit_thr[3]) {
                qd_u32x4 s0 = qd_lds_gather16(r1.x), s1 = qd_lds_gather16(r1.y);
                qd_lds_wait(s0, s1);
                QD_BIT_USE(r1.x, s0)
                if (b0 < g.bit_thr[4]) QD_BIT_USE(r1.y, s1)
                if (b0 < g.bit_thr[5]) {
                    qd_u32x4 s2 = qd_lds_gather16(r1.z), s3 = qd_lds_gather16(r1.w);
                    qd_lds_wait(s2, s3);
                    QD_BIT_USE(r1.z, s2)
                    if (b0 < g.bit_thr[6]) QD_BIT_USE(r1.w, s3)
                }
            }
            if (NCH > 2 && b0 < g.bit_thr[7]) {
                qd_u32x4 s0 = qd_lds_gather16(r2.x), s1 = qd_lds_gather16(r2.y), s2 = qd_lds_gather16(r2.z), s3 = qd_lds_gather16(r2.w);
                qd_lds_wait(s0, s1, s2, s3);
                QD_BIT_USE(r2.x, s0) QD_BIT_USE(r2.y, s1) QD_BIT_USE(r2.z, s2) QD_BIT_USE(r2.w, s3)
            }
            if (NCH > 3 && b0 < g.bit_thr[11]) {
                qd_u32x4 s0 = qd_lds_gather16(r3.x), s1 = qd_lds_gather16(r3.y), s2 = qd_lds_gather16(r3.z), s3 = qd_lds_gather16(r3.w);
                qd_lds_wait(s0, s1, s2, s3);
                QD_BIT_USE(r3.x, s0) QD_BIT_USE(r3.y, s1) QD_BIT_USE(r3.z, s2) QD_BIT_USE(r3.w, s3)
            }
            if (NCH > 4 && b0 < g.bit_thr[15]) {
                qd_u32x4 s0 = qd_lds_gather16(r4.x);
                qd_lds_wait(s0);
                QD_BIT_USE(r4.x, s0)
            }
            llr[b] = acc;
            trip |= (sabs >= s_lim);
            if (acc <= 0.f) {
                // hard decision 1 (rare): tell the fault's checks -- one LDS atomic per edge on bit 30 of the state's last word
                // (records beyond the degree point at the dummy check; readers of the word ignore that bit)
                qd_flip_bit30(r0.y); qd_flip_bit30(r0.z); qd_flip_bit30(r0.w);
                if (NCH > 1 && b0 < g.bit_thr[3]) qd_flip_bit30x4(r1);
                if (NCH > 2 && b0 < g.bit_thr[7]) qd_flip_bit30x4(r2);
                if (NCH > 3 && b0 < g.bit_thr[11]) qd_flip_bit30x4(r3);
                if (NCH > 4 && b0 < g.bit_thr[15]) qd_flip_bit30(r4.x);
            }
        }
        QD_BP_TICK(2)
        __syncthreads();
        QD_BP_TICK(3)
        ++t;
    }

    // ---- grid arithmetic: did the bound hold?  (a.s_limit = 0: LLRs are not on a grid, nothing to certify)
    int status_or = a.status_or;
    if (a.s_limit > 0.f) {
        const int tripped = qd_block_or(trip ? 1 : 0, misc, NW, phase);
        if (tripped) {
            if (a.redo_list) {                                     // park the shot for the coarse-grid pass, if there is room
                if (tid == 0) misc[33] = atomicAdd(a.redo_count, 1);
                __syncthreads();
                const int at = misc[33];
                if (at < a.redo_cap) {
                    if (tid == 0) a.redo_list[at] = (int32_t)shot;
                    return;
                }
            }
            status_or |= QD_STATUS_INEXACT;
        }
    }
    // ---- hard decision, packed by fault index; a shot that did not converge leaves its posteriors for the post-processor
    qd_gather_publish<T>(g, a, shot, llr, outw, misc, !converged && a.want_llr);
    if (tid == 0) a.status[shot] = t | (converged * QD_STATUS_CONVERGED) | status_or;
#ifdef QD_BP_TIMING
    QD_BP_TICK(5)
    if (tid == 0) {
        for (int i = 0; i < 6; ++i) atomicAdd(&a.dbg[i], acc_[i]);
        atomicAdd(&a.dbg[6], 1ull); atomicAdd(&a.dbg[7], (unsigned long long)t);
    }
#endif
}

// ---- launch: the 36 instantiations a graph can select, threads x record chunks x sign mode.  The kernel is the recheck / coarse-grid pass
// of the scatter kernels and the flooding min-sum kernel of the windows they do not take; it is on no timed path.
// Waves per SIMD the register allocator must leave room for: at 8 wavefronts per SIMD (64 registers: two 1024-thread workgroups per CU) every
// instantiation spilled 12-16 bytes per lane, so the budget is the one that keeps it out of scratch (tests/test_api.py asserts it)
constexpr int qd_bp_minwaves(int T) { return T == 1024 ? 4 : 6; }

hipError_t qd_launch_bp(const BpGraphDev &g, const DecodeArgs &a, int64_t B, hipStream_t s)
{
    return qd_gather_dispatch(g, [&](auto t, auto nch, auto sm) {
        constexpr int T = decltype(t)::value;
        return qd_gather_launch(qd_bp_minsum_kernel<T, decltype(nch)::value, decltype(sm)::value, qd_bp_minwaves(T)>, T, g.lds_bytes, B, s, g, a);
    });
}
