// bp_scatter_wide.hip -- flooding min-sum belief propagation on an LLR grid, scatter form: one workgroup per shot, CPL checks per lane
// with NSW 32-bit sign words each, the checks' message state in their lane's REGISTERS, the faults' posteriors as 32-bit integers (grid
// units) in LDS.  The only scatter kernel, and the default of flooding min-sum on the grid for the windows ScatGraphDev::ok admits.
//
// Replaces ldpc.BpOsdDecoder.decode -> BpDecoder::bp_decode_parallel (MINIMUM_SUM, ms_scaling_factor 1) as the reference calls it at
// quits/decoder/sliding_window.py:171,182.  Returns exactly what qd_bp_minsum_kernel (bp_kernels.hip) returns -- hard decisions,
// iteration counts, status words, posteriors of the shots that go to OSD -- bit for bit; oracle: oracle/bp_core.inc bp_parallel_edge in
// double on the same LLR grid.
//
// Why a scatter form.  bp_kernels.hip spends 8.3 vector instructions and one 16-byte LDS gather per edge in its bit pass (a fault
// rebuilding every check's message from the check's packed state).  On the grid every message is an integer multiple of 2^-k, so a
// posterior is an INTEGER sum -- and integer LDS atomics run at the rate of a 4-byte gather (ds_add_u32: 2.2 ns per wavefront
// instruction per CU, scattered addresses; ds_add_f32: 80 ns, profiles/r03z_lds_atomic_rates.txt).  So the check that has just
// computed (min1, min2, argmin, signs) adds +-min1 to each of its faults' accumulators itself (one sign mask, one v_bitop3,
// one ds_add_u32 per edge), corrects the argmin fault by +-(min2 - min1), and the bit pass is gone.  The check state never leaves the
// lane, so the LDS holds one int32 accumulator per fault and nothing per check: 38 KB + 2 KB at the headline window, 76 KB for a QLP
// window of BASELINE configs[4] where qd_bp_minsum_kernel needs 112 KB (ONE workgroup of 1024 threads per CU; here two: BP 36.8 ->
// 19.0 ms per 8192-shot window launch).
//
// The shapes (graph_layout.hip: build_scatter chooses, qd_launch_bp_scatter_wide below instantiates):
//   * a window with a lane for every check and rows of up to 64 faults runs on HALF the lanes with two checks each where the LDS holds
//     twice the workgroups -- the headline window (1008 checks) on 512 lanes: the same 32 wavefronts per CU in four workgroups instead
//     of two, i.e. half as many wavefronts per barrier (BP 50.3 -> 44.2 ms per 65 536 shots); 512-thread windows on 256 lanes, windows
//     of <= 128 checks on 128;
//   * where it does not, or under QD_SCATTER_CPL1=1, on 256 / 512 / 1024 lanes with one check each;
//   * more checks than a workgroup has lanes, or rows of 65..96 faults (three sign words): 512 lanes x 3 checks (or 704 / 1024 x 2) --
//     the windows of BASELINE configs[4] (QLP [[1020,136]], W = 3: 1350 checks of up to 78 faults, 18 900 faults).
//
// A lane's checks keep their state in registers (two minima, argmin position, the sign words), ONE set per check: what was sent last
// until the gather walk commits what it found, which the scatter pass then sends.
// Check slots are sorted by degree; a wavefront's 64 checks of one round are 64 consecutive slots (sg.wave_map), so
// the trip count stays wave-uniform, and the rounds are dealt out so that the wavefronts of a workgroup walk equally many edges between
// two barriers.
//
// One iteration = [gather pass of check 0 .. CPL-1 over L(t): new minima and signs, and the syndrome of L(t)'s hard decision] barrier
// [converged? | accumulators := priors] barrier [scatter pass of check 0 .. CPL-1] barrier.  Every gather of the iteration precedes
// the vote's barrier, so behind it the one buffer can go back to the priors (qs_reset_to_priors, bp_scatter_edge.h: the decoder's
// constant image ScatArgs::prior_g, L2-resident and shared by every shot, copied by global_load_lds_dwordx4 without passing through
// registers; the prologue's fill is the same routine), and behind the second barrier an edge adds its new message and nothing else:
// L(t+1) = prior + sum of the new messages, the integer the in-place form (each accumulator moved by new message - message sent
// last time: five vector instructions per edge, a second atomic per check for the old argmin edge) arrived at.  Two vector
// instructions per edge; the price is 4 bytes of L2 traffic per slot and iteration and the third barrier
// (profiles/bp_scatter_reset_ab.txt).  The reset waits for the vote: a shot that has converged, or has run its last iteration, keeps
// L(t) in the buffer for the epilogue.  An accumulator holds L - 1, so that (L <= 0) is its sign bit: a check gets the parity
// of its faults' hard decisions with one XOR per edge, and (bit->check message <= 0) is the sign bit of the difference it computes anyway.
//
// Exactness.  Integer accumulation cannot round; what must not round are the float operations of the gather
// pass, on integer-valued floats: exact below 2^24.  Every |posterior partial sum| and |bit->check message| of fault j is at most
// S_j = |prior_j| + sum_i |c2b_ij| <= max|prior| + max_cdeg * max_i min2_i, so max over checks and iterations of min2 <
// (2^23 - max|prior|) / max_cdeg - 1 (ScatArgs::m2_limit; one v_max per CHECK per iteration) certifies the run.  That bound is
// looser than qd_bp_minsum_kernel's per-fault one, which the oracle restates: a shot it cannot certify is parked and decoded again
// by qd_bp_minsum_kernel (recheck pass), which then decides about the coarse grid as before.  A certified shot is exact in both
// kernels, hence identical.
#include "qd_internal.h"
#include "qd_host.h"
#include "../../include/quits_amd.h"
#include "bp_scatter_edge.h"

// Wavefront priorities.  A wavefront raises its priority for its last gather round (0 -> 2; the scatter pass runs at QS_PRIO = 1,
// bp_scatter_edge.h): the wavefronts closest to the barrier go first, so a workgroup's stragglers are fewer.  Headline BP stage 44.1 ->
// 43.2 ms per 65 536 shots; the other way round (first round high) 43.7, scatter pass at 0 / 2 / 3 no change, alternate wavefronts
// high no change (profiles/r03x_wavefront_priority_ab.txt).  Between the passes the kernel runs at priority 0: every priority raised by one, so that
// a kernel beside this one (the pipelined driver's post-processing) only issues when this one does not, was no faster (profiles/r06_bp_stream_bubble.txt).
#define QSW_GATHER_PRIO(j_) if ((j_) == 0) __builtin_amdgcn_s_setprio(0); else if ((j_) == CPL - 1) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(1);

template <int T, int MW, int CPL, int NSW>
__global__ void __launch_bounds__(T, MW) qd_bp_scatter_wide_kernel(BpGraphDev g, ScatGraphDev sg, DecodeArgs a, ScatArgs x)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem;
    if (lds_base != 0u) __builtin_trap();   // no static LDS in this kernel: byte offsets into smem are LDS addresses
    uint32_t *outw = reinterpret_cast<uint32_t *>(smem + sg.off_out);
    int *misc = reinterpret_cast<int *>(smem + sg.off_misc);             // [0..31] qd_block_or, [32..35] convergence flags (one BYTE per wavefront), [48] fail slot
    constexpr int NW = T / 64;
    static_assert(T % 64 == 0 && NW <= 16, "workgroup shape");

    const int tid = threadIdx.x;
    const int64_t shot = blockIdx.x;
    const uint8_t *det = a.det + shot * a.det_stride + a.det_offset;
    const uint8_t *upd = a.upd ? a.upd + shot * a.upd_stride : nullptr;
    const int m_pad = g.m_pad, n_pad = g.n_pad;

    // ---- the window syndrome (sliding_window.py:168-169), the accumulators at the priors (minus one)
    int any = 0;
    uint32_t synd[CPL];                                // the check's syndrome bit, at bit 31: where the accumulators keep the hard decision (the vote XORs the two)
    int dcs[CPL];
    bool act[CPL];
    if (tid < 64) misc[tid] = 0;
    int cs[CPL];                                       // my check slot of round j (sg.wave_map: 64 consecutive slots per wavefront and round)
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int sw = __builtin_amdgcn_readfirstlane(sg.wave_map[j * NW + (tid >> 6)]);
        const int c = sw * 64 + (tid & 63);
        cs[j] = c;
        act[j] = sw >= 0 && c < g.m;
        synd[j] = 0u; dcs[j] = 0;
        if (act[j]) {
            const uint32_t o = g.chk_orig[c];
            synd[j] = det[o] & 1u;
            if (upd && (int)o < a.upd_rows) synd[j] ^= upd[o] & 1u;
            synd[j] <<= 31;
            any |= (int)synd[j];
            dcs[j] = sg.chk_deg[c];
        }
    }
    // per wavefront and round: trip count | largest degree << 8 | smallest << 16 (scalar); a round whose 64 slots lie beyond the window has 0
    // (read in front of the fill: behind a load that writes LDS the compiler no longer takes a global load for a scalar one)
    int dws[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int wslot = __builtin_amdgcn_readfirstlane(cs[j] >> 6);
        dws[j] = wslot >= 0 ? (int)sg.deg_w[wslot] : 0;
    }
    qs_reset_to_priors<NW>(x.prior_g, (uint32_t)sg.offA, sg.nslots, tid);               // (unused slots and the trash slots of the short rows hold 0 there)
    for (int w = tid; w < g.out_words; w += T) outw[w] = 0u;
    __syncthreads();
    any = qd_block_or(any, misc, NW, 0);
    if (!any) {   // bposd_decoder.pyx: an all-zero syndrome returns the zero vector without running BP
        for (int w = tid; w < g.out_words; w += T) a.err_bits[shot * g.out_words + w] = 0u;
        if (tid == 0) a.status[shot] = QD_STATUS_CONVERGED | QD_STATUS_ZERO | a.status_or;
        return;
    }
    // check state, in registers, one set per check: the two minima, the position of the argmin edge, the outgoing signs (edge k of a word of
    // kend edges at bit kend - 1 - k).  A gather walk reads what the check SENT in the last scatter pass, works on locals and commits what it
    // found at its end (QSW_WALKED); the scatter pass sends what it finds there and nothing reads the set between the two, so the live ranges of
    // "sent" and "found" are disjoint and there is nothing to copy back (two sets cost ten moves per wavefront-iteration, profiles/bp_per_check_ab.txt).
    float S1[CPL], S2[CPL], mx2 = 0.f;
    uint32_t KOLD[CPL], O[CPL][NSW];
    uint32_t FX[CPL];                                   // LDS offset of the argmin edge's accumulator (QS_FIX_ADDR), asked for in front of the barriers the scatter pass starts behind
#ifdef QSW_STATS
    float P1[CPL], P2[CPL];                             // what was sent before the last commit: the statistics compare the two
    uint32_t PK[CPL], PO[CPL][NSW];
#endif
    [[maybe_unused]] uint32_t cmpf = 0u;                // bit j: round j of this wavefront walks in the compare form from now on (two-word shapes; see the gather pass)
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        S1[j] = 0.f; S2[j] = 0.f; KOLD[j] = 0xFFFFFFFFu; FX[j] = 0u;
#pragma unroll
        for (int w = 0; w < NSW; ++w) O[j][w] = 0u;
#ifdef QSW_STATS
        P1[j] = 0.f; P2[j] = 0.f; PK[j] = 0xFFFFFFFFu;
#pragma unroll
        for (int w = 0; w < NSW; ++w) PO[j][w] = 0u;
#endif
    }
    const uint32_t cur = (uint32_t)sg.offA;
    const __amdgpu_buffer_rsrc_t adj_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)sg.adjA, 0, (g.max_rdeg_pad / 4 + 2) * m_pad * 16, 0x00020000);
    const int adj_row = m_pad * 16;
#define QS_ADJ(row_) qs_as_uint4(__builtin_amdgcn_raw_buffer_load_b128(adj_rsrc, adj_voff, (row_) * adj_row, 0))
    // The first group of offsets of a pass (round 0, word 0) is requested BEFORE the barrier the pass starts behind: every wavefront of the workgroup
    // would otherwise begin the pass by waiting for the same L2 round trip at the same time.
#define QS_ADJ_FIRST qs_as_uint4(__builtin_amdgcn_raw_buffer_load_b128(adj_rsrc, cs[0] * 16, 0, 0))
    // The argmin edge's entry of the adjacency table, one dword per check and pass.  Asked for at the head of the scatter round it would be the OLDEST load
    // in flight there, and the round's first add -- which needs only the prefetched group -- would wait for its round trip (vmcnt counts in order).  Asked
    // for behind the gather pass, with `pf`, it lands while the workgroup stands at the vote's and the reset's barriers.
    // (A 24-bit multiply-add: the group index is below 64 and adj_row = 16 m_pad far below 2^24 for any window whose checks fit a workgroup -- the plain
    //  product compiles to the 64-bit v_mad_u64_u32.)
#define QS_FIX_ADDR(j_) __builtin_amdgcn_raw_buffer_load_b32(adj_rsrc, (int)(__umul24(KOLD[j_] >> 2, (uint32_t)adj_row) + (KOLD[j_] & 3u) * 4u) + cs[j_] * 16, 0, 0)
    uint4 pf = QS_ADJ_FIRST;
    // ---- fast start.  Gather pass 0 reads the priors alone (nothing has been sent: S1 = S2 = 0, O = 0, KOLD none), so the minima, the argmin and
    // the incoming signs it finds are constants of the decoder: they come from the table qd_bp_first_pass_kernel made with the same walk.  Only `flip`
    // depends on the shot, through the check's own syndrome bit; the pass's convergence vote is never read (t >= 1 below).  The kernel then enters
    // the loop at scatter pass 0, behind the barriers of the set-up above.
    // (The table and the thin last pass behind the loop, each measured alone against the generic loop: profiles/bp_fast_start_ab.txt.)
    const bool fast = x.first_pass != nullptr && a.max_iter >= 1;
    bool have = false;                                  // the state set already holds what the gather pass of this iteration would commit
    if (fast) {
#pragma unroll
        for (int j = 0; j < CPL; ++j)
            if (act[j]) {
                const uint4 *rp = reinterpret_cast<const uint4 *>(x.first_pass) + 2 * cs[j];
                const uint4 r0 = rp[0], r1 = rp[1];
                const uint32_t negw[3] = {r0.w, r1.x, r1.y};
                const uint32_t flip = 0u - (((synd[j] >> 31) ^ r1.z) & 1u);
                S1[j] = __uint_as_float(r0.x); S2[j] = __uint_as_float(r0.y); KOLD[j] = r0.z; FX[j] = r1.w;     // (the record holds the entry itself)
#pragma unroll
                for (int w = 0; w < NSW; ++w) O[j][w] = negw[w] ^ flip;
                mx2 = qs_max_f32(mx2, S2[j]);
            }
        have = true;
    }
    // The convergence vote of a gather pass.  A lane collects syndrome ^ hard-decision parity of its rounds in the sign bit of one word `uw_` (one
    // v_bitop3 per round, the other bits are noise); one ballot on the sign, one flag BYTE per wavefront (the bytes of the wavefronts a shape does
    // not have stay 0 from the set-up), read by everybody behind the barrier the pass ends at: 8 or 16 bytes, one read, one or three ORs.
#define QSW_VOTE_ROUND(uw_, synd_, hp_) uw_ = __builtin_amdgcn_bitop3_b32(uw_, synd_, hp_, 0xF6);     /* uw | (synd ^ hp) */
#define QSW_VOTE(uw_, anyun_)                                                                          \
        {                                                                                              \
            const unsigned long long bal = __ballot((int)(uw_) < 0);                                   \
            if ((tid & 63) == 0) reinterpret_cast<unsigned char *>(misc + 32)[tid >> 6] = (unsigned char)(bal != 0ull); \
        }                                                                                              \
        __syncthreads();                                                                               \
        if constexpr (NW <= 8) {                                                                       \
            const int2 v = *reinterpret_cast<const int2 *>(misc + 32);                                 \
            anyun_ = v.x | v.y;                                                                        \
        } else {                                                                                       \
            const int4 v = *reinterpret_cast<const int4 *>(misc + 32);                                 \
            anyun_ = (v.x | v.y) | (v.z | v.w);                                                        \
        }
    int t = 0, converged = 0;
    for (;;) {
      if (!have) {
        // ---- gather pass t+1 over L(t); the parity of the hard decisions it meets is the convergence test of iteration t
        uint32_t us = 0u;
        if (fast && t == a.max_iter) break;      // the last pass runs behind the loop, in its thin form
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            float a1 = FLT_MAX, a2 = FLT_MAX;
            uint32_t kst = 0u;
            QSW_GATHER_PRIO(j)          // the later gather rounds of a wavefront run at a higher priority
            // what a walk leaves behind (a1, a2, kst, hp, par, neg[]) becomes the check's new state: the one commit, of the key walk that holds, of
            // the compare walk, and of the compare walk behind a key walk that did not hold (which has written locals only)
            // outgoing sign on edge k = syndrome ^ (parity of all incoming signs) ^ incoming sign k
#define QSW_WALKED                                                                                     \
                {                                                                                      \
                    const uint32_t flip = 0u - ((uint32_t)__popc(par ^ synd[j]) & 1u);                 \
                    _Pragma("unroll")                                                                  \
                    for (int w = 0; w < NSW; ++w) O[j][w] = neg[w] ^ flip;                             \
                    mx2 = qs_max_f32(mx2, a2);                                                         \
                    QSW_VOTE_ROUND(us, synd[j], hp)                                                    \
                }
            // Rows of at most 64 faults walk in the key form (bp_scatter_edge.h: QS_EDGE_K), which is exact where every check's second key stays below
            // 2^18, i.e. min2 < 2^18 - 1.  Where a round's walk ends at or above that (late iterations of shots that do not converge: 2.1 % of the headline's
            // round-passes, profiles/bp_argmin_keys_ab.txt) the round is walked again in the compare form -- the accumulators do not move during a gather
            // pass and a walk writes only locals -- and the round's bit in `cmpf` sends its later passes there at once.
            bool cmpw = true;
            if constexpr (NSW == 2) cmpw = __builtin_amdgcn_ballot_w64((cmpf >> j) & 1u) != 0ull;       // (wave-uniform: set for all of a round's lanes or none)
#ifdef QSW_STATS
            if ((tid & 63) == 0 && __ballot(act[j])) atomicAdd(&a.dbg[14], 1ull);
            P1[j] = S1[j]; P2[j] = S2[j]; PK[j] = KOLD[j];
#pragma unroll
            for (int w = 0; w < NSW; ++w) PO[j][w] = O[j][w];
#endif
            if (act[j]) {
                if constexpr (NSW == 2) {
                    if (!cmpw) {
#define QS_WALK(p_) QS_KEY_##p_
#include "bp_scatter_wide_walk.inc"
#undef QS_WALK
                        if (keys_ok_) QSW_WALKED
                        else { cmpw = true; cmpf |= 1u << j; a1 = FLT_MAX; a2 = FLT_MAX; kst = 0u; }
                    }
                }
                if (cmpw) {
#ifdef QSW_STATS
                    if ((tid & 63) == 0) atomicAdd(&a.dbg[15], 1ull);        // (lane 0 is on wherever a round has a check: slots fill from the bottom)
#endif
#define QS_WALK(p_) QS_CMP_##p_
#include "bp_scatter_wide_walk.inc"
#undef QS_WALK
                    QSW_WALKED
                }
            }
#undef QSW_WALKED
            S1[j] = a1; S2[j] = a2; KOLD[j] = kst;           // (outside the test: a lane without a check keeps nothing worth a register of its own)
        }
        __builtin_amdgcn_s_setprio(0);
        pf = QS_ADJ_FIRST;              // for the scatter pass behind the barrier
#pragma unroll
        for (int j = 0; j < CPL; ++j)
            if (act[j]) FX[j] = QS_FIX_ADDR(j);
        int anyun;
        QSW_VOTE(us, anyun)
        if (t >= 1 && !anyun) { converged = 1; break; }
        if (t == a.max_iter) break;
        // ---- reset: every read of the pass lies before the vote's barrier, and the accumulators are not the result (both tests above say so), so
        // they go back to the priors; no add may be issued before every wavefront's copies have landed: a second barrier.  (Where `have` skips the
        // gather pass -- the fast start -- the prologue's fill is still there.)
        qs_reset_to_priors<NW>(x.prior_g, cur, sg.nslots, tid);
        __syncthreads();
      }
        have = false;
        // ---- scatter pass over the priors: each edge adds its new message
        __builtin_amdgcn_s_setprio(QS_PRIO);
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
#ifdef QSW_STATS
            {
                bool same = S1[j] == P1[j] && S2[j] == P2[j] && (KOLD[j] == PK[j] || S1[j] == S2[j]);
#pragma unroll
                for (int w = 0; w < NSW; ++w) same = same && O[j][w] == PO[j][w];
                const unsigned long long ba = __ballot(act[j]), bs = __ballot(act[j] && same);
                if ((tid & 63) == 0 && ba) {
                    const int bk = min(t / 10, 4);
                    atomicAdd(&a.dbg[0], 1ull); atomicAdd(&a.dbg[2 + bk], 1ull);
                    if (bs == ba) { atomicAdd(&a.dbg[1], 1ull); atomicAdd(&a.dbg[7 + bk], 1ull); }
                    atomicAdd(&a.dbg[12], (unsigned long long)__popcll(bs)); atomicAdd(&a.dbg[13], (unsigned long long)__popcll(ba));
                }
            }
#endif
            if (act[j]) {
                int dwj = dws[j];
                asm volatile("" : "+s"(dwj));
                const int trip = dwj & 0xFF, wmax = (dwj >> 8) & 0xFF, wmin = (dwj >> 16) & 0xFF, wmin4 = wmin & ~3;
                const int adj_voff = cs[j] * 16;
                const int dc = dcs[j];
                const int n1 = (int)S1[j], nx = n1 ^ -n1;
                const uint32_t kst = KOLD[j];
                const uint32_t fixn_off = FX[j];
                const int ng = trip >> 2;
                // The sign / difference bit of an edge is picked with a scalar bit position (v_bfe_i32 with an SGPR offset) instead of shifting the two
                // words by 4 per group: half a vector instruction per edge moves to the scalar unit.  BP stage 42.35 -> 42.24 ms per 65 536 headline
                // shots against the shifting form (profiles/r05_k1sw_micro_ab.txt).
#define QS_GROUP_POS(gi_) const int b0_ = kendw - 1 - 4 * ((gi_) - 8 * w);      /* (the words are used as they are: edge k of the word at bit kendw - 1 - k) */
                // a group every lane of the wavefront has in full ...
#define QS_GROUP_PLAIN(e4, gi_)                                                                                                      \
                {                                                                                                                    \
                    QS_GROUP_POS(gi_)                                                                                                \
                    QS_SCAT(e4.x, 0, b0_, QS_NOFIX) QS_SCAT(e4.y, 0, b0_ - 1, QS_NOFIX) QS_SCAT(e4.z, 0, b0_ - 2, QS_NOFIX) QS_SCAT(e4.w, 0, b0_ - 3, QS_NOFIX) \
                }
                // ... and one that reaches beyond the smallest degree: lanes past their degree add 0 to a trash slot
#define QS_SCAT_TAIL(off, q_)                                                                                                        \
                    if (k + (q_) < wmin) QS_SCAT(off, 0, b0_ - (q_), QS_NOFIX)                                                       \
                    else if (k + (q_) < wmax) QS_SCAT(off, k + (q_), b0_ - (q_), QS_TAILZERO)
#define QS_GROUP_TAIL(e4, gi_)                                                                                                       \
                {                                                                                                                    \
                    const int k = (gi_) * 4;                                                                                         \
                    QS_GROUP_POS(gi_)                                                                                                \
                    QS_SCAT_TAIL(e4.x, 0) QS_SCAT_TAIL(e4.y, 1) QS_SCAT_TAIL(e4.z, 2) QS_SCAT_TAIL(e4.w, 3)                          \
                }
#pragma unroll
                for (int w = 0; w < NSW; ++w) {
                    if (32 * w < trip) {
                        const int kendw = min(trip - 32 * w, 32);
                        const uint32_t own = O[j][w];
                        const int g1 = min(ng, 8 * w + 8);                    // groups of this word: [8 w, g1)
                        const int gp = min(g1, max(wmin4 >> 2, 8 * w));       // ... of which [8 w, gp) are plain (as in the gather pass: three loops, no test per group)
                        uint4 ea = (j == 0 && w == 0) ? pf : QS_ADJ(8 * w), eb;
                        int gi = 8 * w;
#pragma unroll 1
                        for (; gi + 2 <= gp; gi += 2) {                       // two groups per trip on two register sets
                            eb = QS_ADJ(gi + 1);                              // (the table has two spare group rows)
                            QS_GROUP_PLAIN(ea, gi)
                            ea = QS_ADJ(gi + 2);
                            QS_GROUP_PLAIN(eb, gi + 1)
                        }
#pragma unroll 1
                        for (; gi < gp; ++gi) {
                            const uint4 e4 = ea;
                            ea = QS_ADJ(gi + 1);
                            QS_GROUP_PLAIN(e4, gi)
                        }
#pragma unroll 1
                        for (; gi + 1 < g1; ++gi) {
                            const uint4 e4 = ea;
                            ea = QS_ADJ(gi + 1);
                            QS_GROUP_TAIL(e4, gi)
                        }
                        if (gi < g1) QS_GROUP_TAIL(ea, gi)          // the word's last group: nothing to request behind it, no copy
                    }
                }
#undef QS_GROUP_PLAIN
#undef QS_GROUP_TAIL
#undef QS_SCAT_TAIL
#undef QS_GROUP_POS
                // the argmin edge carries min2, not min1: it gains +-(min2 - min1).  Its sign is bit kend_w - 1 - (kst - 32 w) of its word w (kend_w is
                // wave-uniform: one subtraction from a scalar per word, the word and the bit picked by the same compare), taken as a mask m = 0 / -1 by one
                // v_bfe_i32 and applied as (dlt ^ m) - m; kst < the lane's degree <= trip, so the bit position is within 0..31.
                {
                    uint32_t wd = O[j][0];
                    int bpos = min(trip, 32) - 1 - (int)kst;
#pragma unroll
                    for (int w = 1; w < NSW; ++w) {
                        const bool inw = kst >= 32u * (uint32_t)w;
                        wd = inw ? O[j][w] : wd;
                        bpos = inw ? min(trip - 32 * w, 32) - 1 + 32 * w - (int)kst : bpos;
                    }
                    const int m_ = __builtin_amdgcn_sbfe((int)wd, bpos, 1);
                    const int dlt = (int)S2[j] - n1;
                    const int vn = (dlt ^ m_) - m_;
                    (void)__hip_atomic_fetch_add(QS_LDS(fixn_off), vn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);
        pf = QS_ADJ_FIRST;              // for the next gather pass
        __syncthreads();
        ++t;
    }
    if (fast && !converged) {
        // ---- the gather pass at t = max_iter (the loop left before it).  No scatter pass follows, so its minima, signs and argmin would be thrown
        // away; what is left is the parity of the hard decisions, the convergence test of the last iteration.  Steps beyond a check's degree read a
        // trash slot, which holds 0: they cannot set bit 31.  The pass's second minima do not enter mx2 either: they are magnitudes of messages of
        // iteration max_iter + 1, which nobody sends -- every sum that was computed is covered by the minima of the passes before.
        uint32_t us = 0u;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            QSW_GATHER_PRIO(j)
            if (act[j]) {
                int dwj = dws[j];
                asm volatile("" : "+s"(dwj));
                const int ng = (dwj & 0xFF) >> 2;
                const int adj_voff = cs[j] * 16;
                uint32_t hp = 0u, hpa = 0u;
#define QS_HP_GROUP(e4) { QS_HPA(QS_ACC(e4.x)) QS_HPB(QS_ACC(e4.y)) QS_HPA(QS_ACC(e4.z)) QS_HPB(QS_ACC(e4.w)) }
                uint4 nx = (j == 0) ? pf : QS_ADJ(0);
                int gi = 0;
#pragma unroll 1
                for (; gi + 2 <= ng; gi += 2) {               // two groups per trip on two register sets, as in the full pass
                    const uint4 eb = QS_ADJ(gi + 1);          // (the table has two spare group rows)
                    QS_HP_GROUP(nx)
                    nx = QS_ADJ(gi + 2);
                    QS_HP_GROUP(eb)
                }
                if (gi < ng) QS_HP_GROUP(nx)
#undef QS_HP_GROUP
                QSW_VOTE_ROUND(us, synd[j], hp)
            }
        }
        __builtin_amdgcn_s_setprio(0);
        int anyun;
        QSW_VOTE(us, anyun)
        if (!anyun) converged = 1;                  // (t = max_iter >= 1)
    }
#undef QSW_VOTE
#undef QSW_VOTE_ROUND
#undef QS_ADJ
#undef QS_ADJ_FIRST
#undef QS_FIX_ADDR
#undef QSW_GATHER_PRIO
    // L(t) - 1 is in the buffer: the scatter pass of the last iteration did not run

    // ---- did the bound hold?
    {
        const int tripped = qd_block_or(!(mx2 < x.m2_limit) ? 1 : 0, misc, NW, 0);
        if (tripped) {
            if (tid == 0) {
                const int at = atomicAdd(x.recheck_count, 1);
                if (at < x.recheck_cap) x.recheck_list[at] = (int32_t)shot;
            }
            return;
        }
    }
    // ---- hard decision, packed by fault index
    for (int b = tid; b < sg.nslots; b += T)
        if (*QS_LDS(cur + 4u * (uint32_t)b) < 0) {
            const uint32_t jf = sg.slot_fault[b];
            if (jf != 0xFFFFFFFFu) atomicOr(&outw[jf >> 5], 1u << (jf & 31u));   // (unused and trash slots stay at 0 today; never index LDS with their marker)
        }
    if (!converged && a.want_llr && tid == 0) misc[48] = atomicAdd(a.fail_count, 1);
    __syncthreads();
    for (int w = tid; w < g.out_words; w += T) a.err_bits[shot * g.out_words + w] = outw[w];
    if (!converged && a.want_llr) {
        const int slot = misc[48];
        float *dst = a.llr_ws + (int64_t)slot * n_pad;
        // (rows of the OSD workspace are in the gather kernel's bit-slot order: walk THAT order, so that the stores are whole lines)
        for (int k1 = tid; k1 < g.n; k1 += T) dst[k1] = (float)(*QS_LDS(cur + 4u * sg.k1_slot[k1]) + 1) * x.grid_inv;
        if (tid == 0) a.fail_list[slot] = (int32_t)shot;
    }
    if (tid == 0) a.status[shot] = t | (converged * QD_STATUS_CONVERGED) | a.status_or;
}

// ---- the first-pass table: gather pass 0 of every check slot, once per decoder (qd_decoder_create).  One wavefront per 64 consecutive check slots,
// as a round of the kernel above has them; the walk is that kernel's own program text with the accumulators read from the priors in global memory.
// A record is 8 words (ScatArgs::first_pass), so that a lane fetches its check with two 16-byte loads.
#undef QS_ACC
#define QS_ACC(off) (prior_g[((uint32_t)(off) - (uint32_t)sg.offA) >> 2])
#define QS_ADJ(row_) qs_as_uint4(__builtin_amdgcn_raw_buffer_load_b128(adj_rsrc, adj_voff, (row_) * adj_row, 0))
template <int NSW>
__global__ void __launch_bounds__(64) qd_bp_first_pass_kernel(BpGraphDev g, ScatGraphDev sg, const int32_t *prior_g, uint32_t *rec)
{
    static_assert(NSW == 3, "the record has room for three sign words");
    const int c = (int)blockIdx.x * 64 + (int)threadIdx.x;
    const bool actv = c < g.m;
    constexpr int j = 0;
    const int cs[1] = {c}, dws[1] = {__builtin_amdgcn_readfirstlane((int)sg.deg_w[blockIdx.x])}, dcs[1] = {actv ? (int)sg.chk_deg[c] : 0};
    const float S1[1] = {0.f}, S2[1] = {0.f};           // nothing has been sent
    const uint32_t KOLD[1] = {0xFFFFFFFFu}, O[1][NSW] = {{0u, 0u, 0u}};
    const __amdgpu_buffer_rsrc_t adj_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)sg.adjA, 0, (g.max_rdeg_pad / 4 + 2) * g.m_pad * 16, 0x00020000);
    const int adj_row = g.m_pad * 16;
    const uint4 pf = qs_as_uint4(__builtin_amdgcn_raw_buffer_load_b128(adj_rsrc, c * 16, 0, 0));
    float a1 = FLT_MAX, a2 = FLT_MAX;
    uint32_t kst = 0u;
    uint4 r0 = make_uint4(__float_as_uint(FLT_MAX), __float_as_uint(FLT_MAX), 0u, 0u);      // (a slot beyond the window: what the kernel's own pass leaves there)
    uint4 r1 = make_uint4(0u, 0u, 0u, (uint32_t)sg.offA + (uint32_t)(sg.nslots - 32 + (int)(threadIdx.x & 31)) * 4u);
    if (actv) {
#define QS_WALK(p_) QS_CMP_##p_
#include "bp_scatter_wide_walk.inc"
#undef QS_WALK
        (void)hp;
        r0 = make_uint4(__float_as_uint(a1), __float_as_uint(a2), kst, neg[0]);
        r1 = make_uint4(neg[1], neg[2], (uint32_t)__popc(par) & 1u,
                        __builtin_amdgcn_raw_buffer_load_b32(adj_rsrc, (int)((kst >> 2) * (uint32_t)adj_row + (kst & 3u) * 4u) + c * 16, 0, 0));
    }
    uint4 *out = reinterpret_cast<uint4 *>(rec) + 2 * c;
    out[0] = r0; out[1] = r1;
}
#undef QS_ADJ
#undef QS_ACC

// rec: [m_pad][8] words
hipError_t qd_launch_bp_first_pass(const BpGraphDev &g, const ScatGraphDev &sg, const int32_t *prior_g, uint32_t *rec, hipStream_t s)
{
    if (g.max_rdeg_pad > 96 || g.m_pad % 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qd_bp_first_pass_kernel<3>, dim3((unsigned)(g.m_pad / 64)), dim3(64), 0, s, g, sg, prior_g, rec);
    return hipGetLastError();
}

template <int T, int MW, int CPL, int NSW>
static hipError_t launch_scatter_wide_t(const BpGraphDev &g, const ScatGraphDev &sg, const DecodeArgs &a, const ScatArgs &x, int64_t B, hipStream_t s)
{
    auto k = qd_bp_scatter_wide_kernel<T, MW, CPL, NSW>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, sg.lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(T), sg.lds_bytes, s, g, sg, a, x);
    return hipGetLastError();
}

// (sg.wide_threads, sg.wide_cpl) is one of the shapes instantiated here (qd_graph_create chooses it); rows of up to 64 faults take two
// sign words, up to 96 three
hipError_t qd_launch_bp_scatter_wide(const BpGraphDev &g, const ScatGraphDev &sg, const DecodeArgs &a, const ScatArgs &x, int64_t B, hipStream_t s)
{
    const bool two_words = g.max_rdeg_pad <= 64;
    switch (sg.wide_threads * 8 + sg.wide_cpl) {
    case 512 * 8 + 2:           // headline-size windows (513..1024 checks) on half the lanes: four workgroups per CU
        return two_words ? launch_scatter_wide_t<512, 8, 2, 2>(g, sg, a, x, B, s) : hipErrorInvalidValue;
    case 256 * 8 + 2:           // 257..512 checks: eight workgroups per CU
        return two_words ? launch_scatter_wide_t<256, 8, 2, 2>(g, sg, a, x, B, s) : hipErrorInvalidValue;
    case 128 * 8 + 2:           // <= 256 checks: sixteen workgroups of two wavefronts per CU (ONE wavefront with four checks per lane, no barrier partner: 7.73 -> 8.99 ms on 216-check windows, profiles/r05_scatter_small_ab.txt)
        return two_words ? launch_scatter_wide_t<128, 8, 2, 2>(g, sg, a, x, B, s) : hipErrorInvalidValue;
    case 256 * 8 + 1:           // one check per lane: the windows whose LDS does not hold twice the workgroups, and QD_SCATTER_CPL1
        return two_words ? launch_scatter_wide_t<256, 8, 1, 2>(g, sg, a, x, B, s) : hipErrorInvalidValue;
    case 512 * 8 + 1:
        return two_words ? launch_scatter_wide_t<512, 8, 1, 2>(g, sg, a, x, B, s) : hipErrorInvalidValue;
    case 1024 * 8 + 1:
        return two_words ? launch_scatter_wide_t<1024, 8, 1, 2>(g, sg, a, x, B, s) : hipErrorInvalidValue;
    case 704 * 8 + 2:           // 11 wavefronts; two workgroups per CU: <= 6 per SIMD, 80 registers
        return launch_scatter_wide_t<704, 6, 2, 3>(g, sg, a, x, B, s);
    case 1024 * 8 + 2: return launch_scatter_wide_t<1024, 4, 2, 3>(g, sg, a, x, B, s);      // (a 64-register budget -- two workgroups of 16 wavefronts per CU -- measured no faster on the QLP windows and spills with the prefetch registers)
    case 512 * 8 + 3: return launch_scatter_wide_t<512, 4, 3, 3>(g, sg, a, x, B, s);      // QLP windows: 8 wavefronts x 3 rounds, 89 registers, two workgroups per CU
    default: return hipErrorInvalidValue;
    }
}
