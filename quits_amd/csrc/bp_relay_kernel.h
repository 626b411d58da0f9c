// bp_relay_kernel.h -- Relay-BP: flooding min-sum run as a chain of legs with per-fault memory strengths, one workgroup per shot, persistent
// over all legs; the shot stays on the CU from its syndrome to its answer.  The kernel template of bp_relay.hip (marginals in LDS) and
// bp_relay_device.hip (marginals in a device-memory workspace): one kernel, two forms chosen by the compile-time parameter MD.
//
// The definition and its CPU restatement: quits_amd/relay.py (relay_mirror) -- both forms agree with it bit for bit (tests/test_gpu_relay.py,
// tests/test_gpu_relay_device_marginals.py).
//
// Layout: the gather form's (bp_gather_common.h, shared with qd_bp_minsum_kernel) -- a check keeps (min1, min2, argmin, per-edge sign bits) in
// 16 bytes of LDS, in the same three sign modes, faults read their checks through the same chunked records; check pass (in its float form),
// gathers, prologue and epilogue are that header's -- plus, per fault, a second float and, per shot, the best candidate:
//   llr[slot]  = P_j, what the check pass reads: Lam_j of the coming iteration plus the messages of the last one
//   marg[slot] = M_j, the marginal: Lam_j of the last iteration plus the same messages; kept from leg to leg
//   best[word] = the lightest candidate so far, packed by fault index
// llr and best are in LDS in both forms: the checks gather P_j from any lane.  M_j is only ever touched by the lane that owns the fault
// (slot b belongs to lane b mod T in every loop of this file and of the shared prologue / epilogue), so it needs no LDS:
//   MD = false  marg[] is n_pad + 1 floats of LDS behind the gather layout (RelayArgs::off_marg)
//   MD = true   marg[] is row `shot` of RelayArgs::marg_ws [cap][n_pad] in device memory, slot order: a wavefront's 64 lanes read and write
//               64 consecutive floats.  The bit pass issues its load with the record loads, ahead of the LDS gathers.
// The bit pass gathers a fault's messages once into registers and sums them twice, in ascending detector order both times: M_j from the
// Lam_j that was sent, then P_j from Lam'_j = a_j + gamma_j M_j ("posterior minus own message" reproduces the definition's fault->check
// message only from the NEW Lam).  a_j = (1 - gamma_j) L0_j is recomputed from the prior in the fault's record and the leg's row of the
// gamma table (slot order: coalesced).  No float atomics; the hard decisions' parity reaches the checks through the gather form's
// one-bit integer XOR.  A fault->check message counts as negative iff it is <= 0 as a float: -0.0 occurs here (gamma < 0).
#pragma once
#include "bp_gather_common.h"
#include "qd_host.h"

// the check->fault message on one edge, from the gathered check state
#define RL_MSG(dst, rec, st_)                                                                                \
    {                                                                                                        \
        uint32_t mag_, sg_;                                                                                  \
        qd_msg_decode<SM>(rec, st_, mylabel, csgn_hi, m_pad, mag_, sg_);                                     \
        dst = __uint_as_float(sg_ << 31 | mag_);                                                             \
    }
// the sum of a fault's messages onto `acc`, one at a time in ascending detector order (groups no fault of the wavefront reaches are skipped;
// inside a group the records beyond a fault's degree deliver -0, and x + (-0) = x for every x)
#define RL_SUM(acc)                                                                                          \
    {                                                                                                        \
        acc += mg[0]; acc += mg[1]; acc += mg[2];                                                            \
        if (NCH > 1 && g1) { acc += mg[3]; acc += mg[4]; acc += mg[5]; acc += mg[6]; }                       \
        if (NCH > 2 && g2) { acc += mg[7]; acc += mg[8]; acc += mg[9]; acc += mg[10]; }                      \
        if (NCH > 3 && g3) { acc += mg[11]; acc += mg[12]; acc += mg[13]; acc += mg[14]; }                   \
        if (NCH > 4 && g4) { acc += mg[15]; }                                                                \
    }

template <int T, int NCH, int SM, int MW, bool MD>
__global__ void __launch_bounds__(T, MW) qd_bp_relay_kernel(BpGraphDev g, DecodeArgs a, RelayArgs x)
{
    extern __shared__ __align__(16) unsigned char smem[];
    qd_require_lds_at_zero(smem);
    float4 *chk = reinterpret_cast<float4 *>(smem + g.off_chk);
    uint32_t *csgn_hi = reinterpret_cast<uint32_t *>(smem + g.off_cneg);
    float *llr = reinterpret_cast<float *>(smem + g.off_llr);
    uint32_t *outw = reinterpret_cast<uint32_t *>(smem + g.off_out);
    int *misc = reinterpret_cast<int *>(smem + g.off_misc);   // [0..31] OR flags, [32] fail slot
    uint32_t *best = reinterpret_cast<uint32_t *>(smem + x.off_best);
    unsigned long long *wsum = reinterpret_cast<unsigned long long *>(smem + x.off_wsum);
    constexpr int NW = T / 64;

    const int tid = threadIdx.x;
    const int wave0 = __builtin_amdgcn_readfirstlane(tid & ~63);
    const int64_t shot = blockIdx.x;
    const int m_pad = g.m_pad, n_pad = g.n_pad;
    const uint4 *rec4 = reinterpret_cast<const uint4 *>(g.bit_rec);
    // The shot's marginals.  MD: a row of the workspace, LANE-PRIVATE -- element b is read and written by lane b mod T alone, here (leg start,
    // bit pass, candidate weight, candidate bits) and in qd_gather_prologue's fill and qd_gather_publish's two loops, which walk b = tid + k T
    // like every loop below.  No barrier or fence orders these accesses and none is needed while that holds: a lane sees its own stores.
    typename qd_row<MD>::ptr marg;
    if constexpr (MD) marg = (typename qd_row<MD>::ptr)(x.marg_ws + (size_t)shot * n_pad);
    else marg = reinterpret_cast<float *>(smem + x.off_marg);

    // ---- the window's syndrome; marginals = priors.  Records beyond a fault's degree read the message -0 in every sign mode (magnitude 0,
    // every sign bit set): the identity of the sums
    if (tid == 0) wsum[0] = 0ull;
    for (int w = tid; w < g.out_words; w += T) best[w] = 0u;
    if (!qd_gather_prologue<T>(g, a, shot, chk, llr, marg, outw, misc,
                               make_float4(0.f, 0.f, __uint_as_float(0xFFFFFFFFu), __uint_as_float(0x0FFFFFFFu)), 0)) return;

    int total = 0, ncand = 0, best_leg = 0, leg = 0, phase = 1;
    long long best_w = 0x7FFFFFFFFFFFFFFFll;
    for (;; ++leg) {
        const int t_leg = leg == 0 ? x.pre_iter : x.set_max_iter;
        const float *grow = leg == 0 ? nullptr : x.gammas + (size_t)(leg - 1) * n_pad;
        // ---- start of a leg: every message +0, P_j = Lam_j (+ the zero messages) from the marginals the last leg left
        for (int c = tid; c < g.m; c += T) {
            const uint32_t synd = __float_as_uint(chk[c].w) >> 31;
            chk[c] = qd_chk_reset(synd);
            if (SM == 2)
                for (int w = 1; w < g.neg_words; ++w) csgn_hi[(w - 1) * m_pad + c] = 0u;
        }
        for (int b = tid; b < g.n; b += T) {
            const float gam = grow ? grow[b] : x.gamma0;
            const float aj = (1.0f - gam) * __uint_as_float(rec4[b].x);
            llr[b] = (aj + gam * marg[b]) + 0.0f;
        }
        __syncthreads();
        int t = 0, converged = 0;
        for (;;) {
            const float alpha = (a.ms_scale == 0.f) ? (1.0f - ldexpf(1.0f, -(t + 1))) : a.ms_scale;
            // ---- check pass t+1 in its float form, no early gathers; its parity test is the convergence test of iteration t
            const bool unsat = qd_check_pass<T, SM, /* FLOAT_SIGN */ true, /* PREGATHER */ false>(g, chk, csgn_hi, alpha);
            const int anyun = qd_block_or(unsat ? 1 : 0, misc, NW, phase);
            phase ^= 1;
            if (t >= 1 && !anyun) { converged = 1; break; }
            if (t == t_leg) break;
            // ---- bit pass t+1
            for (int base = 0; base < g.n; base += T) {
                const int b = base + tid;
                if (base + T > g.n && b >= g.n) break;
                const int b0 = base + wave0;
                const uint16_t mylabel = (uint16_t)b;
                const bool g1 = NCH > 1 && b0 < g.bit_thr[3], g2 = NCH > 2 && b0 < g.bit_thr[7], g3 = NCH > 3 && b0 < g.bit_thr[11],
                           g4 = NCH > 4 && b0 < g.bit_thr[15];
                const uint4 r0 = rec4[b];
                uint4 r1, r2, r3, r4;
                if (g1) r1 = rec4[n_pad + b];
                if (g2) r2 = rec4[2 * n_pad + b];
                if (g3) r3 = rec4[3 * n_pad + b];
                if (g4) r4 = rec4[4 * n_pad + b];
                const float gam = grow ? grow[b] : x.gamma0;
                float mprev;
                if constexpr (MD) mprev = marg[b];                  // device memory: in flight behind the LDS gathers
                const float aj = (1.0f - gam) * __uint_as_float(r0.x);
                float mg[16];
                {
                    qd_u32x4 s0 = qd_lds_gather16(r0.y), s1 = qd_lds_gather16(r0.z), s2 = qd_lds_gather16(r0.w);
                    qd_lds_wait(s0, s1, s2);
                    RL_MSG(mg[0], r0.y, s0) RL_MSG(mg[1], r0.z, s1) RL_MSG(mg[2], r0.w, s2)
                }
                if (g1) {
                    qd_u32x4 s0 = qd_lds_gather16(r1.x), s1 = qd_lds_gather16(r1.y), s2 = qd_lds_gather16(r1.z), s3 = qd_lds_gather16(r1.w);
                    qd_lds_wait(s0, s1, s2, s3);
                    RL_MSG(mg[3], r1.x, s0) RL_MSG(mg[4], r1.y, s1) RL_MSG(mg[5], r1.z, s2) RL_MSG(mg[6], r1.w, s3)
                }
                if (g2) {
                    qd_u32x4 s0 = qd_lds_gather16(r2.x), s1 = qd_lds_gather16(r2.y), s2 = qd_lds_gather16(r2.z), s3 = qd_lds_gather16(r2.w);
                    qd_lds_wait(s0, s1, s2, s3);
                    RL_MSG(mg[7], r2.x, s0) RL_MSG(mg[8], r2.y, s1) RL_MSG(mg[9], r2.z, s2) RL_MSG(mg[10], r2.w, s3)
                }
                if (g3) {
                    qd_u32x4 s0 = qd_lds_gather16(r3.x), s1 = qd_lds_gather16(r3.y), s2 = qd_lds_gather16(r3.z), s3 = qd_lds_gather16(r3.w);
                    qd_lds_wait(s0, s1, s2, s3);
                    RL_MSG(mg[11], r3.x, s0) RL_MSG(mg[12], r3.y, s1) RL_MSG(mg[13], r3.z, s2) RL_MSG(mg[14], r3.w, s3)
                }
                if (g4) {
                    qd_u32x4 s0 = qd_lds_gather16(r4.x);
                    qd_lds_wait(s0);
                    RL_MSG(mg[15], r4.x, s0)
                }
                if constexpr (!MD) mprev = marg[b];
                float mj = aj + gam * mprev;                         // the Lam_j these messages answer
                RL_SUM(mj)
                marg[b] = mj;
                float pj = aj + gam * mj;                            // Lam_j of the coming iteration
                RL_SUM(pj)
                llr[b] = pj;
                if (mj <= 0.f) {
                    // hard decision 1 (rare): one LDS atomic per edge on bit 30 of the check state's last word (the dummy check's is never read)
                    qd_flip_bit30(r0.y); qd_flip_bit30(r0.z); qd_flip_bit30(r0.w);
                    if (g1) qd_flip_bit30x4(r1);
                    if (g2) qd_flip_bit30x4(r2);
                    if (g3) qd_flip_bit30x4(r3);
                    if (g4) qd_flip_bit30(r4.x);
                }
            }
            __syncthreads();
            ++t;
        }
        total += t;
        if (converged) {
            // ---- a candidate: e_j = [M_j <= 0], weight sum_j e_j llround(L0_j 2^16) in 64-bit integers (integer atomics: any order, one sum)
            long long wl = 0;
            for (int b = tid; b < g.n; b += T)
                if (marg[b] <= 0.f) wl += llround((double)__uint_as_float(rec4[b].x) * 65536.0);
            if (wl != 0) atomicAdd(wsum, (unsigned long long)wl);
            __syncthreads();
            const long long cw = (long long)wsum[0];
            ++ncand;
            const bool better = cw < best_w;                       // uniform
            if (better)
                for (int w = tid; w < g.out_words; w += T) best[w] = 0u;
            __syncthreads();
            if (tid == 0) wsum[0] = 0ull;
            if (better) {
                best_w = cw; best_leg = leg;
                for (int b = tid; b < g.n; b += T)
                    if (marg[b] <= 0.f) {
                        const uint32_t j = g.bit_orig[b];
                        atomicOr(&best[j >> 5], 1u << (j & 31u));
                    }
            }
            if (ncand >= x.stop_nconv) break;
        }
        if (leg == x.num_sets) break;
    }

    if (ncand > 0) {
        __syncthreads();
        for (int w = tid; w < g.out_words; w += T) a.err_bits[shot * g.out_words + w] = best[w];
        if (tid == 0) a.status[shot] = total | QD_STATUS_CONVERGED | (best_leg << QD_STATUS_RELAY_LEG_SHIFT);
        return;
    }
    // ---- no candidate: the hard decision of the last iteration; the marginals are parked for the decoder's post-processor
    qd_gather_publish<T>(g, a, shot, marg, outw, misc, a.want_llr != 0);
    if (tid == 0) a.status[shot] = total | (leg << QD_STATUS_RELAY_LEG_SHIFT);
}

// ---- launch of one form.  Waves per SIMD the register allocator leaves room for: 4 (128 registers) -- sixteen gathered messages are live
// across the two sums
template <bool MD>
static hipError_t qd_relay_launch_form(const BpGraphDev &g, const DecodeArgs &a, const RelayArgs &x, int64_t B, hipStream_t s)
{
    return qd_gather_dispatch(g, [&](auto t, auto nch, auto sm) {
        constexpr int T = decltype(t)::value;
        return qd_gather_launch(qd_bp_relay_kernel<T, decltype(nch)::value, decltype(sm)::value, 4, MD>, T, x.lds_bytes, B, s, g, a, x);
    });
}
