// bp_relay.hip -- Relay-BP: flooding min-sum run as a chain of legs with per-fault memory strengths, one workgroup per shot, persistent
// over all legs; the shot stays on the CU from its syndrome to its answer.
//
// The definition and its CPU restatement: quits_amd/relay.py (relay_mirror) -- the two agree bit for bit (tests/test_gpu_relay.py).
//
// Layout: qd_bp_minsum_kernel's (bp_kernels.hip) -- a check keeps (min1, min2, argmin, per-edge sign bits) in 16 bytes of LDS, in the same three
// sign modes, faults read their checks through the same chunked records -- plus, per fault, a second float and, per shot, the best candidate:
//   llr[slot]  = P_j, what the check pass reads: Lam_j of the coming iteration plus the messages of the last one
//   marg[slot] = M_j, the marginal: Lam_j of the last iteration plus the same messages; kept from leg to leg
//   best[word] = the lightest candidate so far, packed by fault index
// The bit pass gathers a fault's messages once into registers and sums them twice, in ascending detector order both times: M_j from the
// Lam_j that was sent, then P_j from Lam'_j = a_j + gamma_j M_j ("posterior minus own message" reproduces the definition's fault->check
// message only from the NEW Lam).  a_j = (1 - gamma_j) L0_j is recomputed from the prior in the fault's record and the leg's row of the
// gamma table (slot order: coalesced).  No float atomics; the hard decisions' parity reaches the checks through the gather kernel's
// one-bit integer XOR.  A fault->check message counts as negative iff it is <= 0 as a float: -0.0 occurs here (gamma < 0).
#include "qd_internal.h"
#include "qd_host.h"
#include "../../include/quits_amd.h"
#include <float.h>

template <int I> __device__ __forceinline__ uint32_t rl_adj_get(const uint4 &v) { return I == 0 ? v.x : (I == 1 ? v.y : (I == 2 ? v.z : v.w)); }

// One edge of the check pass (bp_kernels.hip's QD_CHECK_EDGE with the float comparison for the sign)
#define RL_CHECK_EDGE(off, sb)                                                                               \
    {                                                                                                        \
        const float L_ = *(const __attribute__((address_space(3))) float *)(uintptr_t)(uint32_t)(off);       \
        const float mag_ = ((off) == idx_old) ? st.y : st.x;                                                 \
        const float prev_ = __uint_as_float(((sgnw >> (sb)) & 1u) << 31 | __float_as_uint(mag_));            \
        const float bm_ = L_ - prev_;                                                                        \
        const float ab_ = fabsf(bm_);                                                                        \
        neww = (neww << 1) | (bm_ <= 0.f ? 1u : 0u);                                                         \
        idx = (ab_ < a1) ? (off) : idx;                                                                      \
        a2 = __builtin_amdgcn_fmed3f(a1, a2, ab_);                                                           \
        a1 = fminf(a1, ab_);                                                                                 \
    }

typedef uint32_t rl_u32x4 __attribute__((ext_vector_type(4)));
// (explicit ds_read_b128 and its wait, as in bp_kernels.hip: the wait names the gathered registers so that nothing reads them early)
__device__ __forceinline__ rl_u32x4 rl_lds_gather16(uint32_t lds_addr)
{
    rl_u32x4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(lds_addr) : "memory");
    return v;
}
#define RL_LOAD(rec) rl_lds_gather16((rec) >> 16)
#define RL_WAIT1(a) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a) : : "memory")
#define RL_WAIT3(a, b, c) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c) : : "memory")
#define RL_WAIT4(a, b, c, d) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : : "memory")
#define RL_FLIP(rec) __hip_atomic_fetch_xor((__attribute__((address_space(3))) uint32_t *)(uintptr_t)(((rec) >> 16) + 12u), 0x40000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
// the check->fault message on one edge, from the gathered check state
#define RL_MSG(dst, rec, st_)                                                                                \
    {                                                                                                        \
        const uint32_t meta_ = (st_).w;                                                                      \
        const uint32_t mag_ = ((uint16_t)meta_ == mylabel) ? (st_).y : (st_).x;                              \
        uint32_t sg_;                                                                                        \
        if (SM == 2) {                                                                                       \
            uint32_t sw_ = (st_).z;                                                                          \
            if ((rec) & 0xE0u) sw_ = csgn_hi[((((rec) >> 5) & 7u) - 1u) * m_pad + ((rec) >> 20)];            \
            sg_ = sw_ >> ((rec) & 31u);                                                                      \
        } else if (SM == 1) {                                                                                \
            sg_ = (uint32_t)((((uint64_t)meta_ << 32) | (st_).z) >> ((rec) & 63u));                          \
        } else {                                                                                             \
            sg_ = (st_).z >> ((rec) & 31u);                                                                  \
        }                                                                                                    \
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

template <int T, int NCH, int SM, int MW>
__global__ void __launch_bounds__(T, MW) qd_bp_relay_kernel(BpGraphDev g, DecodeArgs a, RelayArgs x)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem;
    if (lds_base != 0u) __builtin_trap();   // no static LDS in this kernel: byte offsets into smem are LDS addresses
    float4 *chk = reinterpret_cast<float4 *>(smem + g.off_chk);
    uint32_t *csgn_hi = reinterpret_cast<uint32_t *>(smem + g.off_cneg);
    float *llr = reinterpret_cast<float *>(smem + g.off_llr);
    uint32_t *outw = reinterpret_cast<uint32_t *>(smem + g.off_out);
    int *misc = reinterpret_cast<int *>(smem + g.off_misc);   // [0..31] OR flags, [32] fail slot
    float *marg = reinterpret_cast<float *>(smem + x.off_marg);
    uint32_t *best = reinterpret_cast<uint32_t *>(smem + x.off_best);
    unsigned long long *wsum = reinterpret_cast<unsigned long long *>(smem + x.off_wsum);
    constexpr int NW = T / 64;

    const int tid = threadIdx.x;
    const int wave0 = __builtin_amdgcn_readfirstlane(tid & ~63);
    const int64_t shot = blockIdx.x;
    const uint8_t *det = a.det + shot * a.det_stride + a.det_offset;
    const uint8_t *upd = a.upd ? a.upd + shot * a.upd_stride : nullptr;
    const int m_pad = g.m_pad, n_pad = g.n_pad;
    const uint4 *rec4 = reinterpret_cast<const uint4 *>(g.bit_rec);
    const uint4 *adj4 = reinterpret_cast<const uint4 *>(g.chk_adj);
    const uint32_t llr_base = (uint32_t)g.off_llr;

    // ---- the window's syndrome; marginals = priors
    int any = 0;
    if (tid < 64) misc[tid] = 0;
    if (tid == 0) wsum[0] = 0ull;
    for (int c = tid; c < g.m; c += T) {
        const uint32_t o = g.chk_orig[c];
        uint32_t s = det[o] & 1u;
        if (upd && (int)o < a.upd_rows) s ^= upd[o] & 1u;
        any |= (int)s;
        chk[c] = make_float4(0.f, 0.f, __uint_as_float(0u), __uint_as_float(0xFFFFu | (s << 31)));
    }
    for (int b = tid; b < g.n; b += T) marg[b] = __uint_as_float(rec4[b].x);
    for (int w = tid; w < g.out_words; w += T) { outw[w] = 0u; best[w] = 0u; }
    if (tid == 0) {
        llr[g.dummy_bit] = __builtin_inff();                            // padding edge of a short row: never a minimum, never negative
        // padding edge of a short column: the message -0 in every sign mode (magnitude 0, every sign bit set), the identity of the sums
        chk[g.dummy_chk] = make_float4(0.f, 0.f, __uint_as_float(0xFFFFFFFFu), __uint_as_float(0x0FFFFFFFu));
    }
    __syncthreads();
    any = qd_block_or(any, misc, NW, 0);
    if (!any) {   // an all-zero syndrome returns the zero vector without running BP, as every decoder here does
        for (int w = tid; w < g.out_words; w += T) a.err_bits[shot * g.out_words + w] = 0u;
        if (tid == 0) a.status[shot] = QD_STATUS_CONVERGED | QD_STATUS_ZERO;
        return;
    }

    int total = 0, ncand = 0, best_leg = 0, leg = 0, phase = 1;
    long long best_w = 0x7FFFFFFFFFFFFFFFll;
    for (;; ++leg) {
        const int t_leg = leg == 0 ? x.pre_iter : x.set_max_iter;
        const float *grow = leg == 0 ? nullptr : x.gammas + (size_t)(leg - 1) * n_pad;
        // ---- start of a leg: every message +0, P_j = Lam_j (+ the zero messages) from the marginals the last leg left
        for (int c = tid; c < g.m; c += T) {
            const uint32_t synd = __float_as_uint(chk[c].w) >> 31;
            chk[c] = make_float4(0.f, 0.f, __uint_as_float(0u), __uint_as_float(0xFFFFu | (synd << 31)));
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
            // ---- check pass t+1; its parity test is the convergence test of iteration t
            bool unsat = false;
            for (int c = tid; c < g.m; c += T) {
                const float4 st = chk[c];
                const uint32_t meta = __float_as_uint(st.w);
                const uint32_t idx_old = llr_base + ((meta & 0xFFFFu) << 2);
                const uint32_t synd = meta >> 31;
                const int dw = g.chk_degp_w[__builtin_amdgcn_readfirstlane(c) >> 6];
                const int degp = dw & 0xFFFF, wmax = dw >> 16;
                const bool us = (((meta >> 31) ^ (meta >> 30)) & 1u) != 0u;
                uint32_t idx = llr_base + (0xFFFFu << 2);
                float a1 = FLT_MAX, a2 = FLT_MAX;
                uint32_t neg0 = 0u, neg1 = 0u, npar = 0u;
                for (int k0 = 0; k0 < degp; k0 += 32) {
                    uint32_t sgnw = __float_as_uint(st.z);
                    if (SM == 1 && k0 != 0) sgnw = (meta >> 16) & 0x0FFFu;
                    if (SM == 2 && k0 != 0) sgnw = csgn_hi[((k0 >> 5) - 1) * m_pad + c];
                    uint32_t neww = 0u;
                    const int kend = min(degp - k0, 32);                // multiple of 4
                    const uint4 *ap = adj4 + (size_t)(k0 >> 2) * m_pad + c;
                    uint4 nx = ap[0];
                    int kk = 0;
#pragma unroll 1
                    for (; kk + 4 < kend; kk += 4) {
                        const uint4 cur = nx;
                        nx = ap[(size_t)((kk >> 2) + 1) * m_pad];
                        const int sb = kend - 1 - kk;
                        RL_CHECK_EDGE(rl_adj_get<0>(cur), sb)
                        RL_CHECK_EDGE(rl_adj_get<1>(cur), sb - 1)
                        RL_CHECK_EDGE(rl_adj_get<2>(cur), sb - 2)
                        RL_CHECK_EDGE(rl_adj_get<3>(cur), sb - 3)
                    }
                    {
                        // last group: edges beyond the wavefront's largest degree are padding for every lane: only their zero sign bit is shifted in
                        const uint4 cur = nx;
                        const int real = wmax - (k0 + kk);
                        RL_CHECK_EDGE(rl_adj_get<0>(cur), 3)
                        if (real > 1) RL_CHECK_EDGE(rl_adj_get<1>(cur), 2) else neww <<= 1;
                        if (real > 2) RL_CHECK_EDGE(rl_adj_get<2>(cur), 1) else neww <<= 1;
                        if (real > 3) RL_CHECK_EDGE(rl_adj_get<3>(cur), 0) else neww <<= 1;
                    }
                    npar ^= neww;
                    if (k0 == 0) neg0 = neww;
                    else if (SM == 1) neg1 = neww;
                    else if (SM == 2) csgn_hi[((k0 >> 5) - 1) * m_pad + c] = neww;   // fixed up below once the parity is known
                }
                unsat |= us;
                // outgoing sign on edge k = syndrome ^ (parity of all incoming signs) ^ incoming sign k
                const uint32_t flip = 0u - ((synd ^ (uint32_t)__popc(npar)) & 1u);
                if (SM == 2)
                    for (int k0 = 32; k0 < degp; k0 += 32) csgn_hi[((k0 >> 5) - 1) * m_pad + c] ^= flip;
                uint32_t nmeta = ((idx - llr_base) >> 2) | (synd << 31);
                if (SM == 1) nmeta |= ((neg1 ^ flip) & 0x0FFFu) << 16;
                chk[c] = make_float4(a1 * alpha, a2 * alpha, __uint_as_float(neg0 ^ flip), __uint_as_float(nmeta));
            }
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
                const float aj = (1.0f - gam) * __uint_as_float(r0.x);
                float mg[16];
                {
                    rl_u32x4 s0 = RL_LOAD(r0.y), s1 = RL_LOAD(r0.z), s2 = RL_LOAD(r0.w);
                    RL_WAIT3(s0, s1, s2);
                    RL_MSG(mg[0], r0.y, s0) RL_MSG(mg[1], r0.z, s1) RL_MSG(mg[2], r0.w, s2)
                }
                if (g1) {
                    rl_u32x4 s0 = RL_LOAD(r1.x), s1 = RL_LOAD(r1.y), s2 = RL_LOAD(r1.z), s3 = RL_LOAD(r1.w);
                    RL_WAIT4(s0, s1, s2, s3);
                    RL_MSG(mg[3], r1.x, s0) RL_MSG(mg[4], r1.y, s1) RL_MSG(mg[5], r1.z, s2) RL_MSG(mg[6], r1.w, s3)
                }
                if (g2) {
                    rl_u32x4 s0 = RL_LOAD(r2.x), s1 = RL_LOAD(r2.y), s2 = RL_LOAD(r2.z), s3 = RL_LOAD(r2.w);
                    RL_WAIT4(s0, s1, s2, s3);
                    RL_MSG(mg[7], r2.x, s0) RL_MSG(mg[8], r2.y, s1) RL_MSG(mg[9], r2.z, s2) RL_MSG(mg[10], r2.w, s3)
                }
                if (g3) {
                    rl_u32x4 s0 = RL_LOAD(r3.x), s1 = RL_LOAD(r3.y), s2 = RL_LOAD(r3.z), s3 = RL_LOAD(r3.w);
                    RL_WAIT4(s0, s1, s2, s3);
                    RL_MSG(mg[11], r3.x, s0) RL_MSG(mg[12], r3.y, s1) RL_MSG(mg[13], r3.z, s2) RL_MSG(mg[14], r3.w, s3)
                }
                if (g4) {
                    rl_u32x4 s0 = RL_LOAD(r4.x);
                    RL_WAIT1(s0);
                    RL_MSG(mg[15], r4.x, s0)
                }
                float mj = aj + gam * marg[b];                       // the Lam_j these messages answer
                RL_SUM(mj)
                marg[b] = mj;
                float pj = aj + gam * mj;                            // Lam_j of the coming iteration
                RL_SUM(pj)
                llr[b] = pj;
                if (mj <= 0.f) {
                    // hard decision 1 (rare): one LDS atomic per edge on bit 30 of the check state's last word (the dummy check's is never read)
                    RL_FLIP(r0.y) RL_FLIP(r0.z) RL_FLIP(r0.w)
                    if (g1) { RL_FLIP(r1.x) RL_FLIP(r1.y) RL_FLIP(r1.z) RL_FLIP(r1.w) }
                    if (g2) { RL_FLIP(r2.x) RL_FLIP(r2.y) RL_FLIP(r2.z) RL_FLIP(r2.w) }
                    if (g3) { RL_FLIP(r3.x) RL_FLIP(r3.y) RL_FLIP(r3.z) RL_FLIP(r3.w) }
                    if (g4) { RL_FLIP(r4.x) }
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
    for (int b = tid; b < g.n; b += T)
        if (marg[b] <= 0.f) {
            const uint32_t j = g.bit_orig[b];
            atomicOr(&outw[j >> 5], 1u << (j & 31u));
        }
    if (a.want_llr && tid == 0) misc[32] = atomicAdd(a.fail_count, 1);
    __syncthreads();
    for (int w = tid; w < g.out_words; w += T) a.err_bits[shot * g.out_words + w] = outw[w];
    if (a.want_llr) {
        const int slot = misc[32];
        float *dst = a.llr_ws + (int64_t)slot * n_pad;
        for (int b = tid; b < g.n; b += T) dst[b] = marg[b];
        if (tid == 0) a.fail_list[slot] = (int32_t)shot;
    }
    if (tid == 0) a.status[shot] = total | (leg << QD_STATUS_RELAY_LEG_SHIFT);
}

// ---- launch wrappers: threads x record chunks x sign mode, as qd_launch_bp
// Waves per SIMD the register allocator leaves room for: 4 (128 registers) -- sixteen gathered messages are live across the two sums
template <int T, int NCH, int SM>
static hipError_t launch_relay_m(const BpGraphDev &g, const DecodeArgs &a, const RelayArgs &x, int64_t B, hipStream_t s)
{
    auto k = qd_bp_relay_kernel<T, NCH, SM, 4>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, x.lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(T), x.lds_bytes, s, g, a, x);
    return hipGetLastError();
}

template <int T, int NCH>
static hipError_t launch_relay_n(const BpGraphDev &g, const DecodeArgs &a, const RelayArgs &x, int64_t B, hipStream_t s)
{
    if (g.sign_mode == 0) return launch_relay_m<T, NCH, 0>(g, a, x, B, s);
    if (g.sign_mode == 1) return launch_relay_m<T, NCH, 1>(g, a, x, B, s);
    return launch_relay_m<T, NCH, 2>(g, a, x, B, s);
}

template <int T>
static hipError_t launch_relay_t(const BpGraphDev &g, const DecodeArgs &a, const RelayArgs &x, int64_t B, hipStream_t s)
{
    switch (g.rec_words / 4) {
    case 1: return launch_relay_n<T, 1>(g, a, x, B, s);
    case 2: return launch_relay_n<T, 2>(g, a, x, B, s);
    case 3: return launch_relay_n<T, 3>(g, a, x, B, s);
    default: return launch_relay_n<T, 5>(g, a, x, B, s);
    }
}

hipError_t qd_launch_bp_relay(const BpGraphDev &g, const DecodeArgs &a, const RelayArgs &x, int64_t B, hipStream_t s)
{
    switch (g.threads) {
    case 256: return launch_relay_t<256>(g, a, x, B, s);
    case 512: return launch_relay_t<512>(g, a, x, B, s);
    default: return launch_relay_t<1024>(g, a, x, B, s);
    }
}

// LDS of the relay kernel over the gather kernel's layout: marginals, best candidate, the 64-bit weight sum
int qd_relay_layout(const BpGraphDev &g, RelayArgs *x)
{
    int off = (g.lds_bytes + 15) & ~15;
    x->off_marg = off; off += ((g.n_pad + 1) * 4 + 15) & ~15;
    x->off_best = off; off += (g.out_words * 4 + 15) & ~15;
    x->off_wsum = off; off += 16;
    x->lds_bytes = off;
    return off;
}
