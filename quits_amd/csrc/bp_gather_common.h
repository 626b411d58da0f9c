// bp_gather_common.h -- the gather-form min-sum machinery, defined once for the kernels built on it: qd_bp_minsum_kernel (bp_kernels.hip)
// and qd_bp_relay_kernel (bp_relay.hip).  This file is the single definition of the check-state layout.
//
// State of a check in LDS (16 bytes, one ds_read_b128):  x = min1 * alpha,  y = min2 * alpha,
//   z = SIGN bits of the outgoing messages on edges 0..31; inside a word, edge k sits at bit (edges_in_word - 1 - k)
//       (sign of check->bit message k = syndrome ^ parity of all incoming signs ^ incoming sign k),
//   w = slot of the argmin fault (bits 0..15) | (sign mode 1: sign bits of edges 32..43) << 16 | parity of the hard decisions of
//       the check's faults << 30 (flipped by the bit pass) | syndrome bit << 31.
// Sign mode 0: checks of at most 32 faults.  Sign mode 2 (checks wider than 44): edges 32.. keep their sign words in `csgn_hi`.
// Everything here is inlined into the two kernels: registers, occupancy and code size by instantiation in profiles/bp_gather_shared_resources.txt.
#pragma once
#include "qd_internal.h"
#include "../../include/quits_amd.h"
#include <float.h>
#include <type_traits>

// Four LDS byte offsets per vector load of the ELL-transposed check adjacency
template <int I> __device__ __forceinline__ uint32_t qd_adj_get(const uint4 &v) { return I == 0 ? v.x : (I == 1 ? v.y : (I == 2 ? v.z : v.w)); }

// The kernels' dynamic LDS must start at LDS address 0 (no static LDS in them): byte offsets into smem are then LDS addresses, and the
// packed offsets of the adjacency and of the fault records are used as addresses as they are.
__device__ __forceinline__ void qd_require_lds_at_zero(unsigned char *smem)
{
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem != 0u) __builtin_trap();
}
__device__ __forceinline__ float qd_lds_f32(uint32_t lds_addr) { return *(const __attribute__((address_space(3))) float *)(uintptr_t)lds_addr; }

// min(a, |b|) as the single instruction it is: fminf() makes the compiler quiet a possible signalling NaN first
// (v_max_f32 x, x, x -- one more 4-clock instruction per four edges); neither operand can be a NaN here.
__device__ __forceinline__ float qd_min_abs(float a, float b)
{
    float r;
    asm("v_min_f32 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// ---- bit pass primitives.  A fault's record word: rec = (LDS byte offset of the check state) << 16 | where its sign lives.
// The gather is issued as explicit ds_read_b128: left to the compiler, the {z, w} pair is peeled off into its own
// 64-bit load and the state arrives as ds_read2_b64, which measured 40% slower for the whole kernel.  qd_lds_wait
// is the matching s_waitcnt; it names the gathered registers so that nothing reads them early.
typedef uint32_t qd_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ qd_u32x4 qd_lds_gather16(uint32_t rec)
{
    qd_u32x4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(rec >> 16) : "memory");
    return v;
}
__device__ __forceinline__ void qd_lds_wait(qd_u32x4 &a) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a) : : "memory"); }
__device__ __forceinline__ void qd_lds_wait(qd_u32x4 &a, qd_u32x4 &b) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b) : : "memory"); }
__device__ __forceinline__ void qd_lds_wait(qd_u32x4 &a, qd_u32x4 &b, qd_u32x4 &c) { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c) : : "memory"); }
__device__ __forceinline__ void qd_lds_wait(qd_u32x4 &a, qd_u32x4 &b, qd_u32x4 &c, qd_u32x4 &d)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : : "memory");
}
// a fault decided to be 1 tells the check of one record: one LDS atomic on bit 30 of the state's last word
// (records beyond the degree point at the dummy check; readers of the word ignore that bit)
__device__ __forceinline__ void qd_flip_bit30(uint32_t rec)
{
    __hip_atomic_fetch_xor((__attribute__((address_space(3))) uint32_t *)(uintptr_t)((rec >> 16) + 12u), 0x40000000u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <typename REC4> __device__ __forceinline__ void qd_flip_bit30x4(const REC4 &r)   // the four records of one chunk
{
    qd_flip_bit30(r.x); qd_flip_bit30(r.y); qd_flip_bit30(r.z); qd_flip_bit30(r.w);
}
// The check->fault message of one record from the gathered state: magnitude = min2 if this fault is the check's argmin, else min1;
// bit 0 of `sg` = the check's outgoing sign on this edge (the bits above it are whatever the shift left there).  In sign mode 1
// {z, w} is one 64-bit value (signs 0..31 | argmin slot | signs 32..43 | ...), so the sign is a single 64-bit shift by the bit index
// the record carries.
template <int SM>
__device__ __forceinline__ void qd_msg_decode(uint32_t rec, const qd_u32x4 &st, uint16_t mylabel, const uint32_t *csgn_hi, int m_pad,
                                              uint32_t &mag, uint32_t &sg)
{
    const uint32_t meta = st.w;
    mag = ((uint16_t)meta == mylabel) ? st.y : st.x;
    if (SM == 2) {
        uint32_t sw = st.z;
        if (rec & 0xE0u) sw = csgn_hi[(((rec >> 5) & 7u) - 1u) * m_pad + (rec >> 20)];
        sg = sw >> (rec & 31u);
    } else if (SM == 1) {
        sg = (uint32_t)((((uint64_t)meta << 32) | st.z) >> (rec & 63u));
    } else {
        sg = st.z >> (rec & 31u);
    }
}

// ---- check pass t+1 of a workgroup of T lanes, lane = check: min1, min2, argmin and the outgoing signs of every check from the posteriors
// in LDS.  Returns this lane's vote in the convergence test of iteration t: the bit pass flips bit 30 of a check's last word once for
// every fault on it that it decided to be 1 (a few dozen faults per shot), so the parity test costs nothing per edge here.
// One edge (qd_check_edge):
//   off  = LDS address of the fault's posterior L (doubles as the edge's label for the argmin bookkeeping)
//   sb   = bit of `sgnw` that holds the sign of the previous check->bit message on this edge
// Branch-free: the second minimum is the median of (min1, min2, |b|); the new sign bits are shifted in from bit 0.
// Grid form (FLOAT_SIGN = false): (b <= 0) is taken as the sign bit of (bits(b) - 1): exact for every float except -0.0, which cannot
// occur in the min-sum kernel: a prior that rounds to zero is uploaded as +0 (qd_decoder.hip, on_grid), sums and differences of values
// that are not -0 only yield -0 from (-0) - (+0), and a message's sign is ORed onto a magnitude only where it is read, never stored as
// a float.  Float form (FLOAT_SIGN = true): the comparison itself and fminf; the relay's messages can equal -0.0 (gamma < 0).
// PREGATHER: the four posteriors of a trip are gathered before any is used (wide checks, > 44 faults: the QLP windows, one workgroup
// per CU, four wavefronts per SIMD).  +3 % there; -3 % at the headline window, where eight wavefronts per SIMD hide the gather's
// latency and the early loads only add register pressure -- so the min-sum kernel turns it on in sign mode 2 only.
template <bool FLOAT_SIGN>
__device__ __forceinline__ void qd_check_edge(uint32_t off, int sb, float L, float min1, float min2, uint32_t idx_old, uint32_t sgnw,
                                              uint32_t &neww, uint32_t &idx, float &a1, float &a2)
{
    const float mag = (off == idx_old) ? min2 : min1;
    const float prev = __uint_as_float(((sgnw >> sb) & 1u) << 31 | __float_as_uint(mag));
    const float bm = L - prev;                  // bit->check message, "total minus own"
    const float ab = fabsf(bm);
    if (FLOAT_SIGN) neww = (neww << 1) | (bm <= 0.f ? 1u : 0u);
    else neww = __builtin_amdgcn_alignbit(neww, __float_as_uint(bm) - 1u, 31);   // neww = neww << 1 | (bm <= 0)
    idx = (ab < a1) ? off : idx;
    a2 = __builtin_amdgcn_fmed3f(a1, a2, ab);
    a1 = FLOAT_SIGN ? fminf(a1, ab) : qd_min_abs(a1, bm);
}
// (a function of plain values on purpose: with the float4 passed by reference, or as a lambda in the check pass that captures the running
// state, the check pass loads its 16-byte state as two ds_read_b64 and every instantiation grows by 8-16 bytes)
#define QD_EDGE(I, sb, L) qd_check_edge<FLOAT_SIGN>(qd_adj_get<I>(cur), sb, L, st.x, st.y, idx_old, sgnw, neww, idx, a1, a2)
#define QD_EDGE_AT(I, sb) QD_EDGE(I, sb, qd_lds_f32(qd_adj_get<I>(cur)))
template <int T, int SM, bool FLOAT_SIGN, bool PREGATHER>
__device__ __forceinline__ bool qd_check_pass(const BpGraphDev &g, float4 *chk, uint32_t *csgn_hi, float alpha)
{
    const int m_pad = g.m_pad;
    const uint4 *adj4 = reinterpret_cast<const uint4 *>(g.chk_adj);
    const uint32_t llr_base = (uint32_t)g.off_llr;
    bool unsat = false;
    for (int c = threadIdx.x; c < g.m; c += T) {
        const float4 st = chk[c];
        const uint32_t meta = __float_as_uint(st.w);
        const uint32_t idx_old = llr_base + ((meta & 0xFFFFu) << 2);   // label = LDS offset of the argmin fault's posterior
        const uint32_t synd = meta >> 31;
        const int dw = g.chk_degp_w[__builtin_amdgcn_readfirstlane(c) >> 6];       // scalar load
        const int degp = dw & 0xFFFF, wmax = dw >> 16;                             // trip count (multiple of 4), largest degree in this wavefront
        const bool us = (((meta >> 31) ^ (meta >> 30)) & 1u) != 0u;                // syndrome of the hard decision
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
                nx = ap[(size_t)((kk >> 2) + 1) * m_pad];                       // next four fault offsets while these are processed
                const int sb = kend - 1 - kk;
                if constexpr (PREGATHER) {
                    float g0, g1, g2, g3;
                    asm volatile("ds_read_b32 %0, %1" : "=v"(g0) : "v"(qd_adj_get<0>(cur)) : "memory");
                    asm volatile("ds_read_b32 %0, %1" : "=v"(g1) : "v"(qd_adj_get<1>(cur)) : "memory");
                    asm volatile("ds_read_b32 %0, %1" : "=v"(g2) : "v"(qd_adj_get<2>(cur)) : "memory");
                    asm volatile("ds_read_b32 %0, %1" : "=v"(g3) : "v"(qd_adj_get<3>(cur)) : "memory");
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(g0), "+v"(g1), "+v"(g2), "+v"(g3) : : "memory");
                    QD_EDGE(0, sb, g0); QD_EDGE(1, sb - 1, g1);
                    QD_EDGE(2, sb - 2, g2); QD_EDGE(3, sb - 3, g3);
                } else {
                    QD_EDGE_AT(0, sb); QD_EDGE_AT(1, sb - 1);
                    QD_EDGE_AT(2, sb - 2); QD_EDGE_AT(3, sb - 3);
                }
            }
            {
                // last group: edges beyond the wavefront's largest degree are padding for every lane (posterior +inf:
                // never a minimum, never negative) -- only their zero sign bit is shifted in
                const uint4 cur = nx;
                const int real = wmax - (k0 + kk);                              // 1..4 (or more in a non-final word)
                QD_EDGE_AT(0, 3);
                if (real > 1) QD_EDGE_AT(1, 2); else neww <<= 1;
                if (real > 2) QD_EDGE_AT(2, 1); else neww <<= 1;
                if (real > 3) QD_EDGE_AT(3, 0); else neww <<= 1;
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
        if (SM == 1) nmeta |= ((neg1 ^ flip) & 0x0FFFu) << 16;      // at most 44 edges: signs 32..43 in bits 16..27; bit 30 is the decision parity
        chk[c] = make_float4(a1 * alpha, a2 * alpha, __uint_as_float(neg0 ^ flip), __uint_as_float(nmeta));
    }
    return unsat;
}
#undef QD_EDGE
#undef QD_EDGE_AT

// a check that has received no message yet: min1 = min2 = 0, every sign +, no argmin, the decision parity even
__device__ __forceinline__ float4 qd_chk_reset(uint32_t synd)
{
    return make_float4(0.f, 0.f, __uint_as_float(0u), __uint_as_float(0xFFFFu | (synd << 31)));
}

// ---- prologue: the window's syndrome of `shot` (sliding_window.py:168-169, with the carried update) into reset check states, the priors
// into `prior_dst`, the output words and the OR flags cleared, the two dummies set.  `dummy_chk` is the state records beyond a fault's
// degree point at.  Holds the barrier that publishes all of it, and whatever the caller initialised before the call.  An all-zero
// syndrome returns the zero vector without running BP (bposd_decoder.pyx): the answer is written here, with `status_or` in the status
// word, and the function returns false -- the workgroup is done.
// (g and a by value, here and in qd_gather_publish: taken by reference, the min-sum kernel's two scalar loads of the redo pass's shot list
// become vector loads)
//
// A row of one float per fault slot (`prior_dst` here, `vals` in qd_gather_publish) is in LDS or in device memory, by its pointer type:
// qd_row<false>::ptr, a plain pointer into the kernel's LDS (the compiler follows it to ds_* accesses), or qd_row<true>::ptr, a pointer
// into the global address space (global_* accesses, never flat).  A device-memory row is LANE-PRIVATE: both functions touch element b from
// lane b mod T only (b = tid + k T), no barrier publishes it, and the prologue fills it only for a shot that goes on to run BP, behind the
// all-zero test -- a shot that returns there leaves its row as it was.
typedef __attribute__((address_space(1))) float qd_global_f32;
template <bool DEVICE> struct qd_row { typedef float *ptr; };
template <> struct qd_row<true> { typedef qd_global_f32 *ptr; };
template <typename ROW> inline constexpr bool qd_row_in_device_memory = std::is_same<std::remove_cv_t<std::remove_pointer_t<ROW>>, qd_global_f32>::value;

template <int T, typename ROW>
__device__ __forceinline__ bool qd_gather_prologue(const BpGraphDev g, const DecodeArgs a, int64_t shot, float4 *chk, float *llr, ROW prior_dst,
                                                   uint32_t *outw, int *misc, float4 dummy_chk, int status_or)
{
    constexpr bool ROW_DEVICE = qd_row_in_device_memory<ROW>;
    const int tid = threadIdx.x;
    const uint8_t *det = a.det + shot * a.det_stride + a.det_offset;
    const uint8_t *upd = a.upd ? a.upd + shot * a.upd_stride : nullptr;
    const uint4 *rec4 = reinterpret_cast<const uint4 *>(g.bit_rec);
    int any = 0;
    if (tid < 64) misc[tid] = 0;
    for (int c = tid; c < g.m; c += T) {
        const uint32_t o = g.chk_orig[c];
        uint32_t s = det[o] & 1u;
        if (upd && (int)o < a.upd_rows) s ^= upd[o] & 1u;
        any |= (int)s;
        chk[c] = qd_chk_reset(s);
    }
    if constexpr (!ROW_DEVICE)
        for (int b = tid; b < g.n; b += T) prior_dst[b] = __uint_as_float(rec4[b].x);
    for (int w = tid; w < g.out_words; w += T) outw[w] = 0u;
    if (tid == 0) {
        llr[g.dummy_bit] = __builtin_inff();        // padding edge of a short row: |b| = inf, never a minimum, never negative
        chk[g.dummy_chk] = dummy_chk;               // padding edge of a short column
    }
    __syncthreads();
    any = qd_block_or(any, misc, T / 64, 0);
    if (!any) {
        for (int w = tid; w < g.out_words; w += T) a.err_bits[shot * g.out_words + w] = 0u;
        if (tid == 0) a.status[shot] = QD_STATUS_CONVERGED | QD_STATUS_ZERO | status_or;
    } else if constexpr (ROW_DEVICE)
        for (int b = tid; b < g.n; b += T) prior_dst[b] = __uint_as_float(rec4[b].x);
    return any != 0;
}

// ---- epilogue of a shot that returns a hard decision: [vals <= 0] packed by fault index into err_bits; with `park`, the values
// themselves go to a row of llr_ws and the shot onto fail_list for the post-processor.  misc[32] carries the fail slot.
template <int T, typename ROW>
__device__ __forceinline__ void qd_gather_publish(const BpGraphDev g, const DecodeArgs a, int64_t shot, const ROW vals, uint32_t *outw,
                                                  int *misc, bool park)
{
    const int tid = threadIdx.x;
    for (int b = tid; b < g.n; b += T)
        if (vals[b] <= 0.f) {
            const uint32_t j = g.bit_orig[b];
            atomicOr(&outw[j >> 5], 1u << (j & 31u));
        }
    if (park && tid == 0) misc[32] = atomicAdd(a.fail_count, 1);
    __syncthreads();
    for (int w = tid; w < g.out_words; w += T) a.err_bits[shot * g.out_words + w] = outw[w];
    if (park) {
        const int slot = misc[32];
        float *dst = a.llr_ws + (int64_t)slot * g.n_pad;
        for (int b = tid; b < g.n; b += T) dst[b] = vals[b];
        if (tid == 0) a.fail_list[slot] = (int32_t)shot;
    }
}

// ---- launch: (g.threads, g.rec_words / 4, g.sign_mode) -> compile-time (T, NCH, SM) in {256, 512, 1024} x {1, 2, 3, 5} x {0, 1, 2};
// `f` is called with three std::integral_constant arguments and returns the launch's hipError_t.
template <int V> using qd_int = std::integral_constant<int, V>;
template <typename F> static hipError_t qd_gather_dispatch(const BpGraphDev &g, F f)
{
    const int sm = g.sign_mode, chunks = g.rec_words / 4;
    auto by_sm = [&](auto t, auto nch) { return sm == 0 ? f(t, nch, qd_int<0>{}) : (sm == 1 ? f(t, nch, qd_int<1>{}) : f(t, nch, qd_int<2>{})); };
    auto by_nch = [&](auto t) {
        return chunks == 1 ? by_sm(t, qd_int<1>{}) : (chunks == 2 ? by_sm(t, qd_int<2>{}) : (chunks == 3 ? by_sm(t, qd_int<3>{}) : by_sm(t, qd_int<5>{})));
    };
    return g.threads == 256 ? by_nch(qd_int<256>{}) : (g.threads == 512 ? by_nch(qd_int<512>{}) : by_nch(qd_int<1024>{}));
}
// one workgroup of T lanes per shot with lds_bytes of dynamic LDS
template <typename... P, typename... A>
static hipError_t qd_gather_launch(void (*k)(P...), int T, int lds_bytes, int64_t B, hipStream_t s, const A &...args)
{
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(T), lds_bytes, s, args...);
    return hipGetLastError();
}
