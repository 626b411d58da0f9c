// bp_scatter_edge.h -- the per-edge steps of the scatter form of flooding min-sum (gather pass: QS_EDGE_M / QS_EDGE_K, scatter pass: QS_SCAT) of
// qd_bp_scatter_wide_kernel and qd_bp_first_pass_kernel (bp_scatter_wide.hip, bp_scatter_wide_walk.inc).
// The macros work on the enclosing scope's names: s1, s2 (what the check sent last), a1, a2, ltw, neww, hp (what this pass
// collects), dc (the check's degree), n1, nx, own (scatter pass).  qs_reset_to_priors: the one copy of "accumulators := priors".
#pragma once
#include "qd_internal.h"
#include <float.h>

__device__ __forceinline__ float qs_min_abs(float a, float b)       // min(a, |b|) as one instruction (see bp_kernels.hip)
{
    float r;
    asm("v_min_f32 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
typedef uint32_t qs_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 qs_as_uint4(qs_u32x4 v) { return make_uint4(v.x, v.y, v.z, v.w); }
typedef __attribute__((address_space(3))) int32_t qs_lds_i32;
#define QS_LDS(off) ((qs_lds_i32 *)(uintptr_t)(uint32_t)(off))
#define QS_BIG 1.0e30f
#define QS_PRIO 1         // wavefront priority during the scatter pass (short, bound by the LDS): 53.4 -> 52.8 ms at the headline

// Gather pass, one edge.  off = LDS byte offset of the fault's accumulator (L - 1); k_ = position of the edge in the check's walk
// (wave-uniform); SGN_ = the sign of the message this check sent on the edge, at bit 31 (QS_SIGN_TOP: the walk keeps it at the top of the word that
// collects the new signs).
// d_ = (L - 1) - prev = bm - 1 is an integer-valued float, so (bm <= 0) is its sign bit (-0.0 cannot occur: an integer converted to float is never -0,
// and x - y is -0 only for x = -0).
// HP: how the accumulator's bits enter `hp` (only bit 31, the hard decision, is used): QS_HP1 one XOR per edge; QS_HPA / QS_HPB on the
// two edges of a pair -- the first is remembered in `hpa`, the second folds both in with one v_bitop3_b32 (a ^ b ^ c): half an instruction per edge
// QS_SIGN_TOP: bit 31 of `neww` as it stands (bp_scatter_wide_walk.inc starts neww at the sent word, first edge on top): no shift of its own, the v_alignbit
// that collects this edge's new sign brings the next edge's sent sign up (profiles/bp_sign_register_ab.txt).
// QS_ACC(off): the accumulator itself -- an LDS read in the kernels; the first-pass table (bp_scatter_wide.hip) redefines it to read the priors from
// global memory.
#define QS_ACC(off) (*QS_LDS(off))
#define QS_SIGN_TOP (neww & 0x80000000u)
#define QS_HP1(A_) hp ^= (uint32_t)(A_);
#define QS_HPA(A_) hpa = (uint32_t)(A_);
#define QS_HPB(A_) hp = __builtin_amdgcn_bitop3_b32(hp, hpa, (uint32_t)(A_), 0x96);
// MAG_: what this check sent on the edge last time, as a magnitude: min2 on its old argmin edge, min1 elsewhere.  QS_MAG_MASK(q_)
// (bp_scatter_wide_walk.inc) picks by lane masks kept in scalar registers, not with a compare per edge: `gsel_` = the lanes whose
// old argmin lies in this group of four edges (one v_cmp per group), `lq[q_]` = the lanes whose old argmin is edge q_ of its group (one v_cmp per
// check and pass); the AND runs on the scalar unit and the select takes the scalar pair as it is.
#define QS_MAG_MASK(q_) (__builtin_amdgcn_inverse_ballot_w64(gsel_ & lq[q_]) ? s2 : s1)
#define QS_EDGE_M(off, k_, SGN_, TAILFIX, HP, MAG_)                                                          \
    {                                                                                                        \
        const int A_ = QS_ACC(off);                                                                          \
        const float mag_ = MAG_;                                                                             \
        const float prev_ = __uint_as_float((SGN_) | __float_as_uint(mag_));                                 \
        float d_ = (float)A_ - prev_;                                                                        \
        TAILFIX(d_, k_)                                                                                      \
        const float bm_ = d_ + 1.0f;                                                                         \
        HP(A_)                                                                                               \
        neww = __builtin_amdgcn_alignbit(neww, __float_as_uint(d_), 31);                                     \
        /* ltw = ltw << 1 | (|bm| < a1): the argmin is the edge of the LAST strict improvement */           \
        asm("v_cmp_lt_f32 vcc, |%1|, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(ltw) : "v"(bm_), "v"(a1) : "vcc"); \
        a2 = __builtin_amdgcn_fmed3f(a1, a2, fabsf(bm_));                                                    \
        a1 = qs_min_abs(a1, bm_);                                                                            \
    }
// Gather pass, one edge, key form (rows of at most 64 faults): `a1`, `a2` hold the two smallest KEYS, key = |bm| + (1 + k_ / 64): the position rides in
// six fraction bits under the magnitude.  |bm| is an integer-valued float, so a key below 2^18 is exact (24 significant bits), its floor(key) - 1 is the
// magnitude and 64 * its fraction the position; equal magnitudes order by position, so the smallest key is the minimum at its FIRST position -- the edge
// of the last strict improvement -- and the second smallest carries min2, a tied one included.  One v_add_f32 (|bm| as a source modifier, the position
// constant wave-uniform) in place of the compare form's v_cmp_lt_f32 + v_addc_co_u32; no `ltw`.  (The same keys times 64, |bm| * 64 + (64 + k_), would be
// one v_fma_f32 -- but 64.0 is no inline constant, and a VOP3 reads one scalar register: the compiler moves the position constant into a vector
// register first, and the edge costs what the compare form costs.)  A key of 2^18 or more may have been rounded, but only to a value of 2^18 or more:
// the walk ends by testing the second key against QS_KEY_LIMIT (QS_KEYS_DECODE) and the caller walks the round again in the compare form where that
// fails.  1 + k / 64 for k = 0..63 lies in one binade: its bits are QS_KEY_POS0 + (k << 17), which the scalar unit steps with integer adds.
__device__ __forceinline__ float qs_min_f32(float a, float b)       // no canonicalising v_max in front of the v_min (the keys are never NaN)
{
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float qs_max_f32(float a, float b)       // likewise for the certificate's running maximum of the second minima
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
#define QS_KEY_POS0 0x3F800000u           // 1.0f
#define QS_KEY_LIMIT 262144.0f            // 2^18
#define QS_EDGE_K(off, k_, SGN_, TAILFIX, HP, MAG_)                                                          \
    {                                                                                                        \
        const int A_ = QS_ACC(off);                                                                          \
        const float mag_ = MAG_;                                                                             \
        const float prev_ = __uint_as_float((SGN_) | __float_as_uint(mag_));                                 \
        float d_ = (float)A_ - prev_;                                                                        \
        TAILFIX(d_, k_)                                                                                      \
        const float bm_ = d_ + 1.0f;                                                                         \
        HP(A_)                                                                                               \
        neww = __builtin_amdgcn_alignbit(neww, __float_as_uint(d_), 31);                                     \
        const float key_ = fabsf(bm_) + __uint_as_float(QS_KEY_POS0 + ((uint32_t)(k_) << 17));               \
        a2 = __builtin_amdgcn_fmed3f(a1, a2, key_);                                                          \
        a1 = qs_min_f32(a1, key_);                                                                           \
    }
// The end of a key-form walk: keys -> a1, a2, kst, and `keys_ok_` (wave-uniform: every lane's second key is below the limit, hence exact, hence
// both keys are the true two smallest).  The position is clamped below the trip count: a key that is not exact belongs to a pass that is walked
// again, but its position must never address the adjacency table or the LDS beyond the check's row.
#define QS_KEYS_DECODE(trip_)                                                                                \
    const bool keys_ok_ = __builtin_amdgcn_ballot_w64(!(a2 < QS_KEY_LIMIT)) == 0ull;                         \
    {                                                                                                        \
        const float f1_ = __builtin_floorf(a1), f2_ = __builtin_floorf(a2);                                  \
        kst = min((uint32_t)((a1 - f1_) * 64.0f), (uint32_t)max((trip_) - 1, 0));                            \
        a1 = f1_ - 1.0f; a2 = f2_ - 1.0f;                                                                    \
    }
// The two forms of the walk, part by part (bp_scatter_wide_walk.inc asks for QS_WALK(part); its includer says which family answers).
// Compare form: `ltw` per sign word, shifted at pad positions too; a later word's improvement overrides an earlier one's.
#define QS_CMP_EDGE QS_EDGE_M
#define QS_CMP_PAD { neww <<= 1; ltw <<= 1; }
#define QS_CMP_WORD_BEGIN uint32_t ltw = 0u;
#define QS_CMP_WORD_END(k0_, kend_) if (ltw) kst = (uint32_t)((k0_) + (kend_) - 1 - (int)__builtin_ctz(ltw));
#define QS_CMP_END(trip_)
// Key form: nothing per word, the decode at the end.
#define QS_KEY_EDGE QS_EDGE_K
#define QS_KEY_PAD { neww <<= 1; }
#define QS_KEY_WORD_BEGIN
#define QS_KEY_WORD_END(k0_, kend_)
#define QS_KEY_END(trip_) QS_KEYS_DECODE(trip_)
#define QS_NOFIX(x_, k_)
// beyond this lane's degree the walk reads the trash slot (0 for ever: no hard decision); the difference must be neither negative
// nor a minimum
#define QS_TAILFIX(x_, k_) x_ = ((int)(k_) < dc) ? x_ : QS_BIG;

// the scatter pass's one LDS operation per edge (a plain read, a plain store, an add of a constant or nothing in its place: profiles/r05_k1sw_ablation_bounds.txt)
#define QS_ADD(off, v_) (void)__hip_atomic_fetch_add(QS_LDS(off), v_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
// Scatter pass, one edge.  The accumulators stand at the priors when the pass begins (qs_reset_to_priors below), so an edge adds its new message
// and nothing else: +-min1 (the argmin edge is corrected after the loop).  `own` holds the new outgoing signs, edge k of the word at bit_;
// n1 = min1, nx = n1 ^ -n1 (once per check): n1 ^ (nx & sign mask) is n1 or -n1.  Two vector instructions and the LDS add.
#define QS_SCAT(off, k_, bit_, TAILFIX)                                                                      \
    {                                                                                                        \
        const int sm_ = __builtin_amdgcn_sbfe((int)own, bit_, 1);                                            \
        int v_ = (int)__builtin_amdgcn_bitop3_b32((uint32_t)n1, (uint32_t)nx, (uint32_t)sm_, 0x78);          /* n1 ^ (nx & sm) */ \
        TAILFIX(v_, k_)                                                                                      \
        QS_ADD(off, v_)                                                                                      \
    }
#define QS_TAILZERO(v_, k_) v_ = ((int)(k_) < dc) ? v_ : 0;

// Accumulators := priors (minus one), trash slots := 0: the image ScatArgs::prior_g, a constant of the decoder, copied into the accumulator region
// without passing through registers -- global_load_lds_dwordx4, 1 KB per wavefront instruction (the LDS destination is a wave-uniform base + 16 bytes
// per lane), the pieces dealt over the workgroup's NW wavefronts.  `nslots` is a multiple of 32 (graph_layout.hip: 32 banks), so the region is whole
// 16-byte units; in the last, partial piece the lanes beyond the region are switched off, so nothing is read behind prior_g and nothing is written
// behind the region (the output words follow it).  The copies are in flight when this returns: they count on vmcnt, and the caller's __syncthreads()
// waits for them (the compiler puts vmcnt(0) in front of a barrier while a load into LDS is pending) before any wavefront touches the region.
template <int NW>
__device__ __forceinline__ void qs_reset_to_priors(const int32_t *prior_g, uint32_t offA, int nslots, int tid)
{
    const int nbytes = nslots * 4;
    const int lane16 = (tid & 63) * 16;
    for (int p = __builtin_amdgcn_readfirstlane(tid >> 6) * 1024; p < nbytes; p += NW * 1024)
        if (p + lane16 < nbytes)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(reinterpret_cast<const char *>(prior_g) + p + lane16),
                                             (__attribute__((address_space(3))) void *)(uintptr_t)(offA + (uint32_t)p), 16, 0, 0);
}

