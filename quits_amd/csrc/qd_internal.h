// qd_internal.h -- device-side views shared by the kernels and the C-ABI host code (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qd_graph_views.h"

#define QD_WAVE 64

struct ScatArgs {
    const int32_t *prior_g;     // [n_pad] channel LLR of the bit slot in grid units (llr * 2^k, an integer) MINUS ONE: the accumulators hold L - 1
    float grid_inv;             // 2^-k
    float m2_limit;             // the run is certified exact while every check's second minimum stays below it (grid units)
    int32_t *recheck_list;      // shots the cheap bound could not certify: decoded again by qd_bp_minsum_kernel, which carries the per-fault bound
    int32_t *recheck_count;
    int recheck_cap;
    const uint32_t *first_pass; // [m_pad][8] what gather pass 0 finds for each check slot, the same for every shot (qd_bp_first_pass_kernel, bp_scatter_wide.hip):
                                //   a1, a2 (float bits), argmin position, sign words 0..2, parity of all signs, LDS offset of the argmin edge's accumulator.
                                //   null: the kernel runs pass 0 itself and the full last pass (QD_BP_NO_FAST_START)
};

// ... and its per-chunk workspace, [index][shot] with S shots per row
struct GenWs {
    float *b2c, *c2b, *th, *llr;    // [nnz][S] x 3 (th: product-sum only; b2c: not for serial product-sum, which keeps tanh(b2c/2) alone), [n][S]
    float *pre;                     // [m][S]  serial schedule: running prefix of each row (product / minimum + sign parity)
    uint8_t *syn;                   // [m][S]
    int32_t *slot;                  // [S]  fail-list slot of a shot BP could not finish, else -1
    int64_t S;
};
// One launch of the serial schedule = iterations it0 + 1 .. it_end of the shots in its columns.  A launch that is not the last hands the
// shots that have not converged on, PACKED: their state between two sweeps is the message plane and the syndrome plane, nothing else (suffixes,
// prefixes and posteriors are rebuilt by every sweep), so the survivors' columns of those two planes are copied to consecutive columns of `next`
// and the next launch runs on full wavefronts (bp.hpp's shot loop has no such problem: one shot, one thread; here a lane that has converged
// idles until the slowest of its 64 shots is done -- 31 % of the lanes of the reference-settings windows, profiles/r05_k1g_load_curve.txt).
// hipEventQuery without side effects: "not ready" is an answer, not an error -- it must not be what a later hipGetLastError() behind a kernel launch reports
static inline bool qd_event_done(hipEvent_t e)
{
    const hipError_t r = hipEventQuery(e);
    if (r != hipSuccess) (void)hipGetLastError();
    return r == hipSuccess;
}
#define QD_GEN_MAX_STAGES 12
struct GenStagePlan;
struct GenStage {
    const int32_t *in_shot;     // [columns] the shot (index into the batch) of each column; nullptr: column c holds shot shot0 + c (first launch)
    const int32_t *in_count;    // columns in use (device); nullptr: nshots
    int32_t *out_shot;          // the survivors' shots, by column of `next`
    int32_t *out_count;
    int it0, it_end, last;      // last: it_end is max_iter -- shots still running are BP failures, there is no next launch
    GenWs next;
};
struct GenStagePlan {           // host side: the iteration bounds between the launches and what they hand over
    int nbounds;
    int bounds[QD_GEN_MAX_STAGES];
    GenWs w2;                   // the workspace of the odd launches: its own message and syndrome planes (msg2, syn2), everything else shared with the first
    float *msg2;
    uint8_t *syn2;
    int32_t *lists[2];          // [S] each
    int32_t *counts;            // [QD_GEN_MAX_STAGES + 1]
    // what the last staged call packed, read back without waiting (pinned copy + event): a decoder whose shots do not converge -- a window far above
    // threshold -- gains nothing from packing and pays the copies; it then runs in one launch and tries again every QD_GEN_PROBE calls.  Same results either way.
    int32_t *host_counts;
    hipEvent_t counts_ready;
    int pending, pending_shots, pending_nb;
    int one_launch_calls;
};
#define QD_GEN_PROBE 16

struct DecodeArgs {
    const uint8_t *det;         // [B][det_stride] one byte per detector
    int64_t det_stride, det_offset;
    const uint8_t *upd;         // [B][upd_stride] or null
    int64_t upd_stride;
    int upd_rows;
    int max_iter;
    float ms_scale;             // 0 -> 1 - 2^-it
    int want_llr;               // 1: non-converged shots publish their posteriors for OSD
    uint32_t *err_bits;         // [B][out_words]
    int32_t *status;            // [B]
    // workspace
    float *llr_ws;              // [cap][n_pad]  posterior by bit slot, one row per non-converged shot
    int32_t *fail_list;         // [cap]
    int32_t *fail_count;        // [1]
    uint16_t *order_ws;         // [blocks][n]   sorted column order (full OSD kernel)
    uint64_t *q_spill;          // [blocks][(mw - kw_lds)][m_pad]
    uint64_t *q_spill_fast;     // [blocks_fast][(mw - f_kw)][m_pad]   register kernel
    uint64_t *q_spill_sr;       // [blocks_sr][...] spilled Q planes and parked state of qd_osd0_sr_kernel (osd_sr.hip, qd_osd_sr_ws_words)
    uint64_t *mt_ws;            // [blocks_fast][mw * m_pad + 2048]    higher-order OSD: transposed Q + candidate vectors
    int32_t *hard_list;         // [cap]         fail-list slots the first fast OSD pass could not finish
    int32_t *hard_list2;        // [cap]         ... and the second
    int32_t *hard_count;        // [2]
    unsigned long long *dbg;    // [16] phase cycle counters (only written by -DQD_OSD_TIMING builds)
    int osd_w, osd_order, rank; // higher-order OSD: 0 = OSD-0, 1 = combination sweep, 2 = exhaustive; GF(2) rank of the window matrix
    // ---- grid arithmetic of the LDS min-sum kernel (channel LLRs are multiples of 2^-k, ms_scaling = 1: see bp_kernels.hip)
    float s_limit;              // 2^(23-k): the run is exact while every S_j = |llr0_j| + sum |c2b| stays below it; 0 = not on a grid
    const int32_t *shot_list;   // redo pass: workgroup x decodes shot shot_list[x] (x < *shot_count); null = shot x
    const int32_t *shot_count;
    int32_t *redo_list;         // first pass: shots whose bound tripped are parked here for the coarse-grid pass; null = last pass
    int32_t *redo_count;
    int redo_cap;
    int status_or;              // ORed into the status word (QD_STATUS_COARSE_GRID in the redo pass)
};

// Relay-BP (bp_relay.hip): the legs' budgets, the table of memory strengths and the kernel's LDS beyond the gather kernel's layout
struct RelayArgs {
    int pre_iter, num_sets, set_max_iter, stop_nconv;
    float gamma0;
    const float *gammas;        // [num_sets][n_pad] memory strengths of legs 1.., by bit slot (null: num_sets = 0)
    int off_marg, off_best, off_wsum, lds_bytes;   // marginals [n_pad + 1] floats, best candidate [out_words], 64-bit weight sum
    float *marg_ws;             // [cap][n_pad] the device-marginal form's M_j, row = shot, slot order (then off_marg = -1); null in the LDS form
};

// Workgroup-wide OR without static LDS (a static __shared__ object in front of the dynamic region can knock the
// 16-byte alignment the ds_read_b128 gathers rely on).  `red` = 32 ints of dynamic LDS, 16-byte aligned; `phase`
// alternates 0/1 between successive calls so a fast wave cannot overwrite flags a slow wave still reads.  One barrier.
__device__ __forceinline__ int qd_block_or(int pred, int *red, int nwaves, int phase)
{
    const unsigned long long bal = __ballot(pred);
    if ((threadIdx.x & 63) == 0) red[phase * 16 + (threadIdx.x >> 6)] = (bal != 0ull);
    __syncthreads();
    const int4 *r4 = reinterpret_cast<const int4 *>(red + phase * 16);
    int r = 0;
    for (int w = 0; w < (nwaves + 3) / 4; ++w) {
        const int4 v = r4[w];                   // slots beyond nwaves are zero (cleared once at kernel start)
        r |= v.x | v.y | v.z | v.w;
    }
    return r;
}

// Wave-wide reductions on the DPP path (row shifts + row broadcasts: a handful of cycles per step, no LDS traffic);
// the result is uniform (taken from lane 63).
#define QD_DPP(v, old, ctrl, rowmask) ((uint32_t)__builtin_amdgcn_update_dpp((int)(old), (int)(v), (ctrl), (rowmask), 0xf, false))
__device__ __forceinline__ uint32_t qd_wave_umin(uint32_t v)
{
    v = min(v, QD_DPP(v, 0xFFFFFFFFu, 0x111, 0xf));   // row_shr:1
    v = min(v, QD_DPP(v, 0xFFFFFFFFu, 0x112, 0xf));   // row_shr:2
    v = min(v, QD_DPP(v, 0xFFFFFFFFu, 0x114, 0xf));   // row_shr:4
    v = min(v, QD_DPP(v, 0xFFFFFFFFu, 0x118, 0xf));   // row_shr:8   -> lane 15 of each row holds the row minimum
    v = min(v, QD_DPP(v, 0xFFFFFFFFu, 0x142, 0xa));   // row_bcast:15 into rows 1 and 3
    v = min(v, QD_DPP(v, 0xFFFFFFFFu, 0x143, 0xc));   // row_bcast:31 into rows 2 and 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t qd_wave_or(uint32_t v)
{
    v |= QD_DPP(v, 0u, 0x111, 0xf);
    v |= QD_DPP(v, 0u, 0x112, 0xf);
    v |= QD_DPP(v, 0u, 0x114, 0xf);
    v |= QD_DPP(v, 0u, 0x118, 0xf);
    v |= QD_DPP(v, 0u, 0x142, 0xa);
    v |= QD_DPP(v, 0u, 0x143, 0xc);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t qd_wave_add(uint32_t v)
{
    v += QD_DPP(v, 0u, 0x111, 0xf);
    v += QD_DPP(v, 0u, 0x112, 0xf);
    v += QD_DPP(v, 0u, 0x114, 0xf);
    v += QD_DPP(v, 0u, 0x118, 0xf);
    v += QD_DPP(v, 0u, 0x142, 0xa);
    v += QD_DPP(v, 0u, 0x143, 0xc);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

struct SpmatDev {
    int nrows, ncols, nnz;
    const uint32_t *row_ptr;
    const uint32_t *col_idx;
    const uint32_t *colmask;    // [ncols][mask_words] the rows of each column as a bit mask (null when nrows > 512)
    int mask_words;
};

// Philox4x32-10 (Salmon et al., SC'11): the counter-based generator of both samplers, qd_sample_dem (gf2_kernels.hip) and
// qd_sample_circuit (frame_sampler.hip).  CPU restatement: philox4x32_10 in oracle/qd_oracle.c.
__device__ __forceinline__ void qd_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1, uint32_t out[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Circuit program of the frame sampler (frame_sampler.hip); opcodes and layout as quits_amd/frame.py writes them.
enum QdFrameOp { QD_FOP_R = 0, QD_FOP_H, QD_FOP_CX, QD_FOP_M, QD_FOP_MX, QD_FOP_MR, QD_FOP_XERR, QD_FOP_ZERR, QD_FOP_DEP1, QD_FOP_DEP2,
                 QD_FOP_DET, QD_FOP_FLUSH, QD_FOP_OBS, QD_FOP_YERR, QD_FOP_PC1, QD_FOP_PC2, QD_FOP_COUNT };
// Read-only device data addressed identically by every lane (a channel's threshold table): the constant address space makes the
// compiler fetch it with scalar loads into SGPRs instead of one vector load per lane.
typedef const __attribute__((address_space(4))) uint32_t QdUniformU32;
#define QD_FRAME_LDS_MAX (64 * 1024)   // LDS of one wavefront (64 shots): 2 x nq frame words + ring words + observable words, 8 B each
struct FrameDev {
    const int32_t *prog;
    const uint32_t *thr;
    int prog_len, nq, ring, nobs, lds_bytes;
    int channels;               // the program holds Y_ERROR / PAULI_CHANNEL_1 / PAULI_CHANNEL_2: which kernel instantiation runs it
};
