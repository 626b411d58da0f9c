/* quits_amd.h -- C ABI of libquits_amd.so, the MI355X (gfx950) sliding-window BP-OSD decoder.
 *
 * This is the drop-in boundary for the decoding hot path of mkangquantum/quits.  Every entry point names the
 * reference interface it stands in for (paths relative to /root/reference/src/quits/).  The reference reaches its
 * inner decoder through the Python extension `ldpc.bposd_decoder.BpOsdDecoder`; a maintainer would bind this
 * library with ctypes exactly as quits_amd/_lib.py does (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain C types only; no exceptions cross the boundary; return 0 on success, a negative QD_E* code on error,
 *     with a thread-local message behind qd_last_error();
 *   - pointers named d_* are DEVICE pointers owned by the caller (e.g. torch tensors' data_ptr()); the library
 *     allocates only its own graph and workspace memory and frees it in *_destroy;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); NULL = default stream;
 *   - all launches are asynchronous; nothing here synchronises the device unless it says so;
 *   - one process per GPU; distinct decoders are independent, one decoder must not be used concurrently.
 */
#ifndef QUITS_AMD_H
#define QUITS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QD_OK 0
#define QD_EINVAL (-1)      /* bad argument                                             */
#define QD_EUNSUPPORTED (-2)/* legal for ldpc, not implemented on the device path      */
#define QD_EHIP (-3)        /* HIP runtime error                                        */
#define QD_ECAPACITY (-4)   /* graph beyond the kernels' limits (m > 32767, n > 65000, row / column weight; OSD row state) */

/* bp_method / schedule / osd_method: the string options of quits/decoder/bposd.py:27-29 as integers */
#define QD_BP_PRODUCT_SUM 0
#define QD_BP_MINIMUM_SUM 1
#define QD_SCHEDULE_PARALLEL 0
#define QD_SCHEDULE_SERIAL 1
#define QD_OSD_OFF 0
#define QD_OSD_0 1
#define QD_OSD_E 2
#define QD_OSD_CS 3
#define QD_LSD_0 4            /* BP-LSD (ldpc.bplsd_decoder.BpLsdDecoder, quits/decoder/bplsd.py:5) as values of osd_method:       */
#define QD_LSD_E 5            /*   lsd_method 'lsd_0' / 'lsd_e' / 'lsd_cs' (bplsd.py:10,54 forward lsd_method, lsd_order);        */
#define QD_LSD_CS 6           /*   osd_order carries lsd_order (0: the three are the same decoder)                                */

/* status word written per shot by qd_decode_batch */
#define QD_STATUS_ITER_MASK 0x3FFF      /* BP iterations used (max_iter is capped at 16383)           */
#define QD_STATUS_COARSE_GRID (1 << 14) /* flooding min-sum: decoded on the coarse LLR grid (see qd_decoder_info)          */
#define QD_STATUS_INEXACT (1 << 15)     /* ... and even there the exactness bound tripped: float rounding may have occurred.
                                         * Also set, WITHOUT QD_STATUS_COARSE_GRID, on a shot that left the fine grid but found the
                                         * coarse-grid list full: the list holds min(batch, 4096) shots of a call (the whole batch where
                                         * the fine grid sits on the 2^-10 floor, see qd_decoder_info); such a shot keeps its fine-grid result */
#define QD_STATUS_CONVERGED (1 << 16)   /* BP reproduced the syndrome                                 */
#define QD_STATUS_OSD (1 << 17)         /* OSD post-processing produced the output                    */
#define QD_STATUS_INCONSISTENT (1 << 18)/* OSD: syndrome outside the column space of the window matrix */
#define QD_STATUS_ZERO (1 << 19)        /* all-zero syndrome short-circuit                            */
#define QD_STATUS_RELAY_LEG_SHIFT 20    /* Relay-BP (qd_decoder_create_relay): bits 20..29 = the leg that produced the returned candidate */
#define QD_STATUS_RELAY_LEG_MASK (0x3FF << QD_STATUS_RELAY_LEG_SHIFT)   /* (no candidate: the last leg run) */

typedef struct qd_graph qd_graph;       /* one window's Tanner graph + priors, resident on one device */
typedef struct qd_decoder qd_decoder;   /* graph + parameters + device workspace                      */
typedef struct qd_spmat qd_spmat;       /* sparse GF(2) matrix on the device (L_k, U_k, H for sampling) */
typedef struct qd_circuit qd_circuit;   /* compiled circuit program of the frame sampler, on the device */
typedef struct qd_strata qd_strata;     /* threshold table of the stratified DEM sampler, on the device */

/* qd_params.reserved: run flooding min-sum in the one-message-per-edge kernel too (ldpc's own update order, prefix sums
 * instead of "total minus own").  On the LLR grid both kernels compute exactly and agree bit for bit.  Validation aid. */
#define QD_FLAG_EDGE_MESSAGES 1
/* qd_params.reserved: keep the channel LLRs as (float)log((1-p)/p) instead of putting them on a binary grid (round-1
 * arithmetic: float rounding in every sum).  Validation aid; see qd_decoder_info. */
#define QD_FLAG_RAW_LLR 2
/* qd_params.reserved: decode a window that fits the CU the way an off-chip window is decoded (see qd_graph_create): every BP method and
 * schedule in the one-message-per-edge kernel -- flooding min-sum on the LLR grid with the exactness certificate and the coarse-grid redo
 * pass -- and OSD-0 in qd_osd0_offchip_kernel.  Same results as the default kernels, bit for bit.  Validation aid. */
#define QD_FLAG_OFF_CHIP 4

/* Validation switches: environment variables that make a graph (G: read by qd_graph_create) or a decoder (D: read by qd_decoder_create)
 * take an alternative that the tests compare bit for bit against the default.  None changes a result and none is needed in normal
 * use; an object keeps what it read for its whole life, and nothing on the decode path reads the environment.
 *   QD_NO_SCATTER              D  flooding min-sum in the gather kernel (bp_kernels.hip) where a scatter kernel would take the window
 *   QD_SCATTER_M2_LIMIT=<u>    D  lower the scatter kernels' exactness bound to u grid units: shots take the gather kernel's recheck pass
 *   QD_SCATTER_CPL1            G  one check per lane where the default is two per lane on half the lanes (bp_scatter_wide.hip)
 *   QD_SCATTER_WIDE_T704       G  the scatter kernel on 704 lanes x 2 checks instead of 512 x 3
 *   QD_SCATTER_NATURAL_ROUNDS  G  ... its wavefronts take the slot-waves in natural order (no balancing of their rounds)
 *   QD_SCATTER_BANKS_BY_SLOT   G  the scatter accumulators' banks = the degree-sorted bit slots mod 32 (no balancing)
 *   QD_SCATTER_WALK_GREEDY     G  the scatter kernels' walk without matching: every check takes its least busy bank
 *   QD_BP_NO_FAST_START=1      D  the scatter kernel runs gather pass 0 itself and the full last gather pass, instead of starting
 *                                 from the decoder's first-pass table and folding only the hard-decision parity in the last pass
 *   QD_OSDCS_OLD=1             D  higher-order OSD by row (osd_kernels.hip) instead of the panel kernel (osd_cs.hip)
 *   QD_GEN_STAGES="3,6" / =0   D  iteration bounds between the launches of the serial schedule (one-message-per-edge kernel) / one launch */

/* Keyword arguments the reference hands to BpOsdDecoder (decoder/bposd.py:38-49,74-83). */
typedef struct qd_params {
    int32_t bp_method;          /* QD_BP_*        ; MINIMUM_SUM + PARALLEL runs in the compressed LDS kernel,        */
    int32_t schedule;           /* QD_SCHEDULE_*  ; every other pair in the one-message-per-edge kernel (HBM)        */
    int32_t max_iter;           /* 0 -> number of faults n (ldpc convention)                     */
    int32_t osd_method;         /* QD_OSD_* | QD_LSD_* ; device path: OFF, 0, CS (order <= 64), E (order <= 15), LSD-0 / -CS / -E (same limits) */
    int32_t osd_order;
    int32_t reserved;           /* flag bits, QD_FLAG_*; 0 for the reference's behaviour                           */
    double ms_scaling_factor;   /* not exposed by the reference wrapper -> ldpc default 1.0; 0 = 1-2^-it */
} qd_params;

int qd_version(void);                 /* 114 (114: qd_shrink_begin, qd_shrink_step; 113: qd_decoder_relay_info, QD_RELAY_FLAG_MARGINALS_DEVICE; 112: qd_decoder_create_relay, QD_STATUS_RELAY_LEG_*; 111: qd_strata_create, qd_strata_destroy, qd_strata_info, qd_sample_dem_strata; 110: qd_sample_dem_faults, qd_commit_bits, qd_fault_stats_batch; 109: qd_unpack_b8, qd_pack_b8; 108: qd_shot_flags_fold, qd_tally_batch, qd_sample_circuit_shots, qd_sample_dem_shots; 107: off-chip windows decode, QD_FLAG_OFF_CHIP, QD_POST_OSD0_OFFCHIP, no new export; 106: qd_circuit_create accepts the biased-noise opcodes Y_ERROR / PAULI_CHANNEL_1 / PAULI_CHANNEL_2, no new export; 105: qd_decoder_fast_start; 104: qd_circuit_* + qd_sample_circuit; 103: qd_decoder_post_head_start; 101: qd_graph_info wrote 12 entries; 102: 10 again + qd_graph_info_ex) */
const char *qd_last_error(void);
/* Number of visible HIP devices (0 if none): lets a host fail loudly before building anything. */
int qd_device_count(void);

/* ---- graph: replaces the sparse-matrix half of BpOsdDecoder.__init__ (call sites
 *      decoder/sliding_window.py:61,69,149,152).  CSR of the window check matrix (m detectors x n faults, column
 *      indices ascending in each row) and the n channel probabilities (`channel_probs`, sliding_window.py:148,151;
 *      pass n copies of `error_rate` for the phenomenological variant, bposd.py:43,49).
 *      Limits: m <= 32767, n <= 65000, row weight <= 255, column weight <= 16 (QD_ECAPACITY beyond).  A window whose BP state the CU's
 *      LDS cannot hold (16 bytes per detector + 4 per fault > 160 KB, or more than 4094 detectors) is an OFF-CHIP window (since version
 *      107; QD_ECAPACITY before): BP of every method and schedule runs in the one-message-per-edge kernel, messages in HBM -- flooding
 *      min-sum with ms_scaling_factor = 1 on the LLR grid, certified per shot and decoded again on the coarse grid exactly as
 *      qd_decoder_info describes -- and OSD-0 (osd_0, or osd_cs / osd_e of order 0) in qd_osd0_offchip_kernel, which needs 17 bytes of LDS
 *      per detector (m <= 4608 fits for any n; QD_ECAPACITY from qd_decoder_create beyond what fits).  Order > 0 and BP-LSD are
 *      QD_EUNSUPPORTED there. */
int qd_graph_create(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx, const double *priors,
                    int32_t device, qd_graph **out);
void qd_graph_destroy(qd_graph *g);
/* info[0..9] = m, n, nnz, max row weight, max column weight, BP block threads, BP LDS bytes (both 0: an off-chip window), OSD block
 *              threads, OSD LDS bytes, GF(2) rank of the matrix.  Exactly 10 entries are written (as in library version 100; version 101
 *              wrote 12 -- callers built against that header should move to qd_graph_info_ex). */
int qd_graph_info(const qd_graph *g, int32_t *info);
/* The same with the caller saying how many int32 entries `info` has room for; entries 10, 11 = modelled LDS cycles of one pass of
 * the scatter kernels' walk over the accumulators (bank conflicts included) and the same without any conflict (0, 0: the window
 * does not run there); entries 12, 13 = lanes per workgroup and checks per lane of qd_bp_scatter_wide_kernel's instantiation for this
 * window (one check per lane: the gather kernel's lanes, 1; 0, 0: no scatter kernel for this window); entries beyond the ones this version knows are set to 0. */
int qd_graph_info_ex(const qd_graph *g, int32_t *info, int32_t n_entries);

/* ---- decoder: replaces BpOsdDecoder.__init__'s parameter half. */
int qd_decoder_create(const qd_graph *g, const qd_params *params, qd_decoder **out);
void qd_decoder_destroy(qd_decoder *d);

/* ---- Relay-BP (after Mueller et al. 2025): flooding min-sum run as a chain of legs in which fault j mixes its previous marginal into its
 *      prior with a memory strength gamma_j; every leg that reproduces the syndrome yields a candidate, the lightest is returned.  The
 *      definition, bit for bit, is quits_amd/relay.py (relay_mirror).  No reference counterpart (ldpc has no such decoder).
 *      Leg 0: pre_iter iterations with gamma_j = gamma0; leg r = 1 .. num_sets: set_max_iter iterations with gamma_j = gammas[r - 1][j];
 *      the decode stops after stop_nconv candidates or the last leg. */
typedef struct qd_relay_params {
    int32_t pre_iter, num_sets, set_max_iter, stop_nconv;   /* >= 1, 0 .. 1023, >= 1, >= 1; pre_iter + num_sets * set_max_iter <= 16383 */
    float gamma0;
    int32_t reserved;                                       /* flag bits, QD_RELAY_FLAG_*; 0 for the default choice of form */
} qd_relay_params;
/* qd_relay_params.reserved: keep the marginals M_j in the decoder's device-memory workspace (bp_relay_device.hip) on a window whose
 * marginals would fit in LDS too.  Same results as the LDS form, bit for bit.  Validation aid, like QD_FLAG_EDGE_MESSAGES. */
#define QD_RELAY_FLAG_MARGINALS_DEVICE 1
/* A decoder whose stage 1 is qd_bp_relay_kernel (bp_relay.hip) and whose stage 2 is params->osd_method's post-processor, unchanged, over the
 * shots that found no candidate (osd_off: they return their last hard decision).  `gammas`: HOST array [num_sets][n], fault order, copied
 * (may be NULL when num_sets = 0); every value finite and |gamma| < 1.5.  params must name QD_BP_MINIMUM_SUM + QD_SCHEDULE_PARALLEL and
 * no flag bits; params->max_iter is ignored; ms_scaling_factor keeps its meaning (0: 1 - 2^-t, t counted within the leg).  QD_EINVAL
 * otherwise, and for a bit of relay->reserved that is no QD_RELAY_FLAG_*.
 * Two forms of one kernel, the same results bit for bit.  The LDS form keeps a shot's whole state on the CU: the gather kernel's LDS layout
 * (16 bytes per detector + 4 per fault) + 4 more bytes per fault for the marginals + the candidate's bits.  It is taken wherever it fits
 * the CU's 160 KB.  Where it does not, the device-marginal form is: the marginals are a row of n_pad floats per shot in the decoder's
 * workspace (reserved and released with it, 4 n_pad bytes per shot of the batch), touched by the lane that owns the fault only, and the
 * LDS holds the gather layout + the candidate's bits (QLP [[1020,136]] W = 3: about 190 KB -> 115 KB).  QD_ECAPACITY: that does not fit
 * either -- the message gives both byte counts -- or the window is off-chip (the gather layout itself does not fit: "LDS" in the message).
 * qd_decoder_relay_info reports the form.  The channel LLRs stay float32(log((1 - p) / p)): qd_decoder_info reports grid -1.
 * Status word: iterations = the total over all legs; QD_STATUS_CONVERGED iff a candidate was found (or QD_STATUS_ZERO); the leg bits above;
 * QD_STATUS_COARSE_GRID and QD_STATUS_INEXACT are never set. */
int qd_decoder_create_relay(const qd_graph *g, const qd_params *params, const qd_relay_params *relay, const float *gammas, qd_decoder **out);
/* info[0] = where a Relay-BP decoder keeps its marginals: 1 = LDS, 2 = device memory (0: not a Relay-BP decoder, and the rest 0 too);
 * info[1] = dynamic LDS bytes of its kernel; info[2] = what the LDS form takes on this window, whether it fits or not; info[3] = the
 * CU's LDS bytes, the limit both are held against.  Exactly 4 entries are written.  (Since version 113.) */
int qd_decoder_relay_info(const qd_decoder *d, int32_t *info);
/* Arithmetic of this decoder.  info[0] = k: the channel LLRs log((1-p)/p) (computed in double, as ldpc does) are rounded to
 * the nearest multiple of 2^-k before BP starts; -1 = not rounded (product-sum, ms_scaling_factor != 1, QD_FLAG_RAW_LLR).
 * Flooding min-sum with ms_scaling_factor = 1 only adds, subtracts, negates and compares messages, so on such a grid
 * single-precision arithmetic is EXACT while magnitudes stay below 2^(24-k): the kernels then return, bit for bit, what
 * ldpc's double-precision BpDecoder returns for those LLRs, in any summation order.  The LDS kernel proves this per shot
 * (bound S < 2^(23-k), bp_kernels.hip); a shot whose bound trips is decoded again on the coarser grid info[1]
 * (QD_STATUS_COARSE_GRID), and flagged QD_STATUS_INEXACT if that trips too.  k = max(10, r), r = 23 - ceil(log2(8 * max|llr| * max_iter))
 * clamped to [2, 20]; info[1] = max(r - 4, 0) if r >= 10, else r (the rule's own grid takes the shots that outgrow 2^-10).  info[2] = 1 if BP runs in the one-message-per-edge kernel.  info[3] = 1 if the fine-grid pass of flooding min-sum runs in
 * the scatter kernel (bp_scatter_wide.hip: same results, bit for bit; QD_NO_SCATTER=1 in the environment keeps the gather kernel) with
 * one check per lane, 2 if with several (the default shape -- two checks per lane on half the lanes; three per lane for windows of more
 * than 1024 checks or rows of 65..96 faults).
 * No reference counterpart (ldpc computes in double). */
int qd_decoder_info(const qd_decoder *d, int32_t *info);
/* 1 if the scatter kernel of this decoder starts from the first-pass table (gather pass 0 of flooding min-sum reads the
 * priors alone, so what it finds is made once, when the decoder is created) and runs its last gather pass in the thin form; 0 otherwise
 * (another BP kernel, max_iter < 1, QD_BP_NO_FAST_START=1).  Same results either way, bit for bit. */
int qd_decoder_fast_start(const qd_decoder *d);
/* Which kernel post-processes the shots BP leaves unconverged (decoder/device.py reports it; bench.py labels its roofline.osd object
 * with it).  No reference counterpart: ldpc has one OsdDecoder / LsdDecoder. */
#define QD_POST_NONE 0          /* osd_method = osd_off                                                                          */
#define QD_POST_OSD0_SR 1       /* OSD-0, many pivots per barrier round: qd_osd0_sr_kernel (osd_sr.hip)                          */
#define QD_POST_OSD0_REG 2      /* OSD-0, one pivot per round: qd_osd0_reg_kernel (osd_kernels.hip)                              */
#define QD_POST_OSD_W_OLD 3     /* OSD-CS / OSD-E by row (qd_osd0_reg_kernel<.., true>, osd_kernels.hip): windows the panel kernel does not take */
#define QD_POST_OSD_CS_PANEL 4  /* OSD-CS / OSD-E, round 5: qd_osdcs_kernel (osd_cs.hip), one panel of 64 sorted columns at a time */
#define QD_POST_LSD 5           /* BP-LSD: qd_lsd0_kernel (lsd_kernels.hip)                                                      */
#define QD_POST_OSD0_OFFCHIP 6  /* OSD-0 of an off-chip window (or QD_FLAG_OFF_CHIP): qd_osd0_offchip_kernel (osd_offchip.hip)   */
int qd_decoder_postproc_kernel(const qd_decoder *d);
/* Pre-size the device workspace for batches of up to max_batch shots (otherwise grown on demand, which
 * synchronises). */
int qd_decoder_reserve(qd_decoder *d, int64_t max_batch);
/* Cap the message workspace of the one-message-per-edge BP kernel (bytes; default 48 GB).  Larger batches are decoded in
 * equal chunks that fit.  A sliding-window plan holds one decoder per window: the host divides its budget among them (the Python
 * driver's QD_GENERAL_WS_GB: default 96 GB for a plan of several decoders; a plan of one keeps 48 GB unless it is set).  No reference
 * counterpart (memory management). */
int qd_decoder_set_workspace_limit(qd_decoder *d, int64_t bytes);
/* Hand the device workspace back (posteriors, fail lists, message planes, elimination scratch); the decoder stays usable and
 * sizes it again at the next decode.  The host keeps sliding-window plans between calls (the reference is called once per
 * experiment point, bposd.py:54-86) and only the plan in use keeps its workspace.  No reference counterpart (memory management). */
int qd_decoder_release_workspace(qd_decoder *d);

/* ---- decode: replaces the per-shot `decoder.decode(syndrome)` calls (sliding_window.py:85,95,171,182) for a
 *      whole batch of shots, including the syndrome preparation in front of them (:168-169,179-180):
 *        syndrome[b][i] = d_det[b * det_stride + det_offset + i]  (i < m)   XOR   d_upd[b * upd_stride + i] (i < upd_rows)
 *      d_det: one byte per detector (0/1), i.e. the `zcheck_samples` array; d_upd may be NULL.
 *      B = 0 is valid: QD_OK whatever the pointers (NULL included), nothing is read, written or launched.
 *      Outputs: d_err_bits[b][w], w < ceil(n/32): bit (j & 31) of word (j >> 5) = decoded fault j;
 *               d_status[b]: QD_STATUS_* flags | iterations. */
int qd_decode_batch(qd_decoder *d, const uint8_t *d_det, int64_t det_stride, int64_t det_offset,
                    const uint8_t *d_upd, int64_t upd_stride, int32_t upd_rows, int64_t B,
                    uint32_t *d_err_bits, int32_t *d_status, void *stream);

/* The two stages of qd_decode_batch separately: stage 1 = BP (non-converged shots and their posteriors are parked in
 * the decoder's workspace), stage 2 = OSD over the shots parked by the preceding stage-1 call with the SAME
 * arguments, stage 3 = both.  Lets a host overlap the (latency-bound) OSD of one batch with the (ALU-bound) BP of the
 * next on a second stream, using one decoder per batch in flight. */
int qd_decode_stage(qd_decoder *d, const uint8_t *d_det, int64_t det_stride, int64_t det_offset, const uint8_t *d_upd,
                    int64_t upd_stride, int32_t upd_rows, int64_t B, uint32_t *d_err_bits, int32_t *d_status,
                    int32_t stage, void *stream);

/* The decoder's OSD stage alone (OSD-0, or OSD-CS / OSD-E when the decoder was created with them), on caller-supplied soft information: every shot of the batch is post-processed as if BP had failed with
 * posterior LLRs d_llr[b][j] (float, fault order, row stride n).  Same syndrome arguments as qd_decode_batch.  This is
 * ldpc's OsdDecoder.decode(syndrome, log_prob_ratios) (osd.hpp), which BpOsdDecoder.decode calls after a failed BP. */
int qd_osd0_batch(qd_decoder *d, const uint8_t *d_det, int64_t det_stride, int64_t det_offset, const uint8_t *d_upd,
                  int64_t upd_stride, int32_t upd_rows, int64_t B, const float *d_llr, uint32_t *d_err_bits,
                  int32_t *d_status, void *stream);

/* Posterior LLRs of the last qd_decode_batch call for shots whose BP did not converge are kept in the decoder's
 * workspace; this copies shot b's (float[n], fault order) to d_out, or returns QD_EINVAL if b converged.
 * Synchronises.  Test/diagnostic hook (ldpc exposes `log_prob_ratios` the same way). */
int qd_decoder_failed_llr(qd_decoder *d, int64_t b, float *d_out, void *stream);

/* Diagnostic: 16 cycle counters the OSD kernels accumulate per phase when the library is built with -DQD_OSD_TIMING
 * (all zero otherwise); reading clears them.  Synchronises. */
int qd_decoder_debug_counters(qd_decoder *d, uint64_t *out16);

/* Two-stream drivers (qd_decode_stage 1 on one stream, 2 on another; no counterpart in the reference, whose shot loop is sequential,
 * sliding_window.py:162-186): call this on the BP stream right after a stage-1 call.  If that batch's post-processing is heavy (OSD-CS / OSD-E, BP-LSD, or
 * OSD-0 over at least three quarters of the batch -- launched only when an earlier call's failure count, read back without waiting, says so, then decided on the
 * device from the batch's own count) the stream is held for
 * `microseconds` (< 0: the default, 50; at most 5000), so that the post-processor started on the other stream at that moment is on the CUs before the next
 * BP kernel fills them; otherwise it costs one empty launch.  Changes no result. */
int qd_decoder_post_head_start(qd_decoder *d, int32_t microseconds, void *stream);

/* Per-kernel device time of this decoder accumulated between calls (milliseconds, HIP events on `stream`):
 * out[0] BP kernel, out[1] OSD kernel, out[2] number of BP launches, out[3] number of OSD launches.
 * enable != 0 turns event recording on.  qd_decoder_profile synchronises on the recorded events. */
int qd_decoder_set_profiling(qd_decoder *d, int32_t enable);
int qd_decoder_profile(qd_decoder *d, double *out, int32_t reset);

/* ---- GF(2) sparse matrices and the window hand-off: replace `window_observable_set[k] @ e % 2` and
 *      `window_update[k] @ e % 2` (sliding_window.py:172,174,183).  CSR, nrows x ncols. */
int qd_spmat_create(int32_t nrows, int32_t ncols, const int32_t *row_ptr, const int32_t *col_idx, int32_t device,
                    qd_spmat **out);
void qd_spmat_destroy(qd_spmat *s);
/* d_out[b * out_stride + r] (one byte per row) = (accumulate ? old : 0) XOR parity(row r of A AND e_b),
 * where e_b are the packed error bits of shot b (err_stride_words words per shot). */
int qd_gf2_spmv_batch(const qd_spmat *A, const uint32_t *d_err_bits, int64_t err_stride_words, int64_t B,
                      uint8_t *d_out, int64_t out_stride, int32_t accumulate, void *stream);

/* Packed error bits -> one byte per fault (the array ldpc's decode() returns; class-level plug-in). */
int qd_unpack_bits(const uint32_t *d_bits, int64_t stride_words, int32_t nbits, int64_t B, uint8_t *d_out,
                   int64_t out_stride, void *stream);

/* ---- Stim's bit-packed samples (format b8: what `compile_detector_sampler().sample(..., bit_packed=True)` returns and `--out_format b8`
 *      writes), to and from the one byte per detector that qd_decode_batch reads.  The reference takes its `zcheck_samples` unpacked
 *      (sliding_window.py:104-118); a host that holds them packed copies an eighth of the bytes and widens them here. */

/* d_out[b*out_stride + c] = bit (bit0 + c) of packed row b, c < nbits.  Row b starts at d_packed + b*packed_stride (bytes, ANY alignment);
 * bit k of a row is byte k>>3, bit k&7 (Stim's b8).  Writes exactly nbits bytes per row (values 0/1): out may be a column slice of a wider
 * array.  bit0 >= 0 selects a field of a record, e.g. the observables Stim appends after the detectors. */
int qd_unpack_b8(const uint8_t *d_packed, int64_t packed_stride, int64_t bit0, int32_t nbits, int64_t B,
                 uint8_t *d_out, int64_t out_stride, void *stream);
/* d_packed[b*packed_stride + i], i < ceil(nbits/8): bit j = d_in[b*in_stride + 8i + j] & 1; the padding bits of the last byte are 0; bytes
 * of a row past ceil(nbits/8) are not touched. */
int qd_pack_b8(const uint8_t *d_in, int64_t in_stride, int32_t nbits, int64_t B, uint8_t *d_packed, int64_t packed_stride, void *stream);

/* Number of shots whose prediction differs from the observable flips on any of k bits: the `pL` numerator of
 * tests/test_sliding_window.py:83.  d_count (int64 on device) is incremented. */
int qd_count_mismatch(const uint8_t *d_pred, const uint8_t *d_obs, int32_t k, int64_t B, int64_t *d_count,
                      void *stream);

/* ---- a memory experiment's bookkeeping, on the device.  The reference compares on the host (tests/test_sliding_window.py:83:
 *      `pL = np.sum((logical_pred != observable_flips).any(axis=1)) / num_trials`) and has nothing to say about which observable
 *      failed or how the failing shots were decoded; quits_amd.simulation.get_circuit_mem_pL runs sampler -> decoder -> these two. */

/* Flag byte per shot: what happened to it in ANY window of a sliding-window decode. */
#define QD_SHOT_POST 1          /* some window's output came from the post-processor (QD_STATUS_OSD)   */
#define QD_SHOT_INCONSISTENT 2  /* ... QD_STATUS_INCONSISTENT                                          */
#define QD_SHOT_INEXACT 4       /* ... QD_STATUS_INEXACT                                               */
#define QD_SHOT_COARSE 8        /* ... QD_STATUS_COARSE_GRID: the shot left the fine LLR grid          */
/* d_flags[b] |= the QD_SHOT_* bits of d_status[b], b < B: call once per window with that window's status words (qd_decode_batch) on a
 * zeroed d_flags.  Stands in for `(status & QD_STATUS_OSD) != 0` and its kin computed by the host per window and ORed over the windows;
 * no reference counterpart (ldpc's decoders report `converge` per decode call and the reference drops it, sliding_window.py:171). */
int qd_shot_flags_fold(const int32_t *d_status, int64_t B, uint8_t *d_flags, void *stream);

/* Tallies of a decoded batch, accumulated into d_counts (int64 [QD_TALLY_HEAD + k] on the device, zeroed by the caller before the first call):
 *   [0] shots, [1] failing shots -- prediction != observable flips on the low bit of any of the k bytes, exactly what qd_count_mismatch counts
 *   (the `pL` numerator of tests/test_sliding_window.py:83);  [2 + 2j], [3 + 2j], j = 0 .. 3: shots / failing shots with bit j of d_flags[b]
 *   set (QD_SHOT_POST, _INCONSISTENT, _INEXACT, _COARSE; all zero when d_flags is NULL);  [QD_TALLY_HEAD + i]: shots whose observable i is
 *   mispredicted (`(logical_pred != observable_flips).sum(axis=0)`).
 * d_pred, d_obs: B rows of k bytes with row strides pred_stride, obs_stride >= k (column slices of wider arrays are fine), 1 <= k <= QD_TALLY_MAX_K.
 * d_fail_mask, if not NULL: ceil(B / 64) words, WRITTEN (not accumulated): bit l of word w = shot 64 w + l failed; bits past B are zero.
 * One launch; the number of global atomics does not depend on B. */
#define QD_TALLY_HEAD 10
#define QD_TALLY_MAX_K 4096
int qd_tally_batch(const uint8_t *d_pred, int64_t pred_stride, const uint8_t *d_obs, int64_t obs_stride, int32_t k, int64_t B,
                   const uint8_t *d_flags, int64_t *d_counts, uint64_t *d_fail_mask, void *stream);

/* ---- synthetic input: stands in for stim's detector sampler (simulation.py:23-27), absent here.
 *      e_j ~ Bernoulli(priors_j) (Philox4x32-10, key = seed, counter = (shot0 + b, j / 4)), s = H e, o = L e.
 *      Ht / Lt are the TRANSPOSES as CSR (row j = fault j -> detectors / observables it flips).
 *      d_det: B x det_stride bytes (first m columns written), d_obs: B x obs_stride bytes. */
int qd_sample_dem(const qd_spmat *Ht, const qd_spmat *Lt, const double *priors, uint64_t seed, int64_t shot0,
                  int64_t B, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride, void *stream);
/* The same for the shots d_shots[0 .. B - 1] (int64 on the device, >= 0, any order, repeats allowed, not bounded by 2^32): row b is what
 * qd_sample_dem(..., shot0 = d_shots[b], B = 1, ...) writes.  Stands in for sampling a range again and indexing it
 * (`sampler.sample(shots)[0][indices]`, simulation.py:23-27 -- Stim can only draw a whole range again); B <= 2^31 - 1. */
int qd_sample_dem_shots(const qd_spmat *Ht, const qd_spmat *Lt, const double *priors, uint64_t seed, const int64_t *d_shots, int64_t B,
                        uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride, void *stream);

/* The same again -- qd_sample_dem where d_shots is NULL (shots shot0 .. shot0 + B - 1), qd_sample_dem_shots otherwise, the same Philox stream and
 * the same d_det / d_obs -- and WHICH faults fired: bit (j & 31) of word (j >> 5) of row b of d_fault_bits (fault_stride_words words per row) = 1
 * iff fault j fired in row b's shot.  The padding bits of word ceil(n / 32) - 1 are 0; words of a row past it are not touched.  The bitmap is built in
 * the kernel's LDS beside the detector and observable bits and streamed out in whole words; where the three exceed 64 KiB the row is zeroed
 * and set in place with vector atomics, so n is not bounded.  Like its two siblings the call uploads its threshold table and waits for `stream`.
 * No reference counterpart: Stim's detector sampler does not say which mechanisms fired. */
int qd_sample_dem_faults(const qd_spmat *Ht, const qd_spmat *Lt, const double *priors, uint64_t seed, int64_t shot0, const int64_t *d_shots,
                         int64_t B, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride, uint32_t *d_fault_bits,
                         int64_t fault_stride_words, void *stream);

/* ---- fault-level outputs: the space-time correction of a sliding-window decode and what an experiment tallies of it.  The reference computes
 *      a window's correction, keeps `window_observable_set[k] @ e` and `window_update[k] @ e` of it and drops it (sliding_window.py:171-183). */

/* Bits [out_bit0, out_bit0 + nbits) of row b of d_out = bits [0, nbits) of row b of d_err_bits (qd_decode_batch's packed rows), b < B; every
 * other bit of d_out keeps its value; nbits = 0 is a no-op.  One call per window, on the stream of that window's qd_gf2_spmv_batch, with
 * nbits = the window's committed columns and out_bit0 = the columns committed before it, lays the windows' corrections end to end: ranges
 * that share a word compose when the calls are stream-ordered (a boundary word is read, merged and written by one lane; no atomics).
 * Stands in for concatenating `e[:ncommit]` over the windows of sliding_window.py:162-186, which the reference never does. */
int qd_commit_bits(const uint32_t *d_err_bits, int64_t err_stride_words, int32_t nbits, int64_t B, uint32_t *d_out, int64_t out_stride_words,
                   int64_t out_bit0, void *stream);

/* Tallies of a decoded batch by fault weight.  E = row b of d_faults (qd_sample_dem_faults), C = row b of d_corr (qd_commit_bits), both nbits
 * bits in rows of stride_words words; r = 1 iff row b of d_residual (m bytes, row stride res_stride: H C xor det, made by qd_gf2_spmv_batch with
 * accumulate = 1 onto a copy of det) has a non-zero byte; "failing" = bit b of d_fail_mask (qd_tally_batch's mask of the same batch).
 *   d_hist (int64 [3][QD_FAULT_HIST], accumulated): [0][min(|E|, 255)] += 1 for every shot, [1][min(|E|, 255)] += 1 for every failing shot,
 *     [2][min(|E xor C|, 255)] += 1 for every failing shot with r = 0 -- there E xor C is an undetectable logical fault;
 *   d_counts (int64 [4], accumulated): shots, failing shots, shots with r = 1, failing shots with r = 1;
 *   d_best (uint64, initialised to all ones by the caller): the minimum of (|E xor C| << 40) | (shot0 + b) over the failing shots with r = 0:
 *     the lightest such residual and the shot that certifies it (shot0 + B <= 2^40).
 * One launch; the number of global atomics does not depend on B.  No reference counterpart. */
#define QD_FAULT_HIST 256
int qd_fault_stats_batch(const uint32_t *d_faults, const uint32_t *d_corr, int64_t stride_words, int32_t nbits, const uint8_t *d_residual,
                         int64_t res_stride, int32_t m, const uint64_t *d_fail_mask, int64_t B, int64_t shot0, int64_t *d_hist,
                         int64_t *d_counts, uint64_t *d_best, void *stream);

/* ---- soft outputs per shot (version 116).  quits_amd/soft.py states them: a record of QD_SOFT_FIELDS int64 per shot -- [0] weight = the sum of
 *      w_j over the faults of the committed correction, [1] faults = its size, [2] events = the detector bytes with the low bit set, [3] iters,
 *      [4] post, [5] tail = what the windows' status words say -- and a histogram of every field from which the host reads the logical error rate
 *      that remains when the least certain shots are discarded.  The reference returns predictions only (sliding_window.py:171-186 keeps nothing
 *      else of a window's decode).  Rows of d_soft are soft_stride >= QD_SOFT_FIELDS int64 apart; columns past the sixth are never touched. */
#define QD_SOFT_FIELDS 6
#define QD_SOFT_BINS 1024

/* One window's status words (qd_decode_batch) added into rows the caller zeroed, b < B: [3] += status & QD_STATUS_ITER_MASK, [4] += 1 if
 * QD_STATUS_OSD is set, [5] += bits 20 .. 31 of the word (the post-processors' pivot count, saturated at 4095, or Relay-BP's leg).  Bits 14 .. 19
 * enter nothing but [4] (bit 17).  Call once per window, stream-ordered; fields 0 .. 2 stay.  Stands in for summing the fields of the status
 * tensors with torch, window by window.  No reference counterpart (ldpc reports `converge` and `iter` per call and the reference drops both). */
int qd_soft_fold(const int32_t *d_status, int64_t B, int64_t *d_soft, int64_t soft_stride, void *stream);

/* Fields 0 .. 2 of rows b < B, WRITTEN: C = row b of d_corr (qd_commit_bits: nbits bits in rows of stride_words words; bits >= nbits of the last
 * word and the words past it are ignored), d_weights int32 [nbits] on the device (quits_amd.soft.fault_weights: rint(2^16 log((1 - p) / p)), made
 * by the host -- the device computes no logarithm), row b of d_det m bytes with row stride det_stride >= m, of which only the low bit counts, as
 * in qd_tally_batch.  [0] = sum of d_weights[j] over the set bits j, in 64 bits; [1] = |C|; [2] = the number of set detector bits.  One
 * wavefront per shot, coalesced word loads, one gathered weight per set bit.  Stands in for unpacking C on the host and `C @ w`.  No reference
 * counterpart. */
int qd_soft_weigh(const uint32_t *d_corr, int64_t stride_words, int32_t nbits, const int32_t *d_weights, const uint8_t *d_det, int64_t det_stride,
                  int32_t m, int64_t B, int64_t *d_soft, int64_t soft_stride, void *stream);

/* d_hist (int64 [QD_SOFT_FIELDS][2][QD_SOFT_BINS] on the device, accumulated): for every field f and shot b < B the bin
 * min(max(soft[b][f], 0) >> shifts6[f], QD_SOFT_BINS - 1) of plane [f][0] += 1, and of plane [f][1] too if bit b of d_fail_mask is set
 * (qd_tally_batch's mask of the same batch; NULL: plane 1 is not touched).  shifts6: six shifts 0 .. 62 on the HOST.  One launch, a field per
 * blockIdx.y with its two planes in LDS; the number of global atomics does not depend on B.  Stands in for np.bincount of the records on the
 * host, which would need them there.  No reference counterpart. */
int qd_soft_tally(const int64_t *d_soft, int64_t soft_stride, int64_t B, const int32_t *shifts6, const uint64_t *d_fail_mask, int64_t *d_hist,
                  void *stream);

/* ---- shrinking failing fault sets to 1-minimal ones (version 114).  quits_amd/shrink.py states the walk: a parent set S loses fault j whenever
 *      the decoder still fails on S \ {j}, j running cyclically over the members, until |S| trials in a row change nothing.  These two calls are the
 *      whole step between two decodes; the caller decodes the trial rows like sampled shots (qd_decode_batch ... qd_tally_batch) and hands back
 *      qd_tally_batch's fail mask.  Stateless: every array is the caller's, on the device of Ht.  No reference counterpart.
 *        Ht, Lt            the TRANSPOSES of H (m x n) and L (k x n) as CSR, qd_sample_dem's: row j = the detectors / observables fault j flips
 *        d_sets            P rows of set_stride_words >= ceil(n / 32) words: bit (j & 31) of word (j >> 5) = fault j is in the set; shrunk in place
 *        d_state           int32 [P][QD_SHRINK_STATE]: last, quiet, w = |S|, trials so far, QD_SHRINK_* flags, the pending trial's fault (-1: trial
 *                          0, the set itself), the start weight |E|, 0
 *        d_hs, d_ls        P rows of m / k bytes (strides >= m, k): H S and L S of the CURRENT sets, kept incrementally -- an accepted trial flips
 *                          the bytes of column j, nothing recomputes the product.  The caller fills them for the start sets (qd_gf2_spmv_batch).
 *        d_live            int32 [P]: the parents still walking, ascending; d_count[0] their number A (the only word a host reads per round)
 *        d_det, d_obs      row i < A (strides >= m, k): the trial of parent d_live[i] -- H (S \ {j}), L (S \ {j}), every byte written once by one
 *                          lane; bytes outside the first m / k of a row keep their values; d_fault[i] = j, d_parent[i] = d_live[i]
 *      QD_EINVAL with a message: a null argument, Ht / Lt of different row counts or devices, a stride too small, P > 2^31 - 1, A > P,
 *      d_live_next == d_live.  Asynchronous on `stream`. */
#define QD_SHRINK_STATE 8
#define QD_SHRINK_FAILS 1       /* trial 0 failed: the parent is a failing set                              */
#define QD_SHRINK_MINIMAL 2     /* the walk ended with quiet >= w: the set in d_sets is 1-minimal           */
#define QD_SHRINK_ENDED 4       /* the parent left the live list (minimal, or trial 0 did not fail)         */
/* Start: clears the padding bits of every set's last word, counts w, writes the state before trial 0, d_live = 0 .. P - 1, d_count[0] = P, and
 * emits trial 0 of every parent (d_det = d_hs, d_obs = d_ls, d_fault = -1).  Two launches. */
int qd_shrink_begin(const qd_spmat *Ht, const qd_spmat *Lt, uint32_t *d_sets, int64_t set_stride_words, int64_t P, int32_t *d_state,
                    int32_t *d_live, int32_t *d_count, const uint8_t *d_hs, int64_t hs_stride, const uint8_t *d_ls, int64_t ls_stride,
                    uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride, int32_t *d_fault, int32_t *d_parent, void *stream);
/* One round: bit i of d_fail_mask (ceil(A / 64) words, qd_tally_batch's mask of the A trial rows) is the verdict of parent d_live[i].  Applies
 * it (one wavefront per parent), writes the surviving parents in the same order to d_live_next (!= d_live) and their number to d_count[0] (one
 * workgroup), and emits their next trials into rows 0 .. d_count[0] - 1.  Three launches.  A = 0: d_count[0] = 0. */
int qd_shrink_step(const qd_spmat *Ht, const qd_spmat *Lt, uint32_t *d_sets, int64_t set_stride_words, int64_t P, int32_t *d_state,
                   const int32_t *d_live, int64_t A, const uint64_t *d_fail_mask, int32_t *d_live_next, int32_t *d_count, uint8_t *d_hs,
                   int64_t hs_stride, uint8_t *d_ls, int64_t ls_stride, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride,
                   int32_t *d_fault, int32_t *d_parent, void *stream);

/* ---- the directed search for light undetectable logical faults (version 115).  quits_amd/search.py states the search: a breadth-first search
 *      over states (S, o), S a sorted set of at most K <= 8 detectors, o a mask of at most 64 observables; a level-(l + 1) state is a level-l
 *      state xor an admitted fault that contains its smallest detector.  Stands in for Stim's search_for_undetectable_logical_errors, which
 *      the reference's examples/circuit_distance_search.py calls.  A state is a record of QD_SEARCH_RECORD bytes: two 64-bit words of eight
 *      16-bit detectors (ascending from bit 0 of the first word, 0xFFFF = empty), the 64-bit mask, the 32-bit pool index of its parent
 *      (0xFFFFFFFF at level 1) and the 32-bit fault that led to it.  The pool holds the states in level order; logical_search.hip describes
 *      the visited table and the staging area.  One level per call; the host reads the counters after each and decides. */
typedef struct qd_search qd_search;
#define QD_SEARCH_RECORD 32
#define QD_SEARCH_COUNTERS 8
#define QD_SEARCH_OVER_POOL 1   /* counters[3]: more distinct states than max_states (the outcome `capacity`)   */
#define QD_SEARCH_OVER_TABLE 2  /* ... the visited table is full                                                */
#define QD_SEARCH_OVER_STAGE 4  /* ... a chunk staged more candidates than stage_states                         */
#define QD_SEARCH_OVER_FOUND 8  /* ... more than 65536 states (empty, o) in one level                           */
/* row_ptr [ndet + 1], row_faults: the admitted faults of every detector, CSR; fault_dets [n][D]: the detectors of every fault, ascending,
 * 0xFFFF-padded (all 0xFFFF: not admitted); fault_obs [n]: its mask.  1 <= ndet <= 65535, 1 <= K <= 8, 1 <= D <= 16.  Allocates everything a
 * search touches -- 32 max_states + 4 table_size (a power of two) + 40 stage_states bytes and the tables -- and clears the visited table:
 * QD_EHIP when that does not fit, before any launch.  QD_ECAPACITY: max_states + stage_states > 2^32 - 2 (they share the 32-bit index). */
int qd_search_create(int32_t ndet, int32_t n, const int64_t *row_ptr, const int32_t *row_faults, const uint16_t *fault_dets,
                     const uint64_t *fault_obs, int32_t K, int32_t D, int32_t no_increase, int64_t max_states, int64_t table_size,
                     int64_t stage_states, int32_t device, qd_search **out);
void qd_search_destroy(qd_search *s);
/* Back to the state after qd_search_create: empty pool, empty table, counters zero. */
int qd_search_reset(qd_search *s);
/* Level 1: `count` host records (duplicates allowed) are looked up and the new ones appended.  Two launches per stage_states records. */
int qd_search_seed(qd_search *s, const void *records, int64_t count, void *stream);
/* One level: expands the states the previous level appended, chunk_states at a time (chunk_states times the longest row must not exceed
 * stage_states); two launches per chunk, no kernel waits for another workgroup.  The counters of the previous level must have been read. */
int qd_search_level(qd_search *s, int64_t chunk_states, void *stream);
/* Waits for the level and reads counters[QD_SEARCH_COUNTERS] = {states in the pool (counted on past max_states), staged candidates of the
 * last chunk, states (empty, o) of the last level, QD_SEARCH_OVER_* flags, candidates looked up so far, 0, 0, 0}. */
int qd_search_counters(qd_search *s, uint64_t *counters);
/* The last level's states (empty, o): `max` (= counters[2]) masks and pool indices, in no fixed order. */
int qd_search_found(qd_search *s, int64_t max, uint64_t *masks, uint32_t *indices);
/* The faults along the parents of pool state `index` back to level 1: faults[0 .. *len - 1].  QD_EINVAL beyond max_len. */
int qd_search_chain(qd_search *s, uint32_t index, int32_t max_len, int32_t *faults, int32_t *len);

/* ---- the random information-set estimate of the distance (version 117).  quits_amd/distance.py states it: trial t puts the faults in the
 *      order of (key, j), key = word (j & 3) of Philox4x32-10(key = (seed lo, seed hi), counter = (t lo, t hi, j >> 2, 4)), and eliminates along
 *      it; every column that depends on the columns before it closes a kernel vector of weight 1 + the pivots it is a sum of, whose mask is
 *      the XOR of fault_obs over it.  rec[t] = min over the vectors with a non-zero mask of weight * 2^32 + j (2^64 - 1: none): a function of
 *      (model, seed, t) alone.  No reference counterpart (its compute_code_distance enumerates the kernel); Stim has none either.
 *      distance.hip describes the kernel: one workgroup per trial, the row transform by detector in LDS. */
typedef struct qd_isd qd_isd;
#define QD_ISD_HIST 64
/* col_ptr [n + 1], col_rows [nnz]: the detectors of every fault (CSC of H mod 2, every entry checked against ndet); fault_obs [n]: its mask.
 * 1 <= ndet <= 65535, 1 <= n.  Allocates everything a run touches (the column orders of the trials in flight, the histogram).
 * QD_ECAPACITY, with both byte counts in the message: the transform -- 4 (ndet + columns per block) (ceil(ndet / 32) + 2, made odd) bytes and
 * a header -- or the order while it is sorted (8 bytes a fault, rounded up to a power of two: at most 16384 faults) exceeds the 160 KiB of
 * LDS of a CU.  QD_EHIP: a failed allocation, before any launch. */
int qd_isd_create(int32_t ndet, int32_t n, const int64_t *col_ptr, const int32_t *col_rows, const uint64_t *fault_obs, int32_t device,
                  qd_isd **out);
void qd_isd_destroy(qd_isd *s);
/* info[8] = {LDS bytes of a workgroup, threads of a workgroup, workspace bytes (column orders), trials in flight per launch, pivots of the
 * last trial run = the rank of H (-1 before the first run), columns per block, lanes per column, words sorted}.  Waits for the last run. */
int qd_isd_info(qd_isd *s, int64_t *info);
/* Trials trial0 .. trial0 + ntrials - 1 of `seed`: d_records[i] (device memory) = rec[trial0 + i]; the candidates with a non-zero mask are
 * added to the device histogram by weight (bin 63: every weight >= 63).  One launch of min(ntrials, trials in flight) workgroups, each
 * looping over its trials; asynchronous on `stream`. */
int qd_isd_run(qd_isd *s, uint64_t seed, int64_t trial0, int64_t ntrials, uint64_t *d_records, void *stream);
/* Waits for the last run and copies the histogram to hist[QD_ISD_HIST] (host memory). */
int qd_isd_hist(qd_isd *s, uint64_t *hist);
/* Waits for the last run and clears the histogram. */
int qd_isd_reset(qd_isd *s);

/* ---- fitting a model's priors to detector samples (version 118).  quits_amd/calibrate.py states the fit; the device does the one part that
 *      touches every shot: for every column of H with detectors d_0 < .. < d_{s-1} and every mask t = 1 .. 2^s - 1 (bit i = d_i), the number
 *      of shots in which the XOR of the selected detectors is 1.  No reference counterpart (its priors come from the circuit's noise arguments);
 *      the p_ij estimators of the repetition- and surface-code experiments are the pairwise special case.  calibrate.hip describes the kernels. */
typedef struct qd_calib qd_calib;
#define QD_CALIB_MAX_WEIGHT 10
/* One byte per detector (rows b < B of in_stride >= ndet bytes, the low bit counts, as qd_pack_b8 reads them) to one bit plane per detector:
 * bit b & 63 of word d * plane_stride + (b >> 6) of d_planes is detector d of shot b; bits at and beyond B of the last word are 0; words at
 * and beyond ceil(B / 64) of a plane are not touched.  plane_stride >= ceil(B / 64), B <= 2^31.  One wavefront per 64 shots; asynchronous. */
int qd_bit_planes(const uint8_t *d_in, int64_t in_stride, int32_t ndet, int64_t B, uint64_t *d_planes, int64_t plane_stride, void *stream);
/* The column table (HOST arrays): col_ptr [ncols + 1] from 0, col_det the detectors of every column, ascending.  Checked here, before any
 * launch: QD_EINVAL for a null pointer, a negative size, an empty column, detectors that do not ascend or a detector index >= ndet;
 * QD_ECAPACITY for a column of more than QD_CALIB_MAX_WEIGHT detectors (the message names the column and its weight).  The counters of
 * column j are count_ptr[j] .. count_ptr[j + 1] - 1, count_ptr[j + 1] - count_ptr[j] = 2^s_j - 1, mask t at count_ptr[j] + t - 1. */
int qd_calib_create(int32_t ndet, int32_t ncols, const int64_t *col_ptr, const int32_t *col_det, int32_t device, qd_calib **out);
void qd_calib_destroy(qd_calib *s);
/* info[4] = {counters in a row (the sum of 2^s_j - 1), wavefront tasks of a launch, highest column weight, columns} */
int qd_calib_info(const qd_calib *s, int64_t *info);
/* d_counts (int64 [counters in a row] on the device) += the counts of the module text over the shots of the first nwords words of the planes
 * (qd_bit_planes' layout; a partly filled last word must have zero pad bits).  Every counter is owned by one wavefront: no atomics, and the
 * sums depend on neither the grid nor how the shots were batched.  nwords <= 2^25; nwords = 0 changes nothing.  Asynchronous. */
int qd_parity_counts(const qd_calib *s, const uint64_t *d_planes, int64_t plane_stride, int64_t nwords, int64_t *d_counts, void *stream);

/* ---- stratified input: shots of the detector error model CONDITIONED on exactly k faults firing (subset sampling).  Stands in for
 *      rejection -- drawing `sampler.sample(shots)` (simulation.py:23-27) until a shot happens to hold k faults, which Stim could not even
 *      tell -- where P(|E| = k) is 1e-14.  No reference counterpart.
 *      quits_amd/strata.py states the law and computes the table: thresholds[j * (kmax + 1) + r] = floor(q[j][r] 2^32), q[j][r] the probability
 *      that fault j is included when r faults are still to place among j .. n - 1; column r = 0 must be 0 (QD_EINVAL otherwise), states no
 *      walk reaches hold any value.  1 <= n, 0 <= kmax <= 255 (the last bin of QD_FAULT_HIST).  The table is copied to the device, n * (kmax + 1)
 *      words in HBM: 9.7 MB for 9 480 faults at kmax = 255. */
int qd_strata_create(int32_t n, int32_t kmax, const uint32_t *thresholds, int32_t device, qd_strata **out);
void qd_strata_destroy(qd_strata *s);
/* info[4] = {n, kmax, bytes of the table on the device, device} */
int qd_strata_info(const qd_strata *s, int64_t *info);
/* Row b = shot d_shots[b] (shot0 + b where d_shots is NULL) with exactly d_k[b] faults (int32 [B] on the device: one batch may mix strata).
 * The walk: faults in ascending index, r = d_k[b] at the start; fault j is included iff r > 0 and (word < thresholds[j][r] or n - j == r),
 * word = word (j & 3) of Philox4x32-10(key = (seed lo, seed hi), counter = (s lo, s hi, j >> 2, 2)) -- qd_sample_dem's last counter word is 0,
 * qd_sample_circuit's 1 -- and an included fault lowers r by one.  So a row depends on (seed, shot, k) alone.  d_det, d_obs, d_fault_bits: the
 * layout of qd_sample_dem_faults (the first m / nobs bytes and ceil(n / 32) words of a row are written, padding bits 0, nothing else is touched).
 * A d_k[b] outside 0 .. min(kmax, n) is CLAMPED into that range by the kernel (the Python layer refuses it before the launch).
 * One lane per shot, 64 shots of a wavefront walking j together; their detector and observable bits sit in LDS, ceil(m / 32) + ceil(nobs / 32)
 * words per shot: QD_ECAPACITY beyond 64 KiB per wavefront.  B = 0: QD_OK whatever the pointers.  QD_EINVAL: a null argument (d_k included),
 * strides too small, negative shot0, Ht->nrows != n.  Asynchronous on `stream`: nothing is uploaded, nothing waited for. */
int qd_sample_dem_strata(const qd_strata *strata, const qd_spmat *Ht, const qd_spmat *Lt, uint64_t seed, int64_t shot0, const int64_t *d_shots,
                         const int32_t *d_k, int64_t B, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride,
                         uint32_t *d_fault_bits, int64_t fault_stride_words, void *stream);

/* ---- circuit-level input: a Pauli-frame simulation of the circuit itself (what stim's compile_detector_sampler().sample(...,
 *      separate_observables=True) returns, simulation.py:8-28), without gauge randomisation: exact when every detector and observable
 *      is deterministic, as in every QUITS circuit.  quits_amd/frame.py compiles the circuit text into `program` (int32 words; the layout
 *      and the frame rules are in its docstring), one threshold floor(p * 2^32) per distinct noise probability, and the measurement ring
 *      length max_lookback (>= the largest rec[-k] look-back and >= the widest measurement instruction).  A Pauli channel
 *      (PAULI_CHANNEL_1 / PAULI_CHANNEL_2, since version 106) names the first of 3 / 15 consecutive thresholds, floor(2^32 x) of the partial
 *      sums of its probabilities, which must not decrease.  Every index in the program is
 *      checked here; QD_ECAPACITY when 8 * (2 nq + max_lookback + nobs) bytes exceed the kernel's 64 KiB of LDS per 64 shots. */
int qd_circuit_create(const int32_t *program, int64_t program_len, int32_t nq, int32_t nmeas, int32_t ndet, int32_t nobs,
                      const uint32_t *thresholds, int32_t nthr, int32_t max_lookback, int32_t device, qd_circuit **out);
void qd_circuit_destroy(qd_circuit *c);
/* info[8] = {qubits, noise sites, LDS bytes per wavefront of 64 shots, measurements, detectors, observables, ring length, program words} */
int qd_circuit_info(const qd_circuit *c, int64_t *info);
/* Shots shot0 .. shot0 + B - 1.  Noise site j of shot s fires iff r < threshold, r = word (j & 3) of
 * Philox4x32-10(key = (seed lo, seed hi), counter = (s lo, s hi, j >> 2, 1)); a depolarizing site's Pauli comes from the same r
 * (1 + r mod 3, or 1 + r mod 15 split as (v >> 2, v & 3)); a Pauli channel applies component k iff T_{k-1} <= r < T_k.  The stream depends on (seed, shot, site) only: calls with
 * consecutive shot0 compose.  d_det: B x det_stride bytes (first ndet columns written), d_obs: B x obs_stride bytes.  Asynchronous. */
int qd_sample_circuit(const qd_circuit *c, uint64_t seed, int64_t shot0, int64_t B, uint8_t *d_det, int64_t det_stride,
                      uint8_t *d_obs, int64_t obs_stride, void *stream);
/* The same for the shots d_shots[0 .. B - 1] (int64 on the device, >= 0, any order, repeats allowed, not bounded by 2^32): row b is what
 * qd_sample_circuit(..., shot0 = d_shots[b], B = 1, ...) writes -- the stream depends on (seed, shot, site) only, so a shot is regenerated
 * from its index.  Stands in for `compile_detector_sampler(seed).sample(shots)[indices]` (simulation.py:8-28), which has to draw every
 * shot up to the largest index again.  Asynchronous. */
int qd_sample_circuit_shots(const qd_circuit *c, uint64_t seed, const int64_t *d_shots, int64_t B, uint8_t *d_det, int64_t det_stride,
                            uint8_t *d_obs, int64_t obs_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QUITS_AMD_H */
