// qd_host.h -- private to the host side of libquits_amd.so: the handle structs behind include/quits_amd.h and, once, the prototype of every
// launcher and layout function a kernel file defines.  Those files include it too, so declaration and definition meet in the compiler.
#pragma once
#include "../../include/quits_amd.h"
#include "qd_internal.h"
#include "graph_layout.h"

#include <algorithm>
#include <vector>

#define HIP_TRY(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return qd_fail(QD_EHIP, "%s: %s", #expr, hipGetErrorString(e_));           \
    } while (0)

// Device allocations that live and die together
struct DevAllocs {
    std::vector<void *> ptrs;
    template <class Tp> hipError_t alloc(size_t count, Tp **out) { return alloc_bytes(count * sizeof(Tp), out); }
    template <class Tp> hipError_t alloc_bytes(size_t bytes, Tp **out)
    {
        void *d = nullptr;
        const hipError_t e = hipMalloc(&d, bytes);
        if (e != hipSuccess) return e;
        ptrs.push_back(d);
        *out = static_cast<Tp *>(d);
        return hipSuccess;
    }
    // a copy of `bytes` bytes on the device (16 at least are allocated); null: allocation or copy failed
    void *upload(const void *h, size_t bytes)
    {
        unsigned char *d = nullptr;
        if (alloc(std::max<size_t>(bytes, 16), &d) != hipSuccess) return nullptr;
        if (bytes && hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    }
    template <class Tp> int upload(const std::vector<Tp> &h, const Tp **out)
    {
        void *d = upload(h.data(), h.size() * sizeof(Tp));
        if (!d) return -1;
        *out = static_cast<const Tp *>(d);
        return 0;
    }
    void release()
    {
        for (void *p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};

// The image graph_layout.hip laid out, its pointer members set by qd_graph_create's upload
struct qd_graph : GraphImage {
    int device = 0;
    int m = 0, n = 0, nnz = 0, max_rdeg = 0, max_cdeg = 0, rank = -1;
    DevAllocs mem;
    // LDS layout of qd_osd0_offchip_kernel (x_lds = 0: even its row state does not fit): any window can take it (QD_FLAG_OFF_CHIP)
    int x_off[10] = {0}, x_off_sort = 0, x_off_order = 0, x_kw = 0, x_threads = 0, x_per_cu = 0, x_lds = 0;
    ~qd_graph() { mem.release(); }
};
int qd_host_rank(qd_graph *g);       // GF(2) rank of the window matrix, computed once (qd_graph.hip)

// The BP kernel(s) of a decoder's stage 1, chosen once by qd_decoder_create
enum BpPath {
    BP_LDS_EDGE,        // flooding product-sum, one message per edge, every message in LDS (qd_launch_bp_ps_lds)
    BP_HBM_EDGE,        // one message per edge in an HBM workspace (bp_general.hip): every other method / schedule, QD_FLAG_EDGE_MESSAGES, and every
                        // pair of an off-chip decoder (flooding min-sum on the grid: with the exactness certificate and the coarse-grid redo pass)
    BP_SCATTER_WIDE,    // flooding min-sum on the LLR grid, the scatter kernel (bp_scatter_wide.hip: one or several checks per lane); recheck + coarse grid: gather kernel
    BP_GATHER_GRID,     // ... the gather kernel (bp_kernels.hip) on the fine grid, then on the coarse grid
    BP_GATHER_RAW,      // flooding min-sum on float LLRs off the grid (ms_scaling_factor != 1, QD_FLAG_RAW_LLR): the gather kernel
    BP_RELAY,           // Relay-BP on float LLRs (qd_decoder_create_relay): qd_bp_relay_kernel (bp_relay.hip)
};

// What qd_decoder_reserve allocates for a batch size; free_ws gives all of it back
struct Workspace {
    DevAllocs dev;              // every device array below
    float *llr_ws = nullptr;
    float *marg_ws = nullptr;   // [cap][n_pad] Relay-BP with its marginals in device memory (qd_decoder::relay_marg_device): RelayArgs::marg_ws
    int32_t *fail_list = nullptr, *fail_count = nullptr;     // fail_count: the counter set of the call in flight = ctr_base + 64 * cset
    // Two sets of counters (fail / hard / redo / recheck counts), used by alternate calls.  A call's BP stage needs its set at zero; the set is zeroed by
    // the post-processing stage of the call BEFORE, on ITS stream (that set was last used two calls ago) -- not by fills at the head of the BP stage: in the
    // pipelined driver those fills sat between two BP kernels and each chunk lost ~2 ms there (a 4-byte fill launched the moment the other stream's OSD
    // kernel starts takes 1.9-2.1 ms, profiles/r06_bp_stream_bubble.txt).  set_clean: the set has been zeroed by an operation already queued.  After
    // qd_decoder_reserve neither set is: the first call on each zeroes it at its head, on its own stream.
    int32_t *ctr_base = nullptr;
    // the failure count of an earlier call, read back without waiting (pinned copy + event queued behind a post-processing stage): OSD-0 decoders launch the
    // hold of qd_decoder_post_head_start only when that says "heavy" -- even an empty launch between two BP kernels costs the headline 0.8 %
    int32_t *host_fail = nullptr;
    hipEvent_t fail_ready = nullptr;
    bool fail_pending = false;
    uint16_t *order_ws = nullptr;
    uint64_t *q_spill = nullptr, *q_spill_fast = nullptr, *mt_ws = nullptr;
    uint64_t *q_spill_sr = nullptr;
    uint64_t *q_spill_off = nullptr;   // [post_blocks][qd_osd_offchip_ws_words] spilled Q planes of qd_osd0_offchip_kernel
    int32_t *hard_list = nullptr, *hard_list2 = nullptr;
    int post_blocks = 0;        // workgroups of the post-processor's own kernel: qd_osd0_sr_kernel (osd_sr.hip), qd_osdcs_kernel or qd_lsd0_kernel
    uint64_t *cs_ws = nullptr;  // [post_blocks][qd_osdcs_ws_words] Q columns for the candidate sweep
    uint64_t *lsd_ws = nullptr; // [post_blocks][mw][m_pad] Q planes, then the work counter
    GenWs gws{};
    GenStagePlan gsp{};         // serial schedule: the launches' iteration bounds, the second workspace, the survivor lists (nbounds = 0: one launch)
    int32_t *redo_list = nullptr;
    int redo_cap = 0;
    int32_t *recheck_list = nullptr;           // shots the scatter kernel's bound could not certify
    int recheck_cap = 0;
};

struct qd_decoder {
    const qd_graph *g = nullptr;
    qd_params prm{};
    BpPath bp = BP_GATHER_RAW;
    int post = QD_POST_NONE;    // QD_POST_*: the post-processor, chosen once by qd_decoder_create
    int64_t cap = 0;            // the batch size ws is cut for (0: nothing reserved)
    Workspace ws;
    int osd_blocks = 0;
    int cset = 0;               // (see Workspace::ctr_base)
    bool set_clean[2] = {false, false};
    int64_t last_B = 0;         // batch size of the last BP stage (qd_decoder_post_head_start prices its failure count against it)
    int64_t fail_pending_B = 0; // (see Workspace::host_fail)
    double fail_frac_hint = -1.0;
    int osd_blocks_fast = 0;
    int cs_off[16] = {0}, cs_variant = 0, cs_lds = 0, cs_per_cu = 0;
    int osd_w = 0;
    int lsd_w = 0;              // higher-order LSD: 0 = LSD-0, 1 = combination sweep, 2 = exhaustive (order = prm.osd_order)
    int64_t gen_ws_limit = 0;   // bytes; 0 = default
    int gen_bounds[QD_GEN_MAX_STAGES] = {0}, gen_nbounds = 0;   // the bounds every reserve starts ws.gsp from
    // ---- LLR grid (flooding min-sum, ms_scaling 1): decoder-owned prior arrays on the fine and the coarse grid
    int grid_k = -1, grid_kc = -1, grid_floor = 0;   // grid_floor: the fine grid is the 2^-10 floor, not the rule's: any number of shots may need the redo pass
    BpGraphDev bp_fine{}, bp_coarse{};         // copies of g->bp with their own bit_rec
    const float *llr0_q = nullptr;             // fault-order LLRs for the one-message-per-edge kernel (fine grid)
    const float *llr0_qc = nullptr;            // ... on the coarse grid (edge_cert)
    bool off_chip = false;                     // the graph is off-chip, or QD_FLAG_OFF_CHIP: edge kernel, qd_osd0_offchip_kernel
    bool edge_cert = false;                    // off_chip and on the LLR grid: the edge kernel certifies its shots and the tripped ones are decoded again
    const int32_t *prior_g = nullptr;          // [n_pad] fine-grid channel LLRs of the bit slots in grid units (scatter kernels)
    float m2_limit = 0.f;
    const uint32_t *first_pass = nullptr;      // [m_pad][8] gather pass 0 of every check slot (ScatArgs::first_pass); null: the kernel runs it (QD_BP_NO_FAST_START=1)
    RelayArgs relay{};                         // BP_RELAY: budgets, the gamma table in slot order (owned by mem), the kernel's LDS layout
    bool relay_marg_device = false;            // BP_RELAY: the marginals are rows of ws.marg_ws (bp_relay_device.hip), not LDS
    int relay_lds_form = 0;                    // BP_RELAY: what the window's LDS form takes (it may not fit: qd_decoder_relay_info)
    DevAllocs mem;
    int profiling = 0;
    struct Span { int kind; hipEvent_t t0, t1; };   // kind 0 = BP kernel, 1 = OSD kernel(s)
    std::vector<Span> ev;
    double acc_ms[4] = {0, 0, 0, 0};
};

struct qd_spmat {
    int device = 0;
    SpmatDev d{};
    DevAllocs mem;
};

struct qd_circuit {
    int device = 0;
    FrameDev d{};
    int nq = 0, nmeas = 0, ndet = 0, nobs = 0;
    int64_t nsites = 0;
    DevAllocs mem;
};

struct qd_strata {
    int device = 0;
    int n = 0, kmax = 0;
    const uint32_t *thr = nullptr;     // [n][kmax + 1]
    DevAllocs mem;
};

// ---- the launchers and layout functions of the kernel files
hipError_t qd_launch_bp(const BpGraphDev &g, const DecodeArgs &a, int64_t B, hipStream_t s);
hipError_t qd_launch_bp_scatter_wide(const BpGraphDev &g, const ScatGraphDev &sg, const DecodeArgs &a, const ScatArgs &x, int64_t B, hipStream_t s);
hipError_t qd_launch_bp_first_pass(const BpGraphDev &g, const ScatGraphDev &sg, const int32_t *prior_g, uint32_t *rec, hipStream_t s);
hipError_t qd_launch_bp_general(const GenGraphDev &g, const BpGraphDev &bg, const DecodeArgs &a, const GenWs &w, int bp_method,
                                int schedule, int64_t shot0, int nshots, hipStream_t s, GenStagePlan *plan);
hipError_t qd_launch_bp_relay(const BpGraphDev &g, const DecodeArgs &a, const RelayArgs &x, int64_t B, hipStream_t s);
hipError_t qd_launch_bp_relay_device(const BpGraphDev &g, const DecodeArgs &a, const RelayArgs &x, int64_t B, hipStream_t s);   // bp_relay_device.hip
int qd_relay_layout(const BpGraphDev &g, bool marg_device, RelayArgs *x);   // fills the off_* members and lds_bytes, which it returns
hipError_t qd_launch_hold(const int32_t *count, int threshold, int microseconds, hipStream_t s);
int qd_bp_ps_lds_bytes(const GenGraphDev &g, int max_rdeg);
hipError_t qd_launch_bp_ps_lds(const GenGraphDev &g, const BpGraphDev &bg, const DecodeArgs &a, int64_t B, hipStream_t s);
hipError_t qd_launch_osd0(const OsdGraphDev &g, const BpGraphDev &bg, const DecodeArgs &a, int blocks_fast,
                          int blocks_full, hipStream_t s, bool handed_over = false);
int qd_osd_sr_layout(int m, int m_pad, int n, int out_words, int *off13, int *threads, int *rpt);
hipError_t qd_launch_osd0_sr(const OsdGraphDev &g, const BpGraphDev &bg, const DecodeArgs &a, int blocks, hipStream_t s);
// osd_cs.hip: OSD-CS / OSD-E, the rebuilt column-form kernel
int qd_osdcs_layout(int m, int n, int out_words, uint32_t max_wfix, int *off, int *variant, int *per_cu);
size_t qd_osdcs_ws_words(int variant);
hipError_t qd_launch_osdcs(const OsdGraphDev &g, const BpGraphDev &bg, const DecodeArgs &a, const int *off, int variant, int lds,
                           uint64_t *ws, int blocks, hipStream_t s);
size_t qd_osd_sr_ws_words(int m_pad, int mw, int threads, int rpt);
// osd_offchip.hip: OSD-0 for off-chip windows
int qd_osd_offchip_layout(int m, int n, int max_cdeg, int *off, int *off_sort, int *off_order, int *kw, int *threads, int *per_cu);
size_t qd_osd_offchip_ws_words(int m, int kw);
hipError_t qd_launch_osd0_offchip(const OsdGraphDev &g, const BpGraphDev &bg, const DecodeArgs &a, const int *off, int off_sort, int off_order,
                                  int kw, int threads, int lds, uint64_t *q_ws, int blocks, hipStream_t s);
hipError_t qd_launch_lsd0(const GenGraphDev &gg, const BpGraphDev &bg, const DecodeArgs &d, uint64_t *q_ws, int blocks_alloc, int blocks,
                          int lsd_w, int lsd_order, const uint32_t *wfix, hipStream_t s);
size_t qd_lsd_ws_bytes(int m, int n, int blocks, int lsd_w);
int qd_lsd_lds_bytes(int m, int n, int out_words);
hipError_t qd_launch_stage_llr(const float *llr_in, int n, int n_pad, const uint32_t *bit_orig, int64_t B, float *llr_ws,
                               int32_t *fail_list, int32_t *fail_count, int32_t *status, hipStream_t s);
hipError_t qd_launch_spmv(const SpmatDev &A, const uint32_t *err, int64_t err_stride, int64_t B, uint8_t *out,
                          int64_t out_stride, int accumulate, hipStream_t s);
hipError_t qd_launch_unpack(const uint32_t *bits, int64_t stride_words, int nbits, int64_t B, uint8_t *out,
                            int64_t out_stride, hipStream_t s);
hipError_t qd_launch_count(const uint8_t *pred, const uint8_t *obs, int k, int64_t B, int64_t *count, hipStream_t s);
hipError_t qd_launch_sample(const SpmatDev &Ht, const SpmatDev &Lt, const uint32_t *thr, uint64_t seed, int64_t shot0,
                            const int64_t *shot_list, int64_t B, int m, int nobs, uint8_t *det, int64_t det_stride, uint8_t *obs,
                            int64_t obs_stride, hipStream_t s);
#define QD_SAMPLE_LDS_MAX (64 * 1024)   // the DEM sampler's LDS: detector and observable bits, and the fault bitmap where it still fits (else a global row)
// qd_sample.hip: qd_sample_dem / qd_sample_dem_shots / qd_sample_dem_faults (d_fault_bits == nullptr: the faults are not kept)
int qd_sample_dem_impl(const qd_spmat *Ht, const qd_spmat *Lt, const double *priors, uint64_t seed, int64_t shot0, const int64_t *d_shots,
                       int64_t B, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride, uint32_t *d_fault_bits,
                       int64_t fault_stride_words, void *stream);
// faults.hip: the sampler with its fault bitmap, committed corrections and the fault statistics of a memory experiment
hipError_t qd_launch_sample_faults(const SpmatDev &Ht, const SpmatDev &Lt, const uint32_t *thr, uint64_t seed, int64_t shot0,
                                   const int64_t *shot_list, int64_t B, int m, int nobs, uint8_t *det, int64_t det_stride, uint8_t *obs,
                                   int64_t obs_stride, uint32_t *fault_bits, int64_t fault_stride, hipStream_t s);
hipError_t qd_launch_commit_bits(const uint32_t *err, int64_t err_stride, int nbits, int64_t B, uint32_t *out, int64_t out_stride, int64_t out_bit0,
                                 hipStream_t s);
hipError_t qd_launch_fault_stats(const uint32_t *faults, const uint32_t *corr, int64_t stride, int nbits, const uint8_t *residual, int64_t res_stride,
                                 int m, const uint64_t *fail_mask, int64_t B, int64_t shot0, int64_t *hist, int64_t *counts, uint64_t *best, hipStream_t s);
// strata_sampler.hip: the stratified DEM sampler (rows with a prescribed number of faults)
hipError_t qd_launch_sample_strata(const SpmatDev &Ht, const SpmatDev &Lt, const uint32_t *thr, int kmax, uint64_t seed, int64_t shot0,
                                   const int64_t *shot_list, const int32_t *kk, int64_t B, int m, int nobs, uint8_t *det, int64_t det_stride,
                                   uint8_t *obs, int64_t obs_stride, uint32_t *fault_bits, int64_t fault_stride, hipStream_t s);
// experiment.hip: the flag byte per shot and the tallies of a memory experiment
hipError_t qd_launch_shot_flags(const int32_t *status, int64_t B, uint8_t *flags, hipStream_t s);
hipError_t qd_launch_tally(const uint8_t *pred, int64_t pred_stride, const uint8_t *obs, int64_t obs_stride, int k, int64_t B,
                           const uint8_t *flags, int64_t *counts, uint64_t *fail_mask, hipStream_t s);
// frame_sampler.hip: the circuit-level sampler
hipError_t qd_launch_frame_sample(const FrameDev &c, uint64_t seed, int64_t shot0, const int64_t *shot_list, int64_t B, uint8_t *det,
                                  int64_t det_stride, uint8_t *obs, int64_t obs_stride, hipStream_t s);
