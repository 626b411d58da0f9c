// qd_api.hip -- host side of libquits_amd.so: the extern "C" entry points declared in include/quits_amd.h.
#include "../../include/quits_amd.h"
#include "qd_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <vector>

#define QD_GEN_PREFIX_LDS (32 * 1024)   // LDS a workgroup of the serial BP kernel may spend on row prefixes (128 slots x 64 shots): five workgroups per CU stay resident

hipError_t qd_launch_bp(const BpGraphDev &g, const DecodeArgs &a, int64_t B, hipStream_t s);
hipError_t qd_launch_bp_scatter(const BpGraphDev &g, const ScatGraphDev &sg, const DecodeArgs &a, const ScatArgs &x, int64_t B, hipStream_t s);
hipError_t qd_launch_bp_scatter_wide(const BpGraphDev &g, const ScatGraphDev &sg, const DecodeArgs &a, const ScatArgs &x, int64_t B, hipStream_t s);
hipError_t qd_launch_bp_first_pass(const BpGraphDev &g, const ScatGraphDev &sg, const int32_t *prior_g, uint32_t *rec, hipStream_t s);
hipError_t qd_launch_bp_general(const GenGraphDev &g, const BpGraphDev &bg, const DecodeArgs &a, const GenWs &w, int bp_method,
                                int schedule, int64_t shot0, int nshots, hipStream_t s, GenStagePlan *plan);
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
// experiment.hip: the flag byte per shot and the tallies of a memory experiment
hipError_t qd_launch_shot_flags(const int32_t *status, int64_t B, uint8_t *flags, hipStream_t s);
hipError_t qd_launch_tally(const uint8_t *pred, int64_t pred_stride, const uint8_t *obs, int64_t obs_stride, int k, int64_t B,
                           const uint8_t *flags, int64_t *counts, uint64_t *fail_mask, hipStream_t s);

static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(QD_EHIP, "%s: %s", #expr, hipGetErrorString(e_));              \
    } while (0)

struct DevAllocs {
    std::vector<void *> ptrs;
    template <class Tp> int upload(const std::vector<Tp> &h, const Tp **out)
    {
        void *d = nullptr;
        size_t bytes = std::max<size_t>(h.size() * sizeof(Tp), 16);
        if (hipMalloc(&d, bytes) != hipSuccess) return -1;
        ptrs.push_back(d);
        if (!h.empty() && hipMemcpy(d, h.data(), h.size() * sizeof(Tp), hipMemcpyHostToDevice) != hipSuccess) return -1;
        *out = reinterpret_cast<const Tp *>(d);
        return 0;
    }
    void release()
    {
        for (void *p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};

// The validation switches of include/quits_amd.h: each selects an alternative that the tests compare bit for bit against the default.
// Read here alone, when a graph or a decoder is created; nothing on the decode path reads the environment.
struct Switches {
    bool no_scatter, scatter_cpl1, scatter_wide_t704, scatter_natural_rounds, scatter_banks_by_slot, scatter_walk_greedy, osdcs_old, bp_no_fast_start;
    float scatter_m2_limit;             // +inf: not set
    std::vector<int> gen_stages;        // iteration bounds between the launches of the serial schedule in the one-message-per-edge kernel
};

static Switches read_switches()
{
    auto env = [](const char *name) { return std::getenv(name); };
    Switches w{};
    w.no_scatter = env("QD_NO_SCATTER") != nullptr;
    w.scatter_cpl1 = env("QD_SCATTER_CPL1") != nullptr;
    w.scatter_wide_t704 = env("QD_SCATTER_WIDE_T704") != nullptr;
    w.scatter_natural_rounds = env("QD_SCATTER_NATURAL_ROUNDS") != nullptr;
    w.scatter_banks_by_slot = env("QD_SCATTER_BANKS_BY_SLOT") != nullptr;
    w.scatter_walk_greedy = env("QD_SCATTER_WALK_GREEDY") != nullptr;
    const char *ev = env("QD_BP_NO_FAST_START");
    w.bp_no_fast_start = ev && std::atoi(ev) == 1;
    ev = env("QD_OSDCS_OLD");
    w.osdcs_old = ev && std::atoi(ev) == 1;
    ev = env("QD_SCATTER_M2_LIMIT");
    w.scatter_m2_limit = ev ? (float)std::atof(ev) : INFINITY;
    // after iterations 3, 6, 10, 14, 20, ... (x ~1.4); QD_GEN_STAGES="3,6" sets them, QD_GEN_STAGES=0 = one launch
    // (max_iter 10: "3,6" 50.5 ms, "3,5,7" 51.4, "4" 51.4, one launch 56.0: profiles/r06_k1g_staged_ab.txt)
    w.gen_stages = {3, 6, 10, 14, 20, 28, 40, 56, 80, 112};
    if ((ev = env("QD_GEN_STAGES"))) {
        w.gen_stages.clear();
        for (const char *q = ev; *q;) {
            char *end = nullptr;
            const long v = std::strtol(q, &end, 10);
            if (end == q) break;
            if (v > 0) w.gen_stages.push_back((int)v);
            q = *end ? end + 1 : end;
        }
    }
    return w;
}

struct qd_graph {
    int device = 0;
    int m = 0, n = 0, nnz = 0, max_rdeg = 0, max_cdeg = 0, rank = -1;
    BpGraphDev bp{};
    GenGraphDev gen{};
    OsdGraphDev osd{};
    DevAllocs mem;
    std::vector<int32_t> h_cp, h_ri;   // host CSC, for the rank
    std::vector<double> h_llr0;        // log((1-p)/p) in double, fault order
    ScatGraphDev sc{};                 // scatter form of the flooding min-sum kernel (bp_scatter.hip); sc.ok = 0: not for this window
    std::vector<uint32_t> h_bit_rec;   // host copy of bp.bit_rec: a decoder on an LLR grid uploads its own with word 0 replaced
    std::vector<uint32_t> h_bit_orig;  // bit slot -> fault
    std::vector<int32_t> h_sc_slot;    // fault -> accumulator slot of the scatter kernels (empty: they are not used)
    long long sc_walk_cycles = 0, sc_walk_ideal = 0;   // modelled LDS cycles of one pass of the scatter kernels' walk, and without any bank conflict
    // Off-chip window: build_bp cannot lay out the gather kernel's LDS state.  bp then holds the shapes and the slot orders alone (threads = lds_bytes = 0),
    // there is no scatter view, BP runs in the one-message-per-edge kernel and OSD-0 in qd_osd0_offchip_kernel.
    bool off_chip = false;
    // LDS layout of qd_osd0_offchip_kernel (x_lds = 0: even its row state does not fit): any window can take it (QD_FLAG_OFF_CHIP)
    int x_off[10] = {0}, x_off_sort = 0, x_off_order = 0, x_kw = 0, x_threads = 0, x_per_cu = 0, x_lds = 0;
    ~qd_graph() { mem.release(); }
};

// The BP kernel(s) of a decoder's stage 1, chosen once by qd_decoder_create
enum BpPath {
    BP_LDS_EDGE,        // flooding product-sum, one message per edge, every message in LDS (qd_launch_bp_ps_lds)
    BP_HBM_EDGE,        // one message per edge in an HBM workspace (bp_general.hip): every other method / schedule, QD_FLAG_EDGE_MESSAGES, and every
                        // pair of an off-chip decoder (flooding min-sum on the grid: with the exactness certificate and the coarse-grid redo pass)
    BP_SCATTER_WIDE,    // flooding min-sum on the LLR grid, several checks per lane (bp_scatter_wide.hip); recheck + coarse grid: gather kernel
    BP_SCATTER,         // ... one check per lane (bp_scatter.hip); recheck + coarse grid: gather kernel
    BP_GATHER_GRID,     // ... the gather kernel (bp_kernels.hip) on the fine grid, then on the coarse grid
    BP_GATHER_RAW,      // flooding min-sum on float LLRs off the grid (ms_scaling_factor != 1, QD_FLAG_RAW_LLR): the gather kernel
};

struct qd_decoder {
    const qd_graph *g = nullptr;
    qd_params prm{};
    BpPath bp = BP_GATHER_RAW;
    int post = QD_POST_NONE;    // QD_POST_*: the post-processor, chosen once by qd_decoder_create
    int64_t cap = 0;
    int osd_blocks = 0;
    float *llr_ws = nullptr;
    int32_t *fail_list = nullptr, *fail_count = nullptr;     // fail_count: the counter set of the call in flight = ctr_base + 64 * cset
    // Two sets of counters (fail / hard / redo / recheck counts), used by alternate calls.  A call's BP stage needs its set at zero; the set is zeroed by
    // the post-processing stage of the call BEFORE, on ITS stream (that set was last used two calls ago) -- not by fills at the head of the BP stage: in the
    // pipelined driver those fills sat between two BP kernels and each chunk lost ~2 ms there (a 4-byte fill launched the moment the other stream's OSD
    // kernel starts takes 1.9-2.1 ms, profiles/r06_bp_stream_bubble.txt).  set_clean: the set has been zeroed by an operation already queued.  After
    // qd_decoder_reserve neither set is: the first call on each zeroes it at its head, on its own stream.
    int32_t *ctr_base = nullptr;
    int cset = 0;
    bool set_clean[2] = {false, false};
    int64_t last_B = 0;         // batch size of the last BP stage (qd_decoder_post_head_start prices its failure count against it)
    // the failure count of an earlier call, read back without waiting (pinned copy + event queued behind a post-processing stage): OSD-0 decoders launch the
    // hold of qd_decoder_post_head_start only when that says "heavy" -- even an empty launch between two BP kernels costs the headline 0.8 %
    int32_t *host_fail = nullptr;
    hipEvent_t fail_ready = nullptr;
    bool fail_pending = false;
    int64_t fail_pending_B = 0;
    double fail_frac_hint = -1.0;
    uint16_t *order_ws = nullptr;
    uint64_t *q_spill = nullptr, *q_spill_fast = nullptr, *mt_ws = nullptr;
    uint64_t *q_spill_sr = nullptr;
    uint64_t *q_spill_off = nullptr;   // [post_blocks][qd_osd_offchip_ws_words] spilled Q planes of qd_osd0_offchip_kernel
    int32_t *hard_list = nullptr, *hard_list2 = nullptr;
    int osd_blocks_fast = 0;
    int post_blocks = 0;        // workgroups of the post-processor's own kernel: qd_osd0_sr_kernel (osd_sr.hip), qd_osdcs_kernel or qd_lsd0_kernel
    int cs_off[16] = {0}, cs_variant = 0, cs_lds = 0, cs_per_cu = 0;
    uint64_t *cs_ws = nullptr;  // [post_blocks][qd_osdcs_ws_words] Q columns for the candidate sweep
    int osd_w = 0;
    int lsd_w = 0;              // higher-order LSD: 0 = LSD-0, 1 = combination sweep, 2 = exhaustive (order = prm.osd_order)
    uint64_t *lsd_ws = nullptr; // [post_blocks][mw][m_pad] Q planes, then the work counter
    int64_t gen_ws_limit = 0;   // bytes; 0 = default
    GenWs gws{};
    GenStagePlan gsp{};         // serial schedule: the launches' iteration bounds, the second workspace, the survivor lists (nbounds = 0: one launch)
    int gen_bounds[QD_GEN_MAX_STAGES] = {0}, gen_nbounds = 0;   // the bounds every reserve starts gsp from
    // ---- LLR grid (flooding min-sum, ms_scaling 1): decoder-owned prior arrays on the fine and the coarse grid
    int grid_k = -1, grid_kc = -1, grid_floor = 0;   // grid_floor: the fine grid is the 2^-10 floor, not the rule's: any number of shots may need the redo pass
    BpGraphDev bp_fine{}, bp_coarse{};         // copies of g->bp with their own bit_rec
    const float *llr0_q = nullptr;             // fault-order LLRs for the one-message-per-edge kernel (fine grid)
    const float *llr0_qc = nullptr;            // ... on the coarse grid (edge_cert)
    bool off_chip = false;                     // the graph is off-chip, or QD_FLAG_OFF_CHIP: edge kernel, qd_osd0_offchip_kernel
    bool edge_cert = false;                    // off_chip and on the LLR grid: the edge kernel certifies its shots and the tripped ones are decoded again
    int32_t *redo_list = nullptr;
    int redo_cap = 0;
    const int32_t *prior_g = nullptr;          // [n_pad] fine-grid channel LLRs of the bit slots in grid units (scatter kernels)
    float m2_limit = 0.f;
    const uint32_t *first_pass = nullptr;      // [m_pad][8] gather pass 0 of every check slot (ScatArgs::first_pass); null: the kernel runs it (QD_BP_NO_FAST_START=1, one check per lane)
    int32_t *recheck_list = nullptr;           // shots the scatter kernel's bound could not certify
    int recheck_cap = 0;
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

#define QD_GRID_MIN_BITS 10
static inline int align16(int x) { return (x + 15) & ~15; }
static inline int pad64(int x) { return (x + 63) & ~63; }

// ---- LDS banks for the scatter kernels (bp_scatter.hip, bp_scatter_wide.hip) --------------------------------------------------
// Step k of a wavefront's walk is one ds_read_b32 (gather pass) and one ds_add_u32 (scatter pass) over the accumulators of the faults
// its 64 checks meet at that step, serviced in two groups of 32 lanes with bank = (address / 4) mod 32 and one extra LDS cycle per
// additional lane on a busy bank (MI355X_MICROARCH.md, LDS; an atomic does not broadcast).  Two things are free: which bank a fault's
// accumulator lives in (the slot order is the kernels' own) and the order in which a check walks its edges (min, second min and sign
// parity are symmetric).  A group of 32 checks x 32 banks is a bipartite multigraph; if no bank receives more edges from the group
// than the group has steps, it splits into that many matchings (Koenig), i.e. a walk without a single conflict.  So:
//   scatter_banks: choose the banks so that every group's 32 bank loads are as equal as possible (descent on the sum of squared loads,
//                  one fault at a time, deterministic; starts from the degree-sorted bit slots mod 32);
//   scatter_walk:  step by step, a maximum matching of the group's unfinished checks into the banks (banks with the largest remaining
//                  load first: a bank whose remaining load equals the remaining steps must be served now); a check the matching leaves out
//                  takes its edge on the least busy bank; steps beyond a check's degree point at a trash slot on a bank nobody uses.
// Headline window (1008 x 9504): 1932 modelled cycles per pass with the round-3 greedy walk over the degree-sorted slots, 1109 here,
// 1052 without any conflict (WindowGraph.info(): scatter_walk_cycles / _ideal).
// by_slot (QD_SCATTER_BANKS_BY_SLOT): the round-3 assignment, the starting point alone
static void scatter_banks(int m, int n, const int32_t *row_ptr, const int32_t *col_idx, const std::vector<int> &chk_orig,
                          const std::vector<int> &bit_slot_of, bool by_slot, std::vector<int> &bank)
{
    const int nh = (m + 31) / 32;
    bank.resize(n);
    for (int j = 0; j < n; ++j) bank[j] = bit_slot_of[j] & 31;
    if (by_slot) return;
    // fault -> (group, edges from that group)
    std::vector<std::vector<std::pair<int, int>>> fh(n);
    std::vector<int> load((size_t)nh * 32, 0), cnt(32, 0);
    for (int h = 0; h < nh; ++h)
        for (int s = 32 * h; s < std::min(m, 32 * h + 32); ++s) {
            const int i = chk_orig[s];
            for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
                const int j = col_idx[e];
                if (!fh[j].empty() && fh[j].back().first == h) fh[j].back().second++;
                else fh[j].push_back({h, 1});
                load[(size_t)h * 32 + bank[j]]++;
            }
        }
    for (int j = 0; j < n; ++j) cnt[bank[j]]++;
    const int cap = (n + 31) / 32 + 1;                               // slots per bank: the LDS footprint stays within 32 slots of pad64(n)
    for (int pass = 0; pass < 40; ++pass) {
        int moved = 0;
        for (int j = 0; j < n; ++j) {
            if (fh[j].empty()) continue;
            const int b0 = bank[j];
            long long stay = 0;                                      // what the sum of squares gains back when j leaves b0 ...
            for (auto &hm : fh[j]) stay += 2ll * load[(size_t)hm.first * 32 + b0] * hm.second - (long long)hm.second * hm.second;
            long long best = stay;
            int bb = b0;
            for (int b = 0; b < 32; ++b) {
                if (b == b0 || cnt[b] >= cap) continue;
                long long add = 0;                                   // ... and what it pays to enter b
                for (auto &hm : fh[j]) add += 2ll * load[(size_t)hm.first * 32 + b] * hm.second + (long long)hm.second * hm.second;
                if (add < best) { best = add; bb = b; }
            }
            if (bb != b0) {
                for (auto &hm : fh[j]) { load[(size_t)hm.first * 32 + b0] -= hm.second; load[(size_t)hm.first * 32 + bb] += hm.second; }
                cnt[b0]--; cnt[bb]++; bank[j] = bb; ++moved;
            }
        }
        if (!moved) break;
    }
}

// put(s, k, e, trash_bank): check slot s takes CSR edge e at step k (e < 0: a step beyond its degree, reading / adding 0 to the trash slot of trash_bank)
// greedy_only (QD_SCATTER_WALK_GREEDY): no matching, every check takes its least busy bank
template <class Put>
static void scatter_walk(int m, const int32_t *row_ptr, const int32_t *col_idx, const std::vector<int> &chk_orig, const std::vector<int> &bank,
                         bool greedy_only, Put put, long long *cycles, long long *ideal)
{
    std::vector<std::vector<int>> rem(32);
    for (int w0 = 0; w0 < m; w0 += 64) {
        int trip = 0;
        for (int s = w0; s < std::min(m, w0 + 64); ++s) trip = std::max(trip, (int)(row_ptr[chk_orig[s] + 1] - row_ptr[chk_orig[s]]));
        trip = (trip + 3) & ~3;                                      // what the wavefront of these 64 slots walks (ScatGraphDev::deg_w)
        for (int g0 = w0; g0 < std::min(m, w0 + 64); g0 += 32) {
            const int gn = std::min(32, m - g0);
            for (int l = 0; l < gn; ++l) {
                const int i = chk_orig[g0 + l];
                rem[l].assign(col_idx + row_ptr[i], col_idx + row_ptr[i + 1]);     // faults; the CSR edge is found again by its column
            }
            auto take = [&](int l, int b, int k) {                   // lane l takes one of its remaining edges on bank b at step k
                const int i = chk_orig[g0 + l];
                for (size_t y = 0; y < rem[l].size(); ++y)
                    if (bank[rem[l][y]] == b) {
                        const int j = rem[l][y];
                        rem[l].erase(rem[l].begin() + (long)y);
                        const int e = (int)(std::lower_bound(col_idx + row_ptr[i], col_idx + row_ptr[i + 1], j) - col_idx);
                        put(g0 + l, k, e, 0);
                        return;
                    }
            };
            for (int k = 0; k < trip; ++k) {
                int rl[32] = {0}, used[32] = {0}, match_b[32], nact = 0, act[32];
                for (int b = 0; b < 32; ++b) match_b[b] = -1;
                for (int l = 0; l < gn; ++l)
                    if (!rem[l].empty()) { act[nact++] = l; for (int j : rem[l]) rl[bank[j]]++; }
                if (nact) {
                    // options of a lane: the banks of its remaining edges, busiest (remaining load) first
                    std::vector<int> opts[32];
                    for (int x = 0; x < nact; ++x) {
                        const int l = act[x];
                        bool has[32] = {false};
                        for (int j : rem[l]) has[bank[j]] = true;
                        for (int b = 0; b < 32; ++b) if (has[b]) opts[l].push_back(b);
                        std::stable_sort(opts[l].begin(), opts[l].end(), [&](int a, int b) { return rl[a] > rl[b]; });
                    }
                    std::stable_sort(act, act + nact, [&](int a, int b) { return opts[a].size() < opts[b].size(); });
                    bool seen[32];
                    // augmenting paths (Kuhn); 32 x 32, recursion depth <= 32
                    struct Aug {
                        std::vector<int> *opts; int *match_b; bool *seen;
                        bool run(int l) {
                            for (int b : opts[l]) {
                                if (seen[b]) continue;
                                seen[b] = true;
                                if (match_b[b] < 0 || run(match_b[b])) { match_b[b] = l; return true; }
                            }
                            return false;
                        }
                    } aug{opts, match_b, seen};
                    std::vector<int> left;
                    for (int x = 0; x < nact; ++x) {
                        if (greedy_only) { left.push_back(act[x]); continue; }
                        for (int b = 0; b < 32; ++b) seen[b] = false;
                        if (!aug.run(act[x])) left.push_back(act[x]);
                    }
                    for (int b = 0; b < 32; ++b)
                        if (match_b[b] >= 0) { take(match_b[b], b, k); used[b]++; }
                    for (int l : left) {                              // no free bank among its edges: the least busy one
                        int bb = -1;
                        for (int j : rem[l]) if (bb < 0 || used[bank[j]] < used[bb]) bb = bank[j];
                        take(l, bb, k); used[bb]++;
                    }
                    int mx = 0;
                    for (int b = 0; b < 32; ++b) mx = std::max(mx, used[b]);
                    *cycles += mx; *ideal += 1;
                }
                // lanes past their degree: the trash slot of a bank nobody uses at this step (there are 32 banks for 32 lanes)
                int fb = 0;
                for (int l = 0; l < 32; ++l) {
                    const bool real_lane = l < gn;
                    const int deg = real_lane ? (int)(row_ptr[chk_orig[g0 + l] + 1] - row_ptr[chk_orig[g0 + l]]) : 0;
                    if (k < deg) continue;
                    while (fb < 32 && used[fb]) ++fb;
                    const int b = fb < 32 ? fb : (l & 31);
                    if (fb < 32) used[fb]++;
                    if (g0 + l < ((m + 63) & ~63)) put(g0 + l, k, -1, b);
                }
            }
        }
    }
}

extern "C" int qd_version(void) { return 108; }      // 108: qd_shot_flags_fold, qd_tally_batch, qd_sample_circuit_shots, qd_sample_dem_shots (the device-resident memory experiment); 107: off-chip windows decode (qd_graph_create used to refuse them), QD_FLAG_OFF_CHIP, QD_POST_OSD0_OFFCHIP (no new export); 106: qd_circuit_create takes Y_ERROR / PAULI_CHANNEL_1 / PAULI_CHANNEL_2 programs (no new export); 105: qd_decoder_fast_start; 104: qd_circuit_* and qd_sample_circuit; 103: qd_decoder_post_head_start; 102: qd_graph_info fills 10 entries again, qd_graph_info_ex(g, info, n) the rest; 101: qd_decoder_postproc_kernel
extern "C" const char *qd_last_error(void) { return g_err; }
extern "C" int qd_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- qd_graph_create: host_graph validates the window and derives what the builders share, then one builder per device view, in this
// order: build_bp (slot orders and BpGraphDev), build_gen (GenGraphDev), build_scatter (ScatGraphDev), build_osd (OsdGraphDev).
struct HostGraph {
    int m = 0, n = 0, nnz = 0, max_rdeg = 0, max_cdeg = 0, min_rdeg = 0, m_pad = 0, n_pad = 0, max_rdeg_pad = 0;
    const int32_t *row_ptr = nullptr, *col_idx = nullptr;
    const double *priors = nullptr;
    std::vector<int> rdeg, cdeg;
    std::vector<double> llr0;                                        // log((1-p)/p), fault order
    std::vector<int32_t> cp, ri, pos;                                // CSC with the edge's position inside its row
    std::vector<int> chk_orig, chk_slot_of, bit_orig, bit_slot_of;   // slots: degree-descending, stable (build_bp)
    std::vector<uint8_t> chk_deg;                                    // [m_pad] degree of the check slot (build_bp)
};

static int host_graph(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx, const double *priors, HostGraph &h)
{
    if (m <= 0 || n <= 0 || !row_ptr || !col_idx || !priors) return fail(QD_EINVAL, "empty or null graph");
    if (m > 32767) return fail(QD_ECAPACITY, "m = %d detectors per window exceeds 32767", m);
    if (n > 65000) return fail(QD_ECAPACITY, "n = %d faults per window exceeds 65000", n);
    const int nnz = row_ptr[m];
    if (row_ptr[0] != 0 || nnz < 0) return fail(QD_EINVAL, "bad row_ptr");
    std::vector<int> &rdeg = h.rdeg, &cdeg = h.cdeg;
    rdeg.assign(m, 0); cdeg.assign(n, 0);
    for (int i = 0; i < m; ++i) {
        rdeg[i] = row_ptr[i + 1] - row_ptr[i];
        if (rdeg[i] < 0) return fail(QD_EINVAL, "row_ptr not monotone");
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            if (col_idx[e] < 0 || col_idx[e] >= n) return fail(QD_EINVAL, "column index out of range");
            if (e > row_ptr[i] && col_idx[e] <= col_idx[e - 1]) return fail(QD_EINVAL, "columns must ascend in a row");
            cdeg[col_idx[e]]++;
        }
    }
    for (int j = 0; j < n; ++j)
        if (!(priors[j] > 0.0 && priors[j] < 1.0)) return fail(QD_EINVAL, "prior %d = %g outside (0,1)", j, priors[j]);
    h.llr0.resize(n);
    for (int j = 0; j < n; ++j) h.llr0[j] = std::log((1.0 - priors[j]) / priors[j]);
    const int max_rdeg = *std::max_element(rdeg.begin(), rdeg.end());
    const int max_cdeg = *std::max_element(cdeg.begin(), cdeg.end());
    if (max_rdeg > QD_MAX_ROW_DEG || max_rdeg < 1)
        return fail(QD_ECAPACITY, "row weight %d outside 1..%d", max_rdeg, QD_MAX_ROW_DEG);
    if (max_cdeg > QD_MAX_COL_DEG || max_cdeg < 1)
        return fail(QD_ECAPACITY, "column weight %d outside 1..%d", max_cdeg, QD_MAX_COL_DEG);
    h.m = m; h.n = n; h.nnz = nnz; h.max_rdeg = max_rdeg; h.max_cdeg = max_cdeg;
    h.min_rdeg = *std::min_element(rdeg.begin(), rdeg.end());
    h.m_pad = pad64(m); h.n_pad = pad64(n); h.max_rdeg_pad = (max_rdeg + 3) & ~3;
    h.row_ptr = row_ptr; h.col_idx = col_idx; h.priors = priors;
    if (h.n_pad + 1 > 65535) return fail(QD_ECAPACITY, "n = %d faults per window: fault slots exceed 16 bits", n);
    // CSC with the edge's position inside its row
    h.cp.assign(n + 1, 0); h.ri.resize(nnz); h.pos.resize(nnz);
    for (int j = 0; j < n; ++j) h.cp[j + 1] = h.cp[j] + cdeg[j];
    std::vector<int> fill(n, 0);
    for (int i = 0; i < m; ++i)
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const int j = col_idx[e], dst = h.cp[j] + fill[j]++;
            h.ri[dst] = i; h.pos[dst] = e - row_ptr[i];
        }
    return QD_OK;
}

static int bp_block_threads(int m, int n) { return std::max(m, (n + 9) / 10) <= 256 ? 256 : (std::max(m, (n + 9) / 10) <= 512 ? 512 : 1024); }

static int scatter_wide_threads(int m) { return pad64((m + 1) / 2) <= 704 ? 704 : 1024; }

// The shape conditions of the scatter kernels (build_scatter checks their LDS fit).  1: one check per lane (bp_scatter.hip): every check
// has a lane and rows hold 2..64 faults (two sign words; a row of one fault has no second minimum) -- also the windows of <= 256 checks,
// 3.78 -> 3.00 ms per launch on the 108-check and 8.92 -> 7.73 ms on the 216-check windows of the W = 3 plans (profiles/r05_scatter_small_ab.txt).
// 2: several checks per lane (bp_scatter_wide.hip): more checks than a workgroup has lanes, or rows of 65..96 faults -- the QLP windows
// of BASELINE configs[4] (1326 checks of up to 78 faults on 704 lanes).  0: neither.
static int scatter_form(const HostGraph &h)
{
    const int threads = bp_block_threads(h.m, h.n);
    if (h.min_rdeg < 2) return 0;
    if (h.m <= threads && h.max_rdeg_pad <= 64) return 1;
    if (threads == 1024 && h.m <= 2 * scatter_wide_threads(h.m) && h.max_rdeg_pad <= 96 && (h.m > 1024 || h.max_rdeg_pad > 64)) return 2;
    return 0;
}

// Slot orders and the gather kernel's view (BpGraphDev): LDS carve-up, the checks' walk over their edges, the fault records
static int build_bp(qd_graph *g, HostGraph &h, bool walk_for_atomics)
{
    const int m = h.m, n = h.n, nnz = h.nnz, m_pad = h.m_pad, n_pad = h.n_pad, max_rdeg_pad = h.max_rdeg_pad;
    const int32_t *row_ptr = h.row_ptr, *col_idx = h.col_idx;
    const std::vector<int> &rdeg = h.rdeg, &cdeg = h.cdeg;
    const std::vector<int32_t> &cp = h.cp, &ri = h.ri;
    // slots: degree-descending, stable
    std::vector<int> &chk_slot_of = h.chk_slot_of, &chk_orig = h.chk_orig, &bit_slot_of = h.bit_slot_of, &bit_orig = h.bit_orig;
    chk_slot_of.resize(m); chk_orig.resize(m); bit_slot_of.resize(n); bit_orig.resize(n);
    std::iota(chk_orig.begin(), chk_orig.end(), 0);
    std::stable_sort(chk_orig.begin(), chk_orig.end(), [&](int a, int b) { return rdeg[a] > rdeg[b]; });
    for (int s = 0; s < m; ++s) chk_slot_of[chk_orig[s]] = s;
    std::iota(bit_orig.begin(), bit_orig.end(), 0);
    std::stable_sort(bit_orig.begin(), bit_orig.end(), [&](int a, int b) { return cdeg[a] > cdeg[b]; });
    for (int s = 0; s < n; ++s) bit_slot_of[bit_orig[s]] = s;

    BpGraphDev &bp = g->bp;
    bp.m = m; bp.n = n; bp.m_pad = m_pad; bp.n_pad = n_pad; bp.max_rdeg = h.max_rdeg; bp.max_cdeg = h.max_cdeg;
    bp.neg_words = (max_rdeg_pad + 31) / 32; bp.out_words = (n + 31) / 32;
    bp.max_rdeg_pad = max_rdeg_pad;
    bp.dummy_bit = n_pad; bp.dummy_chk = m_pad;        // one extra LDS slot each
    bp.sign_mode = max_rdeg_pad <= 32 ? 0 : (max_rdeg_pad <= 44 ? 1 : 2);    // mode 1: 15 spare bits of the state word hold signs 32..46
    // 32-bit offsets always (round 6: the 16-bit packing -- half of 66 KB of L2-resident adjacency for one more unpacking instruction per
    // edge, 60.4 -> 62.0 ms when K1 was the headline kernel -- was only reachable through an environment knob and doubled K1's instantiations: removed)
    bp.adj32 = 1;
    bp.rec_words = ((1 + h.max_cdeg) + 3) & ~3;
    // LDS carve-up
    int off = 0;
    bp.off_chk = off; off += (m_pad + 4) * 16;                 // + the dummy check
    bp.off_cneg = off; off += (bp.sign_mode == 2 ? align16((bp.neg_words - 1) * m_pad * 4) : 0);
    bp.off_llr = off; off += align16((n_pad + 4) * 4);         // + the dummy bit
    bp.off_out = off; off += align16(bp.out_words * 4);
    bp.off_misc = off; off += 256;
    bp.lds_bytes = off;
    // the state does not fit the CU, or a fault record cannot address a check's state with 16 bits: an off-chip window -- the slot orders alone
    if (bp.lds_bytes > QD_LDS_BYTES || (m_pad + 1) * 16 > 65535) {
        g->off_chip = true;
        bp.off_chk = bp.off_cneg = bp.off_llr = bp.off_out = bp.off_misc = bp.lds_bytes = 0;
        bp.threads = 0;
        std::vector<uint32_t> bit_orig_u(n_pad, 0), slot_of(bit_slot_of.begin(), bit_slot_of.end());
        for (int s = 0; s < n; ++s) bit_orig_u[s] = (uint32_t)bit_orig[s];
        g->h_bit_orig = bit_orig_u;
        if (g->mem.upload(bit_orig_u, &bp.bit_orig) | g->mem.upload(slot_of, &bp.bit_slot_of)) return fail(QD_EHIP, "device allocation/upload failed");
        return QD_OK;
    }
    bp.threads = bp_block_threads(m, n);

    std::vector<uint8_t> &chk_deg = h.chk_deg;
    chk_deg.assign(m_pad, 0);
    std::vector<uint8_t> bit_deg(n_pad, 0);
    std::vector<int32_t> chk_degp_w(m_pad / 64, 0);
    std::vector<uint32_t> chk_orig_u(m_pad, 0), bit_orig_u(n_pad, 0);
    std::vector<uint32_t> bit_rec((size_t)n_pad * bp.rec_words, (uint32_t)(bp.off_chk + bp.dummy_chk * 16) << 16);
    for (int s = 0; s < m; ++s) { chk_deg[s] = (uint8_t)rdeg[chk_orig[s]]; chk_orig_u[s] = (uint32_t)chk_orig[s]; }
    // wave-uniform trip counts (slots are degree-sorted, so a wavefront's lanes nearly agree anyway)
    for (int w0 = 0; w0 < m_pad; w0 += 64) {
        int mx = 0;
        for (int s = w0; s < w0 + 64; ++s) mx = std::max(mx, (int)chk_deg[s]);
        chk_degp_w[w0 / 64] = ((mx + 3) & ~3) | (mx << 16);      // trip count | exact maximum (edges beyond it are padding for every lane)
    }
    // check -> fault adjacency, ELL-transposed, as LDS byte offsets of the posteriors
    std::vector<uint32_t> chk_adj32((size_t)max_rdeg_pad * m_pad, (uint32_t)(bp.off_llr + bp.dummy_bit * 4));
    // Order in which a check walks its edges.  Nothing the check pass computes depends on it (minimum, second minimum and the
    // sign parity are symmetric; a tie for the minimum leaves min1 = min2, so it does not matter which edge carries the argmin
    // label), so it is chosen for the LDS: step k of a wavefront is one ds_read_b32 gather, serviced in two groups of 32 lanes
    // with bank = (address / 4) mod 32 (MI355X_MICROARCH.md, LDS), one extra cycle per additional distinct address on a bank.
    // Greedy per group of 32 check slots: at every step each check takes, among its remaining edges, the one whose bank has
    // the fewest distinct addresses so far in that step.  Headline window: 2918 -> 1463 LDS cycles per iteration for these
    // gathers (1062 without any conflict; tools/lds_model.py).
    // The scatter kernel (bp_scatter.hip) walks the same order with ds_add_u32, and lanes of one instruction that add to the SAME
    // address serialise like any other bank conflict (profiles/r03z_lds_atomic_rates.txt: two lanes per address 2.2 -> 4.7 ns per
    // instruction), where a gather broadcasts for free: for the windows that kernel takes (walk_for_atomics), a lane on a busy bank
    // costs one cycle whatever its address.
    std::vector<int32_t> step_of(nnz);              // CSR edge -> position in its check's walk
    {
        std::vector<std::vector<int>> rem(32);
        std::vector<int> used_cnt(32), order32(32);
        std::vector<std::vector<uint32_t>> used_addr(32);
        for (int g0 = 0; g0 < m; g0 += 32) {
            const int gn = std::min(32, m - g0);
            int kmax = 0;
            for (int l = 0; l < gn; ++l) {
                const int i = chk_orig[g0 + l];
                rem[l].clear();
                for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) rem[l].push_back(e);
                kmax = std::max(kmax, rdeg[i]);
            }
            for (int k = 0; k < kmax; ++k) {
                for (int b = 0; b < 32; ++b) { used_cnt[b] = 0; used_addr[b].clear(); }
                int na = 0;
                for (int l = 0; l < gn; ++l) if (!rem[l].empty()) order32[na++] = l;
                std::stable_sort(order32.begin(), order32.begin() + na, [&](int a, int b) { return rem[a].size() > rem[b].size(); });
                for (int x = 0; x < na; ++x) {
                    std::vector<int> &r = rem[order32[x]];
                    int best = 0, bestc = 1 << 30;
                    for (int y = 0; y < (int)r.size(); ++y) {
                        const uint32_t slot = (uint32_t)bit_slot_of[col_idx[r[y]]];
                        const int b = (int)(slot & 31u);
                        int c = used_cnt[b];
                        if (!walk_for_atomics)
                            for (uint32_t a : used_addr[b]) if (a == slot) { c = 0; break; }  // same address: a broadcast, free
                        if (c < bestc) { bestc = c; best = y; if (c == 0) break; }
                    }
                    const uint32_t slot = (uint32_t)bit_slot_of[col_idx[r[best]]];
                    bool dup = false;
                    for (uint32_t a : used_addr[slot & 31u]) dup |= (a == slot);
                    if (!dup) used_addr[slot & 31u].push_back(slot);
                    if (!dup || walk_for_atomics) used_cnt[slot & 31u]++;
                    step_of[r[best]] = k;
                    r.erase(r.begin() + best);
                }
            }
        }
    }
    std::vector<int32_t> wpos(nnz);                 // CSC edge -> position in its check's walk (pos[] stays the natural position)
    {
        std::vector<int> fill(n, 0);
        for (int i = 0; i < m; ++i)
            for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) wpos[cp[col_idx[e]] + fill[col_idx[e]]++] = step_of[e];
    }
    for (int s = 0; s < m; ++s) {
        const int i = chk_orig[s];
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const int k = step_of[e];
            const uint32_t off = (uint32_t)bp.off_llr + (uint32_t)bit_slot_of[col_idx[e]] * 4u;
            const size_t at = ((size_t)(k >> 2) * m_pad + s) * 4 + (k & 3);      // [group of 4 edges][slot][4]: one vector load per group
            chk_adj32[at] = off;
        }
    }
    // fault records: prior + (check state offset, where that check keeps this edge's sign)
    auto rec_at = [&](int slot, int word) { return ((size_t)(word >> 2) * n_pad + slot) * 4 + (word & 3); };   // [chunk][slot][4]
    for (int s = 0; s < n_pad; ++s) {
        const float one = 1.0f;
        std::memcpy(&bit_rec[rec_at(s, 0)], &one, 4);
    }
    for (int s = 0; s < n; ++s) {
        const int j = bit_orig[s];
        bit_deg[s] = (uint8_t)cdeg[j];
        bit_orig_u[s] = (uint32_t)j;
        const float l0 = (float)h.llr0[j];
        std::memcpy(&bit_rec[rec_at(s, 0)], &l0, 4);
        for (int q = 0; q < cdeg[j]; ++q) {
            const int cs = chk_slot_of[ri[cp[j] + q]];
            const int k = wpos[cp[j] + q];
            const int degp = chk_degp_w[cs / 64] & 0xFFFF;
            const int w = k >> 5, kend = std::min(degp - 32 * w, 32);
            const int sbit = kend - 1 - (k & 31);              // the check pass shifts signs in from bit 0 (v_alignbit)
            // mode 0/1: bit index into the 64-bit value {w : z} of the state (signs 32..46 sit in w's bits 16..30)
            const uint32_t where = bp.sign_mode == 2 ? (((uint32_t)w << 5) | (uint32_t)sbit)
                                                     : (uint32_t)(w == 0 ? sbit : 32 + 16 + sbit);
            bit_rec[rec_at(s, 1 + q)] = ((uint32_t)(bp.off_chk + cs * 16) << 16) | where;
        }
    }
    for (int q = 0; q < QD_MAX_COL_DEG; ++q) {
        int cnt = 0;
        for (int w0 = 0; w0 < n_pad; w0 += 64) {
            int mx = 0;
            for (int s = w0; s < w0 + 64; ++s) mx = std::max(mx, (int)bit_deg[s]);
            if (mx > q) cnt = w0 + 64;
        }
        bp.bit_thr[q] = cnt;
    }
    g->h_bit_rec = bit_rec; g->h_bit_orig = bit_orig_u;
    const std::vector<uint32_t> slot_of(bit_slot_of.begin(), bit_slot_of.end());
    int rc = 0;
    { const uint32_t *p32 = nullptr; rc |= g->mem.upload(chk_adj32, &p32); bp.chk_adj = p32; }
    rc |= g->mem.upload(chk_degp_w, &bp.chk_degp_w);
    rc |= g->mem.upload(chk_orig_u, &bp.chk_orig);
    rc |= g->mem.upload(bit_rec, &bp.bit_rec);
    rc |= g->mem.upload(bit_orig_u, &bp.bit_orig);
    rc |= g->mem.upload(slot_of, &bp.bit_slot_of);
    if (rc) return fail(QD_EHIP, "device allocation/upload failed");
    return QD_OK;
}

// The one-message-per-edge kernels' view (GenGraphDev): CSR / CSC, the serial schedule's levels and its rows' LDS prefix slots
static int build_gen(qd_graph *g, const HostGraph &h)
{
    const int m = h.m, n = h.n, nnz = h.nnz;
    const int32_t *row_ptr = h.row_ptr, *col_idx = h.col_idx;
    const std::vector<int32_t> &cp = h.cp, &ri = h.ri;
    GenGraphDev &gg = g->gen;
    gg.m = m; gg.n = n; gg.nnz = nnz; gg.out_words = (n + 31) / 32;
    std::vector<int32_t> rp_v(row_ptr, row_ptr + m + 1), ci_v(col_idx, col_idx + nnz), c2r(nnz);
    for (int e = 0; e < nnz; ++e) c2r[e] = row_ptr[ri[e]] + h.pos[e];
    const std::vector<float> l0(h.llr0.begin(), h.llr0.end());
    int rcg = 0;
    rcg |= g->mem.upload(rp_v, &gg.rp); rcg |= g->mem.upload(ci_v, &gg.ci);
    rcg |= g->mem.upload(cp, &gg.cp); rcg |= g->mem.upload(ri, &gg.ri);
    rcg |= g->mem.upload(c2r, &gg.c2r); rcg |= g->mem.upload(l0, &gg.llr0);
    gg.frec = nullptr; gg.erow = nullptr;
    if (h.max_cdeg <= 8 && nnz <= 65534) {
        std::vector<uint16_t> erow(nnz);
        for (int i = 0; i < m; ++i)
            for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) erow[e] = (uint16_t)i;
        rcg |= g->mem.upload(erow, &gg.erow);
        std::vector<uint16_t> frec((size_t)n * 16, (uint16_t)0xFFFF);
        for (int j = 0; j < n; ++j)
            for (int e = cp[j]; e < cp[j + 1]; ++e) {
                frec[(size_t)j * 16 + (e - cp[j])] = (uint16_t)c2r[e];
                frec[(size_t)j * 16 + 8 + (e - cp[j])] = (uint16_t)ri[e];
            }
        rcg |= g->mem.upload(frec, &gg.frec);
    }
    {
        gg.ell_w = (h.max_rdeg + 63) / 64 * 64;
        std::vector<int32_t> ell((size_t)m * gg.ell_w * 2, 0);
        for (int i = 0; i < m; ++i)
            for (int x = 0; x < gg.ell_w; ++x) {
                const int e = row_ptr[i] + x;
                const bool in = e < row_ptr[i + 1];
                ell[((size_t)i * gg.ell_w + x) * 2] = in ? col_idx[e] : -1;
                ell[((size_t)i * gg.ell_w + x) * 2 + 1] = in ? h.bit_slot_of[col_idx[e]] : 0;
            }
        rcg |= g->mem.upload(ell, &gg.ell);
    }
    // the records below pack the fault index into 24 bits of their first word (host_graph refuses larger windows long before)
    std::vector<int32_t> last(m, 0), lev(n, 0);
    int nlev = 0;
    for (int j = 0; j < n; ++j) {
        int l = 0;
        for (int e = cp[j]; e < cp[j + 1]; ++e) l = std::max(l, last[ri[e]]);
        lev[j] = l;                                     // 0-based
        for (int e = cp[j]; e < cp[j + 1]; ++e) last[ri[e]] = l + 1;
        nlev = std::max(nlev, l + 1);
    }
    std::vector<int32_t> lp(nlev + 1, 0), lb(n);
    for (int j = 0; j < n; ++j) lp[lev[j] + 1]++;
    for (int l = 0; l < nlev; ++l) lp[l + 1] += lp[l];
    std::vector<int32_t> fillp(lp.begin(), lp.end() - 1);
    for (int j = 0; j < n; ++j) lb[fillp[lev[j]]++] = j;
    // LDS slots of the rows' running prefixes (see GenGraphDev): a slot is handed on only to a row that starts strictly
    // after its previous owner's last level (two faults of one level touch their rows in any order)
    std::vector<int32_t> first(m, nlev), lastl(m, -1), slot(m, 0), order(m);
    for (int i = 0; i < m; ++i)
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            first[i] = std::min(first[i], lev[col_idx[e]]);
            lastl[i] = std::max(lastl[i], lev[col_idx[e]]);
        }
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return first[a] < first[b]; });
    std::vector<int32_t> busy_until;                // per slot: last level of its current owner
    for (int i : order) {
        int sidx = -1;
        for (size_t q = 0; q < busy_until.size(); ++q)
            if (busy_until[q] < first[i]) { sidx = (int)q; break; }
        if (sidx < 0) { sidx = (int)busy_until.size(); busy_until.push_back(-1); }
        busy_until[sidx] = lastl[i];
        slot[i] = sidx;
    }
    gg.nslots = ((int)busy_until.size() * 256 <= QD_GEN_PREFIX_LDS && m < (1 << 23)) ? (int)busy_until.size() : 0;
    // one record per (step, wavefront): see GenGraphDev
    const int G = QD_GEN_GS, D = qd_gen_unroll(h.max_cdeg);
    const int RW = (2 + 2 * D + 3) & ~3;
    size_t nstep = 0;
    for (int l = 0; l < nlev; ++l) nstep += (size_t)(lp[l + 1] - lp[l] + G - 1) / G;
    std::vector<uint32_t> srec(nstep * G * RW, 0u);
    size_t st = 0;
    for (int l = 0; l < nlev; ++l) {
        const int cnt = lp[l + 1] - lp[l], steps = (cnt + G - 1) / G;
        for (int q = 0; q < steps; ++q, ++st)
            for (int wv = 0; wv < G; ++wv) {
                uint32_t *r = &srec[(st * G + wv) * RW];
                const uint32_t bar = (q == steps - 1) ? 0x80000000u : 0u;
                const int x = q * G + wv;
                if (x >= cnt) { r[0] = bar; continue; }
                const int j = lb[lp[l] + x], c0 = cp[j], deg = cp[j + 1] - c0;
                r[0] = (uint32_t)j | ((uint32_t)deg << 24) | bar;
                std::memcpy(&r[1], &l0[j], 4);
                for (int k = 0; k < deg; ++k) {
                    const int i = ri[c0 + k];
                    r[2 + k] = (uint32_t)i;
                    if (gg.nslots > 0) r[2 + k] |= ((uint32_t)slot[i] << 24) | (col_idx[row_ptr[i]] == j ? 0x800000u : 0u);
                    r[2 + D + k] = (uint32_t)c2r[c0 + k];
                }
            }
    }
    gg.nlev = nlev; gg.nstep = (int)nstep; gg.srec_w = RW;
    rcg |= g->mem.upload(srec, &gg.srec);
    if (rcg) return fail(QD_EHIP, "device allocation failed while building the graph");
    return QD_OK;
}

// Scatter form of the flooding min-sum kernel (bp_scatter.hip, bp_scatter_wide.hip; ScatGraphDev): checks in lanes with their state in
// registers, the faults' integer posterior accumulators in LDS.  Taken (sc.ok) for the windows of scatter_form whose accumulators leave
// as many workgroups per CU as the gather kernel's layout does.
static int build_scatter(qd_graph *g, const HostGraph &h, int form, const Switches &env)
{
    ScatGraphDev &sc = g->sc;
    const BpGraphDev &bp = g->bp;
    sc = ScatGraphDev{};
    if (!form) return QD_OK;
    const int m = h.m, n = h.n, m_pad = h.m_pad;
    const int32_t *row_ptr = h.row_ptr, *col_idx = h.col_idx;
    // ---- the accumulators' own slot order: a bank for every fault (scatter_banks), then bank + 32 * (rank inside the bank)
    std::vector<int> sc_bank, sc_slot(n), fillb(32, 0);
    scatter_banks(m, n, row_ptr, col_idx, h.chk_orig, h.bit_slot_of, env.scatter_banks_by_slot, sc_bank);
    for (int j = 0; j < n; ++j) sc_slot[j] = sc_bank[j] + 32 * fillb[sc_bank[j]]++;
    const int sc_trash = 32 * *std::max_element(fillb.begin(), fillb.end());    // 32 trash slots, one per bank, behind the accumulators
    sc.nslots = sc_trash + 32;
    const int buf = align16(sc.nslots * 4);
    sc.offA = 0; sc.offB = 0; sc.off_out = buf;            // one buffer: the scatter pass works in place
    sc.off_bmap = sc.off_out + align16(bp.out_words * 4);
    sc.off_misc = sc.off_bmap;
    sc.lds_bytes = sc.off_misc + 256;
    const int res_old = std::min(2048 / bp.threads, QD_LDS_BYTES / std::max(1, bp.lds_bytes));
    // the shape that will really be launched (the residency test used to look at a shape that never ran): several
    // checks per lane -- see below for the measurements behind each case
    int shape_threads = bp.threads, shape_cpl = 1;
    if (form == 2) {
        shape_threads = scatter_wide_threads(m); shape_cpl = 2;
        if (m <= 1536 && !env.scatter_wide_t704) { shape_threads = 512; shape_cpl = 3; }    // 19.8 -> 19.3 ms per QLP launch
    } else if (!env.scatter_cpl1) {
        if (bp.threads == 1024 && 4 * sc.lds_bytes <= QD_LDS_BYTES) { shape_threads = 512; shape_cpl = 2; }
        else if (bp.threads == 512 && 8 * sc.lds_bytes <= QD_LDS_BYTES) { shape_threads = 256; shape_cpl = 2; }
        else if (bp.threads == 256 && 16 * sc.lds_bytes <= QD_LDS_BYTES) { shape_threads = 128; shape_cpl = 2; }    // (<= 256 checks)
    }
    const int res_new = std::min(2048 / shape_threads, QD_LDS_BYTES / sc.lds_bytes);
    if (res_new < res_old) { sc = ScatGraphDev{}; return QD_OK; }      // (res_old >= 1: build_bp checked the gather kernel's LDS)
    const int rows = h.max_rdeg_pad / 4 + 2;          // two spare group rows: the kernel loads up to two groups ahead unconditionally
    // every entry starts at the trash slot of bank (lane mod 32): the steps nobody reaches and the two spare rows
    std::vector<uint32_t> adjA((size_t)rows * m_pad * 4);
    for (int r = 0; r < rows; ++r)
        for (int s = 0; s < m_pad; ++s)
            for (int q = 0; q < 4; ++q) adjA[((size_t)r * m_pad + s) * 4 + q] = (uint32_t)sc.offA + (uint32_t)(sc_trash + (s & 31)) * 4u;
    long long walk_cyc = 0, walk_ideal = 0;
    std::vector<uint8_t> edge_step((size_t)h.nnz, 0xFF);
    bool walk_ok = true;
    scatter_walk(m, row_ptr, col_idx, h.chk_orig, sc_bank, env.scatter_walk_greedy, [&](int s, int k, int e, int trash_bank) {
        const uint32_t slot = e >= 0 ? (uint32_t)sc_slot[col_idx[e]] : (uint32_t)(sc_trash + trash_bank);
        if (k < 0 || k >= rows * 4 || s < 0 || s >= m_pad) { walk_ok = false; return; }
        if (e >= 0) {                                      // a real edge: once, at a step below its check's degree
            const int i = s < m ? h.chk_orig[s] : -1;
            if (i < 0 || e < row_ptr[i] || e >= row_ptr[i + 1] || k >= h.rdeg[i] || edge_step[e] != 0xFF) { walk_ok = false; return; }
            edge_step[e] = (uint8_t)k;
        }
        adjA[((size_t)(k >> 2) * m_pad + s) * 4 + (k & 3)] = (uint32_t)sc.offA + slot * 4u;
    }, &walk_cyc, &walk_ideal);
    for (int i = 0; i < m && walk_ok; ++i) {               // every step below the degree taken exactly once
        uint64_t seen_lo = 0, seen_hi = 0;
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const int k = edge_step[e];
            if (k == 0xFF) { walk_ok = false; break; }
            uint64_t &w = k < 64 ? seen_lo : seen_hi;
            if ((w >> (k & 63)) & 1u) { walk_ok = false; break; }
            w |= 1ull << (k & 63);
        }
    }
    if (!walk_ok) return fail(QD_ECAPACITY, "scatter walk: an edge was not placed exactly once below its check's degree");
    g->sc_walk_cycles = walk_cyc; g->sc_walk_ideal = walk_ideal;
    std::vector<uint32_t> slot_fault((size_t)sc.nslots, 0xFFFFFFFFu), k1_slot((size_t)n, 0u);
    for (int j = 0; j < n; ++j) { slot_fault[sc_slot[j]] = (uint32_t)j; k1_slot[h.bit_slot_of[j]] = (uint32_t)sc_slot[j]; }
    g->h_sc_slot.assign(sc_slot.begin(), sc_slot.end());
    std::vector<uint32_t> deg_w(m_pad / 64, 0u);
    for (int w0 = 0; w0 < m; w0 += 64) {
        int mx = 0, mn = 255;
        for (int s = w0; s < std::min(m, w0 + 64); ++s) { mx = std::max(mx, (int)h.chk_deg[s]); mn = std::min(mn, (int)h.chk_deg[s]); }
        deg_w[w0 / 64] = (uint32_t)((mx + 3) & ~3) | ((uint32_t)mx << 8) | ((uint32_t)mn << 16);
    }
    int rcs = 0;
    rcs |= g->mem.upload(adjA, &sc.adjA); sc.adjB = sc.adjA;
    rcs |= g->mem.upload(slot_fault, &sc.slot_fault); rcs |= g->mem.upload(k1_slot, &sc.k1_slot);
    rcs |= g->mem.upload(deg_w, &sc.deg_w); rcs |= g->mem.upload(h.chk_deg, &sc.chk_deg);
    if (rcs) return fail(QD_EHIP, "device allocation failed while uploading the scatter adjacency");
    sc.ok = 1;
    // Several checks per lane (bp_scatter_wide.hip).  (a) windows the one-check-per-lane kernel cannot take: three checks per
    // lane on 512 lanes (or two on 704 / 1024).  (b) windows it can take, on HALF the lanes with two checks each: the same number
    // of wavefronts per CU in twice as many workgroups, i.e. half as many wavefronts per barrier -- headline BP 50.3 -> 44.2 ms per
    // 65 536 shots, same bits (profiles/r03x_scatter_cpl2_ab.txt); taken when the LDS holds twice the workgroups.
    // QD_SCATTER_CPL1=1 keeps one check per lane.  Measured and not kept (profiles/r03x_scatter_shapes2_ab.txt): four checks per
    // lane on a quarter of the lanes (headline 46.2 -> 50.9 ms), 384 lanes x 4 checks for the QLP windows (19.2 -> 24.4 ms).
    sc.wide_threads = shape_cpl > 1 ? shape_threads : 0; sc.wide_cpl = shape_cpl > 1 ? shape_cpl : 0;
    if (!sc.wide_threads) return QD_OK;
    // deal the slot-waves (64 consecutive check slots, heaviest first) to the workgroup's wavefronts so that the largest
    // number of edges a wavefront walks between two barriers is small: each goes to the wavefront with the fewest edges so
    // far that still has a free round (longest-processing-time rule), then single moves / swaps out of the heaviest
    // wavefront while they lower the maximum (QLP windows on 8 wavefronts x 3 rounds: 222 -> 202 edge steps)
    const int nw = sc.wide_threads / 64, nsw = m_pad / 64, cpl = sc.wide_cpl;
    const bool natural = env.scatter_natural_rounds;                   // round j of wavefront w = slot-wave j * nw + w
    auto cost = [&](int sw) { return (int)(deg_w[sw] & 0xFF) + 6; };   // trip count + the per-check work outside the edge loops
    std::vector<std::vector<int>> bins(nw);
    std::vector<int> load(nw, 0);
    for (int sw = 0; sw < nsw; ++sw) {
        int best = -1;
        if (natural) best = sw % nw;
        else
            for (int w = 0; w < nw; ++w)
                if ((int)bins[w].size() < cpl && (best < 0 || load[w] < load[best])) best = w;
        if (best < 0 || (int)bins[best].size() >= cpl) return fail(QD_ECAPACITY, "scatter kernel shape does not cover the window");
        bins[best].push_back(sw); load[best] += cost(sw);
    }
    for (int pass = 0; pass < 1000 && !natural; ++pass) {
        const int hi = (int)(std::max_element(load.begin(), load.end()) - load.begin()), Lh = load[hi];
        int gain = 0, bi = -1, bw = -1, bk = -1;
        for (int i = 0; i < (int)bins[hi].size(); ++i) {
            const int x = cost(bins[hi][i]);
            for (int w = 0; w < nw; ++w) {
                if (w == hi) continue;
                if ((int)bins[w].size() < cpl) {
                    const int nl = std::max(Lh - x, load[w] + x);
                    if (Lh - nl > gain) { gain = Lh - nl; bi = i; bw = w; bk = -1; }
                }
                for (int k = 0; k < (int)bins[w].size(); ++k) {
                    const int y = cost(bins[w][k]);
                    if (y >= x) continue;
                    const int nl = std::max(Lh - x + y, load[w] - y + x);
                    if (Lh - nl > gain) { gain = Lh - nl; bi = i; bw = w; bk = k; }
                }
            }
        }
        if (bi < 0) break;
        const int x = cost(bins[hi][bi]);
        if (bk < 0) { bins[bw].push_back(bins[hi][bi]); bins[hi].erase(bins[hi].begin() + bi); load[hi] -= x; load[bw] += x; }
        else { const int y = cost(bins[bw][bk]); std::swap(bins[hi][bi], bins[bw][bk]); load[hi] += y - x; load[bw] += x - y; }
    }
    std::vector<int32_t> wmap((size_t)cpl * nw, -1);
    for (int w = 0; w < nw; ++w)
        for (int j = 0; j < (int)bins[w].size(); ++j) wmap[(size_t)j * nw + w] = bins[w][j];
    if (g->mem.upload(wmap, &sc.wave_map)) return fail(QD_EHIP, "device allocation failed while uploading the scatter wave map");
    return QD_OK;
}

// The elimination kernels' view (OsdGraphDev): fault weights, CSC, the LDS layouts of the OSD kernels and the SR kernel's ELL columns
static int build_osd(qd_graph *g, const HostGraph &h)
{
    const int m = h.m, n = h.n, m_pad = h.m_pad, max_cdeg = h.max_cdeg, out_words = g->bp.out_words;
    OsdGraphDev &od = g->osd;
    std::vector<uint32_t> wfix((size_t)n);
    for (int j = 0; j < n; ++j) {
        double w = std::log(1.0 / h.priors[j]) * 262144.0;
        wfix[j] = (uint32_t)std::llround(std::min(std::max(w, 0.0), 4294967295.0));
        od.max_wfix = std::max(od.max_wfix, wfix[j]);
    }
    od.m = m; od.n = n; od.m_pad = m_pad; od.max_cdeg = max_cdeg; od.mw = (m + 63) / 64;
    int np2 = 64;
    while (np2 < n) np2 <<= 1;
    od.npow2 = np2;
    std::vector<uint32_t> csc_ptr(h.cp.begin(), h.cp.end());
    std::vector<uint16_t> csc_row(h.ri.begin(), h.ri.end());
    int rc = 0;
    rc |= g->mem.upload(wfix, &od.wfix);
    rc |= g->mem.upload(csc_ptr, &od.csc_ptr);
    rc |= g->mem.upload(csc_row, &od.csc_row);
    if (rc) return fail(QD_EHIP, "device allocation/upload failed");
    auto carve = [&](int *offs, int qbytes, int base) {
        int o = base;
        offs[0] = o; o += align16(qbytes);
        offs[1] = o; o += align16(m_pad * 8);          // tb
        offs[2] = o; o += align16(m_pad);              // sp
        offs[3] = o; o += align16(m_pad * 2);          // rowpiv
        offs[4] = o; o += align16(m_pad * 2);          // prow
        offs[5] = o; o += align16(m_pad * 4);          // pcol
        offs[6] = o; o += align16(64 * max_cdeg * 4);  // pairs
        offs[7] = o; o += 256;                         // cols
        offs[8] = o; o += 1024;                        // red: 96 words of pivot/flag/counter scratch + 2 x 64 words of block sums
        offs[9] = o; o += align16(out_words * 4);      // out
        return o;
    };
    int tmp[10];
    const int small = carve(tmp, 0, 0);
    const int q_budget = QD_LDS_BYTES - small - 64;
    const int sort_bytes = np2 * 8;
    od.threads = m <= 256 ? 256 : (m <= 512 ? 512 : 1024);
    od.f_threads = m <= 256 ? 256 : 512;       // (256 threads with 4 rows each measured slower at m = 1008: 20.4 vs 16.3 ms)
    od.lds_bytes = 0; od.kw_lds = 0; od.f_lds_bytes = 0; od.f_kw = 0;
    if (sort_bytes <= q_budget) {
        od.kw_lds = std::min(od.mw, q_budget / (m_pad * 8));
        od.lds_bytes = carve(od.off, std::max(sort_bytes, od.kw_lds * m_pad * 8), 0);
    }
    {
        // register kernel: aim at two workgroups per CU, settle for one; the tier sort buffer and the order live beside the
        // Q mirror, which must hold the kernel's 6 register planes (or all mw planes of a small window)
        const int tier = 1024;
        const int sort_b = tier * 8, order_b = align16(tier * 2);
        od.f_lds_bytes = 0; od.w_lds_bytes = 0;
        // `sweep`: higher-order OSD also keeps a pivot-column bit mask and the list of the first non-pivot columns
        auto lay = [&](int per_cu, bool sweep, int *offs, int &o_sort, int &o_order, int &o_piv, int &o_npl, int &kw) -> int {
            const int extra = sweep ? align16(out_words * 4) + 256 : 0;
            const int f_budget = QD_LDS_BYTES / per_cu - 256 - small - sort_b - order_b - extra;
            kw = std::min(od.mw, std::max(0, f_budget / (m_pad * 8)));
            const int min_planes = sweep ? 6 : 2;          // the Q mirror holds at least the planes the kernel keeps in registers (QD_OSD_KWR / QD_OSD_KWR0)
            if (kw < std::min(min_planes, od.mw) || (m + od.f_threads - 1) / od.f_threads > 4) return 0;
            int o = carve(offs, kw * m_pad * 8, 0);
            o_sort = o; o += sort_b;
            o_order = o; o += order_b;
            o_piv = o; o_npl = o;                       // unused by OSD-0
            if (sweep) { o_piv = o; o += align16(out_words * 4); o_npl = o; o += 256; }
            return o <= QD_LDS_BYTES / per_cu ? o : 0;
        };
        od.f_off_hist = 0;
        // OSD-0: the layout for two workgroups per CU where the window allows it, else for one (the register budget of
        // qd_osd0_reg_kernel<512, ., false> admits two per CU, no more)
        for (int per_cu = 2; per_cu >= 1 && od.f_lds_bytes == 0; --per_cu)
            od.f_lds_bytes = lay(per_cu, false, od.f_off, od.f_off_sort, od.f_off_order, od.f_off_pivmask, od.f_off_npl, od.f_kw);
        od.w_lds_bytes = lay(1, true, od.w_off, od.w_off_sort, od.w_off_order, od.w_off_pivmask, od.w_off_npl, od.w_kw);
    }
    // OSD-0 with simultaneous singleton pivots (osd_sr.hip): columns in ELL form (one load per entry, no pointer chase), its own
    // LDS layout; taken whenever the mirrored register kernel exists too (it decodes the shots the new kernel hands over)
    od.s_lds_bytes = 0; od.s_per_cu = 0; od.csc_ell = nullptr; od.ell_log2 = 0;
    if (od.f_lds_bytes > 0 && m < 65535) {
        int dl = 1;
        while ((1 << dl) < max_cdeg) ++dl;
        std::vector<uint16_t> ell((size_t)n << dl, (uint16_t)0xFFFFu);
        for (int j = 0; j < n; ++j)
            for (int e = h.cp[j]; e < h.cp[j + 1]; ++e) ell[((size_t)j << dl) + (e - h.cp[j])] = (uint16_t)h.ri[e];
        if (g->mem.upload(ell, &od.csc_ell)) return fail(QD_EHIP, "device allocation/upload failed");
        od.ell_log2 = dl;
        const int lds = qd_osd_sr_layout(m, m_pad, n, out_words, od.s_off, &od.s_threads, &od.s_rpt);
        if (lds > 0 && lds <= QD_LDS_BYTES) {
            od.s_lds_bytes = lds;
            od.s_per_cu = std::max(1, std::min(QD_LDS_BYTES / lds, qd_sr_wps(od.s_rpt) * 256 / od.s_threads));   // the kernel's register budget (wavefronts per SIMD)
        }
    }
    // the full kernel sorts all n columns in LDS; windows too large for that rely on the register kernel alone
    if (od.lds_bytes == 0 && od.f_lds_bytes == 0) od.threads = 0;
    g->x_lds = qd_osd_offchip_layout(m, n, max_cdeg, g->x_off, &g->x_off_sort, &g->x_off_order, &g->x_kw, &g->x_threads, &g->x_per_cu);
    return QD_OK;
}

extern "C" int qd_graph_create(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                               const double *priors, int32_t device, qd_graph **out)
{
    if (!out) return fail(QD_EINVAL, "out is null");
    *out = nullptr;
    HostGraph h;
    if (int rc = host_graph(m, n, row_ptr, col_idx, priors, h)) return rc;
    std::unique_ptr<qd_graph> g(new qd_graph());      // (~qd_graph frees what the builders uploaded)
    g->device = device; g->m = m; g->n = n; g->nnz = h.nnz; g->max_rdeg = h.max_rdeg; g->max_cdeg = h.max_cdeg;
    if (hipSetDevice(device) != hipSuccess) return fail(QD_EHIP, "hipSetDevice(%d) failed", device);
    const Switches env = read_switches();
    const int form = scatter_form(h);
    if (int rc = build_bp(g.get(), h, form != 0)) return rc;
    if (int rc = build_gen(g.get(), h)) return rc;
    if (int rc = build_scatter(g.get(), h, g->off_chip ? 0 : form, env)) return rc;
    if (int rc = build_osd(g.get(), h)) return rc;
    g->h_cp = h.cp; g->h_ri = h.ri; g->h_llr0 = h.llr0;
    *out = g.release();
    return QD_OK;
}

extern "C" void qd_graph_destroy(qd_graph *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    delete g;
}

static int host_rank(qd_graph *g)
{
    if (g->rank >= 0) return g->rank;
    const int m = g->m, n = g->n, mw = (m + 63) / 64;
    // column-incremental elimination on m-bit columns
    std::vector<std::vector<uint64_t>> basis;   // reduced columns with distinct leading rows
    std::vector<int> lead_of(m, -1);
    int rank = 0;
    std::vector<uint64_t> v(mw);
    for (int j = 0; j < n && rank < m; ++j) {
        std::fill(v.begin(), v.end(), 0ull);
        for (int e = g->h_cp[j]; e < g->h_cp[j + 1]; ++e) v[g->h_ri[e] >> 6] ^= 1ull << (g->h_ri[e] & 63);
        for (;;) {
            int lead = -1;
            for (int w = 0; w < mw; ++w)
                if (v[w]) { lead = w * 64 + __builtin_ctzll(v[w]); break; }
            if (lead < 0) break;
            if (lead_of[lead] < 0) { lead_of[lead] = (int)basis.size(); basis.push_back(v); ++rank; break; }
            const std::vector<uint64_t> &b = basis[lead_of[lead]];
            for (int w = 0; w < mw; ++w) v[w] ^= b[w];
        }
    }
    g->rank = rank;
    return rank;
}

// qd_graph_info fills exactly 10 entries, as it did in library version 100 (version 101 wrote 12 into the caller's buffer, an
// 8-byte overwrite for a C caller compiled against the older header); whoever wants more says how many it has room for.
static void graph_info_fill(const qd_graph *g, int32_t *info, int n_entries)
{
    // [12], [13]: lanes and checks per lane of qd_bp_scatter_wide_kernel's instantiation for this window (0: the window does not take that kernel)
    const int32_t v[14] = {g->m, g->n, g->nnz, g->max_rdeg, g->max_cdeg, g->bp.threads, g->bp.lds_bytes, g->osd.threads, g->osd.lds_bytes,
                           n_entries > 9 ? host_rank(const_cast<qd_graph *>(g)) : 0, (int32_t)g->sc_walk_cycles, (int32_t)g->sc_walk_ideal,
                           g->sc.wide_threads, g->sc.wide_cpl};
    for (int i = 0; i < n_entries && i < 14; ++i) info[i] = v[i];
    for (int i = 14; i < n_entries; ++i) info[i] = 0;
}

extern "C" int qd_graph_info(const qd_graph *g, int32_t *info)
{
    if (!g || !info) return fail(QD_EINVAL, "null argument");
    graph_info_fill(g, info, 10);
    return QD_OK;
}

extern "C" int qd_graph_info_ex(const qd_graph *g, int32_t *info, int32_t n_entries)
{
    if (!g || !info || n_entries < 0) return fail(QD_EINVAL, "null argument or negative n_entries");
    graph_info_fill(g, info, n_entries);
    return QD_OK;
}

extern "C" int qd_decoder_create(const qd_graph *g, const qd_params *p, qd_decoder **out)
{
    if (!g || !p || !out) return fail(QD_EINVAL, "null argument");
    *out = nullptr;
    if (p->bp_method != QD_BP_MINIMUM_SUM && p->bp_method != QD_BP_PRODUCT_SUM) return fail(QD_EINVAL, "unknown bp_method %d", p->bp_method);
    if (p->schedule != QD_SCHEDULE_PARALLEL && p->schedule != QD_SCHEDULE_SERIAL) return fail(QD_EINVAL, "unknown schedule %d", p->schedule);
    if (p->reserved & ~(QD_FLAG_EDGE_MESSAGES | QD_FLAG_RAW_LLR | QD_FLAG_OFF_CHIP)) return fail(QD_EINVAL, "unknown flag bits 0x%x", p->reserved);
    const bool lsd = p->osd_method == QD_LSD_0 || p->osd_method == QD_LSD_E || p->osd_method == QD_LSD_CS;
    if (lsd && p->osd_order < 0) return fail(QD_EINVAL, "negative lsd_order");
    const bool off_chip = g->off_chip || (p->reserved & QD_FLAG_OFF_CHIP);
    if (off_chip && lsd)
        return fail(QD_EUNSUPPORTED, "BP-LSD is not implemented for the off-chip window %d x %d%s", g->m, g->n, g->off_chip ? "" : " (QD_FLAG_OFF_CHIP)");
    if (p->osd_method == QD_LSD_CS && p->osd_order > 64)
        return fail(QD_EUNSUPPORTED, "lsd_cs: lsd_order %d > 64 is not implemented on the device path", p->osd_order);
    if (p->osd_method == QD_LSD_E && p->osd_order > 15)
        return fail(QD_EUNSUPPORTED, "lsd_e: lsd_order %d > 15 is not implemented on the device path", p->osd_order);
    if (lsd && qd_lsd_lds_bytes(g->m, g->n, g->bp.out_words) > QD_LDS_BYTES)
        return fail(QD_ECAPACITY, "window %d x %d does not fit the LSD kernel's LDS layout", g->m, g->n);
    const bool osd0 = lsd || p->osd_method == QD_OSD_0 || ((p->osd_method == QD_OSD_CS || p->osd_method == QD_OSD_E) && p->osd_order == 0);
    if (p->osd_method != QD_OSD_OFF && !osd0) {
        if (p->osd_method != QD_OSD_CS && p->osd_method != QD_OSD_E) return fail(QD_EINVAL, "unknown osd_method %d", p->osd_method);
        if (p->osd_order < 0) return fail(QD_EINVAL, "negative osd_order");
        if (off_chip)
            return fail(QD_EUNSUPPORTED, "osd_cs / osd_e of order %d are not implemented for the off-chip window %d x %d%s (order 0 is)", p->osd_order, g->m,
                        g->n, g->off_chip ? "" : " (QD_FLAG_OFF_CHIP)");
        if (g->osd.w_lds_bytes == 0)
            return fail(QD_EUNSUPPORTED, "osd_cs / osd_e need the register OSD kernel, which this window (%d detectors) does not fit", g->m);
        if (p->osd_method == QD_OSD_CS && p->osd_order > 64)
            return fail(QD_EUNSUPPORTED, "osd_cs: osd_order %d > 64 is not implemented on the device path", p->osd_order);
        if (p->osd_method == QD_OSD_E && p->osd_order > 15)
            return fail(QD_EUNSUPPORTED, "osd_e: osd_order %d > 15 is not implemented on the device path", p->osd_order);
    }
    if (p->osd_method != QD_OSD_OFF && off_chip && g->x_lds == 0)
        return fail(QD_ECAPACITY, "off-chip window %d x %d: the row state of the OSD-0 kernel (17 bytes per detector) does not fit the CU's LDS", g->m, g->n);
    if (p->osd_method != QD_OSD_OFF && !lsd && !off_chip && g->osd.lds_bytes == 0 && g->osd.f_lds_bytes == 0)
        return fail(QD_ECAPACITY, "window %d x %d does not fit either OSD kernel's LDS layout", g->m, g->n);
    if (p->max_iter < 0 || p->ms_scaling_factor < 0) return fail(QD_EINVAL, "negative max_iter / ms_scaling_factor");
    const Switches env = read_switches();
    qd_decoder *d = new qd_decoder();
    d->g = g; d->prm = *p; d->off_chip = off_chip;
    d->lsd_w = (lsd && p->osd_order > 0) ? (p->osd_method == QD_LSD_CS ? 1 : (p->osd_method == QD_LSD_E ? 2 : 0)) : 0;
    d->osd_w = osd0 || p->osd_method == QD_OSD_OFF ? 0 : (p->osd_method == QD_OSD_CS ? 1 : 2);
    if (d->osd_w) host_rank(const_cast<qd_graph *>(g));     // the sweep needs the complete factorisation: rank pivots
    if (d->prm.max_iter == 0) d->prm.max_iter = g->n;       // ldpc: max_iter = 0 -> number of bits
    if (d->prm.max_iter > QD_STATUS_ITER_MASK) d->prm.max_iter = QD_STATUS_ITER_MASK;
    // ---- the post-processor
    if (p->osd_method == QD_OSD_OFF) d->post = QD_POST_NONE;
    else if (off_chip) d->post = QD_POST_OSD0_OFFCHIP;
    else if (lsd) d->post = QD_POST_LSD;
    else if (d->osd_w) {
        // higher-order OSD: the panel kernel (osd_cs.hip) wherever its layout takes the window, else the row form (osd_kernels.hip)
        if (g->osd.csc_ell && !env.osdcs_old)
            d->cs_lds = qd_osdcs_layout(g->m, g->n, g->bp.out_words, g->osd.max_wfix, d->cs_off, &d->cs_variant, &d->cs_per_cu);
        d->post = d->cs_lds > 0 ? QD_POST_OSD_CS_PANEL : QD_POST_OSD_W_OLD;
    } else
        d->post = g->osd.s_lds_bytes > 0 ? QD_POST_OSD0_SR : QD_POST_OSD0_REG;
    // ---- the BP kernel: one message per edge for every method / schedule but flooding min-sum (and for that one with QD_FLAG_EDGE_MESSAGES),
    // the gather kernel for it off the LLR grid, the gather or a scatter kernel on the grid (below)
    const bool edge = off_chip || p->bp_method != QD_BP_MINIMUM_SUM || p->schedule != QD_SCHEDULE_PARALLEL || (p->reserved & QD_FLAG_EDGE_MESSAGES);
    if (edge)
        d->bp = (!off_chip && p->bp_method == QD_BP_PRODUCT_SUM && p->schedule == QD_SCHEDULE_PARALLEL && qd_bp_ps_lds_bytes(g->gen, g->max_rdeg) > 0) ? BP_LDS_EDGE : BP_HBM_EDGE;
    if (d->bp == BP_HBM_EDGE && p->schedule == QD_SCHEDULE_SERIAL) {
        // the serial schedule in several launches with the survivors packed in between (GenStage), at the bounds that leave two iterations or more
        int prev = 0;
        for (int b : env.gen_stages)
            if (b > prev && b + 2 <= d->prm.max_iter && d->gen_nbounds < QD_GEN_MAX_STAGES - 1) { d->gen_bounds[d->gen_nbounds++] = b; prev = b; }
    }
    d->bp_fine = g->bp; d->bp_coarse = g->bp; d->llr0_q = g->gen.llr0;
    if (p->bp_method == QD_BP_MINIMUM_SUM && p->schedule == QD_SCHEDULE_PARALLEL && p->ms_scaling_factor == 1.0 &&
        !(p->reserved & QD_FLAG_RAW_LLR)) {
        // Channel LLRs on a binary grid: see qd_decoder_info in quits_amd.h.  (oracle/qd_oracle.c restates this rule.)
        double mx = 0.0;
        for (double l : g->h_llr0) mx = std::max(mx, std::fabs(l));
        const double need = 8.0 * mx * (double)std::max(1, d->prm.max_iter);
        int e = 0;
        while (std::ldexp(1.0, e) < need && e < 40) ++e;
        // fine grid: never coarser than 2^-10, whatever max_iter (a large max_iter -- ldpc's max_iter = 0 means n -- would otherwise
        // put every shot on a grid of 1/4 or 1/8 although most shots converge long before their magnitudes get anywhere near the
        // bound); the shots that do outgrow it are certified on the grid the rule gives, by the redo pass
        const int kr = std::min(20, std::max(2, 23 - e));
        d->grid_k = std::max(kr, QD_GRID_MIN_BITS);
        d->grid_kc = kr >= QD_GRID_MIN_BITS ? std::max(0, kr - 4) : kr;
        d->grid_floor = kr < QD_GRID_MIN_BITS ? 1 : 0;
        if (hipSetDevice(g->device) != hipSuccess) { delete d; return fail(QD_EHIP, "hipSetDevice(%d) failed", g->device); }
        // (+ 0.0f: a prior that rounds to zero from below must be +0, not -0 -- the kernel's sign test reads the bit pattern)
        auto on_grid = [&](double l, int k) { return (float)std::ldexp(std::nearbyint(std::ldexp(l, k)), -k) + 0.0f; };
        int rc = 0;
        for (int pass = 0; pass < 2 && !off_chip; ++pass) {
            const int k = pass == 0 ? d->grid_k : d->grid_kc;
            std::vector<uint32_t> rec = g->h_bit_rec;
            for (int s = 0; s < g->n; ++s) {
                const float l0 = on_grid(g->h_llr0[g->h_bit_orig[s]], k);
                std::memcpy(&rec[(size_t)s * 4], &l0, 4);                  // word 0 of chunk 0: [chunk][slot][4]
            }
            rc |= d->mem.upload(rec, pass == 0 ? &d->bp_fine.bit_rec : &d->bp_coarse.bit_rec);
        }
        std::vector<float> lq(g->n);
        for (int j = 0; j < g->n; ++j) lq[j] = on_grid(g->h_llr0[j], d->grid_k);
        rc |= d->mem.upload(lq, &d->llr0_q);
        if (off_chip) {
            for (int j = 0; j < g->n; ++j) lq[j] = on_grid(g->h_llr0[j], d->grid_kc);
            rc |= d->mem.upload(lq, &d->llr0_qc);
            d->edge_cert = true;
        }
        if (!edge) d->bp = BP_GATHER_GRID;
        if (!edge && g->sc.ok && !env.no_scatter) {
            // scatter kernel: fine-grid priors of the bit slots as integers (grid units) and the second-minimum bound that
            // certifies a run (bp_scatter.hip): max|prior| + max_cdeg * max min2 < 2^23
            std::vector<int32_t> pg((size_t)g->sc.nslots, 0);      // (unused and trash slots: 0)
            long long mxp = 0;
            for (int j = 0; j < g->n; ++j) {
                const long long v = std::llround(std::ldexp((double)on_grid(g->h_llr0[j], d->grid_k), d->grid_k));
                pg[g->h_sc_slot[j]] = (int32_t)v - 1;              // an accumulator holds L - 1: (L <= 0) is its sign bit
                mxp = std::max(mxp, std::llabs(v));
            }
            const long long lim = ((1ll << 23) - mxp) / std::max(1, g->max_cdeg) - 1;
            if (mxp < (1ll << 22) && lim > 0) {
                rc |= d->mem.upload(pg, &d->prior_g);
                d->m2_limit = std::min((float)lim, env.scatter_m2_limit);     // (QD_SCATTER_M2_LIMIT: tests force the recheck pass)
                d->bp = g->sc.wide_threads ? BP_SCATTER_WIDE : BP_SCATTER;
                if (d->bp == BP_SCATTER_WIDE && !env.bp_no_fast_start && rc == 0) {
                    // gather pass 0 does not depend on the shot: made here once, on the device, by the kernel's own walk (bp_scatter_wide.hip)
                    const std::vector<uint32_t> zero((size_t)g->bp.m_pad * 8, 0u);
                    rc |= d->mem.upload(zero, &d->first_pass);
                    if (rc == 0 && (qd_launch_bp_first_pass(d->bp_fine, g->sc, d->prior_g, const_cast<uint32_t *>(d->first_pass), nullptr) != hipSuccess ||
                                    hipStreamSynchronize(nullptr) != hipSuccess))
                        rc = -1;
                }
            }
        }
        if (rc) { d->mem.release(); delete d; return fail(QD_EHIP, "device allocation failed while building the LLR grid"); }
    }
    *out = d;
    return QD_OK;
}

extern "C" int qd_decoder_info(const qd_decoder *d, int32_t *info)
{
    if (!d || !info) return fail(QD_EINVAL, "null argument");
    info[0] = d->grid_k; info[1] = d->grid_kc; info[2] = d->bp == BP_LDS_EDGE || d->bp == BP_HBM_EDGE;
    info[3] = d->bp == BP_SCATTER_WIDE ? 2 : (d->bp == BP_SCATTER ? 1 : 0);
    return QD_OK;
}

extern "C" int qd_decoder_fast_start(const qd_decoder *d) { return d ? (d->first_pass != nullptr && d->prm.max_iter >= 1) : -1; }

extern "C" int qd_decoder_postproc_kernel(const qd_decoder *d) { return d ? d->post : -1; }

static void free_ws(qd_decoder *d)
{
    auto dev = [](auto *&p) { if (p) (void)hipFree(p); p = nullptr; };
    auto host = [](auto *&p) { if (p) (void)hipHostFree(p); p = nullptr; };
    auto event = [](hipEvent_t &e) { if (e) (void)hipEventDestroy(e); e = nullptr; };
    dev(d->llr_ws); dev(d->fail_list); dev(d->ctr_base); dev(d->order_ws); dev(d->q_spill); dev(d->q_spill_fast); dev(d->q_spill_sr); dev(d->q_spill_off);
    dev(d->mt_ws); dev(d->cs_ws); dev(d->hard_list); dev(d->hard_list2); dev(d->redo_list); dev(d->recheck_list); dev(d->lsd_ws);
    dev(d->gws.b2c); dev(d->gws.c2b); dev(d->gws.th); dev(d->gws.pre); dev(d->gws.llr); dev(d->gws.syn); dev(d->gws.slot);
    dev(d->gsp.msg2); dev(d->gsp.syn2); dev(d->gsp.lists[0]); dev(d->gsp.lists[1]); dev(d->gsp.counts);
    host(d->host_fail); host(d->gsp.host_counts);
    event(d->fail_ready); event(d->gsp.counts_ready);
    d->gws = GenWs{}; d->gsp = GenStagePlan{};
    d->fail_count = nullptr; d->fail_pending = false;
    d->post_blocks = d->redo_cap = d->recheck_cap = 0; d->cap = 0;
}

extern "C" void qd_decoder_destroy(qd_decoder *d)
{
    if (!d) return;
    (void)hipSetDevice(d->g->device);
    free_ws(d);
    d->mem.release();
    for (auto &sp : d->ev) { (void)hipEventDestroy(sp.t0); (void)hipEventDestroy(sp.t1); }
    delete d;
}

extern "C" int qd_decoder_reserve(qd_decoder *d, int64_t max_batch)
{
    if (!d || max_batch <= 0) return fail(QD_EINVAL, "bad reserve request");
    if (max_batch <= d->cap) return QD_OK;
    HIP_TRY(hipSetDevice(d->g->device));
    HIP_TRY(hipDeviceSynchronize());
    free_ws(d);
    const qd_graph *g = d->g;
    HIP_TRY(hipMalloc((void **)&d->ctr_base, 512));
    HIP_TRY(hipMemset(d->ctr_base, 0, 512));
    d->fail_count = d->ctr_base; d->cset = 0; d->set_clean[0] = d->set_clean[1] = false;     // (see qd_decoder::ctr_base)
    HIP_TRY(hipHostMalloc((void **)&d->host_fail, 2 * sizeof(int32_t)));
    HIP_TRY(hipEventCreateWithFlags(&d->fail_ready, hipEventDisableTiming));
    if (d->bp == BP_SCATTER_WIDE || d->bp == BP_SCATTER || d->bp == BP_GATHER_GRID) {
        d->redo_cap = (int)(d->grid_floor ? max_batch : std::min<int64_t>(max_batch, 4096));
        HIP_TRY(hipMalloc((void **)&d->redo_list, sizeof(int32_t) * (size_t)d->redo_cap));
        if (d->bp != BP_GATHER_GRID) {
            d->recheck_cap = (int)max_batch;
            HIP_TRY(hipMalloc((void **)&d->recheck_list, sizeof(int32_t) * (size_t)d->recheck_cap));
        }
    } else if (d->edge_cert) {
        d->redo_cap = (int)(d->grid_floor ? max_batch : std::min<int64_t>(max_batch, 4096));
        HIP_TRY(hipMalloc((void **)&d->redo_list, sizeof(int32_t) * (size_t)d->redo_cap));
    }
    if (d->post == QD_POST_OSD0_OFFCHIP) {
        int ncu = 256;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, g->device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
        d->post_blocks = ncu * std::max(1, g->x_per_cu);
        const size_t words = qd_osd_offchip_ws_words(g->m, g->x_kw);
        if (words > 0) HIP_TRY(hipMalloc((void **)&d->q_spill_off, sizeof(uint64_t) * (size_t)d->post_blocks * words));
        HIP_TRY(hipMalloc((void **)&d->llr_ws, sizeof(float) * (size_t)max_batch * g->bp.n_pad));
        HIP_TRY(hipMalloc((void **)&d->fail_list, sizeof(int32_t) * (size_t)max_batch));
    } else if (d->post != QD_POST_NONE) {
        int ncu = 256;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, g->device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
        const int per_cu = std::max(1, QD_LDS_BYTES / std::max(1, g->osd.lds_bytes));
        d->osd_blocks = g->osd.lds_bytes > 0 ? ncu * std::min(per_cu, 2048 / std::max(1, g->osd.threads)) : 0;
        const int per_cu_fast = std::max(1, QD_LDS_BYTES / std::max(1, g->osd.f_lds_bytes));
        d->osd_blocks_fast = ncu * std::min(per_cu_fast, 2048 / std::max(1, g->osd.f_threads));
        if (d->osd_w) d->osd_blocks_fast = ncu;                                   // higher-order OSD by row: w_* layout, one workgroup per CU
        if (d->post == QD_POST_LSD) {
            const int lds = qd_lsd_lds_bytes(g->m, g->n, g->bp.out_words);
            d->post_blocks = ncu * std::max(1, std::min(8, QD_LDS_BYTES / std::max(1, lds)));     // one wavefront per shot, several shots per CU
            HIP_TRY(hipMalloc((void **)&d->lsd_ws, qd_lsd_ws_bytes(g->m, g->n, d->post_blocks, d->lsd_w)));   // Q planes + work counter (+ debug timers) + pivot columns (+ sweep scratch)
        } else if (d->post == QD_POST_OSD0_SR) {
            d->post_blocks = ncu * g->osd.s_per_cu;
            HIP_TRY(hipMalloc((void **)&d->q_spill_sr, sizeof(uint64_t) * (size_t)d->post_blocks *
                                                       qd_osd_sr_ws_words(g->osd.m_pad, g->osd.mw, g->osd.s_threads, g->osd.s_rpt)));
        } else if (d->post == QD_POST_OSD_CS_PANEL) {
            d->post_blocks = ncu * d->cs_per_cu;
            HIP_TRY(hipMalloc((void **)&d->cs_ws, sizeof(uint64_t) * (size_t)d->post_blocks * qd_osdcs_ws_words(d->cs_variant)));
        }
        const int spill_fast = g->osd.mw - (d->osd_w ? g->osd.w_kw : g->osd.f_kw);
        if (g->osd.f_lds_bytes > 0 && spill_fast > 0)
            HIP_TRY(hipMalloc((void **)&d->q_spill_fast, sizeof(uint64_t) * (size_t)d->osd_blocks_fast * spill_fast * g->osd.m_pad));
        if (d->osd_w && g->osd.w_lds_bytes > 0)
            HIP_TRY(hipMalloc((void **)&d->mt_ws, sizeof(uint64_t) * (size_t)d->osd_blocks_fast * ((size_t)g->osd.mw * g->osd.m_pad + 64 * 32)));   // + 64 candidate vectors of QD_SWEEP_W words
        HIP_TRY(hipMalloc((void **)&d->hard_list, sizeof(int32_t) * (size_t)max_batch));
        HIP_TRY(hipMalloc((void **)&d->hard_list2, sizeof(int32_t) * (size_t)max_batch));
        HIP_TRY(hipMalloc((void **)&d->llr_ws, sizeof(float) * (size_t)max_batch * g->bp.n_pad));
        HIP_TRY(hipMalloc((void **)&d->fail_list, sizeof(int32_t) * (size_t)max_batch));
        if (d->osd_blocks > 0)
            HIP_TRY(hipMalloc((void **)&d->order_ws, sizeof(uint16_t) * (size_t)d->osd_blocks * g->n));
        const int spill_planes = g->osd.mw - g->osd.kw_lds;
        if (d->osd_blocks > 0 && spill_planes > 0)
            HIP_TRY(hipMalloc((void **)&d->q_spill, sizeof(uint64_t) * (size_t)d->osd_blocks * spill_planes * g->osd.m_pad));
    }
    if (d->bp == BP_HBM_EDGE) {
        // [index][shot] message planes for a chunk of S shots; a batch larger than S is decoded chunk by chunk
        const bool ps = d->prm.bp_method == QD_BP_PRODUCT_SUM, serial = d->prm.schedule == QD_SCHEDULE_SERIAL;
        // edge planes: flooding b2c + c2b (+ th for product-sum); serial: messages (th or b2c) + suffixes (the c2b plane), and a row plane
        const int planes = serial ? 2 : (ps ? 3 : 2);
        const bool pre_plane = serial && g->gen.nslots == 0;       // the rows' running prefixes: LDS slots when the graph allows
        // Serial schedule in several launches (qd_decoder_create chose the bounds): costs a second workspace.
        GenStagePlan &sp = d->gsp;
        sp = GenStagePlan{};
        sp.nbounds = d->gen_nbounds;
        std::copy(d->gen_bounds, d->gen_bounds + d->gen_nbounds, sp.bounds);
        // (the launches alternate between two message planes and two syndrome planes; suffixes, prefixes, posteriors and fail slots are scratch of
        //  ONE launch and shared.  If the second message plane would push the batch into more workspace chunks, the schedule stays in one launch:
        //  a chunk more costs a whole dependency chain, more than packing returns -- W = 3 windows, ten decoders in a 96 GB budget: 98 -> 128 ms)
        const size_t per_shot1 = ((size_t)g->nnz * planes + g->n + (pre_plane ? g->m : 0)) * sizeof(float) + g->m + sizeof(int32_t);
        size_t per_shot = per_shot1 + (sp.nbounds > 0 ? (size_t)g->nnz * sizeof(float) + g->m + 2 * sizeof(int32_t) : 0);
        // Default budget 48 GB of the 288: the kernel is latency-bound (one wavefront per 64 shots), so a launch costs about
        // the same for 8 K or 64 K shots and chunks should be as large as memory allows -- and of equal size.
        const double budget_gb = d->gen_ws_limit > 0 ? (double)d->gen_ws_limit / 1073741824.0 : 48.0;
        const auto chunks_for = [&](size_t ps) { const int64_t s_ = std::max<int64_t>(256, (int64_t)(budget_gb * 1073741824.0 / (double)ps) & ~(int64_t)255); return (max_batch + s_ - 1) / s_; };
        if (sp.nbounds > 0 && chunks_for(per_shot) > chunks_for(per_shot1)) { sp.nbounds = 0; per_shot = per_shot1; }
        int64_t S = (int64_t)(budget_gb * 1073741824.0 / (double)per_shot) & ~(int64_t)255;
        S = std::max<int64_t>(256, S);
        const int64_t nchunks = (max_batch + S - 1) / S;
        S = std::max<int64_t>(256, (((max_batch + nchunks - 1) / nchunks) + 255) & ~(int64_t)255);
        GenWs &w = d->gws;
        w.S = S;
        if (!(ps && serial)) HIP_TRY(hipMalloc((void **)&w.b2c, sizeof(float) * (size_t)g->nnz * S));
        HIP_TRY(hipMalloc((void **)&w.c2b, sizeof(float) * (size_t)g->nnz * S));
        if (ps) HIP_TRY(hipMalloc((void **)&w.th, sizeof(float) * (size_t)g->nnz * S));
        if (pre_plane) HIP_TRY(hipMalloc((void **)&w.pre, sizeof(float) * (size_t)g->m * S));
        HIP_TRY(hipMalloc((void **)&w.llr, sizeof(float) * (size_t)g->n * S));
        HIP_TRY(hipMalloc((void **)&w.syn, (size_t)g->m * S));
        HIP_TRY(hipMalloc((void **)&w.slot, sizeof(int32_t) * (size_t)S));
        if (sp.nbounds > 0) {
            HIP_TRY(hipMalloc((void **)&sp.msg2, sizeof(float) * (size_t)g->nnz * S));
            HIP_TRY(hipMalloc((void **)&sp.syn2, (size_t)g->m * S));
            sp.w2 = w;
            (ps ? sp.w2.th : sp.w2.b2c) = sp.msg2;
            sp.w2.syn = sp.syn2;
            HIP_TRY(hipMalloc((void **)&sp.lists[0], sizeof(int32_t) * (size_t)S));
            HIP_TRY(hipMalloc((void **)&sp.lists[1], sizeof(int32_t) * (size_t)S));
            HIP_TRY(hipMalloc((void **)&sp.counts, sizeof(int32_t) * (QD_GEN_MAX_STAGES + 1)));
            HIP_TRY(hipHostMalloc((void **)&sp.host_counts, sizeof(int32_t) * (QD_GEN_MAX_STAGES + 1)));
            HIP_TRY(hipEventCreateWithFlags(&sp.counts_ready, hipEventDisableTiming));
        }
    }
    d->cap = max_batch;
    return QD_OK;
}

extern "C" int qd_decoder_set_workspace_limit(qd_decoder *d, int64_t bytes)
{
    if (!d || bytes <= 0) return fail(QD_EINVAL, "bad workspace limit");
    d->gen_ws_limit = bytes;
    if (d->bp == BP_HBM_EDGE && d->cap > 0) {          // takes effect at the next reserve: drop what is there
        HIP_TRY(hipSetDevice(d->g->device));
        HIP_TRY(hipDeviceSynchronize());
        free_ws(d);
    }
    return QD_OK;
}

extern "C" int qd_decoder_release_workspace(qd_decoder *d)
{
    if (!d) return fail(QD_EINVAL, "null decoder");
    HIP_TRY(hipSetDevice(d->g->device));
    HIP_TRY(hipDeviceSynchronize());
    free_ws(d);
    return QD_OK;
}

extern "C" int qd_decoder_set_profiling(qd_decoder *d, int32_t enable)
{
    if (!d) return fail(QD_EINVAL, "null decoder");
    d->profiling = enable ? 1 : 0;
    return QD_OK;
}

extern "C" int qd_decoder_profile(qd_decoder *d, double *out, int32_t reset)
{
    if (!d || !out) return fail(QD_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(d->g->device));
    for (auto &sp : d->ev) {
        HIP_TRY(hipEventSynchronize(sp.t1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, sp.t0, sp.t1));
        d->acc_ms[sp.kind] += ms; d->acc_ms[2 + sp.kind] += 1;
        (void)hipEventDestroy(sp.t0); (void)hipEventDestroy(sp.t1);
    }
    d->ev.clear();
    for (int i = 0; i < 4; ++i) out[i] = d->acc_ms[i];
    if (reset) for (int i = 0; i < 4; ++i) d->acc_ms[i] = 0;
    return QD_OK;
}

// The batch arguments of qd_decode_batch / qd_decode_stage / qd_osd0_batch (B = 0 is valid and decodes nothing)
static int check_batch(const qd_decoder *d, int64_t det_stride, int64_t det_offset, const uint8_t *d_upd, int64_t upd_stride, int32_t upd_rows, int64_t B)
{
    if (B < 0 || B > 0x7FFFFFFF) return fail(QD_EINVAL, "batch size out of range");
    if (B == 0) return QD_OK;
    if (det_offset < 0 || det_stride < det_offset + d->g->m) return fail(QD_EINVAL, "detector slice [%lld, %lld) exceeds the row stride %lld", (long long)det_offset, (long long)(det_offset + d->g->m), (long long)det_stride);
    if (d_upd && (upd_rows < 0 || upd_rows > d->g->m || upd_stride < upd_rows)) return fail(QD_EINVAL, "bad syndrome-update shape");
    return QD_OK;
}

// The kernels' arguments for one call: the caller's buffers and the decoder's workspace, with the counter set of the call in flight
static DecodeArgs decode_args(const qd_decoder *d, const uint8_t *d_det, int64_t det_stride, int64_t det_offset, const uint8_t *d_upd,
                              int64_t upd_stride, int32_t upd_rows, uint32_t *d_err_bits, int32_t *d_status)
{
    DecodeArgs a{};
    a.det = d_det; a.det_stride = det_stride; a.det_offset = det_offset;
    a.upd = d_upd; a.upd_stride = upd_stride; a.upd_rows = d_upd ? upd_rows : 0;
    a.max_iter = d->prm.max_iter; a.ms_scale = (float)d->prm.ms_scaling_factor; a.want_llr = d->post != QD_POST_NONE ? 1 : 0;
    a.err_bits = d_err_bits; a.status = d_status;
    a.llr_ws = d->llr_ws; a.fail_list = d->fail_list; a.fail_count = d->fail_count;
    a.order_ws = d->order_ws; a.q_spill = d->q_spill; a.q_spill_fast = d->q_spill_fast; a.q_spill_sr = d->q_spill_sr; a.mt_ws = d->mt_ws;
    a.hard_list = d->hard_list; a.hard_list2 = d->hard_list2; a.hard_count = d->fail_count + 1;
    a.dbg = reinterpret_cast<unsigned long long *>(d->ctr_base) + 2;   // bytes 16..143 of the counter block (first set, never zeroed by a call)
    a.osd_w = d->osd_w; a.osd_order = d->prm.osd_order; a.rank = d->g->rank;
    return a;
}

// Stage 1: BP over the batch
static int launch_bp(qd_decoder *d, const DecodeArgs &a, int64_t B, hipStream_t s)
{
    const qd_graph *g = d->g;
    GenGraphDev gg = g->gen;
    gg.llr0 = d->llr0_q;
    switch (d->bp) {
    case BP_LDS_EDGE: HIP_TRY(qd_launch_bp_ps_lds(gg, g->bp, a, B, s)); break;
    case BP_GATHER_RAW: HIP_TRY(qd_launch_bp(g->bp, a, B, s)); break;
    case BP_HBM_EDGE: {
        // edge_cert (off-chip decoder on the LLR grid): the first pass parks the shots whose exactness bound tripped, the redo pass decodes them
        // on the coarse grid -- the gather kernel's rule (BP_GATHER_GRID below), chunk by chunk of the message workspace
        int32_t *redo_count = d->fail_count + 40;
        DecodeArgs a1 = a;
        if (d->edge_cert) {
            a1.s_limit = std::ldexp(1.0f, 23 - d->grid_k);
            a1.redo_list = d->redo_list; a1.redo_count = redo_count; a1.redo_cap = d->redo_cap;
        }
        for (int64_t b0 = 0; b0 < B; b0 += d->gws.S)
            HIP_TRY(qd_launch_bp_general(gg, g->bp, a1, d->gws, d->prm.bp_method, d->prm.schedule, b0,
                                         (int)std::min<int64_t>(d->gws.S, B - b0), s, d->gsp.nbounds > 0 ? &d->gsp : nullptr));
        if (d->edge_cert) {
            DecodeArgs a2 = a;
            a2.s_limit = std::ldexp(1.0f, 23 - d->grid_kc);
            a2.shot_list = d->redo_list; a2.shot_count = redo_count; a2.status_or = QD_STATUS_COARSE_GRID;
            gg.llr0 = d->llr0_qc;
            const int64_t parked_max = std::min<int64_t>(B, d->redo_cap);
            for (int64_t c0 = 0; c0 < parked_max; c0 += d->gws.S)
                HIP_TRY(qd_launch_bp_general(gg, g->bp, a2, d->gws, d->prm.bp_method, d->prm.schedule, c0,
                                             (int)std::min<int64_t>(d->gws.S, parked_max - c0), s, nullptr));
        }
        break;
    }
    case BP_SCATTER_WIDE:
    case BP_SCATTER:
    case BP_GATHER_GRID: {
        // grid arithmetic: first pass on the fine grid parks the shots whose exactness bound tripped; they are decoded
        // again on the coarse grid by a second launch (one workgroup per parked shot; the others exit at once)
        int32_t *redo_count = d->fail_count + 40;       // bytes 160..163 of the counter set (16..143 of the first set are the debug counters)
        DecodeArgs a1 = a;
        a1.s_limit = std::ldexp(1.0f, 23 - d->grid_k);
        a1.redo_list = d->redo_list; a1.redo_count = redo_count; a1.redo_cap = d->redo_cap;
        if (d->bp == BP_GATHER_GRID)
            HIP_TRY(qd_launch_bp(d->bp_fine, a1, B, s));
        else {
            // scatter kernel first; the shots its (looser) bound cannot certify are decoded again by the gather kernel,
            // which carries the per-fault bound the coarse-grid rule is stated on
            int32_t *recheck_count = d->fail_count + 41;
            ScatArgs x{};
            x.prior_g = d->prior_g; x.grid_inv = std::ldexp(1.0f, -d->grid_k); x.m2_limit = d->m2_limit;
            x.recheck_list = d->recheck_list; x.recheck_count = recheck_count; x.recheck_cap = d->recheck_cap;
            x.first_pass = d->first_pass;
            if (d->bp == BP_SCATTER_WIDE) HIP_TRY(qd_launch_bp_scatter_wide(d->bp_fine, g->sc, a1, x, B, s));
            else HIP_TRY(qd_launch_bp_scatter(d->bp_fine, g->sc, a1, x, B, s));
            a1.shot_list = d->recheck_list; a1.shot_count = recheck_count;
            HIP_TRY(qd_launch_bp(d->bp_fine, a1, std::min<int64_t>(B, d->recheck_cap), s));
        }
        DecodeArgs a2 = a;
        a2.s_limit = std::ldexp(1.0f, 23 - d->grid_kc);
        a2.shot_list = d->redo_list; a2.shot_count = redo_count; a2.status_or = QD_STATUS_COARSE_GRID;
        HIP_TRY(qd_launch_bp(d->bp_coarse, a2, std::min<int64_t>(B, d->redo_cap), s));
        break;
    }
    }
    return QD_OK;
}

// Stage 2: the post-processor over the shots BP parked
static int launch_post(const qd_decoder *d, const DecodeArgs &a, int64_t B, hipStream_t s)
{
    const qd_graph *g = d->g;
    const int blocks = (int)std::min<int64_t>(B, d->post_blocks);
    const int fast = (int)std::min<int64_t>(B, d->osd_blocks_fast), full = (int)std::min<int64_t>(B, d->osd_blocks);
    switch (d->post) {
    case QD_POST_OSD0_OFFCHIP:
        HIP_TRY(qd_launch_osd0_offchip(g->osd, g->bp, a, g->x_off, g->x_off_sort, g->x_off_order, g->x_kw, g->x_threads, g->x_lds, d->q_spill_off, blocks, s));
        break;
    case QD_POST_LSD:
        HIP_TRY(qd_launch_lsd0(g->gen, g->bp, a, d->lsd_ws, d->post_blocks, blocks, d->lsd_w, d->prm.osd_order, g->osd.wfix, s));
        break;
    case QD_POST_OSD_CS_PANEL:
        HIP_TRY(qd_launch_osdcs(g->osd, g->bp, a, d->cs_off, d->cs_variant, d->cs_lds, d->cs_ws, blocks, s));
        break;
    case QD_POST_OSD0_SR:
        // OSD-0: many pivots per round (osd_sr.hip); shots whose syndrome is outside the column space come back on the hard list
        // and are decoded by the one-pivot-per-round kernel, whose lowest-row rule defines their answer
        HIP_TRY(qd_launch_osd0_sr(g->osd, g->bp, a, blocks, s));
        HIP_TRY(qd_launch_osd0(g->osd, g->bp, a, fast, full, s, true));
        break;
    default:                                            // QD_POST_OSD0_REG, QD_POST_OSD_W_OLD
        HIP_TRY(qd_launch_osd0(g->osd, g->bp, a, fast, full, s));
    }
    return QD_OK;
}

static int decode_impl(qd_decoder *d, const uint8_t *d_det, int64_t det_stride, int64_t det_offset, const uint8_t *d_upd,
                       int64_t upd_stride, int32_t upd_rows, int64_t B, uint32_t *d_err_bits, int32_t *d_status, int stage,
                       void *stream)
{
    if (!d) return fail(QD_EINVAL, "null decoder");
    if (stage < 1 || stage > 3) return fail(QD_EINVAL, "stage must be 1 (BP), 2 (OSD) or 3 (both)");
    if (int rc = check_batch(d, det_stride, det_offset, d_upd, upd_stride, upd_rows, B)) return rc;
    if (B == 0) return QD_OK;                            // whatever the pointers: an empty batch has none (a torch tensor of no rows: data_ptr() = 0)
    if (!d_det || !d_err_bits || !d_status) return fail(QD_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(d->g->device));
    if (B > d->cap && stage == 2) return fail(QD_EINVAL, "OSD stage without a preceding BP stage of this batch size");
    if (int rc = B > d->cap ? qd_decoder_reserve(d, B) : QD_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool post = d->post != QD_POST_NONE;
    if (stage & 1) {                                     // a new call: the other counter set (see qd_decoder::ctr_base)
        d->cset ^= 1;
        d->fail_count = d->ctr_base + 64 * d->cset;
        if (!d->set_clean[d->cset]) {
            HIP_TRY(hipMemsetAsync(d->fail_count, 0, 3 * sizeof(int32_t), s));
            HIP_TRY(hipMemsetAsync(d->fail_count + 40, 0, 2 * sizeof(int32_t), s));
        }
        d->set_clean[d->cset] = false;
        d->last_B = B;
    }
    const DecodeArgs a = decode_args(d, d_det, det_stride, det_offset, d_upd, upd_stride, upd_rows, d_err_bits, d_status);
    auto span = [&](int kind) -> int {
        if (!d->profiling) return QD_OK;
        hipEvent_t t0, t1;
        HIP_TRY(hipEventCreate(&t0)); HIP_TRY(hipEventCreate(&t1));
        d->ev.push_back({kind, t0, t1});
        HIP_TRY(hipEventRecord(t0, s));
        return QD_OK;
    };
    if (stage & 1) {
        if (int rc = span(0)) return rc;
        if (int rc = launch_bp(d, a, B, s)) return rc;
        if (d->profiling) HIP_TRY(hipEventRecord(d->ev.back().t1, s));
    }
    if ((stage & 2) && post) {
        if (int rc = span(1)) return rc;
        if (int rc = launch_post(d, a, B, s)) return rc;
        if (d->profiling) HIP_TRY(hipEventRecord(d->ev.back().t1, s));
        if (!d->fail_pending && d->host_fail) {          // (see qd_decoder::host_fail)
            HIP_TRY(hipMemcpyAsync(d->host_fail, d->fail_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipEventRecord(d->fail_ready, s));
            d->fail_pending = true; d->fail_pending_B = d->last_B;
        }
    }
    if ((stage & 2) && !d->set_clean[d->cset ^ 1]) {     // the next call's counters, zeroed behind this call's last stage (nothing waits for these fills)
        int32_t *other = d->ctr_base + 64 * (d->cset ^ 1);
        HIP_TRY(hipMemsetAsync(other, 0, 3 * sizeof(int32_t), s));
        HIP_TRY(hipMemsetAsync(other + 40, 0, 2 * sizeof(int32_t), s));
        d->set_clean[d->cset ^ 1] = true;
    }
    return QD_OK;
}

// See include/quits_amd.h.  Heavy = the post-processor will want whole CUs for about as long as a BP stage or longer: OSD-CS / OSD-E (two workgroups of
// 78 KB of LDS per CU), BP-LSD, and OSD-0 when at least three quarters of the batch failed (headline p = 3e-3: 48 %, p = 5e-3: 95 %).  Measured, same box, 30 us
// against none: OSD-CS(1) 361 -> 482 k shots/s, lsd_cs(1) 888 -> 940 k, p = 6e-3 488 -> 569 k, W = 5 / F = 3 1.125 -> 1.153 M; the headline (OSD-0 over
// 48 % of the shots, 4.4 ms beside 40 ms of BP) is the one that loses, 1.552 -> 1.539 M -- even to an EMPTY launch at this point of the BP stream, so an
// OSD-0 decoder launches nothing unless an earlier call's failure count (qd_decoder::host_fail) says "heavy" (profiles/r06_post_head_start.txt).
extern "C" int qd_decoder_post_head_start(qd_decoder *d, int32_t microseconds, void *stream)
{
    if (!d) return fail(QD_EINVAL, "null decoder");
    if (microseconds < 0) microseconds = 50;
    if (microseconds <= 0 || d->post == QD_POST_NONE || !d->ctr_base || d->last_B <= 0) return QD_OK;
    microseconds = std::min(microseconds, 5000);
    HIP_TRY(hipSetDevice(d->g->device));
    const bool always = d->post == QD_POST_LSD || d->post == QD_POST_OSD_CS_PANEL;
    const double frac = 0.75;
    if (d->fail_pending && qd_event_done(d->fail_ready)) {
        d->fail_pending = false;
        if (d->fail_pending_B > 0) d->fail_frac_hint = (double)d->host_fail[0] / (double)d->fail_pending_B;
    }
    if (!always && d->fail_frac_hint < 0.8 * frac) return QD_OK;        // OSD-0 over a minority of the shots (or nothing known yet): no launch at all
    const int threshold = (int)std::min<double>(2147483647.0, std::max(1.0, frac * (double)d->last_B));
    HIP_TRY(qd_launch_hold(always ? nullptr : d->fail_count, threshold, microseconds, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

extern "C" int qd_decode_batch(qd_decoder *d, const uint8_t *d_det, int64_t det_stride, int64_t det_offset,
                               const uint8_t *d_upd, int64_t upd_stride, int32_t upd_rows, int64_t B,
                               uint32_t *d_err_bits, int32_t *d_status, void *stream)
{
    return decode_impl(d, d_det, det_stride, det_offset, d_upd, upd_stride, upd_rows, B, d_err_bits, d_status, 3, stream);
}

extern "C" int qd_decode_stage(qd_decoder *d, const uint8_t *d_det, int64_t det_stride, int64_t det_offset,
                               const uint8_t *d_upd, int64_t upd_stride, int32_t upd_rows, int64_t B,
                               uint32_t *d_err_bits, int32_t *d_status, int32_t stage, void *stream)
{
    return decode_impl(d, d_det, det_stride, det_offset, d_upd, upd_stride, upd_rows, B, d_err_bits, d_status, stage, stream);
}

extern "C" int qd_osd0_batch(qd_decoder *d, const uint8_t *d_det, int64_t det_stride, int64_t det_offset,
                             const uint8_t *d_upd, int64_t upd_stride, int32_t upd_rows, int64_t B, const float *d_llr,
                             uint32_t *d_err_bits, int32_t *d_status, void *stream)
{
    if (!d) return fail(QD_EINVAL, "null decoder");
    if (d->post == QD_POST_NONE) return fail(QD_EINVAL, "decoder was created with osd_method = off");
    if (int rc = check_batch(d, det_stride, det_offset, d_upd, upd_stride, upd_rows, B)) return rc;
    if (B == 0) return QD_OK;
    if (!d_det || !d_llr || !d_err_bits || !d_status) return fail(QD_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(d->g->device));
    if (int rc = B > d->cap ? qd_decoder_reserve(d, B) : QD_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const DecodeArgs a = decode_args(d, d_det, det_stride, det_offset, d_upd, upd_stride, upd_rows, d_err_bits, d_status);
    HIP_TRY(hipMemsetAsync(d->fail_count, 0, 3 * sizeof(int32_t), s));
    d->set_clean[d->cset] = false;
    HIP_TRY(qd_launch_stage_llr(d_llr, d->g->n, d->g->bp.n_pad, d->g->bp.bit_orig, B, d->llr_ws, d->fail_list, d->fail_count,
                                d_status, s));
    return launch_post(d, a, B, s);
}

extern "C" int qd_decoder_debug_counters(qd_decoder *d, uint64_t *out16)
{
    if (!d || !out16 || !d->fail_count) return fail(QD_EINVAL, "no workspace yet");
    HIP_TRY(hipSetDevice(d->g->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out16, reinterpret_cast<char *>(d->ctr_base) + 16, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(reinterpret_cast<char *>(d->ctr_base) + 16, 0, 16 * sizeof(uint64_t)));
    return QD_OK;
}

extern "C" int qd_decoder_failed_llr(qd_decoder *d, int64_t b, float *d_out, void *stream)
{
    if (!d || !d_out || !d->llr_ws) return fail(QD_EINVAL, "no posterior workspace (OSD off or nothing decoded yet)");
    HIP_TRY(hipSetDevice(d->g->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipStreamSynchronize(s));
    int32_t nfail = 0;
    HIP_TRY(hipMemcpy(&nfail, d->fail_count, sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int32_t> list((size_t)std::max(nfail, 1));
    if (nfail > 0) HIP_TRY(hipMemcpy(list.data(), d->fail_list, sizeof(int32_t) * (size_t)nfail, hipMemcpyDeviceToHost));
    for (int i = 0; i < nfail; ++i)
        if (list[i] == (int32_t)b) {
            // workspace rows are in bit-slot order; hand back fault order
            const qd_graph *g = d->g;
            std::vector<float> slot(g->bp.n_pad), outv(g->n);
            std::vector<uint32_t> orig(g->bp.n_pad);
            HIP_TRY(hipMemcpy(slot.data(), d->llr_ws + (size_t)i * g->bp.n_pad, sizeof(float) * g->bp.n_pad, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(orig.data(), g->bp.bit_orig, sizeof(uint32_t) * g->bp.n_pad, hipMemcpyDeviceToHost));
            for (int sidx = 0; sidx < g->n; ++sidx) outv[orig[sidx]] = slot[sidx];
            HIP_TRY(hipMemcpy(d_out, outv.data(), sizeof(float) * g->n, hipMemcpyHostToDevice));
            return QD_OK;
        }
    return fail(QD_EINVAL, "shot %lld converged (no stored posterior)", (long long)b);
}

extern "C" int qd_spmat_create(int32_t nrows, int32_t ncols, const int32_t *row_ptr, const int32_t *col_idx,
                               int32_t device, qd_spmat **out)
{
    if (!out) return fail(QD_EINVAL, "out is null");
    *out = nullptr;
    if (nrows < 0 || ncols < 0 || !row_ptr) return fail(QD_EINVAL, "bad shape");
    const int nnz = row_ptr[nrows];
    if (nnz > 0 && !col_idx) return fail(QD_EINVAL, "null col_idx");
    for (int e = 0; e < nnz; ++e)
        if (col_idx[e] < 0 || col_idx[e] >= ncols) return fail(QD_EINVAL, "column index out of range");
    if (hipSetDevice(device) != hipSuccess) return fail(QD_EHIP, "hipSetDevice(%d) failed", device);
    qd_spmat *s = new qd_spmat();
    s->device = device;
    std::vector<uint32_t> rp(row_ptr, row_ptr + nrows + 1), ci(col_idx, col_idx + nnz);
    int rc = s->mem.upload(rp, &s->d.row_ptr) | s->mem.upload(ci, &s->d.col_idx);
    if (rc) { s->mem.release(); delete s; return fail(QD_EHIP, "device allocation/upload failed"); }
    s->d.nrows = nrows; s->d.ncols = ncols; s->d.nnz = nnz;
    s->d.colmask = nullptr; s->d.mask_words = 0;
    if (nrows > 0 && nrows <= 512 && ncols > 0) {
        const int mw = (nrows + 31) / 32;
        std::vector<uint32_t> cm((size_t)ncols * mw, 0u);
        for (int r = 0; r < nrows; ++r)
            for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) cm[(size_t)col_idx[e] * mw + (r >> 5)] ^= 1u << (r & 31);
        if (s->mem.upload(cm, &s->d.colmask)) { s->mem.release(); delete s; return fail(QD_EHIP, "device allocation/upload failed"); }
        s->d.mask_words = mw;
    }
    *out = s;
    return QD_OK;
}

extern "C" void qd_spmat_destroy(qd_spmat *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    s->mem.release();
    delete s;
}

extern "C" int qd_gf2_spmv_batch(const qd_spmat *A, const uint32_t *d_err_bits, int64_t err_stride_words, int64_t B,
                                 uint8_t *d_out, int64_t out_stride, int32_t accumulate, void *stream)
{
    if (!A || !d_err_bits || !d_out) return fail(QD_EINVAL, "null argument");
    if (err_stride_words * 32 < A->d.ncols) return fail(QD_EINVAL, "error rows hold %lld bits, matrix has %d columns", (long long)err_stride_words * 32, A->d.ncols);
    if (out_stride < A->d.nrows) return fail(QD_EINVAL, "out_stride smaller than the row count");
    HIP_TRY(hipSetDevice(A->device));
    HIP_TRY(qd_launch_spmv(A->d, d_err_bits, err_stride_words, B, d_out, out_stride, accumulate, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

extern "C" int qd_unpack_bits(const uint32_t *d_bits, int64_t stride_words, int32_t nbits, int64_t B, uint8_t *d_out,
                              int64_t out_stride, void *stream)
{
    if (!d_bits || !d_out || nbits < 0 || stride_words * 32 < nbits || out_stride < nbits) return fail(QD_EINVAL, "bad unpack arguments");
    HIP_TRY(qd_launch_unpack(d_bits, stride_words, nbits, B, d_out, out_stride, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

extern "C" int qd_count_mismatch(const uint8_t *d_pred, const uint8_t *d_obs, int32_t k, int64_t B, int64_t *d_count,
                                 void *stream)
{
    if (!d_pred || !d_obs || !d_count || k <= 0) return fail(QD_EINVAL, "bad count arguments");
    HIP_TRY(qd_launch_count(d_pred, d_obs, k, B, d_count, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

// qd_sample_dem (d_shots == nullptr: shots shot0 .. shot0 + B - 1) and qd_sample_dem_shots (row b = shot d_shots[b])
static int sample_dem_impl(const qd_spmat *Ht, const qd_spmat *Lt, const double *priors, uint64_t seed, int64_t shot0, const int64_t *d_shots,
                           int64_t B, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride, void *stream)
{
    if (!Ht || !Lt || !priors || !d_det || !d_obs) return fail(QD_EINVAL, "null argument");
    if (Ht->d.nrows != Lt->d.nrows) return fail(QD_EINVAL, "Ht and Lt must both have one row per fault");
    const int n = Ht->d.nrows, m = Ht->d.ncols, nobs = Lt->d.ncols;
    if (det_stride < m || obs_stride < nobs) return fail(QD_EINVAL, "output strides too small");
    if (((m + 31) / 32 + (nobs + 31) / 32) * 4 > 64 * 1024) return fail(QD_ECAPACITY, "too many detectors for the sampler's LDS bit array");
    HIP_TRY(hipSetDevice(Ht->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    std::vector<uint32_t> thr((size_t)n);
    for (int j = 0; j < n; ++j) {
        double t = std::floor(priors[j] * 4294967296.0);
        thr[j] = (uint32_t)std::min(std::max(t, 0.0), 4294967295.0);
    }
    uint32_t *d_thr = nullptr;
    HIP_TRY(hipMalloc((void **)&d_thr, sizeof(uint32_t) * (size_t)std::max(n, 4)));
    hipError_t e = hipMemcpy(d_thr, thr.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = qd_launch_sample(Ht->d, Lt->d, d_thr, seed, shot0, d_shots, B, m, nobs, d_det, det_stride, d_obs, obs_stride, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_thr);
    if (e != hipSuccess) return fail(QD_EHIP, "sampler: %s", hipGetErrorString(e));
    return QD_OK;
}

extern "C" int qd_sample_dem(const qd_spmat *Ht, const qd_spmat *Lt, const double *priors, uint64_t seed, int64_t shot0,
                             int64_t B, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride,
                             void *stream)
{
    return sample_dem_impl(Ht, Lt, priors, seed, shot0, nullptr, B, d_det, det_stride, d_obs, obs_stride, stream);
}

extern "C" int qd_sample_dem_shots(const qd_spmat *Ht, const qd_spmat *Lt, const double *priors, uint64_t seed, const int64_t *d_shots,
                                   int64_t B, uint8_t *d_det, int64_t det_stride, uint8_t *d_obs, int64_t obs_stride, void *stream)
{
    if (B == 0) return QD_OK;
    if (B < 0 || B > INT32_MAX) return fail(QD_EINVAL, "bad shot count (one workgroup per shot: at most 2^31 - 1 in one call)");
    if (!d_shots) return fail(QD_EINVAL, "null shot list");
    return sample_dem_impl(Ht, Lt, priors, seed, 0, d_shots, B, d_det, det_stride, d_obs, obs_stride, stream);
}

// ---- circuit-level sampler (frame_sampler.hip): the program comes from quits_amd/frame.py; everything the kernel indexes with is
// checked here once, so the kernel trusts the program.
hipError_t qd_launch_frame_sample(const FrameDev &c, uint64_t seed, int64_t shot0, const int64_t *shot_list, int64_t B, uint8_t *det,
                                  int64_t det_stride, uint8_t *obs, int64_t obs_stride, hipStream_t s);

struct qd_circuit {
    int device = 0;
    FrameDev d{};
    int nq = 0, nmeas = 0, ndet = 0, nobs = 0;
    int64_t nsites = 0;
    DevAllocs mem;
};

static int frame_check_program(const int32_t *p, int64_t len, int nq, int nmeas, int ndet, int nobs, const uint32_t *thr, int nthr, int ring,
                               int64_t *nsites, int *channels)
{
    *channels = 0;
    std::vector<int64_t> seen((size_t)nq, -1);     // qubit -> pc of the last gate part that used it
    int64_t pc = 0, sites = 0, meas = 0;
    int next_det = 0;
    auto bad = [&](const char *what) { return fail(QD_EINVAL, "circuit program word %lld: %s", (long long)pc, what); };
    while (pc < len) {
        if (len - pc < 2) return bad("truncated instruction");
        const int op = p[pc], n = p[pc + 1];
        if (op < 0 || op >= QD_FOP_COUNT) return bad("unknown opcode");
        if (n < 0) return bad("negative count");
        int64_t width;
        switch (op) {
        case QD_FOP_R: case QD_FOP_H: width = 2 + (int64_t)n; break;
        case QD_FOP_CX: case QD_FOP_M: case QD_FOP_MX: case QD_FOP_MR: width = 2 + 2 * (int64_t)n; break;
        case QD_FOP_XERR: case QD_FOP_ZERR: case QD_FOP_DEP1: case QD_FOP_YERR: case QD_FOP_PC1: width = 4 + (int64_t)n; break;
        case QD_FOP_DEP2: case QD_FOP_PC2: width = 4 + 2 * (int64_t)n; break;
        case QD_FOP_FLUSH: width = 3; break;
        default: width = 3 + (int64_t)n; break;                 // DET, OBS
        }
        if (width > len - pc) return bad("instruction runs past the end of the program");
        const int32_t *a = p + pc + 2;
        if (op <= QD_FOP_MR) {
            const int per = (op == QD_FOP_R || op == QD_FOP_H) ? 1 : 2;
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < (op == QD_FOP_CX ? 2 : 1); ++k) {
                    const int q = a[per * i + k];
                    if (q < 0 || q >= nq) return bad("qubit out of range");
                    if (seen[q] == pc) return bad("a qubit repeats inside one gate part");
                    seen[q] = pc;
                }
            if (op >= QD_FOP_M) {
                for (int i = 0; i < n; ++i)
                    if (a[2 * i + 1] < 0 || a[2 * i + 1] >= ring) return bad("ring slot out of range");
                meas += n;
            }
        } else if (op <= QD_FOP_DEP2 || op >= QD_FOP_YERR) {
            if (op >= QD_FOP_YERR) *channels = 1;
            const int K = op == QD_FOP_PC1 ? 3 : (op == QD_FOP_PC2 ? 15 : 1);      // thresholds the instruction reads: a[0] .. a[0] + K - 1
            if (a[0] < 0 || a[0] >= nthr) return bad("threshold index out of range");
            if ((int64_t)a[0] + K > nthr) return bad("threshold table runs past the end of the thresholds");
            for (int k = 1; k < K; ++k)
                if (thr[a[0] + k] < thr[a[0] + k - 1]) return bad("threshold table must be non-decreasing (cumulative)");
            if (a[1] < 0 || (a[1] & 3)) return bad("first site must be a non-negative multiple of 4");
            const bool pairs = op == QD_FOP_DEP2 || op == QD_FOP_PC2;
            const int nt = pairs ? 2 * n : n;
            for (int i = 0; i < nt; ++i)
                if (a[2 + i] < 0 || a[2 + i] >= nq) return bad("qubit out of range");
            if (op == QD_FOP_PC2)
                for (int i = 0; i < n; ++i)
                    if (a[2 + 2 * i] == a[3 + 2 * i]) return bad("the two targets of a pair must differ");
            sites += n;
        } else if (op == QD_FOP_FLUSH) {
            if (n < 1 || n > QD_WAVE || a[0] < 0 || (a[0] & (QD_WAVE - 1)) || a[0] + n > ndet) return bad("bad detector block");
            if (a[0] + n != next_det) return bad("a flush must close the detector block just produced");
        } else {
            if (op == QD_FOP_DET) {
                if (a[0] != next_det) return bad("detectors must come in order");
                ++next_det;
            } else if (a[0] < 0 || a[0] >= nobs) return bad("observable out of range");
            for (int i = 0; i < n; ++i)
                if (a[1 + i] < 0 || a[1 + i] >= ring) return bad("ring slot out of range");
        }
        pc += width;
    }
    if (meas != nmeas) return fail(QD_EINVAL, "program measures %lld times, nmeas = %d", (long long)meas, nmeas);
    if (next_det != ndet) return fail(QD_EINVAL, "program defines %d detectors, ndet = %d", next_det, ndet);
    *nsites = sites;
    return QD_OK;
}

extern "C" int qd_circuit_create(const int32_t *program, int64_t program_len, int32_t nq, int32_t nmeas, int32_t ndet, int32_t nobs,
                                 const uint32_t *thresholds, int32_t nthr, int32_t max_lookback, int32_t device, qd_circuit **out)
{
    if (!out) return fail(QD_EINVAL, "out is null");
    *out = nullptr;
    if (!program || program_len < 0 || program_len > INT32_MAX) return fail(QD_EINVAL, "bad program");
    if (nq < 0 || nmeas < 0 || ndet < 0 || nobs < 0 || nthr < 0 || max_lookback < 1) return fail(QD_EINVAL, "bad sizes");
    if (nthr > 0 && !thresholds) return fail(QD_EINVAL, "null thresholds");
    const int64_t lds = 8 * (2 * (int64_t)nq + max_lookback + nobs);
    if (lds > QD_FRAME_LDS_MAX)
        return fail(QD_ECAPACITY, "circuit needs %lld B of LDS per wavefront (%d qubits, %d-measurement ring, %d observables), budget %d B",
                    (long long)lds, nq, max_lookback, nobs, QD_FRAME_LDS_MAX);
    int64_t nsites = 0;
    int channels = 0;
    int rc = frame_check_program(program, program_len, nq, nmeas, ndet, nobs, thresholds, nthr, max_lookback, &nsites, &channels);
    if (rc) return rc;
    if (hipSetDevice(device) != hipSuccess) return fail(QD_EHIP, "hipSetDevice(%d) failed", device);
    qd_circuit *c = new qd_circuit();
    c->device = device;
    std::vector<int32_t> prog(program, program + program_len);
    std::vector<uint32_t> thr(thresholds, thresholds + nthr);
    if (c->mem.upload(prog, &c->d.prog) || c->mem.upload(thr, &c->d.thr)) {
        c->mem.release(); delete c; return fail(QD_EHIP, "device allocation/upload failed");
    }
    c->d.prog_len = (int)program_len; c->d.nq = nq; c->d.ring = max_lookback; c->d.nobs = nobs; c->d.lds_bytes = (int)lds;
    c->d.channels = channels;
    c->nq = nq; c->nmeas = nmeas; c->ndet = ndet; c->nobs = nobs; c->nsites = nsites;
    *out = c;
    return QD_OK;
}

extern "C" void qd_circuit_destroy(qd_circuit *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    c->mem.release();
    delete c;
}

extern "C" int qd_circuit_info(const qd_circuit *c, int64_t *info)
{
    if (!c || !info) return fail(QD_EINVAL, "null argument");
    const int64_t v[8] = {c->nq, c->nsites, c->d.lds_bytes, c->nmeas, c->ndet, c->nobs, c->d.ring, c->d.prog_len};
    for (int i = 0; i < 8; ++i) info[i] = v[i];
    return QD_OK;
}

extern "C" int qd_sample_circuit(const qd_circuit *c, uint64_t seed, int64_t shot0, int64_t B, uint8_t *d_det, int64_t det_stride,
                                 uint8_t *d_obs, int64_t obs_stride, void *stream)
{
    if (!c) return fail(QD_EINVAL, "null circuit");
    if (B < 0 || shot0 < 0) return fail(QD_EINVAL, "negative shot count or shot0");
    if (B > (int64_t)QD_WAVE * INT32_MAX) return fail(QD_EINVAL, "too many shots in one call");
    if ((c->ndet > 0 && !d_det) || (c->nobs > 0 && !d_obs)) return fail(QD_EINVAL, "null output");
    if (det_stride < c->ndet || obs_stride < c->nobs) return fail(QD_EINVAL, "output strides too small");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(qd_launch_frame_sample(c->d, seed, shot0, nullptr, B, d_det, det_stride, d_obs, obs_stride, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

extern "C" int qd_sample_circuit_shots(const qd_circuit *c, uint64_t seed, const int64_t *d_shots, int64_t B, uint8_t *d_det, int64_t det_stride,
                                       uint8_t *d_obs, int64_t obs_stride, void *stream)
{
    if (B == 0) return QD_OK;
    if (!c) return fail(QD_EINVAL, "null circuit");
    if (B < 0) return fail(QD_EINVAL, "negative shot count");
    if (B > (int64_t)QD_WAVE * INT32_MAX) return fail(QD_EINVAL, "too many shots in one call");
    if (!d_shots) return fail(QD_EINVAL, "null shot list");
    if ((c->ndet > 0 && !d_det) || (c->nobs > 0 && !d_obs)) return fail(QD_EINVAL, "null output");
    if (det_stride < c->ndet || obs_stride < c->nobs) return fail(QD_EINVAL, "output strides too small");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(qd_launch_frame_sample(c->d, seed, 0, d_shots, B, d_det, det_stride, d_obs, obs_stride, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

// ---- the memory experiment's bookkeeping (experiment.hip)
extern "C" int qd_shot_flags_fold(const int32_t *d_status, int64_t B, uint8_t *d_flags, void *stream)
{
    if (B == 0) return QD_OK;
    if (B < 0) return fail(QD_EINVAL, "negative shot count");
    if (!d_status || !d_flags) return fail(QD_EINVAL, "null status or flags");
    if (B > 256ll * INT32_MAX) return fail(QD_EINVAL, "too many shots in one call");
    HIP_TRY(qd_launch_shot_flags(d_status, B, d_flags, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}

extern "C" int qd_tally_batch(const uint8_t *d_pred, int64_t pred_stride, const uint8_t *d_obs, int64_t obs_stride, int32_t k, int64_t B,
                              const uint8_t *d_flags, int64_t *d_counts, uint64_t *d_fail_mask, void *stream)
{
    if (B == 0) return QD_OK;
    if (B < 0) return fail(QD_EINVAL, "negative shot count");
    if (!d_pred || !d_obs || !d_counts) return fail(QD_EINVAL, "null predictions, observables or counts");
    if (k <= 0 || k > QD_TALLY_MAX_K) return fail(QD_EINVAL, "k = %d observables outside 1 .. %d", k, QD_TALLY_MAX_K);
    if (pred_stride < k || obs_stride < k) return fail(QD_EINVAL, "row strides smaller than k");
    HIP_TRY(qd_launch_tally(d_pred, pred_stride, d_obs, obs_stride, k, B, d_flags, d_counts, d_fail_mask, reinterpret_cast<hipStream_t>(stream)));
    return QD_OK;
}
