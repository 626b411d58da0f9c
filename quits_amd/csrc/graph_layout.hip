// graph_layout.hip -- the host-only combinatorics of qd_graph_create (graph_layout.h).  Plain C++ under a .hip name (the Makefile's pattern rule
// builds it with the library): no HIP header, no HIP extension, so `g++ -x c++` and `clang++ -x c++` compile it for tests/layout_check.cpp.
#include "graph_layout.h"
#include "../../include/quits_amd.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>


static inline int align16(int x) { return (x + 15) & ~15; }
static inline int pad64(int x) { return (x + 63) & ~63; }

Switches qd_read_switches()
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

// ---- LDS banks for the scatter kernel (bp_scatter_wide.hip) -------------------------------------------------------------------
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

int qd_host_graph(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx, const double *priors, HostGraph &h)
{
    if (m <= 0 || n <= 0 || !row_ptr || !col_idx || !priors) return qd_fail(QD_EINVAL, "empty or null graph");
    if (m > 32767) return qd_fail(QD_ECAPACITY, "m = %d detectors per window exceeds 32767", m);
    if (n > 65000) return qd_fail(QD_ECAPACITY, "n = %d faults per window exceeds 65000", n);
    const int nnz = row_ptr[m];
    if (row_ptr[0] != 0 || nnz < 0) return qd_fail(QD_EINVAL, "bad row_ptr");
    std::vector<int> &rdeg = h.rdeg, &cdeg = h.cdeg;
    rdeg.assign(m, 0); cdeg.assign(n, 0);
    for (int i = 0; i < m; ++i) {
        rdeg[i] = row_ptr[i + 1] - row_ptr[i];
        if (rdeg[i] < 0) return qd_fail(QD_EINVAL, "row_ptr not monotone");
        for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            if (col_idx[e] < 0 || col_idx[e] >= n) return qd_fail(QD_EINVAL, "column index out of range");
            if (e > row_ptr[i] && col_idx[e] <= col_idx[e - 1]) return qd_fail(QD_EINVAL, "columns must ascend in a row");
            cdeg[col_idx[e]]++;
        }
    }
    for (int j = 0; j < n; ++j)
        if (!(priors[j] > 0.0 && priors[j] < 1.0)) return qd_fail(QD_EINVAL, "prior %d = %g outside (0,1)", j, priors[j]);
    h.llr0.resize(n);
    for (int j = 0; j < n; ++j) h.llr0[j] = std::log((1.0 - priors[j]) / priors[j]);
    const int max_rdeg = *std::max_element(rdeg.begin(), rdeg.end());
    const int max_cdeg = *std::max_element(cdeg.begin(), cdeg.end());
    if (max_rdeg > QD_MAX_ROW_DEG || max_rdeg < 1)
        return qd_fail(QD_ECAPACITY, "row weight %d outside 1..%d", max_rdeg, QD_MAX_ROW_DEG);
    if (max_cdeg > QD_MAX_COL_DEG || max_cdeg < 1)
        return qd_fail(QD_ECAPACITY, "column weight %d outside 1..%d", max_cdeg, QD_MAX_COL_DEG);
    h.m = m; h.n = n; h.nnz = nnz; h.max_rdeg = max_rdeg; h.max_cdeg = max_cdeg;
    h.min_rdeg = *std::min_element(rdeg.begin(), rdeg.end());
    h.m_pad = pad64(m); h.n_pad = pad64(n); h.max_rdeg_pad = (max_rdeg + 3) & ~3;
    h.row_ptr = row_ptr; h.col_idx = col_idx; h.priors = priors;
    if (h.n_pad + 1 > 65535) return qd_fail(QD_ECAPACITY, "n = %d faults per window: fault slots exceed 16 bits", n);
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

// The shape conditions of the scatter kernel (build_scatter checks the LDS fit and chooses the shape).  1: every check can have a lane of
// its own (one check per lane, or two on half the lanes) and rows hold 2..64 faults (two sign words; a row of one fault has no second minimum) -- also the windows of <= 256 checks,
// 3.78 -> 3.00 ms per launch on the 108-check and 8.92 -> 7.73 ms on the 216-check windows of the W = 3 plans (profiles/r05_scatter_small_ab.txt).
// 2: several checks per lane always: more checks than a workgroup has lanes, or rows of 65..96 faults -- the QLP windows
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
static void build_bp(GraphImage *g, HostGraph &h, bool walk_for_atomics)
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
        g->stage(std::move(bit_orig_u), &bp.bit_orig); g->stage(std::move(slot_of), &bp.bit_slot_of);
        return;
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
    // The scatter kernel (bp_scatter_wide.hip) walks the same order with ds_add_u32, and lanes of one instruction that add to the SAME
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
    std::vector<uint32_t> slot_of(bit_slot_of.begin(), bit_slot_of.end());
    g->stage(std::move(chk_adj32), &bp.chk_adj);
    g->stage(std::move(chk_degp_w), &bp.chk_degp_w);
    g->stage(std::move(chk_orig_u), &bp.chk_orig);
    g->stage(std::move(bit_rec), &bp.bit_rec);
    g->stage(std::move(bit_orig_u), &bp.bit_orig);
    g->stage(std::move(slot_of), &bp.bit_slot_of);
}

// The one-message-per-edge kernels' view (GenGraphDev): CSR / CSC, the serial schedule's levels and its rows' LDS prefix slots
static void build_gen(GraphImage *g, const HostGraph &h)
{
    const int m = h.m, n = h.n, nnz = h.nnz;
    const int32_t *row_ptr = h.row_ptr, *col_idx = h.col_idx;
    const std::vector<int32_t> &cp = h.cp, &ri = h.ri;
    GenGraphDev &gg = g->gen;
    gg.m = m; gg.n = n; gg.nnz = nnz; gg.out_words = (n + 31) / 32;
    std::vector<int32_t> rp_v(row_ptr, row_ptr + m + 1), ci_v(col_idx, col_idx + nnz), c2r(nnz);
    for (int e = 0; e < nnz; ++e) c2r[e] = row_ptr[ri[e]] + h.pos[e];
    const std::vector<float> l0(h.llr0.begin(), h.llr0.end());
    g->stage(std::move(rp_v), &gg.rp); g->stage(std::move(ci_v), &gg.ci);
    g->stage(cp, &gg.cp); g->stage(ri, &gg.ri);
    g->stage(c2r, &gg.c2r); g->stage(l0, &gg.llr0);
    gg.frec = nullptr; gg.erow = nullptr;
    if (h.max_cdeg <= 8 && nnz <= 65534) {
        std::vector<uint16_t> erow(nnz);
        for (int i = 0; i < m; ++i)
            for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) erow[e] = (uint16_t)i;
        g->stage(std::move(erow), &gg.erow);
        std::vector<uint16_t> frec((size_t)n * 16, (uint16_t)0xFFFF);
        for (int j = 0; j < n; ++j)
            for (int e = cp[j]; e < cp[j + 1]; ++e) {
                frec[(size_t)j * 16 + (e - cp[j])] = (uint16_t)c2r[e];
                frec[(size_t)j * 16 + 8 + (e - cp[j])] = (uint16_t)ri[e];
            }
        g->stage(std::move(frec), &gg.frec);
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
        g->stage(std::move(ell), &gg.ell);
    }
    // the records below pack the fault index into 24 bits of their first word (qd_host_graph refuses larger windows long before)
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
    g->stage(std::move(srec), &gg.srec);
}

// Scatter form of the flooding min-sum kernel (bp_scatter_wide.hip; ScatGraphDev): checks in lanes with their state in
// registers, the faults' integer posterior accumulators in LDS.  Taken (sc.ok) for the windows of scatter_form whose accumulators leave
// as many workgroups per CU as the gather kernel's layout does.
static int build_scatter(GraphImage *g, const HostGraph &h, int form, const Switches &env)
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
    if (!walk_ok) return qd_fail(QD_ECAPACITY, "scatter walk: an edge was not placed exactly once below its check's degree");
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
    g->stage(std::move(adjA), &sc.adjA); g->alias(&sc.adjB);
    g->stage(std::move(slot_fault), &sc.slot_fault); g->stage(std::move(k1_slot), &sc.k1_slot);
    g->stage(deg_w, &sc.deg_w); g->stage(h.chk_deg, &sc.chk_deg);
    sc.ok = 1;
    // The shape of qd_bp_scatter_wide_kernel (bp_scatter_wide.hip).  (a) windows with more checks than lanes or rows of three sign
    // words: three checks per lane on 512 lanes (or two on 704 / 1024).  (b) windows with a lane for every check, on HALF the lanes
    // with two checks each: the same number of wavefronts per CU in twice as many workgroups, i.e. half as many wavefronts per
    // barrier -- headline BP 50.3 -> 44.2 ms per 65 536 shots, same bits (profiles/r03x_scatter_cpl2_ab.txt); taken when the LDS
    // holds twice the workgroups.  (c) the rest of (b), and all of it under QD_SCATTER_CPL1=1: one check per lane on bp.threads
    // lanes.  Measured and not kept (profiles/r03x_scatter_shapes2_ab.txt): four checks per lane on a quarter of the lanes
    // (headline 46.2 -> 50.9 ms), 384 lanes x 4 checks for the QLP windows (19.2 -> 24.4 ms).
    sc.wide_threads = shape_threads; sc.wide_cpl = shape_cpl;
    // deal the slot-waves (64 consecutive check slots, heaviest first) to the workgroup's wavefronts so that the largest
    // number of edges a wavefront walks between two barriers is small: each goes to the wavefront with the fewest edges so
    // far that still has a free round (longest-processing-time rule), then single moves / swaps out of the heaviest
    // wavefront while they lower the maximum (QLP windows on 8 wavefronts x 3 rounds: 222 -> 202 edge steps).  With one
    // round there is nothing to balance: every slot-wave gets a wavefront of its own.
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
        if (best < 0 || (int)bins[best].size() >= cpl) return qd_fail(QD_ECAPACITY, "scatter kernel shape does not cover the window");
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
    g->stage(std::move(wmap), &sc.wave_map);
    return QD_OK;
}

// The elimination kernels' view (OsdGraphDev): fault weights, CSC, the LDS layouts of the OSD kernels and the SR kernel's ELL columns
static void build_osd(GraphImage *g, const HostGraph &h)
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
    g->stage(std::move(wfix), &od.wfix);
    g->stage(std::move(csc_ptr), &od.csc_ptr);
    g->stage(std::move(csc_row), &od.csc_row);
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
    // LDS layout (qd_graph_create asks osd_sr.hip for it); taken whenever the mirrored register kernel exists too (it decodes the shots the new kernel hands over)
    od.s_lds_bytes = 0; od.s_per_cu = 0; od.csc_ell = nullptr; od.ell_log2 = 0;
    if (od.f_lds_bytes > 0 && m < 65535) {
        int dl = 1;
        while ((1 << dl) < max_cdeg) ++dl;
        std::vector<uint16_t> ell((size_t)n << dl, (uint16_t)0xFFFFu);
        for (int j = 0; j < n; ++j)
            for (int e = h.cp[j]; e < h.cp[j + 1]; ++e) ell[((size_t)j << dl) + (e - h.cp[j])] = (uint16_t)h.ri[e];
        g->stage(std::move(ell), &od.csc_ell);
        od.ell_log2 = dl;
    }
    // the full kernel sorts all n columns in LDS; windows too large for that rely on the register kernel alone
    if (od.lds_bytes == 0 && od.f_lds_bytes == 0) od.threads = 0;
}

int qd_layout_graph(HostGraph &h, const Switches &env, GraphImage *g)
{
    const int form = scatter_form(h);
    build_bp(g, h, form != 0);
    build_gen(g, h);
    if (int rc = build_scatter(g, h, g->off_chip ? 0 : form, env)) return rc;
    build_osd(g, h);
    g->h_cp = h.cp; g->h_ri = h.ri; g->h_llr0 = h.llr0;
    return QD_OK;
}
