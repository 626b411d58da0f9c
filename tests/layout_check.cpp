// layout_check.cpp -- lays out one window with quits_amd/csrc/graph_layout.hip and checks what the kernels rely on.  No device, no Python:
// tests/test_graph_layout.py builds it with the address and undefined-behaviour sanitizers and runs it once per window.
//   layout_check WINDOW [DUMP]    WINDOW: int32 m, n, nnz, row_ptr[m + 1], col_idx[nnz], double priors[n]
//                                 DUMP:   every staged array, then the views bp, gen, sc, osd, each as uint64 size + bytes
#include "../quits_amd/csrc/graph_layout.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>

int qd_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return code;
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "layout_check:%d: %s\n", __LINE__, #c); return 1; } } while (0)

// the staged array a pointer member of the image will point at (null: none was staged)
static const GraphImage::Staged *staged_for(const GraphImage &g, const void *field)
{
    for (const GraphImage::Staged &a : g.staged)
        if (std::count(a.fields.begin(), a.fields.end(), g.offset_of(field))) return &a;
    return nullptr;
}
template <class Tp, class Fp> static std::vector<Tp> arr(const GraphImage &g, Fp *const *field)
{
    const GraphImage::Staged *a = staged_for(g, field);
    std::vector<Tp> v(a ? a->size / sizeof(Tp) : 0);
    if (a && !v.empty()) std::memcpy(v.data(), a->data, v.size() * sizeof(Tp));
    return v;
}

// an LDS carve-up of {offset, bytes the kernel puts there}: 16-byte aligned, ascending, no region reaching into the next, inside `total`, which fits the CU
using Regions = std::vector<std::pair<int, int>>;
static bool carve(const Regions &regions, int total)
{
    int end = 0;
    for (const auto &r : regions) { if (r.first % 16 || r.first < end || r.second < 0) return false; end = r.first + r.second; }
    return end <= total && total <= QD_LDS_BYTES;
}

static int check(const HostGraph &h, const GraphImage &g)
{
    const BpGraphDev &bp = g.bp;
    const int m = h.m, n = h.n, m_pad = bp.m_pad, n_pad = bp.n_pad;
    // ---- slot orders: permutations with matching inverses, degree non-increasing
    const auto bit_orig = arr<uint32_t>(g, &bp.bit_orig), slot_of = arr<uint32_t>(g, &bp.bit_slot_of);
    CHECK((int)bit_orig.size() == n_pad && (int)slot_of.size() == n);
    for (int s = 0; s < n; ++s) CHECK((int)bit_orig[s] < n && (int)slot_of[bit_orig[s]] == s && (s == 0 || h.cdeg[bit_orig[s - 1]] >= h.cdeg[bit_orig[s]]));
    if (g.off_chip) {
        CHECK(bp.threads == 0 && bp.lds_bytes == 0 && g.sc.ok == 0 && arr<uint32_t>(g, &bp.chk_adj).empty());
    } else {
        const auto chk_orig = arr<uint32_t>(g, &bp.chk_orig), adj = arr<uint32_t>(g, &bp.chk_adj), rec = arr<uint32_t>(g, &bp.bit_rec);
        std::vector<int> chk_slot(m, -1);
        CHECK((int)chk_orig.size() == m_pad);
        for (int s = 0; s < m; ++s) {
            CHECK((int)chk_orig[s] < m && chk_slot[chk_orig[s]] < 0 && (s == 0 || h.rdeg[chk_orig[s - 1]] >= h.rdeg[chk_orig[s]]));
            chk_slot[chk_orig[s]] = s;
        }
        CHECK(carve({{bp.off_chk, (m_pad + 4) * 16}, {bp.off_cneg, bp.sign_mode == 2 ? (bp.neg_words - 1) * m_pad * 4 : 0}, {bp.off_llr, (n_pad + 4) * 4},   // + the dummy check, + the dummy bit
                     {bp.off_out, bp.out_words * 4}, {bp.off_misc, 256}}, bp.lds_bytes) && bp.off_misc + 256 == bp.lds_bytes);
        // ---- chk_adj: a check's faults' posterior offsets at the steps below its degree, the dummy bit everywhere else
        const uint32_t dummy = (uint32_t)(bp.off_llr + bp.dummy_bit * 4);
        CHECK(adj.size() == (size_t)bp.max_rdeg_pad * m_pad);
        for (int s = 0; s < m_pad; ++s) {
            const int i = s < m ? (int)chk_orig[s] : -1, deg = s < m ? h.rdeg[i] : 0;
            std::set<uint32_t> want, got;
            for (int e = 0; e < deg; ++e) want.insert((uint32_t)bp.off_llr + slot_of[h.col_idx[h.row_ptr[i] + e]] * 4u);
            for (int k = 0; k < bp.max_rdeg_pad; ++k) {
                const uint32_t a = adj[((size_t)(k >> 2) * m_pad + s) * 4 + (k & 3)];
                if (k < deg) got.insert(a); else CHECK(a == dummy);
            }
            CHECK(got == want);
        }
        // ---- fault records: the checks' state offsets, sign positions distinct within a check and inside the sign words of the mode
        auto rec_at = [&](int s, int w) { return rec[((size_t)(w >> 2) * n_pad + s) * 4 + (w & 3)]; };
        std::vector<std::set<uint32_t>> signs(m);
        CHECK(rec.size() == (size_t)n_pad * bp.rec_words && bp.rec_words % 4 == 0 && bp.rec_words > h.max_cdeg);
        const auto degp_w = arr<int32_t>(g, &bp.chk_degp_w);
        CHECK((int)degp_w.size() == m_pad / 64 && bp.neg_words == (bp.max_rdeg_pad + 31) / 32);
        for (int w0 = 0; w0 < m_pad; w0 += 64) {            // trip count of a wavefront: its largest degree (slots descend) rounded up to 4 | that degree
            const int mx = w0 < m ? h.rdeg[chk_orig[w0]] : 0;
            CHECK(degp_w[w0 / 64] == (((mx + 3) & ~3) | (mx << 16)));
        }
        for (int s = 0; s < n_pad; ++s) {
            const int j = s < n ? (int)bit_orig[s] : -1, deg = s < n ? h.cdeg[j] : 0;
            const float l0 = s < n ? (float)h.llr0[j] : 1.0f;
            CHECK(std::memcmp(&l0, &rec[(size_t)s * 4], 4) == 0);
            for (int q = 0; q < bp.rec_words - 1; ++q) {
                const uint32_t r = rec_at(s, 1 + q), where = r & 0xFFFFu;
                if (q >= deg) { CHECK(r == (uint32_t)(bp.off_chk + bp.dummy_chk * 16) << 16); continue; }
                const int i = h.ri[h.cp[j] + q];
                CHECK((int)(r >> 16) == bp.off_chk + chk_slot[i] * 16 && signs[i].insert(where).second);
                CHECK(bp.sign_mode == 2 ? (int)(where >> 5) < bp.neg_words : (where < 32 || (bp.sign_mode == 1 && where >= 48 && where < 63)));
                // the sign sits where the check pass puts it: step k of the walk lands on bit kend - 1 - (k & 31) of word k >> 5 (kend = the word's
                // share of the wavefront's trip count), and step k of this check's walk is this fault -- in every sign word and every record slot
                const int w = bp.sign_mode == 2 ? (int)(where >> 5) : (where < 32 ? 0 : 1), bit = bp.sign_mode == 2 ? (int)(where & 31u) : (int)(where < 32 ? where : where - 48);
                const int kend = std::min((degp_w[chk_slot[i] / 64] & 0xFFFF) - 32 * w, 32), k = 32 * w + kend - 1 - bit;
                CHECK(bit < kend && k >= 0 && k < h.rdeg[i] && adj[((size_t)(k >> 2) * m_pad + chk_slot[i]) * 4 + (k & 3)] == (uint32_t)bp.off_llr + (uint32_t)s * 4u);
                CHECK(s < bp.bit_thr[q]);                   // the bit pass reads record slot q of this fault's wavefront
            }
        }
        for (int i = 0; i < m; ++i) CHECK((int)signs[i].size() == h.rdeg[i]);
        for (int q = 0; q < QD_MAX_COL_DEG; ++q) CHECK(bp.bit_thr[q] % 64 == 0 && bp.bit_thr[q] <= n_pad && (q == 0 || bp.bit_thr[q] <= bp.bit_thr[q - 1]));
    }
    // ---- the per-edge view: c2r, every fault once in srec, faults of a check in index order on rising levels, prefix slots
    const GenGraphDev &gg = g.gen;
    const auto c2r = arr<int32_t>(g, &gg.c2r);
    const auto srec = arr<uint32_t>(g, &gg.srec);
    CHECK((int)c2r.size() == h.nnz && (arr<uint16_t>(g, &gg.frec).empty() || h.max_cdeg <= 8));
    for (int j = 0; j < n; ++j)
        for (int e = h.cp[j]; e < h.cp[j + 1]; ++e)
            CHECK(c2r[e] >= h.row_ptr[h.ri[e]] && c2r[e] < h.row_ptr[h.ri[e] + 1] && h.col_idx[c2r[e]] == j);
    const int G = QD_GEN_GS, D = qd_gen_unroll(h.max_cdeg), RW = gg.srec_w;
    std::vector<int> level(n, -1), first(m, 1 << 30), last(m, -1), slot(m, -1);
    int lev = 0;
    CHECK(RW >= 2 + 2 * D && srec.size() == (size_t)gg.nstep * G * RW && gg.nslots * 256 <= QD_GEN_PREFIX_LDS);
    for (int st = 0; st < gg.nstep; ++st) {
        const uint32_t bar = srec[(size_t)st * G * RW] >> 31;
        for (int wv = 0; wv < G; ++wv) {
            const uint32_t *r = &srec[((size_t)st * G + wv) * RW];
            const int j = (int)(r[0] & 0xFFFFFFu), deg = (int)(r[0] >> 24) & 0x7F;
            CHECK(r[0] >> 31 == bar);                       // one barrier decision per step ...
            if (!deg) continue;
            CHECK(j < n && level[j] < 0 && deg == h.cdeg[j]);
            level[j] = lev;
            for (int k = 0; k < deg; ++k) {
                const int i = (int)(r[2 + k] & (gg.nslots ? 0x7FFFFFu : 0xFFFFFFFFu));
                CHECK(i == h.ri[h.cp[j] + k] && (int)r[2 + D + k] == c2r[h.cp[j] + k]);
                CHECK(last[i] < lev);                       // (faults come in index order: an earlier fault of this check sits on a lower level)
                first[i] = std::min(first[i], lev); last[i] = lev;
                if (gg.nslots) { CHECK(slot[i] < 0 || slot[i] == (int)(r[2 + k] >> 24)); slot[i] = (int)(r[2 + k] >> 24); CHECK(slot[i] < gg.nslots); }
            }
        }
        lev += (int)bar;
        CHECK(st + 1 < gg.nstep || bar);                    // ... and the last step of the last level carries it
    }
    CHECK(lev == gg.nlev && std::count(level.begin(), level.end(), -1) == 0);
    for (int i = 0; i < m; ++i)                             // index order within a check = rising levels
        for (int e = h.row_ptr[i] + 1; e < h.row_ptr[i + 1]; ++e) CHECK(level[h.col_idx[e - 1]] < level[h.col_idx[e]]);
    std::map<int, std::vector<std::pair<int, int>>> owners;
    for (int i = 0; i < m && gg.nslots; ++i) owners[slot[i]].push_back({first[i], last[i]});
    for (auto &o : owners) {
        std::sort(o.second.begin(), o.second.end());
        for (size_t x = 1; x < o.second.size(); ++x) CHECK(o.second[x - 1].second < o.second[x].first);
    }
    // ---- the scatter view
    const ScatGraphDev &sc = g.sc;
    if (sc.ok) {
        const auto chk_orig = arr<uint32_t>(g, &bp.chk_orig), adjA = arr<uint32_t>(g, &sc.adjA), slot_fault = arr<uint32_t>(g, &sc.slot_fault), k1 = arr<uint32_t>(g, &sc.k1_slot);
        const int rows = bp.max_rdeg_pad / 4 + 2, trash = sc.nslots - 32;
        CHECK(staged_for(g, &sc.adjB) == staged_for(g, &sc.adjA) && sc.nslots % 4 == 0 && sc.offA == 0 && sc.offB == 0);
        CHECK(carve({{sc.offA, sc.nslots * 4}, {sc.off_out, bp.out_words * 4}, {sc.off_misc, 256}}, sc.lds_bytes));
        CHECK((int)slot_fault.size() == sc.nslots && (int)k1.size() == n && adjA.size() == (size_t)rows * m_pad * 4);
        CHECK(std::count(slot_fault.begin(), slot_fault.end(), 0xFFFFFFFFu) == sc.nslots - n);
        for (int b = 0; b < n; ++b) CHECK((int)k1[b] < trash && slot_fault[k1[b]] == bit_orig[b] && (int)k1[b] == g.h_sc_slot[bit_orig[b]]);
        for (int s = 0; s < m_pad; ++s) {
            const int i = s < m ? (int)chk_orig[s] : -1, deg = s < m ? h.rdeg[i] : 0;
            std::multiset<uint32_t> want, got;
            for (int e = 0; e < deg; ++e) want.insert(k1[slot_of[h.col_idx[h.row_ptr[i] + e]]] * 4u);
            for (int k = 0; k < rows * 4; ++k) {
                const uint32_t a = adjA[((size_t)(k >> 2) * m_pad + s) * 4 + (k & 3)];
                CHECK(a % 4 == 0 && (int)a < sc.nslots * 4);
                if (k < deg) got.insert(a); else CHECK((int)a / 4 >= trash);
            }
            CHECK(got == want);
        }
        const auto wmap = arr<int32_t>(g, &sc.wave_map);
        CHECK(wmap.size() == (size_t)sc.wide_cpl * (sc.wide_threads / 64));
        for (int sw = 0; sw < m_pad / 64; ++sw) CHECK(std::count(wmap.begin(), wmap.end(), sw) == 1);
        for (int32_t x : wmap) CHECK(x >= -1 && x < m_pad / 64);
    }
    // ---- the elimination kernels' carve-ups (the s_* layout of osd_sr.hip is not here: qd_graph_create asks that kernel file for it after this layout)
    const OsdGraphDev &od = g.osd;
    // Q (the sort buffer of the full kernel shares it), tb, sp, rowpiv, prow, pcol, pairs, cols, red, out; then the register kernels' tier sort buffer and order
    auto osd = [&](const int *o, int qbytes, Regions more) {
        Regions r = {{o[0], qbytes}, {o[1], m_pad * 8}, {o[2], m_pad}, {o[3], m_pad * 2}, {o[4], m_pad * 2}, {o[5], m_pad * 4}, {o[6], 64 * od.max_cdeg * 4}, {o[7], 256}, {o[8], 1024}, {o[9], bp.out_words * 4}};
        r.insert(r.end(), more.begin(), more.end());
        return r;
    };
    CHECK(!od.lds_bytes || carve(osd(od.off, std::max(od.npow2 * 8, od.kw_lds * m_pad * 8), {}), od.lds_bytes));
    CHECK(!od.f_lds_bytes || carve(osd(od.f_off, od.f_kw * m_pad * 8, {{od.f_off_sort, 1024 * 8}, {od.f_off_order, 1024 * 2}}), od.f_lds_bytes));
    CHECK(!od.w_lds_bytes || carve(osd(od.w_off, od.w_kw * m_pad * 8, {{od.w_off_sort, 1024 * 8}, {od.w_off_order, 1024 * 2}, {od.w_off_pivmask, bp.out_words * 4}, {od.w_off_npl, 256}}), od.w_lds_bytes));
    return 0;
}

int main(int argc, char **argv)
{
    FILE *fp = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    int32_t hd[3];
    if (!fp || fread(hd, 4, 3, fp) != 3 || hd[0] < 0 || hd[1] < 0 || hd[2] < 0) return qd_fail(2, "usage: layout_check WINDOW [DUMP]");
    std::vector<int32_t> rp((size_t)hd[0] + 1), ci((size_t)hd[2]);
    std::vector<double> pri((size_t)hd[1]);
    if (fread(rp.data(), 4, rp.size(), fp) != rp.size() || fread(ci.data(), 4, ci.size(), fp) != ci.size() || fread(pri.data(), 8, pri.size(), fp) != pri.size())
        return qd_fail(2, "short window file");
    fclose(fp);
    HostGraph h;
    GraphImage g;
    if (qd_host_graph(hd[0], hd[1], rp.data(), ci.data(), pri.data(), h) || qd_layout_graph(h, qd_read_switches(), &g)) return 3;
    if (argc > 2) {
        FILE *out = fopen(argv[2], "wb");
        auto put = [&](const void *p, uint64_t bytes) { return out && fwrite(&bytes, 8, 1, out) == 1 && (!bytes || fwrite(p, 1, bytes, out) == bytes); };
        bool ok = true;
        for (const GraphImage::Staged &a : g.staged) ok = ok && put(a.data, a.size);
        ok = ok && put(&g.bp, sizeof(g.bp)) && put(&g.gen, sizeof(g.gen)) && put(&g.sc, sizeof(g.sc)) && put(&g.osd, sizeof(g.osd));
        if (!ok || fclose(out)) return qd_fail(2, "cannot write the dump");
    }
    printf("off_chip=%d sign_mode=%d threads=%d sc_ok=%d wide_threads=%d wide_cpl=%d frec=%d unroll=%d nslots=%d min_rdeg=%d walk=%lld/%lld\n", (int)g.off_chip, g.bp.sign_mode,
           g.bp.threads, g.sc.ok, g.sc.wide_threads, g.sc.wide_cpl, (int)(staged_for(g, &g.gen.frec) != nullptr), qd_gen_unroll(h.max_cdeg), g.gen.nslots, h.min_rdeg,
           g.sc_walk_cycles, g.sc_walk_ideal);
    return check(h, g);
}
