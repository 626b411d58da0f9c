// qd_graph.hip -- qd_graph_*: a window's graph on the device (laid out by graph_layout.hip, uploaded here), and the library's version and error message.
#include "qd_host.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>

static thread_local char g_err[512] = "";

int qd_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" int qd_version(void) { return 118; }      // 118: qd_bit_planes, qd_calib_create, qd_calib_destroy, qd_calib_info, qd_parity_counts (fitting priors to detector samples, calibrate.hip); 117: qd_isd_create, qd_isd_destroy, qd_isd_info, qd_isd_run, qd_isd_hist, qd_isd_reset (the random information-set estimate of the distance, distance.hip); 116: qd_soft_fold, qd_soft_weigh, qd_soft_tally (soft outputs per shot, soft.hip); 115: qd_search_create, qd_search_destroy, qd_search_reset, qd_search_seed, qd_search_level, qd_search_counters, qd_search_found, qd_search_chain (the search for undetectable logical faults, logical_search.hip); 114: qd_shrink_begin, qd_shrink_step (shrinking failing fault sets, shrink.hip); 113: qd_decoder_relay_info, QD_RELAY_FLAG_MARGINALS_DEVICE (Relay-BP with its marginals in device memory, bp_relay_device.hip); 112: qd_decoder_create_relay (Relay-BP, bp_relay.hip); 111: qd_strata_create, qd_strata_destroy, qd_strata_info, qd_sample_dem_strata (stratified DEM sampling, strata_sampler.hip); 110: qd_sample_dem_faults, qd_commit_bits, qd_fault_stats_batch (fault-level outputs, faults.hip); 109: qd_unpack_b8, qd_pack_b8 (Stim's bit-packed samples, bitpack.hip); 108: qd_shot_flags_fold, qd_tally_batch, qd_sample_circuit_shots, qd_sample_dem_shots (the device-resident memory experiment); 107: off-chip windows decode (qd_graph_create used to refuse them), QD_FLAG_OFF_CHIP, QD_POST_OSD0_OFFCHIP (no new export); 106: qd_circuit_create takes Y_ERROR / PAULI_CHANNEL_1 / PAULI_CHANNEL_2 programs (no new export); 105: qd_decoder_fast_start; 104: qd_circuit_* and qd_sample_circuit; 103: qd_decoder_post_head_start; 102: qd_graph_info fills 10 entries again, qd_graph_info_ex(g, info, n) the rest; 101: qd_decoder_postproc_kernel
extern "C" const char *qd_last_error(void) { return g_err; }
extern "C" int qd_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int qd_graph_create(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                               const double *priors, int32_t device, qd_graph **out)
{
    if (!out) return qd_fail(QD_EINVAL, "out is null");
    *out = nullptr;
    HostGraph h;
    if (int rc = qd_host_graph(m, n, row_ptr, col_idx, priors, h)) return rc;
    std::unique_ptr<qd_graph> g(new qd_graph());      // (~qd_graph frees what has been uploaded)
    g->device = device; g->m = m; g->n = n; g->nnz = h.nnz; g->max_rdeg = h.max_rdeg; g->max_cdeg = h.max_cdeg;
    if (hipSetDevice(device) != hipSuccess) return qd_fail(QD_EHIP, "hipSetDevice(%d) failed", device);
    if (int rc = qd_layout_graph(h, qd_read_switches(), g.get())) return rc;
    // the staged arrays, in staging order; each pointer member of the views takes its array's device address
    GraphImage *img = g.get();
    for (GraphImage::Staged &a : img->staged) {
        void *dev = g->mem.upload(a.data, a.size);
        if (!dev) return qd_fail(QD_EHIP, "device allocation/upload failed");
        for (size_t f : a.fields) std::memcpy(reinterpret_cast<unsigned char *>(img) + f, &dev, sizeof(dev));
        a.owner.reset();
    }
    img->staged.clear();
    // The kernels' own LDS layouts stay with their kernels.  OSD-0 with simultaneous singleton pivots (osd_sr.hip) is taken whenever its ELL
    // columns were made, i.e. whenever the mirrored register kernel exists too (it decodes the shots the new kernel hands over)
    OsdGraphDev &od = g->osd;
    if (od.csc_ell) {
        const int lds = qd_osd_sr_layout(m, od.m_pad, n, g->bp.out_words, od.s_off, &od.s_threads, &od.s_rpt);
        if (lds > 0 && lds <= QD_LDS_BYTES) {
            od.s_lds_bytes = lds;
            od.s_per_cu = std::max(1, std::min(QD_LDS_BYTES / lds, qd_sr_wps(od.s_rpt) * 256 / od.s_threads));   // the kernel's register budget (wavefronts per SIMD)
        }
    }
    g->x_lds = qd_osd_offchip_layout(m, n, h.max_cdeg, g->x_off, &g->x_off_sort, &g->x_off_order, &g->x_kw, &g->x_threads, &g->x_per_cu);
    *out = g.release();
    return QD_OK;
}

extern "C" void qd_graph_destroy(qd_graph *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    delete g;
}

int qd_host_rank(qd_graph *g)
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
    // [12], [13]: lanes and checks per lane of qd_bp_scatter_wide_kernel's instantiation for this window (0, 0: no scatter kernel)
    const int32_t v[14] = {g->m, g->n, g->nnz, g->max_rdeg, g->max_cdeg, g->bp.threads, g->bp.lds_bytes, g->osd.threads, g->osd.lds_bytes,
                           n_entries > 9 ? qd_host_rank(const_cast<qd_graph *>(g)) : 0, (int32_t)g->sc_walk_cycles, (int32_t)g->sc_walk_ideal,
                           g->sc.wide_threads, g->sc.wide_cpl};
    for (int i = 0; i < n_entries && i < 14; ++i) info[i] = v[i];
    for (int i = 14; i < n_entries; ++i) info[i] = 0;
}

extern "C" int qd_graph_info(const qd_graph *g, int32_t *info)
{
    if (!g || !info) return qd_fail(QD_EINVAL, "null argument");
    graph_info_fill(g, info, 10);
    return QD_OK;
}

extern "C" int qd_graph_info_ex(const qd_graph *g, int32_t *info, int32_t n_entries)
{
    if (!g || !info || n_entries < 0) return qd_fail(QD_EINVAL, "null argument or negative n_entries");
    graph_info_fill(g, info, n_entries);
    return QD_OK;
}
