// qd_decoder.hip -- qd_decoder_*: which kernels a decoder runs (chosen once, at creation), its workspace, and the two stages of a decode call.
#include "qd_host.h"

#include <cmath>
#include <cstring>

#define QD_GRID_MIN_BITS 10

extern "C" int qd_decoder_create(const qd_graph *g, const qd_params *p, qd_decoder **out)
{
    if (!g || !p || !out) return qd_fail(QD_EINVAL, "null argument");
    *out = nullptr;
    if (p->bp_method != QD_BP_MINIMUM_SUM && p->bp_method != QD_BP_PRODUCT_SUM) return qd_fail(QD_EINVAL, "unknown bp_method %d", p->bp_method);
    if (p->schedule != QD_SCHEDULE_PARALLEL && p->schedule != QD_SCHEDULE_SERIAL) return qd_fail(QD_EINVAL, "unknown schedule %d", p->schedule);
    if (p->reserved & ~(QD_FLAG_EDGE_MESSAGES | QD_FLAG_RAW_LLR | QD_FLAG_OFF_CHIP)) return qd_fail(QD_EINVAL, "unknown flag bits 0x%x", p->reserved);
    const bool lsd = p->osd_method == QD_LSD_0 || p->osd_method == QD_LSD_E || p->osd_method == QD_LSD_CS;
    if (lsd && p->osd_order < 0) return qd_fail(QD_EINVAL, "negative lsd_order");
    const bool off_chip = g->off_chip || (p->reserved & QD_FLAG_OFF_CHIP);
    if (off_chip && lsd)
        return qd_fail(QD_EUNSUPPORTED, "BP-LSD is not implemented for the off-chip window %d x %d%s", g->m, g->n, g->off_chip ? "" : " (QD_FLAG_OFF_CHIP)");
    if (p->osd_method == QD_LSD_CS && p->osd_order > 64)
        return qd_fail(QD_EUNSUPPORTED, "lsd_cs: lsd_order %d > 64 is not implemented on the device path", p->osd_order);
    if (p->osd_method == QD_LSD_E && p->osd_order > 15)
        return qd_fail(QD_EUNSUPPORTED, "lsd_e: lsd_order %d > 15 is not implemented on the device path", p->osd_order);
    if (lsd && qd_lsd_lds_bytes(g->m, g->n, g->bp.out_words) > QD_LDS_BYTES)
        return qd_fail(QD_ECAPACITY, "window %d x %d does not fit the LSD kernel's LDS layout", g->m, g->n);
    const bool osd0 = lsd || p->osd_method == QD_OSD_0 || ((p->osd_method == QD_OSD_CS || p->osd_method == QD_OSD_E) && p->osd_order == 0);
    if (p->osd_method != QD_OSD_OFF && !osd0) {
        if (p->osd_method != QD_OSD_CS && p->osd_method != QD_OSD_E) return qd_fail(QD_EINVAL, "unknown osd_method %d", p->osd_method);
        if (p->osd_order < 0) return qd_fail(QD_EINVAL, "negative osd_order");
        if (off_chip)
            return qd_fail(QD_EUNSUPPORTED, "osd_cs / osd_e of order %d are not implemented for the off-chip window %d x %d%s (order 0 is)", p->osd_order, g->m,
                        g->n, g->off_chip ? "" : " (QD_FLAG_OFF_CHIP)");
        if (g->osd.w_lds_bytes == 0)
            return qd_fail(QD_EUNSUPPORTED, "osd_cs / osd_e need the register OSD kernel, which this window (%d detectors) does not fit", g->m);
        if (p->osd_method == QD_OSD_CS && p->osd_order > 64)
            return qd_fail(QD_EUNSUPPORTED, "osd_cs: osd_order %d > 64 is not implemented on the device path", p->osd_order);
        if (p->osd_method == QD_OSD_E && p->osd_order > 15)
            return qd_fail(QD_EUNSUPPORTED, "osd_e: osd_order %d > 15 is not implemented on the device path", p->osd_order);
    }
    if (p->osd_method != QD_OSD_OFF && off_chip && g->x_lds == 0)
        return qd_fail(QD_ECAPACITY, "off-chip window %d x %d: the row state of the OSD-0 kernel (17 bytes per detector) does not fit the CU's LDS", g->m, g->n);
    if (p->osd_method != QD_OSD_OFF && !lsd && !off_chip && g->osd.lds_bytes == 0 && g->osd.f_lds_bytes == 0)
        return qd_fail(QD_ECAPACITY, "window %d x %d does not fit either OSD kernel's LDS layout", g->m, g->n);
    if (p->max_iter < 0 || p->ms_scaling_factor < 0) return qd_fail(QD_EINVAL, "negative max_iter / ms_scaling_factor");
    const Switches env = qd_read_switches();
    qd_decoder *d = new qd_decoder();
    d->g = g; d->prm = *p; d->off_chip = off_chip;
    d->lsd_w = (lsd && p->osd_order > 0) ? (p->osd_method == QD_LSD_CS ? 1 : (p->osd_method == QD_LSD_E ? 2 : 0)) : 0;
    d->osd_w = osd0 || p->osd_method == QD_OSD_OFF ? 0 : (p->osd_method == QD_OSD_CS ? 1 : 2);
    if (d->osd_w) qd_host_rank(const_cast<qd_graph *>(g));     // the sweep needs the complete factorisation: rank pivots
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
        if (hipSetDevice(g->device) != hipSuccess) { delete d; return qd_fail(QD_EHIP, "hipSetDevice(%d) failed", g->device); }
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
            // certifies a run (bp_scatter_wide.hip): max|prior| + max_cdeg * max min2 < 2^23
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
                d->bp = BP_SCATTER_WIDE;
                if (!env.bp_no_fast_start && rc == 0) {
                    // gather pass 0 does not depend on the shot: made here once, on the device, by the kernel's own walk (bp_scatter_wide.hip)
                    const std::vector<uint32_t> zero((size_t)g->bp.m_pad * 8, 0u);
                    rc |= d->mem.upload(zero, &d->first_pass);
                    if (rc == 0 && (qd_launch_bp_first_pass(d->bp_fine, g->sc, d->prior_g, const_cast<uint32_t *>(d->first_pass), nullptr) != hipSuccess ||
                                    hipStreamSynchronize(nullptr) != hipSuccess))
                        rc = -1;
                }
            }
        }
        if (rc) { d->mem.release(); delete d; return qd_fail(QD_EHIP, "device allocation failed while building the LLR grid"); }
    }
    *out = d;
    return QD_OK;
}

// Relay-BP: the decoder qd_decoder_create makes for flooding min-sum on float LLRs (its post-processor, workspace and stage 2 as they are), with
// qd_bp_relay_kernel as its stage 1
extern "C" int qd_decoder_create_relay(const qd_graph *g, const qd_params *p, const qd_relay_params *r, const float *gammas, qd_decoder **out)
{
    if (!g || !p || !r || !out) return qd_fail(QD_EINVAL, "null argument");
    *out = nullptr;
    if (p->bp_method != QD_BP_MINIMUM_SUM || p->schedule != QD_SCHEDULE_PARALLEL)
        return qd_fail(QD_EINVAL, "Relay-BP is flooding min-sum: bp_method %d / schedule %d are not QD_BP_MINIMUM_SUM / QD_SCHEDULE_PARALLEL", p->bp_method, p->schedule);
    if (p->reserved != 0 || (r->reserved & ~QD_RELAY_FLAG_MARGINALS_DEVICE))
        return qd_fail(QD_EINVAL, "Relay-BP takes no flag bits but QD_RELAY_FLAG_MARGINALS_DEVICE in qd_relay_params (0x%x, 0x%x)", p->reserved, r->reserved);
    if (r->pre_iter < 1 || r->set_max_iter < 1 || r->stop_nconv < 1 || r->num_sets < 0 || r->num_sets > (QD_STATUS_RELAY_LEG_MASK >> QD_STATUS_RELAY_LEG_SHIFT))
        return qd_fail(QD_EINVAL, "relay budgets out of range: pre_iter %d, num_sets %d, set_max_iter %d, stop_nconv %d", r->pre_iter, r->num_sets, r->set_max_iter, r->stop_nconv);
    const long long total = (long long)r->pre_iter + (long long)r->num_sets * r->set_max_iter;
    if (total > QD_STATUS_ITER_MASK) return qd_fail(QD_EINVAL, "%lld iterations over all legs exceed the status word's %d", total, QD_STATUS_ITER_MASK);
    if (r->num_sets > 0 && !gammas) return qd_fail(QD_EINVAL, "num_sets = %d without a gamma table", r->num_sets);
    const auto bad_gamma = [](float v) { return !std::isfinite(v) || std::fabs(v) >= 1.5f; };
    if (bad_gamma(r->gamma0)) return qd_fail(QD_EINVAL, "gamma0 = %g: memory strengths must be finite with |gamma| < 1.5", (double)r->gamma0);
    for (size_t i = 0; i < (size_t)r->num_sets * g->n; ++i)
        if (bad_gamma(gammas[i])) return qd_fail(QD_EINVAL, "gammas[%zu][%zu] = %g: memory strengths must be finite with |gamma| < 1.5", i / g->n, i % g->n, (double)gammas[i]);
    RelayArgs x{};
    x.pre_iter = r->pre_iter; x.num_sets = r->num_sets; x.set_max_iter = r->set_max_iter; x.stop_nconv = r->stop_nconv; x.gamma0 = r->gamma0;
    if (g->off_chip)
        return qd_fail(QD_ECAPACITY, "Relay-BP keeps a shot's state in LDS: the off-chip window %d x %d (16 bytes per detector + 8 per fault > %d) does not fit", g->m,
                       g->n, QD_LDS_BYTES);
    // the form: marginals in LDS wherever that fits (unless QD_RELAY_FLAG_MARGINALS_DEVICE), else in a device-memory workspace
    const int lds_form = qd_relay_layout(g->bp, false, &x);
    const bool marg_device = (r->reserved & QD_RELAY_FLAG_MARGINALS_DEVICE) != 0 || lds_form > QD_LDS_BYTES;
    if (qd_relay_layout(g->bp, marg_device, &x) > QD_LDS_BYTES)
        return qd_fail(QD_ECAPACITY, "Relay-BP state of window %d x %d: %d bytes of LDS with the marginals in LDS, %d with them in device memory (%d of either the "
                       "min-sum layout), the CU has %d", g->m, g->n, lds_form, x.lds_bytes, g->bp.lds_bytes, QD_LDS_BYTES);
    qd_params q = *p;
    q.reserved = QD_FLAG_RAW_LLR;                        // float LLRs as they are: no grid, nothing certified
    q.max_iter = (int32_t)total;
    qd_decoder *d = nullptr;
    if (int rc = qd_decoder_create(g, &q, &d)) return rc;
    std::vector<float> slot((size_t)std::max(1, r->num_sets) * g->bp.n_pad, 0.f);
    for (int s = 0; s < r->num_sets; ++s)
        for (int b = 0; b < g->n; ++b) slot[(size_t)s * g->bp.n_pad + b] = gammas[(size_t)s * g->n + g->h_bit_orig[b]];
    if (hipSetDevice(g->device) != hipSuccess || d->mem.upload(slot, &x.gammas)) {
        qd_decoder_destroy(d);
        return qd_fail(QD_EHIP, "device allocation failed for the gamma table");
    }
    d->bp = BP_RELAY;
    d->relay = x;
    d->relay_marg_device = marg_device;
    d->relay_lds_form = lds_form;
    *out = d;
    return QD_OK;
}

extern "C" int qd_decoder_relay_info(const qd_decoder *d, int32_t *info)
{
    if (!d || !info) return qd_fail(QD_EINVAL, "null argument");
    const bool relay = d->bp == BP_RELAY;
    info[0] = relay ? (d->relay_marg_device ? 2 : 1) : 0;
    info[1] = relay ? d->relay.lds_bytes : 0;
    info[2] = relay ? d->relay_lds_form : 0;
    info[3] = QD_LDS_BYTES;
    return QD_OK;
}

extern "C" int qd_decoder_info(const qd_decoder *d, int32_t *info)
{
    if (!d || !info) return qd_fail(QD_EINVAL, "null argument");
    info[0] = d->grid_k; info[1] = d->grid_kc; info[2] = d->bp == BP_LDS_EDGE || d->bp == BP_HBM_EDGE;
    info[3] = d->bp == BP_SCATTER_WIDE ? (d->g->sc.wide_cpl > 1 ? 2 : 1) : 0;
    return QD_OK;
}

extern "C" int qd_decoder_fast_start(const qd_decoder *d) { return d ? (d->first_pass != nullptr && d->prm.max_iter >= 1) : -1; }

extern "C" int qd_decoder_postproc_kernel(const qd_decoder *d) { return d ? d->post : -1; }

static void free_ws(qd_decoder *d)
{
    Workspace &ws = d->ws;
    ws.dev.release();
    if (ws.host_fail) (void)hipHostFree(ws.host_fail);
    if (ws.gsp.host_counts) (void)hipHostFree(ws.gsp.host_counts);
    if (ws.fail_ready) (void)hipEventDestroy(ws.fail_ready);
    if (ws.gsp.counts_ready) (void)hipEventDestroy(ws.gsp.counts_ready);
    ws = Workspace{};
    d->cap = 0;
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
    if (!d || max_batch <= 0) return qd_fail(QD_EINVAL, "bad reserve request");
    if (max_batch <= d->cap) return QD_OK;
    HIP_TRY(hipSetDevice(d->g->device));
    HIP_TRY(hipDeviceSynchronize());
    free_ws(d);
    const qd_graph *g = d->g;
    Workspace &ws = d->ws;      // (a failed allocation returns with cap = 0: the next reserve frees what was taken)
    HIP_TRY(ws.dev.alloc(128, &ws.ctr_base));
    HIP_TRY(hipMemset(ws.ctr_base, 0, 512));
    ws.fail_count = ws.ctr_base; d->cset = 0; d->set_clean[0] = d->set_clean[1] = false;     // (see Workspace::ctr_base)
    HIP_TRY(hipHostMalloc((void **)&ws.host_fail, 2 * sizeof(int32_t)));
    HIP_TRY(hipEventCreateWithFlags(&ws.fail_ready, hipEventDisableTiming));
    const bool grid = d->bp == BP_SCATTER_WIDE || d->bp == BP_GATHER_GRID;
    if (grid || d->edge_cert) {
        ws.redo_cap = (int)(d->grid_floor ? max_batch : std::min<int64_t>(max_batch, 4096));
        HIP_TRY(ws.dev.alloc((size_t)ws.redo_cap, &ws.redo_list));
        if (grid && d->bp != BP_GATHER_GRID) {
            ws.recheck_cap = (int)max_batch;
            HIP_TRY(ws.dev.alloc((size_t)ws.recheck_cap, &ws.recheck_list));
        }
    }
    // Relay-BP, marginals in device memory: a row per shot of the batch, reserved and released with llr_ws.  Never cleared: a shot that runs BP
    // fills its row with the priors first, a shot that does not never reads it
    if (d->bp == BP_RELAY && d->relay_marg_device) HIP_TRY(ws.dev.alloc((size_t)max_batch * g->bp.n_pad, &ws.marg_ws));
    int ncu = 256;
    hipDeviceProp_t prop;
    if (d->post != QD_POST_NONE && hipGetDeviceProperties(&prop, g->device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
    if (d->post == QD_POST_OSD0_OFFCHIP) {
        ws.post_blocks = ncu * std::max(1, g->x_per_cu);
        const size_t words = qd_osd_offchip_ws_words(g->m, g->x_kw);
        if (words > 0) HIP_TRY(ws.dev.alloc((size_t)ws.post_blocks * words, &ws.q_spill_off));
        HIP_TRY(ws.dev.alloc((size_t)max_batch * g->bp.n_pad, &ws.llr_ws));
        HIP_TRY(ws.dev.alloc((size_t)max_batch, &ws.fail_list));
    } else if (d->post != QD_POST_NONE) {
        const int per_cu = std::max(1, QD_LDS_BYTES / std::max(1, g->osd.lds_bytes));
        d->osd_blocks = g->osd.lds_bytes > 0 ? ncu * std::min(per_cu, 2048 / std::max(1, g->osd.threads)) : 0;
        const int per_cu_fast = std::max(1, QD_LDS_BYTES / std::max(1, g->osd.f_lds_bytes));
        d->osd_blocks_fast = ncu * std::min(per_cu_fast, 2048 / std::max(1, g->osd.f_threads));
        if (d->osd_w) d->osd_blocks_fast = ncu;                                   // higher-order OSD by row: w_* layout, one workgroup per CU
        if (d->post == QD_POST_LSD) {
            const int lds = qd_lsd_lds_bytes(g->m, g->n, g->bp.out_words);
            ws.post_blocks = ncu * std::max(1, std::min(8, QD_LDS_BYTES / std::max(1, lds)));     // one wavefront per shot, several shots per CU
            // Q planes + work counter (+ debug timers) + pivot columns (+ sweep scratch): the one size that comes in bytes
            HIP_TRY(ws.dev.alloc_bytes(qd_lsd_ws_bytes(g->m, g->n, ws.post_blocks, d->lsd_w), &ws.lsd_ws));
        } else if (d->post == QD_POST_OSD0_SR) {
            ws.post_blocks = ncu * g->osd.s_per_cu;
            HIP_TRY(ws.dev.alloc((size_t)ws.post_blocks * qd_osd_sr_ws_words(g->osd.m_pad, g->osd.mw, g->osd.s_threads, g->osd.s_rpt), &ws.q_spill_sr));
        } else if (d->post == QD_POST_OSD_CS_PANEL) {
            ws.post_blocks = ncu * d->cs_per_cu;
            HIP_TRY(ws.dev.alloc((size_t)ws.post_blocks * qd_osdcs_ws_words(d->cs_variant), &ws.cs_ws));
        }
        const int spill_fast = g->osd.mw - (d->osd_w ? g->osd.w_kw : g->osd.f_kw);
        if (g->osd.f_lds_bytes > 0 && spill_fast > 0)
            HIP_TRY(ws.dev.alloc((size_t)d->osd_blocks_fast * spill_fast * g->osd.m_pad, &ws.q_spill_fast));
        if (d->osd_w && g->osd.w_lds_bytes > 0)
            HIP_TRY(ws.dev.alloc((size_t)d->osd_blocks_fast * ((size_t)g->osd.mw * g->osd.m_pad + 64 * 32), &ws.mt_ws));   // + 64 candidate vectors of QD_SWEEP_W words
        HIP_TRY(ws.dev.alloc((size_t)max_batch, &ws.hard_list));
        HIP_TRY(ws.dev.alloc((size_t)max_batch, &ws.hard_list2));
        HIP_TRY(ws.dev.alloc((size_t)max_batch * g->bp.n_pad, &ws.llr_ws));
        HIP_TRY(ws.dev.alloc((size_t)max_batch, &ws.fail_list));
        if (d->osd_blocks > 0)
            HIP_TRY(ws.dev.alloc((size_t)d->osd_blocks * g->n, &ws.order_ws));
        const int spill_planes = g->osd.mw - g->osd.kw_lds;
        if (d->osd_blocks > 0 && spill_planes > 0)
            HIP_TRY(ws.dev.alloc((size_t)d->osd_blocks * spill_planes * g->osd.m_pad, &ws.q_spill));
    }
    if (d->bp == BP_HBM_EDGE) {
        // [index][shot] message planes for a chunk of S shots; a batch larger than S is decoded chunk by chunk
        const bool ps = d->prm.bp_method == QD_BP_PRODUCT_SUM, serial = d->prm.schedule == QD_SCHEDULE_SERIAL;
        // edge planes: flooding b2c + c2b (+ th for product-sum); serial: messages (th or b2c) + suffixes (the c2b plane), and a row plane
        const int planes = serial ? 2 : (ps ? 3 : 2);
        const bool pre_plane = serial && g->gen.nslots == 0;       // the rows' running prefixes: LDS slots when the graph allows
        // Serial schedule in several launches (qd_decoder_create chose the bounds): costs a second workspace.
        GenStagePlan &sp = d->ws.gsp;
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
        GenWs &w = d->ws.gws;
        w.S = S;
        if (!(ps && serial)) HIP_TRY(ws.dev.alloc((size_t)g->nnz * S, &w.b2c));
        HIP_TRY(ws.dev.alloc((size_t)g->nnz * S, &w.c2b));
        if (ps) HIP_TRY(ws.dev.alloc((size_t)g->nnz * S, &w.th));
        if (pre_plane) HIP_TRY(ws.dev.alloc((size_t)g->m * S, &w.pre));
        HIP_TRY(ws.dev.alloc((size_t)g->n * S, &w.llr));
        HIP_TRY(ws.dev.alloc((size_t)g->m * S, &w.syn));
        HIP_TRY(ws.dev.alloc((size_t)S, &w.slot));
        if (sp.nbounds > 0) {
            HIP_TRY(ws.dev.alloc((size_t)g->nnz * S, &sp.msg2));
            HIP_TRY(ws.dev.alloc((size_t)g->m * S, &sp.syn2));
            sp.w2 = w;
            (ps ? sp.w2.th : sp.w2.b2c) = sp.msg2;
            sp.w2.syn = sp.syn2;
            HIP_TRY(ws.dev.alloc((size_t)S, &sp.lists[0]));
            HIP_TRY(ws.dev.alloc((size_t)S, &sp.lists[1]));
            HIP_TRY(ws.dev.alloc(QD_GEN_MAX_STAGES + 1, &sp.counts));
            HIP_TRY(hipHostMalloc((void **)&sp.host_counts, sizeof(int32_t) * (QD_GEN_MAX_STAGES + 1)));
            HIP_TRY(hipEventCreateWithFlags(&sp.counts_ready, hipEventDisableTiming));
        }
    }
    d->cap = max_batch;
    return QD_OK;
}

extern "C" int qd_decoder_set_workspace_limit(qd_decoder *d, int64_t bytes)
{
    if (!d || bytes <= 0) return qd_fail(QD_EINVAL, "bad workspace limit");
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
    if (!d) return qd_fail(QD_EINVAL, "null decoder");
    HIP_TRY(hipSetDevice(d->g->device));
    HIP_TRY(hipDeviceSynchronize());
    free_ws(d);
    return QD_OK;
}

extern "C" int qd_decoder_set_profiling(qd_decoder *d, int32_t enable)
{
    if (!d) return qd_fail(QD_EINVAL, "null decoder");
    d->profiling = enable ? 1 : 0;
    return QD_OK;
}

extern "C" int qd_decoder_profile(qd_decoder *d, double *out, int32_t reset)
{
    if (!d || !out) return qd_fail(QD_EINVAL, "null argument");
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
    if (B < 0 || B > 0x7FFFFFFF) return qd_fail(QD_EINVAL, "batch size out of range");
    if (B == 0) return QD_OK;
    if (det_offset < 0 || det_stride < det_offset + d->g->m) return qd_fail(QD_EINVAL, "detector slice [%lld, %lld) exceeds the row stride %lld", (long long)det_offset, (long long)(det_offset + d->g->m), (long long)det_stride);
    if (d_upd && (upd_rows < 0 || upd_rows > d->g->m || upd_stride < upd_rows)) return qd_fail(QD_EINVAL, "bad syndrome-update shape");
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
    a.llr_ws = d->ws.llr_ws; a.fail_list = d->ws.fail_list; a.fail_count = d->ws.fail_count;
    a.order_ws = d->ws.order_ws; a.q_spill = d->ws.q_spill; a.q_spill_fast = d->ws.q_spill_fast; a.q_spill_sr = d->ws.q_spill_sr; a.mt_ws = d->ws.mt_ws;
    a.hard_list = d->ws.hard_list; a.hard_list2 = d->ws.hard_list2; a.hard_count = d->ws.fail_count + 1;
    a.dbg = reinterpret_cast<unsigned long long *>(d->ws.ctr_base) + 2;   // bytes 16..143 of the counter block (first set, never zeroed by a call)
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
    case BP_RELAY:
        if (d->relay_marg_device) {
            RelayArgs x = d->relay;
            x.marg_ws = d->ws.marg_ws;                   // (rows 0 .. B - 1 of the cap the workspace was cut for: decode_impl reserved B <= cap)
            HIP_TRY(qd_launch_bp_relay_device(g->bp, a, x, B, s));
        } else
            HIP_TRY(qd_launch_bp_relay(g->bp, a, d->relay, B, s));
        break;
    case BP_HBM_EDGE: {
        // edge_cert (off-chip decoder on the LLR grid): the first pass parks the shots whose exactness bound tripped, the redo pass decodes them
        // on the coarse grid -- the gather kernel's rule (BP_GATHER_GRID below), chunk by chunk of the message workspace
        int32_t *redo_count = d->ws.fail_count + 40;
        DecodeArgs a1 = a;
        if (d->edge_cert) {
            a1.s_limit = std::ldexp(1.0f, 23 - d->grid_k);
            a1.redo_list = d->ws.redo_list; a1.redo_count = redo_count; a1.redo_cap = d->ws.redo_cap;
        }
        for (int64_t b0 = 0; b0 < B; b0 += d->ws.gws.S)
            HIP_TRY(qd_launch_bp_general(gg, g->bp, a1, d->ws.gws, d->prm.bp_method, d->prm.schedule, b0,
                                         (int)std::min<int64_t>(d->ws.gws.S, B - b0), s, d->ws.gsp.nbounds > 0 ? &d->ws.gsp : nullptr));
        if (d->edge_cert) {
            DecodeArgs a2 = a;
            a2.s_limit = std::ldexp(1.0f, 23 - d->grid_kc);
            a2.shot_list = d->ws.redo_list; a2.shot_count = redo_count; a2.status_or = QD_STATUS_COARSE_GRID;
            gg.llr0 = d->llr0_qc;
            const int64_t parked_max = std::min<int64_t>(B, d->ws.redo_cap);
            for (int64_t c0 = 0; c0 < parked_max; c0 += d->ws.gws.S)
                HIP_TRY(qd_launch_bp_general(gg, g->bp, a2, d->ws.gws, d->prm.bp_method, d->prm.schedule, c0,
                                             (int)std::min<int64_t>(d->ws.gws.S, parked_max - c0), s, nullptr));
        }
        break;
    }
    case BP_SCATTER_WIDE:
    case BP_GATHER_GRID: {
        // grid arithmetic: first pass on the fine grid parks the shots whose exactness bound tripped; they are decoded
        // again on the coarse grid by a second launch (one workgroup per parked shot; the others exit at once)
        int32_t *redo_count = d->ws.fail_count + 40;       // bytes 160..163 of the counter set (16..143 of the first set are the debug counters)
        DecodeArgs a1 = a;
        a1.s_limit = std::ldexp(1.0f, 23 - d->grid_k);
        a1.redo_list = d->ws.redo_list; a1.redo_count = redo_count; a1.redo_cap = d->ws.redo_cap;
        if (d->bp == BP_GATHER_GRID)
            HIP_TRY(qd_launch_bp(d->bp_fine, a1, B, s));
        else {
            // scatter kernel first; the shots its (looser) bound cannot certify are decoded again by the gather kernel,
            // which carries the per-fault bound the coarse-grid rule is stated on
            int32_t *recheck_count = d->ws.fail_count + 41;
            ScatArgs x{};
            x.prior_g = d->prior_g; x.grid_inv = std::ldexp(1.0f, -d->grid_k); x.m2_limit = d->m2_limit;
            x.recheck_list = d->ws.recheck_list; x.recheck_count = recheck_count; x.recheck_cap = d->ws.recheck_cap;
            x.first_pass = d->first_pass;
            HIP_TRY(qd_launch_bp_scatter_wide(d->bp_fine, g->sc, a1, x, B, s));
            a1.shot_list = d->ws.recheck_list; a1.shot_count = recheck_count;
            HIP_TRY(qd_launch_bp(d->bp_fine, a1, std::min<int64_t>(B, d->ws.recheck_cap), s));
        }
        DecodeArgs a2 = a;
        a2.s_limit = std::ldexp(1.0f, 23 - d->grid_kc);
        a2.shot_list = d->ws.redo_list; a2.shot_count = redo_count; a2.status_or = QD_STATUS_COARSE_GRID;
        HIP_TRY(qd_launch_bp(d->bp_coarse, a2, std::min<int64_t>(B, d->ws.redo_cap), s));
        break;
    }
    }
    return QD_OK;
}

// Stage 2: the post-processor over the shots BP parked
static int launch_post(const qd_decoder *d, const DecodeArgs &a, int64_t B, hipStream_t s)
{
    const qd_graph *g = d->g;
    const int blocks = (int)std::min<int64_t>(B, d->ws.post_blocks);
    const int fast = (int)std::min<int64_t>(B, d->osd_blocks_fast), full = (int)std::min<int64_t>(B, d->osd_blocks);
    switch (d->post) {
    case QD_POST_OSD0_OFFCHIP:
        HIP_TRY(qd_launch_osd0_offchip(g->osd, g->bp, a, g->x_off, g->x_off_sort, g->x_off_order, g->x_kw, g->x_threads, g->x_lds, d->ws.q_spill_off, blocks, s));
        break;
    case QD_POST_LSD:
        HIP_TRY(qd_launch_lsd0(g->gen, g->bp, a, d->ws.lsd_ws, d->ws.post_blocks, blocks, d->lsd_w, d->prm.osd_order, g->osd.wfix, s));
        break;
    case QD_POST_OSD_CS_PANEL:
        HIP_TRY(qd_launch_osdcs(g->osd, g->bp, a, d->cs_off, d->cs_variant, d->cs_lds, d->ws.cs_ws, blocks, s));
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
    if (!d) return qd_fail(QD_EINVAL, "null decoder");
    if (stage < 1 || stage > 3) return qd_fail(QD_EINVAL, "stage must be 1 (BP), 2 (OSD) or 3 (both)");
    if (int rc = check_batch(d, det_stride, det_offset, d_upd, upd_stride, upd_rows, B)) return rc;
    if (B == 0) return QD_OK;                            // whatever the pointers: an empty batch has none (a torch tensor of no rows: data_ptr() = 0)
    if (!d_det || !d_err_bits || !d_status) return qd_fail(QD_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(d->g->device));
    if (B > d->cap && stage == 2) return qd_fail(QD_EINVAL, "OSD stage without a preceding BP stage of this batch size");
    if (int rc = B > d->cap ? qd_decoder_reserve(d, B) : QD_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool post = d->post != QD_POST_NONE;
    if (stage & 1) {                                     // a new call: the other counter set (see Workspace::ctr_base)
        d->cset ^= 1;
        d->ws.fail_count = d->ws.ctr_base + 64 * d->cset;
        if (!d->set_clean[d->cset]) {
            HIP_TRY(hipMemsetAsync(d->ws.fail_count, 0, 3 * sizeof(int32_t), s));
            HIP_TRY(hipMemsetAsync(d->ws.fail_count + 40, 0, 2 * sizeof(int32_t), s));
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
        if (!d->ws.fail_pending && d->ws.host_fail) {          // (see Workspace::host_fail)
            HIP_TRY(hipMemcpyAsync(d->ws.host_fail, d->ws.fail_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipEventRecord(d->ws.fail_ready, s));
            d->ws.fail_pending = true; d->fail_pending_B = d->last_B;
        }
    }
    if ((stage & 2) && !d->set_clean[d->cset ^ 1]) {     // the next call's counters, zeroed behind this call's last stage (nothing waits for these fills)
        int32_t *other = d->ws.ctr_base + 64 * (d->cset ^ 1);
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
// OSD-0 decoder launches nothing unless an earlier call's failure count (Workspace::host_fail) says "heavy" (profiles/r06_post_head_start.txt).
extern "C" int qd_decoder_post_head_start(qd_decoder *d, int32_t microseconds, void *stream)
{
    if (!d) return qd_fail(QD_EINVAL, "null decoder");
    if (microseconds < 0) microseconds = 50;
    if (microseconds <= 0 || d->post == QD_POST_NONE || !d->ws.ctr_base || d->last_B <= 0) return QD_OK;
    microseconds = std::min(microseconds, 5000);
    HIP_TRY(hipSetDevice(d->g->device));
    const bool always = d->post == QD_POST_LSD || d->post == QD_POST_OSD_CS_PANEL;
    const double frac = 0.75;
    if (d->ws.fail_pending && qd_event_done(d->ws.fail_ready)) {
        d->ws.fail_pending = false;
        if (d->fail_pending_B > 0) d->fail_frac_hint = (double)d->ws.host_fail[0] / (double)d->fail_pending_B;
    }
    if (!always && d->fail_frac_hint < 0.8 * frac) return QD_OK;        // OSD-0 over a minority of the shots (or nothing known yet): no launch at all
    const int threshold = (int)std::min<double>(2147483647.0, std::max(1.0, frac * (double)d->last_B));
    HIP_TRY(qd_launch_hold(always ? nullptr : d->ws.fail_count, threshold, microseconds, reinterpret_cast<hipStream_t>(stream)));
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
    if (!d) return qd_fail(QD_EINVAL, "null decoder");
    if (d->post == QD_POST_NONE) return qd_fail(QD_EINVAL, "decoder was created with osd_method = off");
    if (int rc = check_batch(d, det_stride, det_offset, d_upd, upd_stride, upd_rows, B)) return rc;
    if (B == 0) return QD_OK;
    if (!d_det || !d_llr || !d_err_bits || !d_status) return qd_fail(QD_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(d->g->device));
    if (int rc = B > d->cap ? qd_decoder_reserve(d, B) : QD_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const DecodeArgs a = decode_args(d, d_det, det_stride, det_offset, d_upd, upd_stride, upd_rows, d_err_bits, d_status);
    HIP_TRY(hipMemsetAsync(d->ws.fail_count, 0, 3 * sizeof(int32_t), s));
    d->set_clean[d->cset] = false;
    HIP_TRY(qd_launch_stage_llr(d_llr, d->g->n, d->g->bp.n_pad, d->g->bp.bit_orig, B, d->ws.llr_ws, d->ws.fail_list, d->ws.fail_count,
                                d_status, s));
    return launch_post(d, a, B, s);
}

extern "C" int qd_decoder_debug_counters(qd_decoder *d, uint64_t *out16)
{
    if (!d || !out16 || !d->ws.fail_count) return qd_fail(QD_EINVAL, "no workspace yet");
    HIP_TRY(hipSetDevice(d->g->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out16, reinterpret_cast<char *>(d->ws.ctr_base) + 16, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(reinterpret_cast<char *>(d->ws.ctr_base) + 16, 0, 16 * sizeof(uint64_t)));
    return QD_OK;
}

extern "C" int qd_decoder_failed_llr(qd_decoder *d, int64_t b, float *d_out, void *stream)
{
    if (!d || !d_out || !d->ws.llr_ws) return qd_fail(QD_EINVAL, "no posterior workspace (OSD off or nothing decoded yet)");
    HIP_TRY(hipSetDevice(d->g->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipStreamSynchronize(s));
    int32_t nfail = 0;
    HIP_TRY(hipMemcpy(&nfail, d->ws.fail_count, sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int32_t> list((size_t)std::max(nfail, 1));
    if (nfail > 0) HIP_TRY(hipMemcpy(list.data(), d->ws.fail_list, sizeof(int32_t) * (size_t)nfail, hipMemcpyDeviceToHost));
    for (int i = 0; i < nfail; ++i)
        if (list[i] == (int32_t)b) {
            // workspace rows are in bit-slot order; hand back fault order
            const qd_graph *g = d->g;
            std::vector<float> slot(g->bp.n_pad), outv(g->n);
            std::vector<uint32_t> orig(g->bp.n_pad);
            HIP_TRY(hipMemcpy(slot.data(), d->ws.llr_ws + (size_t)i * g->bp.n_pad, sizeof(float) * g->bp.n_pad, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(orig.data(), g->bp.bit_orig, sizeof(uint32_t) * g->bp.n_pad, hipMemcpyDeviceToHost));
            for (int sidx = 0; sidx < g->n; ++sidx) outv[orig[sidx]] = slot[sidx];
            HIP_TRY(hipMemcpy(d_out, outv.data(), sizeof(float) * g->n, hipMemcpyHostToDevice));
            return QD_OK;
        }
    return qd_fail(QD_EINVAL, "shot %lld converged (no stored posterior)", (long long)b);
}
