// osd_offchip.hip -- OSD-0 for off-chip windows: windows whose BP state does not fit the CU (build_bp, graph_layout.hip) and whose
// column order fits neither OSD kernel of osd_kernels.hip -- qd_osd0_reg_kernel stops at four rows per thread (2048 detectors),
// qd_osd0_full_kernel sorts every column in LDS (about 16 384 faults).  QLP [[1020,136]] at W = 5 / F = 3: 2250 x 31 500.
//
// One persistent workgroup per failing shot, as in qd_osd0_full_kernel, with the same elimination (qd_osd_eliminate, osd_shared.h:
// all row state in LDS, Q planes beyond the LDS budget in a per-workgroup HBM buffer, early stop) -- but the column order is drawn
// lazily, as in qd_osd0_reg_kernel: the next <= QD_OSD_TIER columns in ascending (posterior, fault index) are selected by key value,
// sorted in LDS and eliminated, and the next tier is drawn only if the syndrome is not resolved yet (qd_osd_draw_tier, osd_shared.h).
// So LDS holds 17 bytes per padded detector + one tier, whatever n is, and a shot that stops after a few hundred columns (the usual
// case) never sorts the other 30 000.  The order is the same total order every OSD kernel here consumes and the elimination depends on
// nothing else, so results equal qd_osd0_full_kernel's and the oracle's (oq_osd0) bit for bit.
//
// Every loop is bounded: a tier that is not the last consumes at least one column (at most n tiers), the elimination takes at most
// rank pivots.  Workspaces (Q spill planes) are private to the workgroup.
#include "osd_shared.h"
#include "qd_host.h"
#include "../../include/quits_amd.h"
#include <algorithm>

struct OsdOffArgs {
    int n;                      // (qd_osd_draw_tier reads n and bit_orig)
    const uint32_t *bit_orig;   // [n_pad] bit slot (row layout of llr_ws) -> fault
    int n_pad, out_words, kw;   // kw: Q planes in LDS
    int off[10], off_sort, off_order;
};

// LDS layout for a window, or 0 if even the row state does not fit: off[] as qd_osd_carve takes it, then the tier's sort buffer and order.
// Two workgroups per CU where the Q planes of two (or all of them) still fit half the LDS, else one with as many planes as fit.
int qd_osd_offchip_layout(int m, int n, int max_cdeg, int *off, int *off_sort, int *off_order, int *kw, int *threads, int *per_cu)
{
    const int m_pad = (m + 63) & ~63, mw = (m + 63) / 64, out_words = (n + 31) / 32;
    auto a16 = [](int x) { return (x + 15) & ~15; };
    auto carve = [&](int qbytes) {
        int o = 0;
        off[0] = o; o += a16(qbytes);
        off[1] = o; o += a16(m_pad * 8);            // tb
        off[2] = o; o += a16(m_pad);                // sp
        off[3] = o; o += a16(m_pad * 2);            // rowpiv
        off[4] = o; o += a16(m_pad * 2);            // prow
        off[5] = o; o += a16(m_pad * 4);            // pcol
        off[6] = o; o += a16(64 * max_cdeg * 4);    // pairs
        off[7] = o; o += 256;                       // cols
        off[8] = o; o += 1024;                      // red: pivot keys / flags, pair counter, [80] gather counter, [96..223] block sums
        off[9] = o; o += a16(out_words * 4);        // out
        *off_sort = o; o += QD_OSD_TIER * 8;
        *off_order = o; o += a16(QD_OSD_TIER * 2);
        return o;
    };
    *threads = m <= 256 ? 256 : (m <= 1024 ? 512 : 1024);
    const int fixed = carve(0);
    for (int pc = 2; pc >= 1; --pc) {
        const int budget = QD_LDS_BYTES / pc - fixed;
        if (budget < 0) continue;
        const int planes = std::min(mw, budget / (m_pad * 8));
        if (pc == 2 && planes < std::min(mw, 2)) continue;
        *kw = planes; *per_cu = std::min(pc, 2048 / *threads);
        return carve(planes * m_pad * 8);
    }
    return 0;
}

size_t qd_osd_offchip_ws_words(int m, int kw)
{
    const int m_pad = (m + 63) & ~63, mw = (m + 63) / 64;
    return (size_t)std::max(0, mw - kw) * m_pad;
}

template <int T>
__global__ void __launch_bounds__(T) qd_osd0_offchip_kernel(OsdGraphDev g, OsdOffArgs x, DecodeArgs a, uint64_t *q_ws)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int nfail = *a.fail_count;
    OsdLds S;
    qd_osd_carve(smem, x.off, S);
    uint64_t *sortbuf = reinterpret_cast<uint64_t *>(smem + x.off_sort);        // [QD_OSD_TIER]
    uint16_t *order = reinterpret_cast<uint16_t *>(smem + x.off_order);         // [QD_OSD_TIER]
    uint32_t *red = S.red, *sumbuf = red + 96;
    uint64_t *qglb = g.mw > x.kw ? q_ws + (size_t)blockIdx.x * (size_t)(g.mw - x.kw) * g.m_pad : nullptr;
    for (int slot = blockIdx.x; slot < nfail; slot += gridDim.x) {
        const int64_t shot = a.fail_list[slot];
        const float *llr = a.llr_ws + (int64_t)slot * x.n_pad;
        const uint8_t *det = a.det + shot * a.det_stride + a.det_offset;
        const uint8_t *upd = a.upd ? a.upd + shot * a.upd_stride : nullptr;
        int npiv = 0, inconsistent = 0, sphase = 0, consumed = 0, pending = 1;
        uint32_t lo_key = 0, lo_idx = 0;             // every column with (key, fault index) < (lo_key, lo_idx) has been consumed
        // OSD-0 stops after a few hundred columns at the usual operating points: a first tier of 256 costs a third of a full one
        for (int tier = 0; tier <= g.n && pending; ++tier) {
            TierState ts{lo_key, lo_idx, sphase, 0, tier == 0 ? QD_OSD_TIER_FIRST : QD_OSD_TIER};
            int cnt = qd_osd_draw_tier<T, 1, OsdOffArgs, 4>(x, llr, sortbuf, order, red, sumbuf, ts);
            lo_key = ts.lo_key; lo_idx = ts.lo_idx; sphase = ts.sphase;
            if (ts.exhausted) cnt = 0;
            consumed += cnt;
            const int last = ts.exhausted || consumed >= g.n;
            pending = qd_osd_eliminate<T, true, true>(g, S, qglb, x.kw, g.m, order, cnt, det, upd, a.upd_rows, x.out_words, &npiv, &inconsistent,
                                                      nullptr, tier == 0, last);
        }
        for (int w = tid; w < x.out_words; w += T) a.err_bits[shot * x.out_words + w] = S.outw[w];
        if (tid == 0) a.status[shot] = (a.status[shot] & 0xFFFF) | (1 << 17) | (inconsistent ? (1 << 18) : 0) | (min(npiv, 4095) << 20);
        __syncthreads();   // LDS is recycled by the next shot
    }
}

template <int T>
static hipError_t launch_offchip(const OsdGraphDev &g, const OsdOffArgs &x, const DecodeArgs &a, int lds, uint64_t *q_ws, int blocks, hipStream_t s)
{
    auto k = qd_osd0_offchip_kernel<T>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(T), (size_t)lds, s, g, x, a, q_ws);
    return hipGetLastError();
}

hipError_t qd_launch_osd0_offchip(const OsdGraphDev &g, const BpGraphDev &bg, const DecodeArgs &a, const int *off, int off_sort, int off_order,
                                  int kw, int threads, int lds, uint64_t *q_ws, int blocks, hipStream_t s)
{
    if (blocks <= 0) return hipSuccess;
    OsdOffArgs x{};
    x.n = g.n; x.bit_orig = bg.bit_orig; x.n_pad = bg.n_pad; x.out_words = bg.out_words; x.kw = kw;
    for (int i = 0; i < 10; ++i) x.off[i] = off[i];
    x.off_sort = off_sort; x.off_order = off_order;
    switch (threads) {
    case 256: return launch_offchip<256>(g, x, a, lds, q_ws, blocks, s);
    case 512: return launch_offchip<512>(g, x, a, lds, q_ws, blocks, s);
    default: return launch_offchip<1024>(g, x, a, lds, q_ws, blocks, s);
    }
}
