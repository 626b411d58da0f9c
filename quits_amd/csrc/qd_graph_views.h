// qd_graph_views.h -- one window's graph as the kernels read it: the four views graph_layout.hip fills and the limits they are cut to.
// Plain C++ (no HIP header): the layout code that includes it also builds and runs on a machine without the runtime.
#pragma once
#include <stdint.h>

#define QD_MAX_COL_DEG 16      // bit-side sign copy is a uint16 per fault
#define QD_MAX_ROW_DEG 255     // edge position inside a check is a byte
#define QD_LDS_BYTES (160 * 1024)
// wavefronts per SIMD the register budget of qd_osd0_sr_kernel (osd_sr.hip) is cut for at rpt rows per thread: 128 / 256 registers -- no instantiation may
// spill vector registers (scalar registers it cannot keep live in lanes of vector registers)
constexpr int qd_sr_wps(int rpt) { return rpt <= 2 ? 4 : 2; }

// One window's Tanner graph as the BP kernel wants it.
//   check slots: checks sorted by degree (descending); bit slots: faults sorted by degree (descending), so that a
//   wavefront's lanes run the same trip count.  Indices refer to SLOTS; the LDS arrays are indexed by slot.
//   Everything is pre-scaled to LDS byte offsets so the kernel does no address arithmetic on the gathers.
struct BpGraphDev {
    int m, n, m_pad, n_pad;
    int max_rdeg, max_cdeg, neg_words, out_words;
    int max_rdeg_pad;           // max_rdeg rounded up to a multiple of 4
    int dummy_bit, dummy_chk;   // LDS slots that pad short rows/columns: llr[dummy_bit] = +inf, chk[dummy_chk] = zero message
    int rec_words;              // uint32 words per fault record (multiple of 4)
    int sign_mode;              // 0: every check has <= 32 (padded) edges; 1: <= 44, signs 32..46 ride in the state's meta word;
                                // 2: wider, signs 32.. live in separate LDS words
    int adj32;                  // 1: chk_adj holds uint32 entries (windows with more than 16379 fault slots), else uint16
    const void *chk_adj;        // [max_rdeg_pad/4][m_pad][4] absolute LDS byte offset (off_llr + slot * 4) of the posterior of the k-th
                                //                        fault of the check, k ascending = original column order; the dummy bit beyond the degree
    const int32_t *chk_degp_w;  // [m_pad / 64]           low 16 bits: trip count of a wavefront of check slots (its max degree rounded up
                                //                        to 4); high 16 bits: that max degree itself
    const uint32_t *chk_orig;   // [m_pad]                detector index of the check slot
    const uint32_t *bit_rec;    // [rec_words/4][n_pad][4] word 0 = prior LLR (float bits: log((1-p)/p) computed in double, rounded once);
                                //                        word 1+q = (LDS byte offset of the check state) << 16 | where the check keeps this edge's
                                //                        sign (mode 0/1: bit index 0..63 into {w, z}; mode 2: word index << 5 | bit index)
                                //                        for the q-th check of the fault (q ascending = original row order)
    const uint32_t *bit_orig;   // [n_pad]                fault index of the bit slot
    const uint32_t *bit_slot_of;// [n]                    bit slot of a fault (inverse of bit_orig)
    int bit_thr[QD_MAX_COL_DEG];// bit_thr[q] = number of bit slots (multiple of 64) whose wavefront has a fault of degree > q
    // LDS carve-up (byte offsets, 16-byte aligned)
    int off_chk, off_cneg, off_llr, off_out, off_misc, lds_bytes;   // off_misc: 64 ints of reduction scratch
    int threads;
};

// The scatter form of the flooding min-sum kernel (bp_scatter_wide.hip): a check keeps its state in the registers of its lane and ADDS its
// messages to the faults' integer accumulators in LDS (ds_add_u32), so there is no bit pass.  One posterior buffer, updated in place
// (offA = offB, adjA = adjB: the kernel reads the A members); the adjacency holds LDS byte offsets so that a gather / scatter needs no address add.
struct ScatGraphDev {
    int ok;                     // 1: this window runs in the scatter kernel (a shape of bp_scatter_wide.hip covers it, rows of 2..96 faults, the LDS fit of build_scatter)
    const uint32_t *adjA, *adjB;// [max_rdeg_pad/4 + 2][m_pad][4] LDS byte offset of the fault's accumulator, in the walk order of scatter_walk
                                //                        (graph_layout.hip); a trash slot beyond a check's degree and in the two spare rows
    const uint32_t *deg_w;      // [m_pad/64]             per wavefront of check slots: trip count (multiple of 4) | largest degree << 8 | smallest << 16
    const uint8_t *chk_deg;     // [m_pad]                degree of the check slot (0 beyond m)
    int offA, offB, off_out, off_bmap, off_misc, lds_bytes;
    // The accumulators have their own slot order (not BpGraphDev's bit slots): bank = slot mod 32 is chosen per fault so that the 32 lanes of a
    // half-wavefront can meet 32 different banks at every step of the walk (graph_layout.hip: scatter_banks / scatter_walk).
    int nslots;                 // accumulators incl. unused slots and 32 trash slots (one per bank) for the steps beyond a check's degree; multiple of 4
    const uint32_t *slot_fault; // [nslots] fault of the slot, 0xFFFFFFFF: none (its accumulator stays 0)
    const uint32_t *k1_slot;    // [n] BpGraphDev's bit slot (the OSD workspace's row layout) -> accumulator slot of that fault
    const int32_t *wave_map;    // [wide_cpl][wide_threads / 64] the 64 consecutive check slots (index / 64) a wavefront takes in its j-th round, -1:
                                //                        none; chosen so that the wavefronts of a workgroup walk equally many edges (slots are sorted by degree)
    int wide_threads, wide_cpl; // the workgroup size and the checks per lane of qd_bp_scatter_wide_kernel (bp_scatter_wide.hip); (0, 0): no scatter kernel (ok = 0)
};

// The general (one message per edge) BP kernel's view: plain CSR + CSC in fault / detector order, prior LLRs in float.
// column-weight bound the per-edge kernel's serial schedule unrolls for (register arrays of that length, record width)
// (a weight-6 instantiation between 4 and 8 was no faster: profiles/r05_k1g_register_budget_ab.txt)
static inline int qd_gen_unroll(int max_cdeg) { return max_cdeg <= 4 ? 4 : (max_cdeg <= 8 ? 8 : QD_MAX_COL_DEG); }
#define QD_GEN_GS 4           // wavefronts per 64 shots in the serial schedule (faults of one dependency level in parallel)
struct GenGraphDev {
    int m, n, nnz, out_words;
    const int32_t *rp, *ci;     // [m + 1], [nnz]   CSR, columns ascending in a row
    const int32_t *cp, *ri;     // [n + 1], [nnz]   CSC, rows ascending in a column
    const int32_t *c2r;         // [nnz]            CSC edge -> CSR edge
    const uint16_t *erow;       // [nnz]            CSR edge -> its row
    const uint16_t *frec;       // [n][16]          the CSR edges of a fault's column (8 entries), then their rows (8), 0xFFFF beyond its weight
                                //                  (null if a column is heavier than 8 or nnz > 65534)
    const float *llr0;          // [n]              (float)log((1 - p) / p), the log in double
    const int32_t *ell;         // [m][ell_w][2]    rows in ELL form for BP-LSD: {fault, its posterior column}, {-1, 0} padding
    int ell_w;                  //                  max row weight rounded up to a multiple of 64
    // serial schedule: faults grouped into dependency levels.  Two faults that share no check commute, so natural order
    // is reproduced by any order that keeps every pair of faults with a common check in index order; level(j) = 1 + the
    // highest level among earlier faults on j's checks.  Faults of one level are mutually independent.
    // The G = QD_GEN_GS wavefronts that share 64 shots take the faults of a level in parallel, one barrier per level.  What a
    // wavefront needs to know about its next fault -- index, weight, prior LLR, the rows and CSR edges of its column -- is ONE record
    // of srec_w dwords, read with one scalar load a whole step ahead (the adjacency arrays cost 3 + 2 * weight dependent scalar
    // round trips per fault):  srec[(step * G + wavefront) * srec_w + ...] =
    //   [0] fault | weight << 24 | (barrier after this step) << 31     (weight 0: nothing to do in this step)
    //   [1] prior LLR (float bits)      [2 .. 2 + D) rows      [2 + D .. 2 + 2 D) CSR edges      D = 4, 8 or QD_MAX_COL_DEG
    int nlev, nstep, srec_w;
    const uint32_t *srec;       // [nstep][G][srec_w]
    // Row i's running prefix is live from the level of its first fault to the level of its last; rows whose intervals do not
    // overlap share one of `nslots` LDS slots (64 floats each; greedy interval colouring = the minimum), so the 8 bytes per
    // edge and sweep the prefixes would move through HBM stay on the CU.  Then a row entry of a record is
    //   row | (first entry of its row: the prefix starts at +-1 / +-max, sign = syndrome bit) << 23 | slot << 24.
    // nslots = 0: too many slots for the LDS budget, the prefixes live in the [m][S] plane GenWs::pre and the entry is the row.
    int nslots;
};

// Elimination (OSD) view: original indexing.
struct OsdGraphDev {
    int m, n, m_pad, max_cdeg;
    int mw;                     // words per Q row = ceil(m / 64)
    int npow2;                  // bitonic sort size of the full kernel
    int kw_lds;                 // full kernel: Q word-planes that live in LDS; planes >= kw_lds spill to global
    const uint32_t *csc_ptr;    // [n + 1]
    const uint16_t *csc_row;    // [nnz]  detector index, ascending inside a column
    // LDS carve-up of the full kernel: off[] = q, tb, sp, rowpiv, prow, pcol, pairs, cols, red, out
    int off[10], lds_bytes;
    // ... of the register kernel for OSD-0 (aims at two workgroups per CU; f_lds_bytes = 0 disables it)
    int f_off[10], f_off_hist, f_off_sort, f_off_order, f_off_pivmask, f_off_npl, f_kw, f_lds_bytes, f_threads;
    // ... and of the register kernel for OSD-CS / OSD-E (one workgroup per CU, as many Q planes in LDS as fit: the
    //     candidate sweep reads arbitrary Q bits of every pivot row)
    int w_off[10], w_off_sort, w_off_order, w_off_pivmask, w_off_npl, w_kw, w_lds_bytes;
    const uint32_t *wfix;       // [n] integer candidate costs round(log(1/p) * 2^18) for OSD-CS / OSD-E
    uint32_t max_wfix;          // largest of them (the rebuilt OSD-CS / OSD-E kernel adds 64 of them in 32 bits)
    int threads;
    // OSD-0 with simultaneous singleton pivots (osd_sr.hip, qd_osd0_sr_kernel): its LDS layout (s_lds_bytes = 0: not taken),
    // instantiation and the columns in ELL form
    int s_off[13], s_lds_bytes, s_threads, s_rpt, s_per_cu;
    const uint16_t *csc_ell;    // [n][1 << ell_log2] detector indices of a fault, ascending, 0xFFFF beyond its weight
    int ell_log2;
};
