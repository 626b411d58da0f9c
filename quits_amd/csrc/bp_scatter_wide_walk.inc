// bp_scatter_wide_walk.inc -- the edge walk of one gather pass of one check (bp_scatter_wide.hip), as program text: included by
// qd_bp_scatter_wide_kernel for every pass and by qd_bp_first_pass_kernel, which runs pass 0 once per decoder -- the same QS_EDGE_H / QS_EDGE
// steps, trip counts, tail rules and argmin rule, so the table cannot drift from what the loop would have found.
// In scope at the point of inclusion: j, dws, cs, S1, S2, KOLD, dcs, O, pf, a1, a2, kst, adj_row, QS_ADJ, QS_ABL_ADJC, QS_ACC.  Leaves hp, par, neg[].
                // (the round's loop bounds are re-derived from one scalar every pass: hoisted out of the iteration loop they, and everything computed
                //  from them for CPL rounds x NSW words, outgrow the scalar registers and come back through v_readlane)
                int dwj = dws[j];
                asm volatile("" : "+s"(dwj));
                const int trip = dwj & 0xFF, wmax = (dwj >> 8) & 0xFF, wmin = (dwj >> 16) & 0xFF, wmin4 = wmin & ~3;
                const int adj_voff = cs[j] * 16;
                QS_ABL_ADJC
                const float s1 = S1[j], s2 = S2[j];
                const uint32_t kold = KOLD[j];
                const int dc = dcs[j];
                uint32_t hp = 0u, hpa = 0u, par = 0u;
                uint32_t neg[NSW];
#pragma unroll
                for (int w = 0; w < NSW; ++w) {
                    neg[w] = 0u;
                    const int k0 = 32 * w;
                    if (k0 < trip) {
                        const uint32_t sgnw = O[j][w];
                        uint32_t neww = 0u, ltw = 0u;
                        const int kend = min(trip - k0, 32);                  // multiple of 4
                        const int kplain = min(max(wmin4 - k0, 0), kend);     // groups every lane of the wavefront has in full
                        const int row0 = k0 >> 2;
                        uint4 nx = (QSW_PREFETCH && j == 0 && w == 0) ? pf : QS_ADJ(row0);
                        int kk = 0;
                        {
                            uint4 eb;                                         // two groups per trip on two register sets (bp_scatter.hip)
#pragma unroll 1
                            for (; kk + 8 <= kplain; kk += 8) {
                                eb = QS_ADJ(row0 + (kk >> 2) + 1);            // (the table has spare group rows)
                                {
                                    const int sb = kend - 1 - kk, k = k0 + kk;
                                    QS_EDGE_H(nx.x, k, sb, QS_NOFIX, QS_HPA) QS_EDGE_H(nx.y, k + 1, sb - 1, QS_NOFIX, QS_HPB)
                                    QS_EDGE_H(nx.z, k + 2, sb - 2, QS_NOFIX, QS_HPA) QS_EDGE_H(nx.w, k + 3, sb - 3, QS_NOFIX, QS_HPB)
                                }
                                nx = QS_ADJ(row0 + (kk >> 2) + 2);
                                {
                                    const int sb = kend - 5 - kk, k = k0 + kk + 4;
                                    QS_EDGE_H(eb.x, k, sb, QS_NOFIX, QS_HPA) QS_EDGE_H(eb.y, k + 1, sb - 1, QS_NOFIX, QS_HPB)
                                    QS_EDGE_H(eb.z, k + 2, sb - 2, QS_NOFIX, QS_HPA) QS_EDGE_H(eb.w, k + 3, sb - 3, QS_NOFIX, QS_HPB)
                                }
                            }
                        }
#pragma unroll 1
                        for (; kk < kplain; kk += 4) {
                            const uint4 e4 = nx;
                            nx = QS_ADJ(row0 + (kk >> 2) + 1);
                            const int sb = kend - 1 - kk, k = k0 + kk;
                            QS_EDGE_H(e4.x, k, sb, QS_NOFIX, QS_HPA)
                            QS_EDGE_H(e4.y, k + 1, sb - 1, QS_NOFIX, QS_HPB)
                            QS_EDGE_H(e4.z, k + 2, sb - 2, QS_NOFIX, QS_HPA)
                            QS_EDGE_H(e4.w, k + 3, sb - 3, QS_NOFIX, QS_HPB)
                        }
                        // an edge below the smallest degree of the wavefront is real on every lane (no fix), one at or beyond the largest is
                        // nobody's; only in between does a lane have to ask (wave-uniform tests; k < wmax: a group starts below the largest degree)
#define QS_TAIL_EDGE(off, q_)                                                                                     \
                            if (k + (q_) < wmin) QS_EDGE(off, k + (q_), sb - (q_), QS_NOFIX)                      \
                            else if (k + (q_) < wmax) QS_EDGE(off, k + (q_), sb - (q_), QS_TAILFIX)               \
                            else { neww <<= 1; ltw <<= 1; }
#pragma unroll 1
                        for (; kk + 4 < kend; kk += 4) {
                            const uint4 e4 = nx;
                            nx = QS_ADJ(row0 + (kk >> 2) + 1);
                            const int sb = kend - 1 - kk, k = k0 + kk;
                            QS_TAIL_EDGE(e4.x, 0) QS_TAIL_EDGE(e4.y, 1) QS_TAIL_EDGE(e4.z, 2) QS_TAIL_EDGE(e4.w, 3)
                        }
                        if (kk < kend) {              // the word's last group (for rows of 33..36 faults the second word's only one): nothing to request behind it, no copy
                            const int sb = kend - 1 - kk, k = k0 + kk;
                            QS_TAIL_EDGE(nx.x, 0) QS_TAIL_EDGE(nx.y, 1) QS_TAIL_EDGE(nx.z, 2) QS_TAIL_EDGE(nx.w, 3)
                        }
#undef QS_TAIL_EDGE
                        neg[w] = neww;
                        par ^= neww;
                        if (ltw) kst = (uint32_t)(k0 + kend - 1 - (int)__builtin_ctz(ltw));   // a later word's improvement overrides an earlier one's
                    }
                }
