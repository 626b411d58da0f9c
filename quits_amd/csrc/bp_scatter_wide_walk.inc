// bp_scatter_wide_walk.inc -- the edge walk of one gather pass of one check (bp_scatter_wide.hip), as program text: included by
// qd_bp_scatter_wide_kernel for every pass and by qd_bp_first_pass_kernel, which runs pass 0 once per decoder -- the same QS_EDGE_M
// steps (bp_scatter_edge.h, with QS_MAG_MASK and QS_SIGN_TOP), trip counts, tail rules and argmin rule, so the table cannot drift from what the loop would have found.
// Two forms of one text, chosen by the includer's QS_WALK(part) (bp_scatter_edge.h: #define QS_WALK(p_) QS_CMP_##p_ or QS_KEY_##p_).  The compare form
// (QS_EDGE_M: a bit history `ltw` of the strict improvements, a1 / a2 the minima) and the key form for rows of at most 64 faults (QS_EDGE_K: a1 / a2 collect
// position-carrying keys, there is no `ltw`, and the walk ends with QS_KEYS_DECODE, which leaves a1, a2, kst as the compare form would and `keys_ok_` --
// false where some lane's second key is too large to be exact; the includer then walks the round again in the compare form: the walk writes locals only).
// In scope at the point of inclusion: j, dws, cs, S1, S2, KOLD, dcs, O, pf, a1, a2, kst, adj_row, QS_ADJ, QS_ACC.  Leaves hp, par, neg[].
// "Is this the edge my last minimum came from" (min2 goes back on that edge, min1 on the others) is asked through lane masks in scalar registers, not per edge
// on the vector ALU: lq[q] once per check and pass, gsel_ once per group of four edges (the group index is wave-uniform in all four loop forms), their AND
// on the scalar unit, one v_cndmask per edge that takes the scalar pair -- 8-edge block of <512,8,2,2>: 101 -> 95 vector instructions (profiles/bp_argmin_masks_ab.txt).
// The masks are ballots, so lanes that are off (act[j], a partial last wavefront) contribute 0 and read nothing.
                // (the round's loop bounds are re-derived from one scalar every pass: hoisted out of the iteration loop they, and everything computed
                //  from them for CPL rounds x NSW words, outgrow the scalar registers and come back through v_readlane)
                int dwj = dws[j];
                asm volatile("" : "+s"(dwj));
                const int trip = dwj & 0xFF, wmax = (dwj >> 8) & 0xFF, wmin = (dwj >> 16) & 0xFF, wmin4 = wmin & ~3;
                const int adj_voff = cs[j] * 16;
                const float s1 = S1[j], s2 = S2[j];
                // the old argmin edge as lane masks (QS_MAG_MASK): position kold = 4 khi + klo; "none" (0xFFFFFFFF) has a khi no group reaches
                const uint32_t khi = KOLD[j] >> 2, klo = KOLD[j] & 3u;
                const unsigned long long lq[4] = {__builtin_amdgcn_ballot_w64(klo == 0u), __builtin_amdgcn_ballot_w64(klo == 1u),
                                                  __builtin_amdgcn_ballot_w64(klo == 2u), __builtin_amdgcn_ballot_w64(klo == 3u)};
#define QS_GSEL(k_) const unsigned long long gsel_ = __builtin_amdgcn_ballot_w64(khi == (uint32_t)((k_) >> 2));
                const int dc = dcs[j];
                uint32_t hp = 0u, hpa = 0u, par = 0u;
                uint32_t neg[NSW];
#pragma unroll
                for (int w = 0; w < NSW; ++w) {
                    neg[w] = 0u;
                    const int k0 = 32 * w;
                    if (k0 < trip) {
                        const int kend = min(trip - k0, 32);                  // multiple of 4
                        // One register for the signs sent last time and the signs collected now.  The sent word O[j][w] has edge i of the word at bit
                        // kend - 1 - i; shifted left by 32 - kend (0 for a full word: & 31) edge 0 stands at bit 31, where QS_SIGN_TOP reads it.  Every position
                        // of the walk -- an edge's v_alignbit, a pad position's shift -- then moves the word up by one and enters its new sign at bit 0, so
                        // the next edge's sent sign is at bit 31 when that edge asks.  After the word's kend positions the kend new signs fill bits
                        // kend - 1 .. 0 and everything the word started with has left at the top: the sent signs, and whatever `flip` set above bit
                        // kend - 1 of O (all ones for a check with syndrome ^ parity = 1), which the pre-shift already dropped; the 32 - kend zeros the
                        // pre-shift brought in at the bottom are the bits above kend - 1 now.  The result is bit for bit the word that started from 0.
                        // (Lanes past their degree collect QS_BIG's sign, 0, whatever they read as the sent sign; the first-pass table walks with O = 0.)
                        uint32_t neww = O[j][w] << ((32 - kend) & 31);
                        QS_WALK(WORD_BEGIN)
                        const int kplain = min(max(wmin4 - k0, 0), kend);     // groups every lane of the wavefront has in full
                        const int row0 = k0 >> 2;
                        uint4 nx = (j == 0 && w == 0) ? pf : QS_ADJ(row0);
                        int kk = 0;
                        {
                            uint4 eb;                                         // two groups per trip on two register sets: the next group's offsets are requested while this one is worked on, without copying them
#pragma unroll 1
                            for (; kk + 8 <= kplain; kk += 8) {
                                eb = QS_ADJ(row0 + (kk >> 2) + 1);            // (the table has spare group rows)
                                {
                                    const int k = k0 + kk;
                                    QS_GSEL(k)
                                    QS_WALK(EDGE)(nx.x, k, QS_SIGN_TOP, QS_NOFIX, QS_HPA, QS_MAG_MASK(0)) QS_WALK(EDGE)(nx.y, k + 1, QS_SIGN_TOP, QS_NOFIX, QS_HPB, QS_MAG_MASK(1))
                                    QS_WALK(EDGE)(nx.z, k + 2, QS_SIGN_TOP, QS_NOFIX, QS_HPA, QS_MAG_MASK(2)) QS_WALK(EDGE)(nx.w, k + 3, QS_SIGN_TOP, QS_NOFIX, QS_HPB, QS_MAG_MASK(3))
                                }
                                nx = QS_ADJ(row0 + (kk >> 2) + 2);
                                {
                                    const int k = k0 + kk + 4;
                                    QS_GSEL(k)
                                    QS_WALK(EDGE)(eb.x, k, QS_SIGN_TOP, QS_NOFIX, QS_HPA, QS_MAG_MASK(0)) QS_WALK(EDGE)(eb.y, k + 1, QS_SIGN_TOP, QS_NOFIX, QS_HPB, QS_MAG_MASK(1))
                                    QS_WALK(EDGE)(eb.z, k + 2, QS_SIGN_TOP, QS_NOFIX, QS_HPA, QS_MAG_MASK(2)) QS_WALK(EDGE)(eb.w, k + 3, QS_SIGN_TOP, QS_NOFIX, QS_HPB, QS_MAG_MASK(3))
                                }
                            }
                        }
#pragma unroll 1
                        for (; kk < kplain; kk += 4) {
                            const uint4 e4 = nx;
                            nx = QS_ADJ(row0 + (kk >> 2) + 1);
                            const int k = k0 + kk;
                            QS_GSEL(k)
                            QS_WALK(EDGE)(e4.x, k, QS_SIGN_TOP, QS_NOFIX, QS_HPA, QS_MAG_MASK(0))
                            QS_WALK(EDGE)(e4.y, k + 1, QS_SIGN_TOP, QS_NOFIX, QS_HPB, QS_MAG_MASK(1))
                            QS_WALK(EDGE)(e4.z, k + 2, QS_SIGN_TOP, QS_NOFIX, QS_HPA, QS_MAG_MASK(2))
                            QS_WALK(EDGE)(e4.w, k + 3, QS_SIGN_TOP, QS_NOFIX, QS_HPB, QS_MAG_MASK(3))
                        }
                        // an edge below the smallest degree of the wavefront is real on every lane (no fix), one at or beyond the largest is
                        // nobody's; only in between does a lane have to ask (wave-uniform tests; k < wmax: a group starts below the largest degree)
#define QS_TAIL_EDGE(off, q_)                                                                                     \
                            if (k + (q_) < wmin) QS_WALK(EDGE)(off, k + (q_), QS_SIGN_TOP, QS_NOFIX, QS_HP1, QS_MAG_MASK(q_))         \
                            else if (k + (q_) < wmax) QS_WALK(EDGE)(off, k + (q_), QS_SIGN_TOP, QS_TAILFIX, QS_HP1, QS_MAG_MASK(q_))  \
                            else QS_WALK(PAD)
#pragma unroll 1
                        for (; kk + 4 < kend; kk += 4) {
                            const uint4 e4 = nx;
                            nx = QS_ADJ(row0 + (kk >> 2) + 1);
                            const int k = k0 + kk;
                            QS_GSEL(k)
                            QS_TAIL_EDGE(e4.x, 0) QS_TAIL_EDGE(e4.y, 1) QS_TAIL_EDGE(e4.z, 2) QS_TAIL_EDGE(e4.w, 3)
                        }
                        if (kk < kend) {              // the word's last group (for rows of 33..36 faults the second word's only one): nothing to request behind it, no copy
                            const int k = k0 + kk;
                            QS_GSEL(k)
                            QS_TAIL_EDGE(nx.x, 0) QS_TAIL_EDGE(nx.y, 1) QS_TAIL_EDGE(nx.z, 2) QS_TAIL_EDGE(nx.w, 3)
                        }
#undef QS_TAIL_EDGE
                        neg[w] = neww;
                        par ^= neww;
                        QS_WALK(WORD_END)(k0, kend)
                    }
                }
#undef QS_GSEL
                QS_WALK(END)(trip)
