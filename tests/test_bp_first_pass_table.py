"""The first-pass table of the several-checks-per-lane min-sum kernel (ScatArgs::first_pass, bp_scatter_wide.hip), restated in plain
numpy for the headline window: what gather pass 0 finds for a check when nothing has been sent -- the two smallest |L| over its
faults, the position of the first smallest one in column order, the sign of every L and their parity.  No device: this pins the
record's meaning (a1 <= a2, argmin inside the row, sign words that fit the row) before any GPU call reads it."""
import numpy as np

import helpers
import oracle as orc


def first_pass_table(H, priors, max_iter):
    """Per check (row of H, faults in column order): a1, a2 in grid units, argmin position, sign bits (1 = L <= 0), parity."""
    k, _ = orc.grid_bits(priors, max_iter)
    pri = np.asarray(priors, dtype=np.float64)
    Lg = np.rint(np.ldexp(np.log((1.0 - pri) / pri), k)).astype(np.int64)      # the channel LLRs on the 2^-k grid, in grid units
    Hr = H.tocsr()
    Hr.sort_indices()
    rows = []
    for i in range(Hr.shape[0]):
        cols = Hr.indices[Hr.indptr[i]:Hr.indptr[i + 1]]
        mag = np.abs(Lg[cols])
        kst = int(np.argmin(mag))                      # first occurrence = the last strict improvement of a walk in this order
        rest = np.delete(mag, kst)
        neg = (Lg[cols] <= 0).astype(np.uint8)
        rows.append((int(mag[kst]), int(rest.min()), kst, neg, int(neg.sum() & 1), len(cols)))
    return k, rows


def test_first_pass_table_of_the_headline_window():
    H, L, pri = helpers.dem_matrices("bb144_custom_r12_p0.003")
    k, rows = first_pass_table(H, pri, 50)
    assert k >= 10 and len(rows) == 1008
    for a1, a2, kst, neg, par, deg in rows:
        assert 0 < a1 <= a2 < (1 << 22)                # magnitudes an int32 accumulator and a float hold exactly
        assert 2 <= deg <= 64 and 0 <= kst < deg       # two sign words; the argmin is an edge of the row
        assert neg.size == deg and not neg.any() and par == 0      # p < 0.5 everywhere: no sign set, even parity
    # a prior above one half sets the sign bit of its edges and flips the parity of the checks it touches
    pri2 = np.array(pri, dtype=np.float64)
    j = int(H.tocsr()[0].indices[0])
    pri2[j] = 0.75
    _, rows2 = first_pass_table(H, pri2, 50)
    touched = set(H.tocsc()[:, j].indices.tolist())
    for i, (a1, a2, kst, neg, par, deg) in enumerate(rows2):
        assert a1 <= a2 and kst < deg
        assert par == (1 if i in touched else 0) and int(neg.sum()) == (1 if i in touched else 0)
