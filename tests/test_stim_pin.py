"""quits_amd/dem.py against Stim's own detector error models and samples, through files (tools/pin_stim.py writes them where Stim is at
hand: tests/golden/stim_pin/<name>.dem[.gz], <name>.b8).  While no pin file is here the same comparison runs on a stand-in: the own model
printed with six digits, and 4096 shots drawn from it on the host, so that the tolerance logic below is exercised either way.

Tolerances.  A prior: the file prints every probability rounded to some digit, so it is off by at most half a unit of that digit; the
other half unit covers the second rounding on this side (the extractor's double is itself a rounded value).  A column of the check matrix
folds the entries that share its detectors by p <- p(1 - q) + q(1 - p), which moves by at most |dq| when q moves, so a column's tolerance
is the sum of its entries' units.  A marginal: 5 sigma of the binomial at the model's own marginal, N = the file's shots."""
import glob
import gzip
import os
import re

import numpy as np
import pytest

import helpers
from quits_amd.decoder.base import detector_error_model_to_matrix
from quits_amd.dem import Circuit, dem_to_text, parse_dem
from quits_amd.samples import read_shots, write_shots

PIN = os.path.join(helpers.GOLD, "stim_pin")
SAMPLED = ("bb72_custom_r6_p0.003", "hgp225_cardinal_r3_p0.01")


def _last_digit_unit(literal):
    """The literal with every mantissa digit zeroed but the last, which becomes 1: '0.00123' -> '0.00001', '1.25e-05' -> '0.01e-05'."""
    m = re.fullmatch(r"([0-9.]*?)([0-9])(\.?)([eE][-+]?[0-9]+)?", literal.strip())
    assert m, literal
    return re.sub(r"[0-9]", "0", m.group(1)) + "1" + m.group(3) + (m.group(4) or "")


def units_text(text):
    """The same model with every probability replaced by one unit of its last printed digit: parsed, it carries each entry's tolerance."""
    return re.sub(r"(?i)(error\s*(?:\[[^\]]*\])?\s*\()([^)]*)(\))", lambda m: m.group(1) + _last_digit_unit(m.group(2)) + m.group(3), text)


def compare_dem_text(text, own):
    """Stim-made (or stand-in) DEM text against the own extractor's model: matrices column for column, priors to one unit per folded entry."""
    theirs = parse_dem(text)
    assert (theirs.num_detectors, theirs.num_observables) == (own.num_detectors, own.num_observables)
    H1, L1, p1 = detector_error_model_to_matrix(theirs)
    H0, L0, p0 = detector_error_model_to_matrix(own)
    assert helpers.same_sparse(H1, H0), "check matrices differ"
    assert helpers.same_sparse(L1, L0), "observable matrices differ"
    units = parse_dem(units_text(text))
    assert len(units.errors) == len(theirs.errors)
    tol = np.zeros(H0.shape[1])
    col_of = {}
    for (u, dets, _), (_, dets_t, _) in zip(units.errors, theirs.errors):
        assert dets == dets_t
        tol[col_of.setdefault(frozenset(dets), len(col_of))] += u
    assert len(col_of) == H0.shape[1]
    worst = np.abs(p1 - p0) / tol
    print("priors: %d columns, largest |difference| / tolerance = %.3f" % (len(tol), worst.max()))
    assert (np.abs(p1 - p0) <= tol).all(), "column %d: %r vs %r, tolerance %g" % (int(worst.argmax()), p1[worst.argmax()], p0[worst.argmax()], tol[worst.argmax()])


def model_marginals(H, priors):
    """P(detector i fires) = (1 - prod over its faults of (1 - 2 p_j)) / 2 for independent faults."""
    A = H.tocsr()
    logs = np.log1p(-2.0 * np.asarray(priors))
    return np.array([(1.0 - np.exp(logs[A.indices[A.indptr[i]:A.indptr[i + 1]]].sum())) / 2.0 for i in range(A.shape[0])])


def compare_sampled_file(path, own):
    H, L, pri = detector_error_model_to_matrix(own)
    rec = read_shots(path, "b8", own.num_detectors, own.num_observables)
    N = len(rec)
    assert N > 0
    for mat, field in ((H, rec.field(0, own.num_detectors)), (L, rec.field(own.num_detectors, own.num_observables))):
        q = model_marginals(mat, pri)
        seen = np.asarray(field).mean(axis=0)
        sigma = np.sqrt(q * (1.0 - q) / N)
        z = np.abs(seen - q) / np.maximum(sigma, 1e-300)
        print("%s: %d shots, %d marginals, largest deviation %.2f sigma" % (os.path.basename(path), N, len(q), z.max()))
        assert (np.abs(seen - q) <= 5.0 * sigma).all(), "bit %d: %.5f seen, %.5f modelled" % (int(z.argmax()), seen[z.argmax()], q[z.argmax()])


_OWN = {}


def own_dem(name):
    if name not in _OWN:
        _OWN[name] = Circuit(helpers.circuit_text(name)).detector_error_model()
    return _OWN[name]


def _pin_files(pattern):
    return sorted(glob.glob(os.path.join(PIN, pattern)))


def test_stim_pin_files_match_the_own_extractor_and_sampler():
    """Every pin file that is here (none until tools/pin_stim.py has run where Stim is; the stand-in below runs the same code meanwhile)."""
    for path in _pin_files("*.dem") + _pin_files("*.dem.gz"):
        text = gzip.open(path, "rb").read().decode() if path.endswith(".gz") else open(path).read()
        compare_dem_text(text, own_dem(os.path.basename(path).split(".dem")[0]))
    for path in _pin_files("*.b8"):
        compare_sampled_file(path, own_dem(os.path.basename(path)[:-3]))


@pytest.mark.parametrize("name", SAMPLED)
def test_stand_in_goes_through_the_same_comparison(name, tmp_path):
    """No Stim here: the own model printed with six digits stands in for Stim's file, host-drawn shots of it for Stim's samples.  A prior
    moved by three units of its last printed digit, and a detector that fires far too often, must both be caught."""
    own = own_dem(name)
    text = dem_to_text(own, digits=6)
    compare_dem_text(text, own)
    # ... and the tolerance bites: move the first probability by three units of its last digit
    first = re.search(r"error\(([^)]*)\)", text).group(1)
    with pytest.raises(AssertionError, match="column 0"):
        compare_dem_text(text.replace("error(%s)" % first, "error(%s)" % _bump(first), 1), own)
    H, L, pri = detector_error_model_to_matrix(own)
    rng = np.random.default_rng(1)
    shots = 4096
    e = (rng.random((shots, len(pri))) < pri[None, :]).astype(np.uint8)
    det = np.asarray((H.tocsr() @ e.T.astype(np.int32)).T % 2, dtype=np.uint8)
    obs = np.asarray((L.tocsr() @ e.T.astype(np.int32)).T % 2, dtype=np.uint8)
    path = str(tmp_path / (name + ".b8"))
    write_shots(path, np.concatenate([det, obs], axis=1), "b8")
    assert os.path.getsize(path) == shots * ((own.num_detectors + own.num_observables + 7) // 8)
    compare_sampled_file(path, own)
    det[:, 0] |= (rng.random(shots) < 0.2).astype(np.uint8)
    write_shots(path, np.concatenate([det, obs], axis=1), "b8")
    with pytest.raises(AssertionError, match="bit 0"):
        compare_sampled_file(path, own)


def _bump(literal):
    """The literal plus three units of its last digit, printed with the same number of digits after the point / the same exponent."""
    m = re.fullmatch(r"([0-9.]+)([eE][-+]?[0-9]+)?", literal)
    mant, exp = m.group(1), m.group(2) or ""
    decimals = len(mant.split(".")[1]) if "." in mant else 0
    return "%.*f%s" % (decimals, float(mant) + 3.0 * 10.0 ** -decimals, exp)
