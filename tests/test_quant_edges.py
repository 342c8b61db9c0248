"""k_loop's quantise+count pass at its edges, on the CPU (tests/quant_edges.py has the sets S1..S7): the oracle's quantize() +
count_bits() against the plain definition of the quantiser and against the unmodified reference's own functions, and the
emulated build of the pass (mp3mi_debug_quantize_count) against the oracle on a fixed subsample.  The device runs every granule
(test_gpu_quant_edges.py)."""
import os

import numpy as np
import pytest

import quant_edges as qe
from mp3common import Mp3mi, Oracle

EMU_PER_SET = 150  # granules of every set and rate through the emulated build: ~13 s for the three rates


@pytest.fixture(scope="module")
def sets():
    return {r: qe.Sets(r) for r in qe.RATES}


@pytest.fixture(scope="module")
def oracle_out(sets):
    orc = Oracle()
    return {r: qe.run_oracle(orc.lib, r, S.xr, S.gran) for r, S in sets.items()}


@pytest.mark.parametrize("rate", qe.RATES)
def test_oracle_quantiser_is_the_definition(sets, oracle_out, rate):
    """ix = min(2047, max{p : tab[p] <= |xr| / step}) on every line of S1..S3 (on the rescaled xr), and the boundary lines
    really straddle: both sides of every boundary p = 1..2047 occur in S1"""
    S = sets[rate]
    ix, xo, _ = oracle_out[rate]
    sel = np.flatnonzero(np.isin(S.set, ["S1", "S2", "S3"]))
    want = qe.ix_definition(xo[sel], S.gran[sel, 0])
    bad = np.flatnonzero((want != ix[sel]).any(axis=1))
    assert bad.size == 0, "granule %d (%s): the oracle's pow_nint is not the definition" % (sel[bad[0]], S.set[sel[bad[0]]])
    s1 = S.set == "S1"
    for p in (1, 2, 15, 16, 1000, 2046, 2047):
        assert (ix[s1] == p).any() and (ix[s1] == p - 1).any(), p


@pytest.mark.skipif(not os.path.exists(qe.REF_HARNESS_QC), reason="oracle/_ref/ref_harness_qc is built only where the reference sources are")
@pytest.mark.parametrize("rate", qe.RATES)
def test_oracle_is_the_unmodified_reference(sets, oracle_out, rate):
    """every field of every granule of S1..S7: the oracle's quantize() / count_bits() against the reference's own"""
    S = sets[rate]
    ix, xo, f = oracle_out[rate]
    rix, rf = qe.run_reference(rate, xo, S.gran)
    bad = np.flatnonzero((rix != ix).any(axis=1) | (rf != f).any(axis=1))
    assert bad.size == 0, "granule %d (%s): ix %s, fields %s vs the reference's %s" % (
        bad[0], S.set[bad[0]], np.array_equal(rix[bad[0]], ix[bad[0]]), f[bad[0]].tolist(), rf[bad[0]].tolist())


@pytest.mark.parametrize("rate", qe.RATES)
def test_emulated_pass_is_the_oracle(sets, oracle_out, rate):
    """the emulated build's hook (k_loop's own pass, first and rare tier) against the oracle: every line, every field"""
    S = sets[rate]
    ix, xo, f = oracle_out[rate]
    idx = S.subsample(EMU_PER_SET)
    rc, hix, hxo, hf = qe.run_hook(Mp3mi(emu=True).lib, rate, S.xr[idx], S.gran[idx])
    assert rc == 0
    msg = qe.first_mismatch(S, idx, hix, hxo, hf, ix[idx], xo[idx], f[idx])
    assert msg is None, msg


def test_hook_refuses_what_it_cannot_run():
    lib = Mp3mi(emu=True).lib
    xr = np.zeros((1, 576))
    for gran in ([0, 0, 0, 0], [-401, 0, 0, 0], [401, 0, 0, 0], [0, 4, 0, 0], [0, 0, 17, 0], [0, 2, 0, 1], [0, 0, 0, 2]):
        rc, _, _, _ = qe.run_hook(lib, 44100 if gran != [0, 0, 0, 0] else 22050, xr, np.array([gran], np.int32))
        assert rc == -1, gran
