"""The regions of k_loop's bit count on the CPU (tests/count_regions.py has the sets R1..R4): the oracle alone reaches what the sets
are for, and the emulated build of the pass (mp3mi_debug_quantize_count) returns the oracle's values and fields on every granule.
The device runs the same granules (test_gpu_count_regions.py)."""
import numpy as np
import pytest

import count_regions as cr
import quant_edges as qe
from mp3common import Oracle


@pytest.fixture(scope="module")
def sets():
    return {r: cr.Sets(r) for r in qe.RATES}


@pytest.fixture(scope="module")
def oracle_out(sets):
    orc = Oracle()
    return {r: qe.run_oracle(orc.lib, r, S.xr, S.gran) for r, S in sets.items()}


@pytest.mark.parametrize("rate", qe.RATES)
def test_the_sets_reach_what_they_are_for(sets, oracle_out, rate):
    S = sets[rate]
    ix, xo, f = oracle_out[rate]
    assert 300 <= len(S.xr) <= 1200
    assert np.array_equal(xo, S.xr)  # (no rescale plan)
    cr.coverage(S, ix, f)


@pytest.mark.parametrize("rate", qe.RATES)
def test_emulated_pass_is_the_oracle(emu, sets, oracle_out, rate):
    S = sets[rate]
    ix, xo, f = oracle_out[rate]
    idx = np.arange(len(S.xr))
    rc, hix, hxo, hf = qe.run_hook(emu.lib, rate, S.xr, S.gran)
    assert rc == 0
    msg = qe.first_mismatch(S, idx, hix, hxo, hf, ix, xo, f)
    assert msg is None, msg

