"""The regions of k_loop's bit count on the DEVICE (mp3mi_debug_quantize_count, csrc/k_loop_qc.hip) against the oracle on every
granule of the sets R1..R4 (tests/count_regions.py) at every rate: ix and every field, bit for bit -- subdivide by classes of
big_values at every big_values, every step count and walk variant of every region, the count1 region at its step boundaries,
start and stop blocks.  The sets' coverage is asserted from the oracle's outputs."""
import numpy as np
import pytest

import count_regions as cr
import quant_edges as qe
from mp3common import Oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rate", qe.RATES)
def test_device_regions_are_the_oracle(product, rate):
    S = cr.Sets(rate)
    ix, xo, f = qe.run_oracle(Oracle().lib, rate, S.xr, S.gran)
    cr.coverage(S, ix, f)
    idx = np.arange(len(S.xr))
    rc, hix, hxo, hf = qe.run_hook(product.lib, rate, S.xr, S.gran)
    assert rc == 0
    msg = qe.first_mismatch(S, idx, hix, hxo, hf, ix, xo, f)
    assert msg is None, msg
