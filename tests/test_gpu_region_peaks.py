"""k_loop's region maxima from per-cell peak lines on the DEVICE: the crafted granules of tests/region_peaks.py, one launch per
rate, through mp3mi_debug_quantize_count against the oracle's quantise + count for equality (ix, big_values, count1, the tables,
the region counts, the addresses, the bit count); and the peak lines the device records for them against the spectra."""
import pytest

import quant_edges as qe
import region_peaks as rp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rate", qe.RATES)
def test_device_pass_with_peak_maxima_is_the_oracle(product, oracle, rate):
    C, ix, f = rp.run_and_compare(product.lib, oracle.lib, rate)
    peak, first = rp.peak_lines(product.lib, rate, C.xr)
    rp.check_peaks_of(C.xr, peak, first, rate)
