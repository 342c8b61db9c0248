"""k12_feed alone (mp3mi_debug_l12_feed, include/mp3mi_l12.h) on the emulated build: the kernel that cuts the rows of a tick of the
Layer I / II feeder out of rings that keep history, and writes a resumed slot's two history rows out of the same ring.  Five lanes,
three slots, rows of 384 and 1152 samples, mono and stereo, a ring whose length is no multiple of 8 samples; the cases and the numpy
model: kernel_case() of tests/l12_feed.py.  The same cases run on the device in tests/test_gpu_l12_feed.py."""
import os
import shutil
import tempfile

import pytest

from l12_feed import kernel_case
from test_kernel_budgets import HIPCC, resources, the


@pytest.mark.parametrize("row", [384, 1152])
@pytest.mark.parametrize("ch", [1, 2])
def test_l12_feed_kernel_emulated(emu, ch, row):
    kernel_case(emu, ch, row)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_k12_feed_needs_neither_scratch_nor_lds():
    """k_format.hip compiled for gfx950 with the compiler's resource remarks (no GPU)"""
    tmp = tempfile.mkdtemp(prefix="mp3mi_budget_l12_feed_")
    try:
        kernels = resources("k_format", tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    k = the(kernels, r"^_Z\d+k12_feedP")
    assert k["ScratchSize"] == 0 and k["LDS"] == 0, k
