"""k_loop's region maxima from per-cell peak lines (csrc/loop_pass.h, loop_count_bits; csrc/mp3mi_dev.h), on the CPU emulator:
the crafted granules of tests/region_peaks.py through the pass's self-test hook against the oracle's quantise + count -- ix,
big_values, count1, the three tables, the region counts, the addresses and the bit count, for equality --, and the property the
fast path rests on, on 2000 random granules: after ANY per-band amplification the line with the largest original |xr| of a cell
holds the cell's largest quantised value, so the maxima taken from the peaks are the maxima taken from all lines."""
import numpy as np
import pytest

import quant_edges as qe
import region_peaks as rp


@pytest.mark.parametrize("rate", qe.RATES)
def test_emulated_pass_with_peak_maxima_is_the_oracle(emu, oracle, rate):
    C, ix, f = rp.run_and_compare(emu.lib, oracle.lib, rate)
    # and the hook's peaks are the pipeline's: the same walk (mp3mi_cell_peak) that k_mdct's tail runs, here on the cases' spectra
    peak, first = rp.peak_lines(emu.lib, rate, C.xr)
    rp.check_peaks_of(C.xr, peak, first, rate)


def maxima_from_peaks(ix, peak, first, n_big, a1, a2, e2):
    """loop_count_bits' fast path, restated: a cell belongs to the region its first line lies in; the cell that starts at or behind
    n_big (and below e2) stands for the one pair in front of e2"""
    v = np.append(ix, 0)[peak]  # (an empty cell names line 576: the zero behind the values)
    cut = (first[:-1] >= n_big) & (first[:-1] < e2)
    v = np.where(cut, ix[e2 - 2:e2].max() if e2 >= 2 else 0, v)
    s = first[:-1]
    return [int(v[s < a1].max(initial=0)), int(v[(s >= a1) & (s < a2)].max(initial=0)), int(v[(s >= a2) & (s < e2)].max(initial=0))]


@pytest.mark.parametrize("rate", qe.RATES)
def test_peak_lines_carry_the_region_maxima_through_any_amplification(emu, rate):
    rng = np.random.default_rng(0xC311 + rate)
    n = 2000 if rate == 44100 else 500  # 2000 at the flagship rate; the other band tables on fewer
    sfb = np.array(qe.SFB_L[rate])
    band_of_line = np.searchsorted(sfb, np.arange(576), side="right") - 1
    xr = rng.laplace(size=(n, 576)) * (10.0 ** rng.uniform(-2, 3, (n, 22)))[:, band_of_line]
    xr[rng.random((n, 576)) < 0.15] = 0.0
    xr[:, :] *= np.exp(-np.arange(576)[None, :] / rng.uniform(20, 2000, (n, 1)))
    dup = rng.random((n, 576)) < 0.1  # ties: a line repeats its neighbour's magnitude with the other sign
    xr[:, 1:] = np.where(dup[:, 1:], -xr[:, :-1], xr[:, 1:])
    peak, first = rp.peak_lines(emu.lib, rate, xr)
    rp.check_peaks_of(xr, peak, first, rate)
    # per-band rescale plans, applied as the search applies them: one rounded multiplication after the other
    n_amp = rng.integers(0, 17, (n, 22))
    n_amp[:, 21] = 0
    pre = rng.integers(0, 2, n)
    y = xr.copy()
    pf = np.array([np.power(qe.SQRT2, p) for p in qe.PRETAB] + [1.0])[band_of_line]
    y = np.where(pre[:, None] == 1, y * pf[None, :], y)
    for k in range(16):
        y = np.where(n_amp[:, band_of_line] > k, y * qe.SQRT2, y)
    q = np.round(4 * np.log2(np.maximum(np.abs(y).max(axis=1), 1e-30) / 10.0 ** rng.uniform(0, 4.4, n))).astype(int)
    q = np.clip(q, qe.Q_LO, qe.Q_HI)
    ix = qe.ix_definition(y, q)
    rows = np.arange(n)
    for c in range(rp.CELLS):
        if first[c + 1] > first[c]:
            assert (ix[rows, peak[:, c]] == ix[:, first[c]:first[c + 1]].max(axis=1)).all(), "cell %d" % c
    # the regions: the run lengths of the quantised values, every pair of band edges a1 <= a2 <= e2 a subdivision could name
    checked = 0
    for g in range(n):
        pairs = ix[g].reshape(288, 2).max(axis=1)
        nz, big = np.flatnonzero(pairs > 0), np.flatnonzero(pairs > 1)
        i0 = 2 * (nz[-1] + 1) if nz.size else 0
        n_big = 2 * (big[-1] + 1) if big.size else 0
        e2 = n_big + ((i0 - n_big) & 3)
        if e2 == 0:
            continue
        cand = sfb[sfb <= e2]
        a1 = int(rng.choice(cand))
        a2 = int(rng.choice(cand[cand >= a1]))
        for a1_, a2_ in ((a1, a2), (min(sfb[8], e2), e2)):
            want = [int(ix[g, :a1_].max(initial=0)), int(ix[g, a1_:a2_].max(initial=0)), int(ix[g, a2_:e2].max(initial=0))]
            assert maxima_from_peaks(ix[g], peak[g], first, n_big, a1_, a2_, e2) == want, (g, a1_, a2_, e2, n_big)
        checked += 1
    assert checked > 0.9 * n
