"""Granules built for the way k_loop takes its region maxima (csrc/loop_pass.h, loop_count_bits; csrc/mp3mi_dev.h, peak cells): one
read per cell, at the line of the cell whose |xr| is largest, instead of a walk over the region.  What can go wrong there: the
cell that the end of the big-values region cuts, the fallback to the walks (big_values == 0, an address past the region's end),
a peak at the edge of its cell, ties, the cells above the last scalefactor band, and whether the peak of the ORIGINAL spectrum
still names the cell's largest value after pre-emphasis and amplification.

Everything is generated here, deterministically, from tests/quant_edges.py's helpers (imported, not copied).  Used by
tests/test_emu_region_peaks.py (CPU emulator) and tests/test_gpu_region_peaks.py (device).

Two things the issue's list of cases asks for do not exist and are replaced by what does, not dropped:
  * e2 - n_big of 1 and 3: n_big (lines up to the last PAIR holding a value above 1) and i0 (lines up to the last non-zero pair) are
    both even, so e2 = n_big + ((i0 - n_big) & 3) is n_big or n_big + 2.  The sweep instead puts the last value above 1 at each of the
    four lines around a band edge (and around a pair inside a band) and the last non-zero line 0..7 lines behind it: every
    alignment of the two run lengths, both values of e2 - n_big among them.
  * a region maximum of 8191 + 14: the quantiser's table ends at 2047 (ix = min(2047, ..)), the largest value a line can take; the
    case uses a line far above the table's end, which arms the clamp.
And one goes another way: the self-test hook (like the oracle's entry point it is compared with) amplifies EVERY band n_amp times,
so "every band amplified a different number of times" cannot be put through it.  Through the hook: n_amp 0..16 with and without
pre-emphasis (which scales bands 11..20 by four different factors) on spectra whose largest lines sit ABOVE the last band -- never
scaled -- so that the largest quantised value moves into the scaled bands as n_amp grows.  Per-band amplification counts are what
the property test of test_emu_region_peaks.py draws."""
import numpy as np

import quant_edges as qe

CELLS = 32


def cell_edges(rate):
    """first lines of the 32 peak cells and, last, 576 (csrc/mp3mi_dev.h, mp3mi_peak_cell): bands 0..20 and the lines above them, each
    cut into cells of at most 32 lines, in line order; the cells behind the last one are empty (first line 576)"""
    sfb = qe.SFB_L[rate]
    first = [lo + k for lo, hi in zip(sfb[:-1], sfb[1:]) for k in range(0, hi - lo, 32)]
    assert len(first) <= CELLS
    return first + [576] * (CELLS + 1 - len(first))


class Cases:
    """.xr (N, 576), .gran (N, 4) [q, block_type, n_amp, pre], .set (N,) case names, .rate -- the attributes quant_edges.first_mismatch reads"""

    def __init__(self, rate, seed=0x9EA4):
        self.rate = rate
        self.rng = np.random.default_rng(seed + rate)
        self.xr, self.gran, self.set = [], [], []
        self.expect = []  # (granule, oracle field, value): what a case is FOR, checked on the oracle's output
        self.build()
        self.xr = np.ascontiguousarray(np.stack(self.xr))
        self.gran = np.ascontiguousarray(np.array(self.gran, np.int32))
        self.set = np.array(self.set)

    def add(self, name, xr, q=0, bt=0, n_amp=0, pre=0, expect=()):
        for field, value in expect:
            self.expect.append((len(self.xr), field, value))
        self.xr.append(np.asarray(xr, np.float64))
        self.gran.append([q, bt, n_amp, pre])
        self.set.append(name)

    def vals(self, name, vals, q=0, bt=0, signs=True, expect=()):
        """a granule that quantises to vals at step q (every line in the middle of its cell of the quantiser's table)"""
        xr = qe.mid_cell(np.asarray(vals, np.int64), qe.step_of(q))
        if signs:
            xr = xr * np.where(self.rng.random(576) < 0.5, -1.0, 1.0)
        self.add(name, xr, q, bt, expect=expect)

    def build(self):
        rng, sfb, edges = self.rng, qe.SFB_L[self.rate], cell_edges(self.rate)
        # (a) the cut cell.  Values above 1 up to line b - 1, the pair (b, b + 1) as given, a 1 at line b + 5: i0 = b + 6, n_big = b,
        # one count1 quadruple, e2 = b + 2.  Long blocks: for every band edge b from 24 on (bands of at least six lines) the cut pair ends a
        # longer region 2.  Start / stop blocks: b = sfb_l[8] = address1, region 1 is that pair alone.
        for pair in ((0, 0), (1, 0), (0, 1)):
            for b in [e for e in sfb[6:22] if e + 6 <= 576]:
                v = np.zeros(576, np.int64)
                v[:b] = rng.integers(0, 4, b)
                v[b - 1] = 2
                v[b], v[b + 1] = pair
                v[b + 5] = 1
                self.vals("cut", v, q=int(rng.integers(-40, 40)), expect=(("big_values", (b + 2) // 2), ("count1", 1)))
            # (subdivide names an address2 two lines below e2 only at e2 = 10: regions [0, 4), [4, 8), [8, 10).  Band 2 is lines 8..11:
            # its later 1 sits at line 11, inside the count1 quadruple 10..13 that a 1 at line 13 closes)
            v = np.zeros(576, np.int64)
            v[:8] = rng.integers(2, 6, 8)
            v[8], v[9] = pair
            v[11], v[13] = 1, 1
            self.vals("cut", v, expect=(("big_values", 5), ("count1", 1), ("address1", 4), ("address2", 8), ("table_select2", 1 if max(pair) else 0)))
            for bt in (1, 3):
                b = sfb[8]
                v = np.zeros(576, np.int64)
                v[:b] = rng.integers(0, 4, b)
                v[b - 1] = 3
                v[b], v[b + 1] = pair
                v[b + 5] = 1
                self.vals("cut-wsf", v, bt=bt, expect=(("big_values", (b + 2) // 2), ("address1", b), ("address2", b + 2),
                                                       ("table_select1", 1 if max(pair) else 0)))
        # the two run lengths in every alignment: the last value above 1 at line L around a band edge / a pair inside a band,
        # the last non-zero line d lines behind it
        for base in (sfb[9], sfb[12] + 6):
            for L in (base - 2, base - 1, base, base + 1):
                for d in range(8):
                    v = np.zeros(576, np.int64)
                    v[:L] = rng.integers(0, 3, L)
                    v[L] = 2
                    if d:
                        v[L + d] = 1
                    self.vals("runs", v, bt=(0, 1, 3)[(L + d) % 3])
        # a peak on the first and on the last line of every cell (line 575 among them), alone above a floor of twos: another
        # line read in its place changes the region's table
        for c in range(CELLS):
            if edges[c + 1] > edges[c]:
                for line in (edges[c], edges[c + 1] - 1):
                    v = np.full(576, 2, np.int64)
                    v[line] = 9
                    self.vals("edge", v, q=int(rng.integers(-40, 40)))
        # ties: two and three lines of a band equal in |xr|, signs mixed (+x against -x), anywhere in the band
        for c in (3, 8, 14, 20, 22):  # (cells, not bands: every cell lies inside one band)
            for n in (2, 3):
                xr = qe.mid_cell(np.full(576, 2, np.int64), 1.0)
                lines = np.sort(rng.choice(np.arange(edges[c], edges[c + 1]), n, replace=False))
                xr[lines] = qe.mid_cell(np.array(17), 1.0) * np.array([1.0, -1.0, 1.0])[:n]
                self.add("tie", xr)
        # big_values == 0: ones spread over everything the addresses of an earlier granule would cover (the hook starts every
        # granule from cleared addresses, so the stale ones cannot be staged; the fallback is reached by an address past e2, below)
        for p in (0.1, 0.5, 1.0):
            for bt in (0, 1, 3):
                v = (rng.random(576) < p).astype(np.int64)
                v[575] = 1  # i0 = 576, a multiple of four: quadruples all the way down
                self.vals("ones", v, bt=bt, expect=(("big_values", 0),))
                v = v.copy()
                v[574:] = 0
                v[573] = 1  # i0 = 574: the quadruples leave one pair of values <= 1 as the big-values region, below every address
                self.vals("ones", v, bt=bt, expect=(("big_values", 1),))
        # an address past the end of the big-values region: e2 below the first band edges (long), below sfb_l[8] (start / stop);
        # ones behind it, inside what the addresses cover
        for e2 in (2, 4, 6, 10, 20, 34):
            for bt in (0, 1, 3):
                v = (rng.random(576) < 0.6).astype(np.int64)
                v[:e2] = rng.integers(0, 20, e2)
                v[e2 - 1] = 5
                v[e2], v[e2 + 1] = 1, 1
                v[574:] = (0, 0) if e2 % 4 else (0, 1)  # (i0 - e2 a multiple of four: the quadruples end on e2)
                v[573] = 1
                self.vals("past", v, bt=bt, expect=(("big_values", e2 // 2),))
        self.add("zero", np.zeros(576))
        # the rescale plan: the largest lines sit above the last band, where nothing is scaled; the bands below them grow by
        # sqrt(2)^n_amp (and by pre-emphasis: four different factors), so the largest value moves from cell to cell
        k = np.arange(576)
        for n_amp in range(17):
            for pre in (0, 1):
                scale = np.repeat(10.0 ** rng.uniform(-0.5, 0.5, 22), np.diff(sfb))
                xr = rng.laplace(size=576) * scale * 40.0
                xr[sfb[21]:] *= 2.0 ** rng.uniform(0.0, 0.5 * n_amp + 1.0)
                q = int(np.clip(np.round(4 * np.log2(np.abs(xr).max() * 2.0 ** (0.5 * n_amp) / 60.0 ** (4.0 / 3.0))), -100, 200))
                self.add("amp", xr, q, bt=(0, 0, 1, 3)[n_amp % 4], n_amp=n_amp, pre=pre)
        # region maxima of exactly 15, of 16 (the first table with linbits) and at the quantiser's clamp, in each region
        lo, hi = sfb[6], sfb[15]
        for m in (15, 16, 2047):
            for r, (a, b) in enumerate(((0, lo), (lo, hi), (hi, 576))):
                v = rng.integers(0, 15, 576)
                v[575] = 14
                v[int(rng.integers(a, b))] = m
                xr = qe.mid_cell(v, 1.0)
                if m == 2047:
                    xr[v == m] = qe.TAB[2047] * 1e4
                self.add("max", xr)
        # short blocks: the untouched path
        for m in (3, 40):
            self.vals("short", rng.integers(0, m, 576), bt=2)


def check_expectations(C, f_oracle):
    """the cases are what they claim to be, on the ORACLE's output (independent of the code under test)"""
    F = {n: i for i, n in enumerate(qe.ORACLE_FIELDS)}
    for g, field, value in C.expect:
        assert f_oracle[g, F[field]] == value, "case %d (%s): %s is %d, built for %d" % (g, C.set[g], field, f_oracle[g, F[field]], value)
    past = np.flatnonzero(C.set == "past")
    assert (f_oracle[past, F["address1"]] > 2 * f_oracle[past, F["big_values"]]).any()


def run_and_compare(lib, orc_lib, rate):
    C = Cases(rate)
    ix, xo, f = qe.run_oracle(orc_lib, rate, C.xr, C.gran)
    check_expectations(C, f)
    rc, hix, hxo, hf = qe.run_hook(lib, rate, C.xr, C.gran)
    assert rc == 0, rc
    msg = qe.first_mismatch(C, np.arange(len(C.xr)), hix, hxo, hf, ix, xo, f)
    assert msg is None, msg
    return C, ix, f


def peak_lines(lib, rate, xr):
    """mp3mi_debug_peak_lines: (peaks (N, 32), first lines of the cells and 576)"""
    import ctypes
    xr = np.ascontiguousarray(xr, np.float64)
    peak = np.zeros((len(xr), CELLS), np.uint16)
    first = np.zeros(CELLS + 1, np.int32)
    lib.mp3mi_debug_peak_lines.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    rc = lib.mp3mi_debug_peak_lines(rate, len(xr), xr.ctypes.data, peak.ctypes.data, first.ctypes.data)
    assert rc == 0, rc
    return peak.astype(np.int64), first.astype(np.int64)


def check_peaks_of(xr, peak, first, rate):
    """every cell's peak lies in the cell and no line of the cell is larger; the cells are the documented ones"""
    assert first.tolist() == cell_edges(rate)
    a = np.abs(xr)
    for c in range(CELLS):
        lo, hi = first[c], first[c + 1]
        if hi == lo:
            assert (peak[:, c] == min(lo, 576)).all(), c
            continue
        assert ((peak[:, c] >= lo) & (peak[:, c] < hi)).all(), c
        assert (a[np.arange(len(xr)), peak[:, c]] == a[:, lo:hi].max(axis=1)).all(), c
