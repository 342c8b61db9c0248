"""Granules built to sit on the edges of k_loop's quantise+count pass (csrc/loop_pass.h: loop_quantize, loop_count_bits), and the
three implementations that take them: the product's self-test hook mp3mi_debug_quantize_count (the device, or the emulated CPU
build), the oracle's mp3o_quantize_count and the unmodified reference's quantize() / count_bits() (oracle/_ref/ref_harness_qc).
Everything is generated here, deterministically; nothing is read from files.

A granule is 576 xr, a step q, a block type (0 long, 2 short; 1 / 3 start / stop in S7) and a rescale plan (n_amp amplifications
of every band by sqrt(2), before them pre = 1: one pre-emphasis).  The sets (tests/test_quant_edges.py, test_gpu_quant_edges.py):
  S1  every table boundary p = 1..2047 at steps covering both ends of [Q_LO, Q_HI] and every q % 4: the largest double whose
      product with 1 / step lies below tab[p], the smallest on or above it, and the doubles where the float that feeds
      |xr|^(3/4) crosses the boundary, one and two float ulps either side
  S2  the same after 1..16 amplifications, with and without a pre-emphasis (pretab 1, 2, 3 by band): pre-images whose
      RESCALED double lands on either side of a boundary -- the rescaling budget of the quantiser's guard band
  S3  the ends of the range: tab[2047] and far above (the clamp, `over`), granules whose largest line sits at the 0 / 1
      boundary and at the all-zero shortcut's threshold, zeros and subnormals
  S4  run lengths: one non-zero line at each of the 576 positions (values 1, 2, 15, 16, 2047), the big_values / count1
      boundary at every pair, all lines non-zero, all zero
  S5  table choice: each region's maximum at the edges of the Huffman groups and linbits tables, the rest random below it
  S6  short blocks: the maxima of interleaved lines [0, 36) and [36, 576) at the same edges, on both sides of line 36
  S7  Laplacian spectra at random steps, every block type
In S4..S7 a value v is placed in the middle of its cell (between tab[v] and tab[v + 1], times the step): there the bit count is
under test and the quantiser is not."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_HARNESS_QC = os.path.join(ROOT, "oracle", "_ref", "ref_harness_qc")
RATES = (44100, 48000, 32000)
STEP_MIN, STEP_MAX = -400, 400
# The steps the sets use.  loop_power34 forms |xr| * sqrt(|xr|) in float: above 4.9e25 it overflows (every estimate then says
# 2047) and below 5.2e-26 it is no longer a normal float (the device flushes it to 0: every estimate says 0).  Either is only
# wrong where the exact answer is not 2047 / not 0, i.e. at q > 282 (a value below 2047 needs |xr| < 2.6e4 * 2^(q / 4)) and at
# q < -332 (a value above 0 needs |xr| >= 0.5 * 2^(q / 4)).  The encoder never gets there: the reference dies at
# global_gain = q + 210 >= 256 (src/loop.c:358), and q0 that low needs a spectrum below 1e-25.
Q_LO, Q_HI = -328, 280

# include/mp3mi.h: MP3MI_QC_*; the oracle's fields (oracle/mp3_oracle.h, mp3o_quantize_count) are words 4..15 of these
QC = ["n_nz", "n_big", "m1", "m2", "bits", "big_values", "count1", "count1table_select", "table_select0", "table_select1",
      "table_select2", "region0_count", "region1_count", "address1", "address2", "address3", "all_zero", "rare_tier", "n_differ",
      "over"]
QCI = {n: i for i, n in enumerate(QC)}
ORACLE_FIELDS = QC[4:16]

# ISO 11172-3 Table B.8 (MPEG-1 scalefactor bands) and the pre-emphasis table
SFB_L = {44100: [0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 90, 110, 134, 162, 196, 238, 288, 342, 418, 576],
         48000: [0, 4, 8, 12, 16, 20, 24, 30, 36, 42, 50, 60, 72, 88, 106, 128, 156, 190, 230, 276, 330, 384, 576],
         32000: [0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 54, 66, 82, 102, 126, 156, 194, 240, 296, 364, 448, 550, 576]}
SFB_S = {44100: [0, 4, 8, 12, 16, 22, 30, 40, 52, 66, 84, 106, 136, 192],
         48000: [0, 4, 8, 12, 16, 22, 28, 38, 50, 64, 80, 100, 126, 192],
         32000: [0, 4, 8, 12, 16, 22, 30, 42, 58, 78, 104, 138, 180, 192]}
PRETAB = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 3, 2]
SQRT2 = math.sqrt(2.0)

# the quantiser's table, as the reference builds it (src/pow_nint.c): tab[p] = (p - 0.4054)^(4/3); tab[0] is never read
TAB = np.array([0.0] + [math.pow(p - 0.4054, 4.0 / 3.0) for p in range(1, 2048)] + [math.inf])


def step_of(q):
    return 1.0 if q == 0 else math.pow(2.0, q * 0.25)


def ix_definition(xr, q):
    """ix = min(2047, max{p : tab[p] <= |xr| * (1 / step)}) -- the plain definition, for xr AFTER the rescale plan"""
    ostep = np.array([1.0 / step_of(int(v)) for v in np.ravel(q)])
    x = np.abs(xr) * ostep[:, None]
    return np.minimum(np.searchsorted(TAB[1:2048], x, side="right"), 2047).astype(np.int32)


def line_factors(rate, block_type, n_amp, pre):
    """per line: the factors the rescale plan multiplies it by, in order (long blocks: pre-emphasis of sfb < 21 by
    sqrt(2)^pretab, then amplification of sfb < 21; short blocks: amplification of the lines of sfb < 12 of every window)"""
    out = []
    for line in range(576):
        f = []
        if block_type == 2:
            band = np.searchsorted(SFB_S[rate], line // 3, side="right") - 1
            amp = band < 12
        else:
            band = np.searchsorted(SFB_L[rate], line, side="right") - 1
            amp = band < 21
            if pre and amp:
                f.append(math.pow(SQRT2, PRETAB[band]))
        if amp:
            f += [SQRT2] * n_amp
        out.append(f)
    return out


def rescaled(x0, factors):
    v = np.array(x0, dtype=np.float64)
    for f in factors:
        v = v * f
    return v


def boundary_preimages(t, ostep, factors):
    """for each target boundary t[i]: the largest x0 whose rescaled product with ostep lies below t[i] and the smallest on or
    above it (x0 > 0; factors: the line's rescale factors, in order), and which targets were bracketed"""
    tot = 1.0
    for f in factors:
        tot *= f
    x0 = t / ostep / tot
    c = [x0]
    up, dn = x0, x0
    for _ in range(48):  # x0 and 48 ulps either side (x0 itself carries up to ~20 roundings of the factors and of the quotient)
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, 0.0)
        c = [dn] + c + [up]
    c = np.stack(c, axis=1)
    above = rescaled(c, factors) * ostep >= t[:, None]
    first = np.argmax(above, axis=1)  # monotone in x0: the first candidate on or above
    ok = above.any(axis=1) & ~above[:, 0]
    r = np.arange(len(x0))
    return c[r, np.maximum(first - 1, 0)], c[r, first], ok


def float_neighbours(x):
    """the doubles of the float32 nearest x and of its float neighbours one and two ulps either side"""
    f = x.astype(np.float32)
    out = [f]
    up, dn = f.copy(), f.copy()
    for _ in range(2):
        up = np.nextafter(up, np.float32(np.inf))
        dn = np.nextafter(dn, np.float32(0))
        out += [up.copy(), dn.copy()]
    return [o.astype(np.float64) for o in out]


def pack(lines, rng):
    """lines (1-D, any length) into granules of 576, positions shuffled, signs mixed; the last one is padded with zeros"""
    n = (len(lines) + 575) // 576
    a = np.zeros(n * 576)
    a[:len(lines)] = lines
    a = a.reshape(n, 576)
    for g in a:
        rng.shuffle(g)
    return a * np.where(rng.random(a.shape) < 0.5, -1.0, 1.0)


def mid_cell(v, step):
    """xr that quantises to v (0..2047) in the middle of its cell"""
    v = np.asarray(v)
    lo, hi = TAB[np.minimum(v, 2047)], TAB[np.minimum(v + 1, 2048)]
    mid = np.where(v >= 2047, TAB[2047] * 1.5, 0.5 * (lo + hi))
    return np.where(v == 0, 0.25 * TAB[1], mid) * step


class Sets:
    """the granules of one rate: .xr (N, 576) float64, .gran (N, 4) int32 [q, block_type, n_amp, pre], .set (N,) names"""

    def __init__(self, rate, seed=0x51ED):
        self.rate = rate
        self.rng = np.random.default_rng(seed + rate)
        self.xr, self.gran, self.set = [], [], []
        for name in ("S1", "S2", "S3", "S4", "S5", "S6", "S7"):
            getattr(self, name.lower())()
        self.xr = np.ascontiguousarray(np.concatenate(self.xr))
        self.gran = np.ascontiguousarray(np.concatenate(self.gran).astype(np.int32))
        self.set = np.concatenate(self.set)

    def add(self, name, xr, q, bt=0, n_amp=0, pre=0):
        xr = np.atleast_2d(xr)
        n = len(xr)
        g = np.zeros((n, 4), np.int32)
        g[:, 0], g[:, 1], g[:, 2], g[:, 3] = q, bt, n_amp, pre
        self.xr.append(xr)
        self.gran.append(g)
        self.set.append(np.array([name] * n))

    def s1(self):
        qs = list(range(Q_LO, Q_HI + 1, 7))  # every q % 4 (7 is odd)
        qs = qs[self.rate % 7::3] + [Q_LO, Q_LO + 1, Q_LO + 2, Q_LO + 3, Q_HI, Q_HI - 1, Q_HI - 2, Q_HI - 3, -1, 0, 1]  # a third of them at each rate
        p = np.arange(1, 2048)
        for i, q in enumerate(sorted(set(qs))):
            ostep = 1.0 / step_of(q)
            lo, hi, ok = boundary_preimages(TAB[p], ostep, [])
            assert ok.all()
            lines = [lo, hi] + float_neighbours(hi)
            self.add("S1", pack(np.concatenate(lines), self.rng), q, bt=2 if i % 5 == 4 else 0)

    def s2(self):
        rng = self.rng
        for n_amp in list(range(1, 17)) * 4:
            for pre in (0, 1):
                for bt in ((0, 2) if not pre else (0,)):
                    q = int(rng.integers(Q_LO + 60, Q_HI - 60))
                    ostep = 1.0 / step_of(q)
                    fac = line_factors(self.rate, bt, n_amp, pre)
                    # a boundary per line: small p often (the absolute part of the band), the rest spread over the table
                    p = np.where(rng.random(576) < 0.5, rng.integers(1, 16, 576), rng.integers(1, 2048, 576))
                    side = rng.random(576) < 0.5
                    xr = np.zeros(576)
                    for key in set(tuple(f) for f in fac):  # lines with the same factors together
                        lines = np.array([i for i in range(576) if tuple(fac[i]) == key])
                        lo, hi, ok = boundary_preimages(TAB[p[lines]], ostep, list(key))
                        assert ok.all()
                        xr[lines] = np.where(side[lines], hi, lo)
                    self.add("S2", xr * np.where(rng.random(576) < 0.5, -1.0, 1.0), q, bt=bt, n_amp=n_amp, pre=pre)

    def s3(self):
        rng = self.rng
        for q in (Q_LO, -123, 0, 77, Q_HI):
            step = step_of(q)
            ostep = 1.0 / step
            lo, hi, _ = boundary_preimages(TAB[np.array([2047])], ostep, [])
            top = np.array([lo[0], hi[0], np.nextafter(hi[0], np.inf), TAB[2047] * step * 1.0001, TAB[2047] * step * 2,
                            TAB[2047] * step * 100, TAB[2047] * step * 1e4])
            xr = mid_cell(rng.integers(0, 2047, 576), step)
            xr[rng.choice(576, len(top), replace=False)] = top
            self.add("S3", xr * np.where(rng.random(576) < 0.5, -1.0, 1.0), q)
            # the 0 / 1 boundary as the granule's largest line: everything quantises to 0 or one line to 1
            lo1, hi1, _ = boundary_preimages(TAB[np.array([1])], ostep, [])
            for top1 in (lo1[0], hi1[0], np.nextafter(lo1[0], 0), np.nextafter(hi1[0], np.inf)):
                xr = rng.random(576) * lo1[0] * 0.999
                xr[rng.integers(576)] = top1
                self.add("S3", xr, q, bt=int(rng.integers(2)) * 2)
            # the all-zero shortcut's threshold (loop_all_zero: estimate y34max * 2^(-3q/16) + 0.4054 < 0.999)
            thr = (0.999 - 0.4054) ** (4.0 / 3.0) * step
            for r in (1 - 1e-5, 1 - 1e-6, 1 - 1e-7, 1.0, 1 + 1e-7, 1 + 1e-6, 1 + 1e-5):
                xr = rng.random(576) * thr * 0.5
                xr[rng.integers(576)] = thr * r
                self.add("S3", xr, q)
        for q in (Q_LO, 0, Q_HI):
            self.add("S3", np.zeros(576), q)
            sub = np.array([5e-324, 1e-320, 2.2250738585072e-308, 1e-310]) * np.where(rng.random(4) < 0.5, -1, 1)
            self.add("S3", np.resize(sub, 576), q)
            self.add("S3", np.resize(sub, 576), q, bt=2)

    def s4(self):
        rng = self.rng
        for v in (1, 2, 15, 16, 2047):
            for pos0 in range(0, 576, 96):
                # one granule per position: the single line is at pos; q random per granule
                for pos in range(pos0, pos0 + 96):
                    q = int(rng.integers(Q_LO, Q_HI + 1))
                    xr = np.zeros(576)
                    xr[pos] = mid_cell(v, step_of(q)) * (1 if pos % 3 else -1)
                    self.add("S4", xr, q)
        for k in range(288):  # the last pair with a value above 1 is pair k, ones (and zeros) behind it
            q = int(rng.integers(Q_LO, Q_HI + 1))
            vals = rng.integers(0, 4, 576)
            vals[2 * k + 2:] = (rng.random(576 - 2 * k - 2) < 0.5)
            vals[2 * k + int(rng.integers(2))] = int(rng.integers(2, 30))
            self.add("S4", mid_cell(vals, step_of(q)), q)
        for last in (287, 286, 143, 0):
            q = int(rng.integers(-100, 100))
            vals = rng.integers(0, 3, 576)
            vals[2 * last + 2:] = 0
            vals[2 * last + 1] = 1
            self.add("S4", mid_cell(vals, step_of(q)), q)
        for hi in (1, 2, 16, 2047):
            q = int(rng.integers(-100, 100))
            self.add("S4", mid_cell(rng.integers(1, hi + 1, 576), step_of(q)), q)
            self.add("S4", mid_cell(rng.integers(1, hi + 1, 576), step_of(q)), q, bt=2)
        self.add("S4", np.zeros(576), 0)

    MAXIMA = list(range(20)) + [22, 23, 30, 31, 46, 47, 78, 79, 142, 143, 270, 271, 526, 527, 1038, 1039, 2047]

    def s5(self):
        rng = self.rng
        edges = [0, 30, SFB_L[self.rate][15], 576]  # big_values = 288: subdivide's regions [0, 30), [30, sfb_l[15]), [.., 576)
        for r in range(3):
            for m in self.MAXIMA:
                if r == 2 and m < 2:
                    continue  # (region 2 ends with the last value above 1)
                for rep in range(2):
                    q = int(rng.integers(Q_LO, Q_HI + 1))
                    vals = np.zeros(576, np.int64)
                    for rr in range(3):
                        a, b = edges[rr], edges[rr + 1]
                        mm = m if rr == r else int(rng.choice(self.MAXIMA[2:]))
                        vals[a:b] = rng.integers(0, mm + 1, b - a) if rep == 0 else np.minimum(rng.geometric(0.3, b - a) - 1, mm)
                        vals[a + int(rng.integers(b - a))] = mm
                    if vals[574:576].max() < 2:
                        vals[575] = max(2, vals[575]) if r != 2 else m
                    self.add("S5", mid_cell(vals, step_of(q)) * np.where(rng.random(576) < 0.5, -1, 1), q)

    def s6(self):
        rng = self.rng
        for m1 in self.MAXIMA:
            for m2 in (m1, int(rng.choice(self.MAXIMA))):
                q = int(rng.integers(Q_LO, Q_HI + 1))
                vals = np.concatenate([rng.integers(0, m1 + 1, 36), rng.integers(0, m2 + 1, 540)])
                vals[[34, 35][int(rng.integers(2))]] = m1   # on both sides of interleaved line 36
                vals[[36, 37][int(rng.integers(2))]] = m2
                self.add("S6", mid_cell(vals, step_of(q)) * np.where(rng.random(576) < 0.5, -1, 1), q, bt=2)

    def s7(self, per_type=None):
        rng = self.rng
        n = per_type or 600
        k = np.arange(576)
        for bt in (0, 1, 2, 3):
            amp = 10.0 ** rng.uniform(-2, 4, n)
            decay = rng.uniform(30, 300, n)
            xr = rng.laplace(size=(n, 576)) * amp[:, None] * np.exp(-k[None, :] / decay[:, None])
            target = 10.0 ** rng.uniform(-0.5, 3.4, n)  # the largest value the step should give
            q = np.clip(np.round(4 * np.log2(np.abs(xr).max(axis=1) / target ** (4.0 / 3.0))), Q_LO, Q_HI).astype(int)
            for i in range(n):
                self.add("S7", xr[i], int(q[i]), bt=bt, n_amp=int(rng.integers(0, 3)) if rng.random() < 0.3 else 0,
                         pre=int(bt != 2 and rng.random() < 0.1))

    def subsample(self, per_set, seed=7):
        """a fixed subsample: per_set granules of every set (all of a smaller set)"""
        rng = np.random.default_rng(seed + self.rate)
        idx = []
        for name in np.unique(self.set):
            w = np.flatnonzero(self.set == name)
            idx.append(np.sort(rng.choice(w, min(per_set, len(w)), replace=False)))
        return np.concatenate(idx)


# ---- the three implementations ----
def run_hook(lib, rate, xr, gran):
    """mp3mi_debug_quantize_count: (rc, ix (N, 576) int16, xr_out, fields (N, len(QC)))"""
    n = len(xr)
    xr = np.ascontiguousarray(xr, np.float64)
    gran = np.ascontiguousarray(gran, np.int32)
    ix = np.zeros((n, 576), np.int16)
    xo = np.zeros((n, 576), np.float64)
    f = np.zeros((n, len(QC)), np.int32)
    lib.mp3mi_debug_quantize_count.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
    rc = lib.mp3mi_debug_quantize_count(rate, n, xr.ctypes.data, gran.ctypes.data, ix.ctypes.data, xo.ctypes.data, f.ctypes.data)
    return rc, ix, xo, f


def run_oracle(orc_lib, rate, xr, gran):
    """mp3o_quantize_count: (ix (N, 576) int32, xr_out, fields (N, 12) as ORACLE_FIELDS)"""
    n = len(xr)
    xr = np.ascontiguousarray(xr, np.float64)
    gran = np.ascontiguousarray(gran, np.int32)
    ix = np.zeros((n, 576), np.int32)
    xo = np.zeros((n, 576), np.float64)
    f = np.zeros((n, len(ORACLE_FIELDS)), np.int32)
    orc_lib.mp3o_quantize_count.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
    rc = orc_lib.mp3o_quantize_count(rate, n, xr.ctypes.data, gran.ctypes.data, ix.ctypes.data, xo.ctypes.data, f.ctypes.data)
    assert rc == 0
    return ix, xo, f


def run_reference(rate, xr_rescaled, gran):
    """oracle/_ref/ref_harness_qc on already rescaled granules: (ix, fields as ORACLE_FIELDS)"""
    n = len(xr_rescaled)
    rec = np.dtype([("hdr", "<i4", (4,)), ("xr", "<f8", (576,))])
    a = np.zeros(n, rec)
    a["hdr"][:, 0], a["hdr"][:, 1], a["hdr"][:, 2] = rate, gran[:, 1], gran[:, 0]
    a["xr"] = xr_rescaled
    out = np.dtype([("ix", "<i4", (576,)), ("f", "<i4", (len(ORACLE_FIELDS),))])
    with tempfile.TemporaryDirectory() as d:
        fi, fo = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fi, "wb") as fh:
            fh.write(np.int32(n).tobytes())
            fh.write(a.tobytes())
        subprocess.run([REF_HARNESS_QC, fi, fo], check=True, timeout=600)
        r = np.fromfile(fo, out)
    assert len(r) == n
    return r["ix"], r["f"]


def expected_qinfo(ix, gran):
    """what loop_quantize reports besides the values (loop_qinfo), from the oracle's ix: long blocks 2 * (last non-zero pair + 1)
    and 2 * (last pair holding a value above 1, + 1); short blocks the maxima of lines [0, 36) and [36, 576)"""
    n = len(ix)
    out = np.zeros((n, 4), np.int32)
    pairs = np.abs(ix).reshape(n, 288, 2).max(axis=2)
    shortb = gran[:, 1] == 2
    nz, big = pairs > 0, pairs > 1
    last_nz = np.where(nz.any(axis=1), 287 - np.argmax(nz[:, ::-1], axis=1), -1)
    last_big = np.where(big.any(axis=1), 287 - np.argmax(big[:, ::-1], axis=1), -1)
    out[:, 0] = np.where(shortb, 0, 2 * (last_nz + 1))
    out[:, 1] = np.where(shortb, 0, 2 * (last_big + 1))
    out[:, 2] = np.where(shortb, np.abs(ix[:, :36]).max(axis=1), 0)
    out[:, 3] = np.where(shortb, np.abs(ix[:, 36:]).max(axis=1), 0)
    return out


def desc_class(m):
    """k_loop's Huffman descriptor class of a region maximum (loop_desc_index): the group and the linbits tables"""
    m = np.asarray(m)
    return np.where(m < 16, m, 15 + np.floor(np.log2(np.maximum(m - 15, 1))).astype(int) + 1)


def region_maxima(ix, f_oracle):
    """per long granule the maxima of its three regions [0, a1), [a1, a2), [a2, 2 big_values) as the oracle divided them"""
    F = {n: i for i, n in enumerate(ORACLE_FIELDS)}
    out = np.zeros((len(ix), 3), np.int64)
    for g in range(len(ix)):
        a1, a2, e2 = f_oracle[g, F["address1"]], f_oracle[g, F["address2"]], 2 * f_oracle[g, F["big_values"]]
        v = np.abs(ix[g])
        out[g] = [v[:a1].max(initial=0), v[a1:a2].max(initial=0) if a2 > a1 else 0, v[a2:e2].max(initial=0) if e2 > a2 else 0]
    return out


def first_mismatch(S, idx, ix_h, xo_h, f_h, ix_o, xo_o, f_o):
    """None, or a message naming the set, the granule, the first differing line or field and the hook's diagnostics"""
    gran = S.gran[idx]
    want_qi = expected_qinfo(ix_o, gran)
    for k in range(len(idx)):
        where = None
        if not np.array_equal(xo_h[k].view(np.int64), xo_o[k].view(np.int64)):
            j = int(np.flatnonzero(xo_h[k].view(np.int64) != xo_o[k].view(np.int64))[0])
            where = "rescaled xr[%d]: %r vs %r" % (j, xo_h[k, j], xo_o[k, j])
        elif not np.array_equal(ix_h[k].astype(np.int32), ix_o[k]):
            j = int(np.flatnonzero(ix_h[k].astype(np.int32) != ix_o[k])[0])
            where = "ix[%d]: %d vs %d (xr %r)" % (j, ix_h[k, j], ix_o[k, j], xo_o[k, j])
        else:
            for n in ORACLE_FIELDS:
                if f_h[k, QCI[n]] != f_o[k, ORACLE_FIELDS.index(n)]:
                    where = "%s: %d vs %d" % (n, f_h[k, QCI[n]], f_o[k, ORACLE_FIELDS.index(n)])
                    break
            for i, n in enumerate(QC[:4]):
                if where is None and f_h[k, i] != want_qi[k, i]:
                    where = "%s: %d vs %d" % (n, f_h[k, i], want_qi[k, i])
        if where:
            g = int(idx[k])
            return ("rate %d, set %s, granule %d (q %d, block type %d, n_amp %d, pre %d): %s; diagnostics all_zero %d rare_tier %d "
                    "n_differ %d over %d" % (S.rate, S.set[g], g, *gran[k], where, *[f_h[k, QCI[n]] for n in QC[16:]]))
    return None
