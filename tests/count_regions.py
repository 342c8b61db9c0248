"""Granules for the REGIONS of k_loop's bit count (csrc/loop_pass.h, loop_count_bits): subdivide at every big_values, the three
region walks by their number of steps, the count1 region.  Region geometry crossed with table class; every value sits mid-cell (quant_edges.mid_cell), so
the quantiser is not under test.  Generated here, deterministically; nothing is read from files.  The three implementations
that take them are quant_edges.py's: run_hook (the device or the emulated build) and run_oracle.

A long block's regions are lines [0, a1), [a1, a2), [a2, 2 big_values) with a1 <= sfb_l[7] = 30 and a2 <= sfb_l[15] (subdivide's
table), a start / stop block's [0, 36) and [36, 2 big_values).  A walk prices 64 pairs a step: regions 0 and 1 of a long block never
hold a whole step, region 2 up to three and a rest; region 1 of a start / stop block up to four and a rest.  The sets, per rate:
  R1  long blocks, every big_values 1 .. 288 (count1 = 0): 2 big_values on, below and above every band edge, every class of
      subdivide, every step count the regions can take; a walk variant per region at random
  R2  long blocks, every combination of walk variants over the three regions -- plain, third candidate (maximum 4..7), linbits
      (maximum >= 15), empty (all zeros; region 2 ends with a value above 1 and cannot be) -- at big_values with and without a
      partial last step and at 288
  R3  the count1 region: 0, 1, 63, 64, 65, 127, 128, 129, 143 and 144 quadruples behind big_values of 0 and more
  R4  start and stop blocks: big_values around every step count of region 1, 0 .. 4 whole steps with and without a rest, and the
      walk variants of both regions
coverage() states what the sets must reach and checks it on the oracle's outputs."""
import numpy as np

import quant_edges as qe

VARIANTS = ("plain", "third", "linbits", "empty")
COUNT1 = (0, 1, 63, 64, 65, 127, 128, 129, 143, 144)
F = {n: i for i, n in enumerate(qe.ORACLE_FIELDS)}

SUBDV = ((0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 1), (1, 1), (1, 1), (1, 2), (2, 2), (2, 3), (2, 3), (3, 4), (3, 4), (3, 4), (4, 5),
         (4, 5), (4, 6), (5, 6), (5, 6), (5, 7), (6, 7), (6, 7))  # region0_count, region1_count by the number of band edges below 2 big_values


def subdivide_long(rate, bv):
    """(region0_count, region1_count, address1, address2) of a block without window switching, big_values > 0: the counts of the
    table, each lowered while its region would end past 2 big_values"""
    e, bvr = qe.SFB_L[rate], 2 * bv
    c0, c1 = SUBDV[sum(x < bvr for x in e)]
    while c0 and e[c0 + 1] > bvr:
        c0 -= 1
    while c1 and e[c0 + c1 + 2] > bvr:
        c1 -= 1
    return c0, c1, e[c0 + 1], e[c0 + c1 + 2]


def steps_of(lo, hi):
    """(whole steps of 64 pairs, a partial last step?) of a walk over lines [lo, hi)"""
    span = max(hi - lo, 0)
    return span >> 7, (span & 127) != 0


def variant_of(m):
    return "empty" if m == 0 else "third" if 4 <= m <= 7 else "linbits" if m >= 15 else "plain"


class Sets:
    """the granules of one rate: .xr (N, 576) float64, .gran (N, 4) int32 [q, block_type, 0, 0], .set (N,) names"""

    PLAIN = (1, 2, 3, 8, 11, 14)
    THIRD = (4, 5, 6, 7)
    LINBITS = (15, 16, 17, 19, 31, 47, 300, 2047)

    def __init__(self, rate, seed=0xC0DE):
        self.rate = rate
        self.rng = np.random.default_rng(seed + rate)
        self.xr, self.gran, self.set = [], [], []
        self.r1()
        self.r2()
        self.r3()
        self.r4()
        self.xr = np.ascontiguousarray(np.stack(self.xr))
        self.gran = np.ascontiguousarray(np.array(self.gran, np.int32))
        self.set = np.array(self.set)

    def add(self, name, vals, bt=0):
        q = int(self.rng.integers(-60, 60))
        sign = np.where(self.rng.random(576) < 0.5, -1.0, 1.0)
        self.xr.append(qe.mid_cell(vals, qe.step_of(q)) * sign)
        self.gran.append([q, bt, 0, 0])
        self.set.append(name)

    def fill(self, vals, lo, hi, variant):
        """values of lines [lo, hi) for a walk variant: its maximum once, the rest at random below it (zeros among them)"""
        rng = self.rng
        if hi <= lo or variant == "empty":
            return
        m = int(rng.choice({"plain": self.PLAIN, "third": self.THIRD, "linbits": self.LINBITS}[variant]))
        vals[lo:hi] = np.minimum(rng.geometric(0.35, hi - lo) - 1, m) if rng.random() < 0.5 else rng.integers(0, m + 1, hi - lo)
        vals[lo + int(rng.integers(hi - lo))] = m

    def long_block(self, name, bv, variants, count1=0):
        """a long block with this big_values (> 0) and count1: the regions as subdivide will cut them, a variant each; the last pair
        of the big values holds a value above 1, `count1` quadruples of zeros and ones follow, the last pair of them not empty"""
        _, _, a1, a2 = subdivide_long(self.rate, bv)
        e2 = 2 * bv
        vals = np.zeros(576, np.int64)
        a1c, a2c = min(a1, e2), min(a2, e2)  # (an address past 2 big_values: a band edge above a small big_values)
        self.fill(vals, 0, a1c, variants[0])
        self.fill(vals, a1c, a2c, variants[1])
        self.fill(vals, a2c, e2, variants[2])
        if e2 > a2c:
            self.seal(vals, a2c, e2, variants[2])
        elif e2 > a1c:
            self.seal(vals, a1c, e2, variants[1])
        else:
            self.seal(vals, 0, e2, variants[0])
        self.tail(vals, e2, count1)
        self.add(name, vals)

    def seal(self, vals, lo, e2, variant):
        """the last pair of the big values holds a value above 1: one that leaves the variant of its region [lo, e2) as it is (an
        empty one becomes plain: a region that ends the big values is never empty)"""
        if vals[e2 - 2:e2].max() < 2:
            m = int(vals[lo:e2].max())
            vals[e2 - 1 - int(self.rng.integers(2))] = m if m >= 2 else {"plain": 2, "third": 4, "linbits": 15, "empty": 2}[variant]

    def tail(self, vals, e2, count1):
        if count1:
            end = e2 + 4 * count1
            vals[e2:end] = self.rng.random(end - e2) < 0.5
            vals[end - 2 + int(self.rng.integers(2))] = 1

    def r1(self):
        for bv in range(1, 289):
            v = [str(self.rng.choice(VARIANTS[:3])) for _ in range(3)]
            self.long_block("R1", bv, v)

    def r2(self):
        e = qe.SFB_L[self.rate]
        for bv in (288, e[15] // 2 + 64, e[15] // 2 + 64 + 17, e[15] // 2 + 3):
            for v0 in VARIANTS:
                for v1 in VARIANTS:
                    for v2 in VARIANTS[:3]:
                        self.long_block("R2", bv, (v0, v1, v2))

    def r3(self):
        rng = self.rng
        for c1 in COUNT1:
            for bv in (0, 1, 9, 31, 32, 33, 100, 158, 160):
                if bv + 2 * c1 > 288:
                    continue
                if bv == 0:
                    vals = np.zeros(576, np.int64)
                    self.tail(vals, 0, c1)
                    self.add("R3", vals)
                else:
                    self.long_block("R3", bv, [str(rng.choice(VARIANTS[:3])) for _ in range(3)], count1=c1)
            if c1:  # ... and reaching the last line
                bv = 288 - 2 * c1
                if bv:
                    self.long_block("R3", bv, ("plain", "third", "linbits"), count1=c1)

    def r4(self):
        rng = self.rng
        bvs = sorted(set([1, 2, 17, 18, 19, 20] + [18 + 64 * k + d for k in range(1, 5) for d in (-1, 0, 1, 9)] + [287, 288] + list(range(25, 288, 23))))
        for bt in (1, 3):
            for bv in bvs:
                for v0, v1 in ((str(rng.choice(VARIANTS)), str(rng.choice(VARIANTS[:3]))), (str(rng.choice(VARIANTS[:3])), str(rng.choice(VARIANTS[:3])))):
                    e2 = 2 * bv
                    vals = np.zeros(576, np.int64)
                    self.fill(vals, 0, min(36, e2), v0)
                    self.fill(vals, 36, e2, v1)
                    self.seal(vals, 36 if e2 > 36 else 0, e2, v1 if e2 > 36 else v0)
                    if rng.random() < 0.3:
                        self.tail(vals, e2, int(rng.integers(0, (576 - e2) // 4 + 1)))
                    self.add("R4", vals, bt=bt)
            for v0 in VARIANTS:  # the variants of both regions, region 1 with whole steps and a rest
                for v1 in VARIANTS[:3]:
                    vals = np.zeros(576, np.int64)
                    self.fill(vals, 0, 36, v0)
                    self.fill(vals, 36, 400, v1)
                    vals[399] = max(2, int(vals[36:400].max()))
                    self.add("R4", vals, bt=bt)


def coverage(S, ix, f):
    """what the sets are for, read from the ORACLE's values and fields: raises AssertionError naming what is missing"""
    rate, e = S.rate, qe.SFB_L[S.rate]
    bt = S.gran[:, 1]
    bv, c1 = f[:, F["big_values"]], f[:, F["count1"]]
    a1, a2 = f[:, F["address1"]], f[:, F["address2"]]
    longb, ss = (bt == 0) & (bv > 0), ((bt == 1) | (bt == 3)) & (bv > 0)
    assert (bt == 1).any() and (bt == 3).any()
    # subdivide as restated here is the oracle's, on every long granule
    want = np.array([subdivide_long(rate, int(b)) if b else (0, 0, 0, 0) for b in bv])
    got = f[:, [F["region0_count"], F["region1_count"], F["address1"], F["address2"]]]
    assert np.array_equal(got[longb], want[longb])
    assert (a1[ss] == 36).all() and (a2[ss] == 2 * bv[ss]).all()
    # 2 big_values on, just below and just above every band edge; every big_values; every class of subdivide
    have = set(bv[longb].tolist())
    assert have >= set(range(1, 289))
    for edge in e[1:]:
        assert {edge // 2 - 1, edge // 2, min(edge // 2 + 1, 288)} - {0} <= have, edge
    classes = {sum(x < 2 * b for x in e) + sum(x <= 2 * b for x in e) for b in have}
    assert classes == set(range(2, 46)), sorted(classes)
    # step counts: every one a region can take, 0 .. 4 whole steps with and without a partial last one
    regs = lambda g: ((0, a1[g]), (a1[g], a2[g]), (a2[g], 2 * bv[g]))  # (as loop_count_bits walks them; an address can lie past 2 big_values)
    seen = {(k, r): set() for k in ("long", "ss") for r in range(3)}
    for g in np.flatnonzero(longb | ss):
        for r, (lo, hi) in enumerate(regs(g)):
            seen["long" if longb[g] else "ss", r].add(steps_of(int(lo), int(hi)))
    possible = [set(), set(), set()]
    for b in range(1, 289):
        _, _, x1, x2 = subdivide_long(rate, b)
        for r, (lo, hi) in enumerate(((0, x1), (x1, x2), (x2, 2 * b))):
            possible[r].add(steps_of(lo, hi))
    for r in range(3):
        assert seen["long", r] == possible[r], (r, seen["long", r], possible[r])
    assert possible[0] == {(0, True)} and {n for n, _ in possible[1]} == {0}
    assert possible[2] >= {(n, p) for n in range(3) for p in (False, True)} | {(3, True)}  # (long: a2 <= sfb_l[15], 442 lines and more behind it)
    assert seen["ss", 0] == {(0, True)} and seen["ss", 1] == {(n, p) for n in range(5) for p in (False, True)}, seen["ss", 1]
    # walk variants: every one at every region position, and an empty region between (in front of) non-empty ones
    mx = qe.region_maxima(ix, f)
    for kind, sel, nreg in (("long", longb, 3), ("ss", ss, 2)):
        for r in range(nreg):
            var = {variant_of(int(m)) for m in mx[sel, r]}
            assert var >= {"plain", "third", "linbits"}, (kind, r, var)
        others = mx[sel] > 0
        assert ((mx[sel, 0] == 0) & others[:, 1:nreg].all(axis=1)).any(), kind
    lw = np.flatnonzero(longb)
    assert ((mx[lw, 1] == 0) & (mx[lw, 0] > 0) & (mx[lw, 2] > 0) & (a2[lw] > a1[lw])).any()
    combos = {tuple(variant_of(int(m)) for m in row) for row in mx[lw]}
    assert len(combos) >= 4 * 4 * 3, len(combos)
    # long-region step counts crossed with the table class of region 2
    for n in range(4):
        var = {variant_of(int(mx[g, 2])) for g in lw if steps_of(int(a2[g]), int(2 * bv[g]))[0] == n}
        assert var >= {"plain", "third", "linbits"}, (n, var)
    # the count1 region
    assert set(c1[bt != 2].tolist()) >= set(COUNT1)
    assert ((c1 == 144) & (bv == 0)).any() and ((bv > 0) & (c1 > 128)).any() and ((bv + 2 * c1 == 288) & (c1 > 0)).any()
    for k in (1, 64, 65, 128):
        assert ((c1 == k) & (bv > 0) & longb).any(), k
