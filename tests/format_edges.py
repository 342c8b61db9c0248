"""Crafted frame chains for the Layer III formatter (k_format, csrc/k_format.hip; the drop-in III_format_bitstream, csrc/dropin.cpp),
a plain model of what makes a chain legal, and a plain decoder of the finished byte stream.  Deterministic; the one file read is
tests/golden/huff_tables.npz, the reference's Huffman tables as it holds them at run time (fmt_probe_ref --dump-tables).

A chain is a format (rate, channels and header mode, bitrate, crc / copyright / original / emphasis) and N frames; a frame holds
per (granule, channel) signed ix[576] and every mp3mi_gr_side field, scfsi and resvDrain.  main_data_begin comes from the model:
    frame_bytes = 144000 * kbps / rate (floored, never padded); si_bytes = 4 + 2 crc + (32 stereo | 17 mono);
    slot = frame_bytes - si_bytes;  mdb[0] = 0;  mdb[n + 1] = mdb[n] + slot - bits[n] / 8,
    bits[n] = the frame's part2_3_length values + resvDrain.
Chain.check() asserts the legality rules on every chain the generator emits (they are the domain of the formatter: INTEGRATION.md).

The sets (every one at the three rates, whose band tables differ):
  F1 every cell of the 29 tables, and table 0, in each long-block region and both short ones  F5 lengths, drains and header formats
  F2 count1 quadruples and region boundaries                                           F6 reservoir chains and the flush
  F3 scalefac_compress x scfsi                                                         F7 random legal chains
  F4 bit positions: granule starts, code words across word edges, stuffing runs

Three parts that share no code: the generator's bit counter (pair_bits, count1_bits, part2_bits), the Decoder, and the product.
"""
import ctypes
import os
import subprocess

import numpy as np

from mp3common import ROOT, SIDE_DT

RATES = (44100, 48000, 32000)
BITRATES = (32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320)
# ISO 11172-3 table B.8: scalefactor band edges, long and short blocks
SFB_L = {44100: (0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 90, 110, 134, 162, 196, 238, 288, 342, 418, 576),
         48000: (0, 4, 8, 12, 16, 20, 24, 30, 36, 42, 50, 60, 72, 88, 106, 128, 156, 190, 230, 276, 330, 384, 576),
         32000: (0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 54, 66, 82, 102, 126, 156, 194, 240, 296, 364, 448, 550, 576)}
SFB_S = {44100: (0, 4, 8, 12, 16, 22, 30, 40, 52, 66, 84, 106, 136, 192),
         48000: (0, 4, 8, 12, 16, 22, 28, 38, 50, 64, 80, 100, 126, 192),
         32000: (0, 4, 8, 12, 16, 22, 30, 42, 58, 78, 104, 138, 180, 192)}
SLEN1 = (0, 0, 0, 0, 3, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4)
SLEN2 = (0, 1, 2, 3, 0, 1, 2, 3, 1, 2, 3, 1, 2, 3, 2, 3)
TABLES = tuple(t for t in range(1, 32) if t not in (4, 14))  # the 29 tables that have cells (4 and 14 do not exist)
ALL_TABLES = (0,) + TABLES  # ... and table 0, which codes an all-zero region in no bits: the 30 a region may select
IMAGE_BITS = 640 * 32
FLUSH_SLOT = 3  # MP3MI_STREAM_ABORT_FLUSH_SLOT / MP3O_ABORT_FLUSH_SLOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "huff_tables.npz")
REF = os.path.join(ROOT, "oracle", "_ref")
PROBE_REF, PROBE_DEV, PROBE_EMU = (os.path.join(REF, n) for n in ("fmt_probe_ref", "fmt_probe", "fmt_probe_emu"))


class Huff:
    """the fixture: per table xlen, ylen, linbits, linmax and code / length per cell (x * ylen + y); 32 and 33 are the count1 tables"""

    def __init__(self, path=FIXTURE):
        z = np.load(path)
        self.xlen, self.ylen, self.linbits, self.linmax, self.off = (z[k].tolist() for k in ("xlen", "ylen", "linbits", "linmax", "off"))
        self.code, self.length = z["code"].tolist(), z["length"].tolist()

    def cell(self, t, x, y):
        i = self.off[t] + x * self.ylen[t] + y
        return self.code[i], self.length[i]


HT = Huff()


# ---------------------------------------------------------------------------------------------------------------------
# the generator's bit counter
# ---------------------------------------------------------------------------------------------------------------------
def table_takes(t, m):
    """table t may code a region whose largest magnitude is m"""
    if t == 0:
        return m == 0
    if t not in TABLES:
        return False
    return m < HT.xlen[t] if t < 16 else m - 15 <= HT.linmax[t]


def legal_tables(m):
    return [t for t in (0,) + TABLES if table_takes(t, m)]


def pair_bits(t, x, y):
    """(code bits, extension bits) of one pair in table t: the cell's length, linbits per escape, a sign per non-zero value"""
    x, y = abs(int(x)), abs(int(y))
    if t == 0:
        return 0, 0
    sx, sy = int(x != 0), int(y != 0)
    if t > 15:
        lb = int(HT.linbits[t])
        ext = (lb if x > 14 else 0) + (lb if y > 14 else 0) + sx + sy
        return HT.cell(t, min(x, 15), min(y, 15))[1], ext
    return HT.cell(t, x, y)[1] + sx + sy, 0


def count1_bits(sel, q):
    p = sum((abs(int(v)) & 1) << k for k, v in enumerate(q))
    return HT.cell(32 + sel, 0, p)[1] + sum(abs(int(v)) for v in q)


def short_order(rate):
    """line index pairs of a short-block granule in transmission order: band, then window, then line; and the region of each"""
    e = SFB_S[rate]
    pairs, region = [], []
    for sfb in range(13):
        for w in range(3):
            for line in range(e[sfb], e[sfb + 1], 2):
                pairs.append((line * 3 + w, (line + 1) * 3 + w))
                region.append(0 if e[sfb] < 12 else 1)
    return pairs, region


def part2_bits(g, gr, scfsi):
    s1, s2 = SLEN1[g["scalefac_compress"]], SLEN2[g["scalefac_compress"]]
    if g["window_switching_flag"] and g["block_type"] == 2:
        return 18 * s1 + 18 * s2
    return sum(n * s for b, (n, s) in enumerate(((6, s1), (5, s1), (5, s2), (5, s2))) if gr == 0 or not scfsi[b])


def granule_puts(rate, g, ix, gr, scfsi):
    """every field the formatter puts for one granule, in order: (kind, value bits); the lengths are what matter here"""
    puts = []
    s1, s2 = SLEN1[g["scalefac_compress"]], SLEN2[g["scalefac_compress"]]
    shortb = bool(g["window_switching_flag"]) and g["block_type"] == 2
    if shortb:
        puts += [("sf", s1)] * 18 + [("sf", s2)] * 18
    else:
        for b, (n, s) in enumerate(((6, s1), (5, s1), (5, s2), (5, s2))):
            if gr == 0 or not scfsi[b]:
                puts += [("sf", s)] * n
    bv2 = 2 * g["big_values"]
    ts = g["table_select"]
    if bv2:
        if shortb:
            pairs, region = short_order(rate)
            for (a, b), r in zip(pairs, region):
                c, e = pair_bits(ts[r], ix[a], ix[b])
                puts += [("code", c), ("ext", e)]
        else:
            r1 = SFB_L[rate][g["region0_count"] + 1]
            r2 = SFB_L[rate][g["region0_count"] + g["region1_count"] + 2]
            for i in range(0, bv2, 2):
                c, e = pair_bits(ts[0] if i < r1 else (ts[1] if i < r2 else ts[2]), ix[i], ix[i + 1])
                puts += [("code", c), ("ext", e)]
    for i in range(bv2, bv2 + 4 * g["count1"], 4):
        puts.append(("quad", count1_bits(g["count1table_select"], ix[i:i + 4])))
    return [p for p in puts if p[1]]


def region_maxima(rate, g, ix):
    """largest magnitude per table_select entry"""
    a = np.abs(np.asarray(ix, np.int64))
    bv2 = 2 * g["big_values"]
    if g["window_switching_flag"] and g["block_type"] == 2:
        if not bv2:
            return [0, 0, 0]
        pairs, region = short_order(rate)
        m = [0, 0, 0]
        for (p, q), r in zip(pairs, region):
            m[r] = max(m[r], int(a[p]), int(a[q]))
        return m
    r1 = min(SFB_L[rate][g["region0_count"] + 1], bv2)
    r2 = min(SFB_L[rate][g["region0_count"] + g["region1_count"] + 2], bv2)
    return [int(a[lo:hi].max()) if hi > lo else 0 for lo, hi in ((0, r1), (r1, r2), (r2, bv2))]


# ---------------------------------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------------------------------
def frame_bytes_of(rate, kbps):
    return 144000 * kbps // rate


def granule(ix=None, bt=0, tables=(0, 0, 0), bv=0, c1=0, r0=0, r1=0, sfc=0, sf=None, c1sel=0, preflag=0, gain=210, stuff=0):
    """one (granule, channel) as the generator writes it down; stuff = bits of stuffing behind the code words"""
    g = dict(big_values=bv, count1=c1, global_gain=gain, scalefac_compress=sfc, window_switching_flag=int(bt != 0), block_type=bt,
             table_select=list(tables) + [0] * (3 - len(tables)), region0_count=r0, region1_count=r1, preflag=preflag,
             count1table_select=c1sel, scalefac=np.zeros(39, np.int32) if sf is None else np.asarray(sf, np.int32), stuff=stuff)
    if bt in (1, 3):
        g["region0_count"], g["region1_count"] = 7, 13
    if bt == 2:
        g["region0_count"], g["region1_count"] = 8, 36  # (src/loop.c:1688-1689; the formatter does not read them)
    g["ix"] = np.zeros(576, np.int16) if ix is None else np.asarray(ix, np.int16)
    return g


class Chain:
    def __init__(self, set_name, name, rate, channels=1, kbps=320, mode=None, mode_ext=0, crc=0, copyright=0, original=0, emphasis=0):
        self.set, self.name, self.rate, self.channels, self.kbps = set_name, name, rate, channels, kbps
        self.mode = (3 if channels == 1 else 0) if mode is None else mode
        self.mode_ext, self.crc, self.copyright, self.original, self.emphasis = mode_ext, crc, copyright, original, emphasis
        self.frame_bytes = frame_bytes_of(rate, kbps)
        self.si_bytes = 4 + 2 * crc + (32 if channels == 2 else 17)
        self.slot = self.frame_bytes - self.si_bytes
        self.sides, self.ixs, self.grs = [], [], []
        self.mdb = [0]

    n_frames = property(lambda self: len(self.sides))
    hdr_flags = property(lambda self: self.mode_ext << 4 | self.copyright << 3 | self.original << 2 | self.emphasis)

    def room(self):
        """bytes the next frame may take at most: what the reservoir holds and its own slot"""
        return self.mdb[-1] + self.slot

    def frame(self, grs, scfsi=None, drain=None, take=None, spill="stuff"):
        """append a frame of 2 * channels granules ([gr][ch] order).  take = bytes of main data the frame consumes (None: what
        it needs, but enough to keep the next back pointer <= 511 and off a flush that dies); drain = resvDrain (None: whatever
        the granules' stuffing cannot hold; with spill = "drain" all of them, so that the granules' lengths stay as given).  Bits
        beyond the granules' own stuffing go to the last granules' stuffing."""
        C = self.channels
        assert len(grs) == 2 * C
        scfsi = np.zeros((2, 4), np.int32) if scfsi is None else np.asarray(scfsi, np.int32).reshape(2, 4)
        p23 = []
        for k, g in enumerate(grs):
            gr, ch = divmod(k, C)
            g["part2_length"] = part2_bits(g, gr, scfsi[ch])
            g["code_bits"] = sum(n for _, n in granule_puts(self.rate, g, g["ix"], gr, scfsi[ch])) - g["part2_length"]
            p23.append(g["part2_length"] + g["code_bits"] + g["stuff"])
        mdb, slot = self.mdb[-1], self.slot
        fixed = sum(p23) + (drain or 0)
        if take is None:
            take = (fixed + 7) // 8
            take = max(take, mdb + slot - 511)
            nxt = mdb + slot - take
            if nxt > 0 and nxt % slot == 0 and (nxt // slot * slot * 8) % 32 == 0:
                take += 1  # (the reference's flush would die were this the last frame)
        extra = 8 * take - fixed
        assert extra >= 0 and take <= mdb + slot, (self.name, take, fixed, mdb, slot)
        for k in range(len(grs) - 1, -1, -1):  # stuffing first, the last granule first
            n = min(extra, 4095 - p23[k]) if drain is not None or spill == "stuff" else 0
            p23[k] += n
            grs[k]["stuff"] += n
            extra -= n
        if drain is None:
            drain, extra = extra, 0
        assert extra == 0, (self.name, "the frame cannot hold %d more bits" % extra)
        sd = np.zeros((), SIDE_DT)
        sd["main_data_begin"], sd["resvDrain"], sd["scfsi"] = mdb, drain, scfsi
        ix = np.zeros((2, C, 576), np.int16)
        for k, g in enumerate(grs):
            gr, ch = divmod(k, C)
            q = sd["gr"][gr][ch]
            q["part2_3_length"] = p23[k]
            for f in ("big_values", "count1", "global_gain", "scalefac_compress", "window_switching_flag", "block_type", "table_select",
                      "region0_count", "region1_count", "preflag", "count1table_select", "part2_length", "scalefac"):
                q[f] = g[f]
            ix[gr, ch] = g["ix"]
        self.sides.append(sd)
        self.ixs.append(ix)
        self.grs.append(grs)
        self.mdb.append(mdb + slot - take)
        return self

    # -- the arrays the three implementations take
    def side_array(self):
        return np.array(self.sides, SIDE_DT) if self.sides else np.zeros(0, SIDE_DT)

    def ix_array(self):
        return np.array(self.ixs, np.int16).reshape(self.n_frames, 2, self.channels, 576) if self.ixs else np.zeros((0, 2, self.channels, 576), np.int16)

    def format_key(self):
        return (self.rate, self.channels, self.kbps, self.mode, self.hdr_flags, self.crc)

    # -- the model
    def flush_dies(self):
        """the reference's flush asks for a header its queue no longer has (src/formatBitstream.c:87-105, 225-230, 381-390): the
        main data ends exactly on a slot boundary, k >= 1 frames' slots are still unwritten and k * slot * 8 is a multiple of 32"""
        if not self.n_frames:
            return False
        m_end = self.n_frames * self.slot - self.mdb[-1]
        written = -(-m_end // self.slot)
        queued = self.n_frames - written
        return queued >= 1 and written * self.slot == m_end and (queued * self.slot * 8) % 32 == 0

    def check(self):
        """the legality rules, asserted on every chain the generator emits"""
        assert self.slot > 0 and (self.channels == 1) == (self.mode == 3)
        for n, (sd, ix) in enumerate(zip(self.sides, self.ixs)):
            bits = int(sd["resvDrain"])
            assert sd["resvDrain"] >= 0 and sd["main_data_begin"] == self.mdb[n] and 0 <= self.mdb[n] <= 511, (self.name, n)
            for gr in range(2):
                for ch in range(self.channels):
                    q = sd["gr"][gr][ch]
                    g = {f: (q[f].tolist() if f == "table_select" else int(q[f])) for f in q.dtype.names if f != "scalefac"}
                    v = ix[gr, ch].astype(np.int64)
                    where = (self.name, n, gr, ch)
                    assert 0 <= g["part2_3_length"] <= 4095, where
                    bits += g["part2_3_length"]
                    assert g["part2_length"] == part2_bits(g, gr, sd["scfsi"][ch]), where
                    code = sum(k for _, k in granule_puts(self.rate, g, v, gr, sd["scfsi"][ch])) - g["part2_length"]
                    assert g["part2_3_length"] >= g["part2_length"] + code, where
                    assert all(table_takes(t, m) for t, m in zip(g["table_select"], region_maxima(self.rate, g, v))), where
                    assert 2 * g["big_values"] + 4 * g["count1"] <= 576, where
                    if g["window_switching_flag"]:
                        assert g["block_type"] in (1, 2, 3), where
                        if g["block_type"] == 2:
                            assert (g["big_values"], g["count1"]) in ((288, 0), (0, 0)), where
                        else:
                            assert (g["region0_count"], g["region1_count"]) == (7, 13), where
                    else:
                        assert g["block_type"] == 0 and g["region0_count"] <= 15 and g["region1_count"] <= 7, where
                        assert g["region0_count"] + g["region1_count"] + 2 <= 22, where
                    c1 = v[2 * g["big_values"]:2 * g["big_values"] + 4 * g["count1"]]
                    assert np.abs(c1).max(initial=0) <= 1 and not v[2 * g["big_values"] + 4 * g["count1"]:].any(), where
                    s1, s2 = SLEN1[g["scalefac_compress"]], SLEN2[g["scalefac_compress"]]
                    sf = q["scalefac"]
                    if g["window_switching_flag"] and g["block_type"] == 2:
                        assert (sf[:18] < (1 << s1)).all() and (sf[18:36] < (1 << s2)).all() and (sf >= 0).all(), where
                    else:
                        assert (sf[:11] < (1 << s1)).all() and (sf[11:21] < (1 << s2)).all() and (sf >= 0).all(), where
            assert bits % 8 == 0 and bits <= IMAGE_BITS and self.mdb[n + 1] == self.mdb[n] + self.slot - bits // 8 >= 0, (self.name, n)
        return self


# ---------------------------------------------------------------------------------------------------------------------
# the sets
# ---------------------------------------------------------------------------------------------------------------------
def _signs(x, y):
    return [(sx * x, sy * y) for sx in ((1, -1) if x else (1,)) for sy in ((1, -1) if y else (1,))]


def table_cells(t):
    """every (x, y) of table t with its sign combinations; the escape cells of tables >= 16 with linbits values 0, 1, a middle
    one and the largest (tables 23 and 31: 15 + 8191 = 8206)"""
    out = []
    if t < 16:
        for x in range(HT.xlen[t]):
            for y in range(HT.ylen[t]):
                out += _signs(x, y)
        return out
    lm = int(HT.linmax[t])
    esc = sorted({15, 16, 15 + lm // 2, 15 + lm})
    for x in range(16):
        for y in range(16):
            for xv in (esc if x == 15 else [x]):
                for yv in (esc if y == 15 else [y]):
                    out += _signs(xv, yv)
    return out


_FILL = [(1, 0), (0, -1), (1, 1), (0, 0), (-1, 1)]  # what the other regions hold: table 1


def _fill(ix, slots, k0=0):
    for k, (a, b) in enumerate(slots):
        ix[a], ix[b] = _FILL[(k + k0) % len(_FILL)]


# where F1 puts a table: name -> (block type, region0_count, region1_count, region index)
F1_POSITIONS = {"long0": (0, 15, 4, 0), "long1": (0, 5, 7, 1), "long2": (0, 0, 0, 2), "short0": (2, 0, 0, 0), "short1": (2, 0, 0, 1)}


def f1_chains(rate):
    out = []
    for pos, (bt, r0, r1, reg) in F1_POSITIONS.items():
        if bt == 2:
            pairs, region = short_order(rate)
            mine = [p for p, r in zip(pairs, region) if r == reg]
            rest = [p for p, r in zip(pairs, region) if r != reg]
        else:
            e = SFB_L[rate]
            edges = (0, e[r0 + 1], e[r0 + r1 + 2], 576)
            mine = [(i, i + 1) for i in range(edges[reg], edges[reg + 1], 2)]
            rest = [(i, i + 1) for i in range(0, edges[reg], 2)]  # the regions in front are full; big_values ends in `mine`
        # table 0: the region all zeros and of non-zero length, inside big_values, full neighbours on both sides (behind the last
        # long region: quadruples), so that a region of another size, or bits for it, would show
        ch = Chain("F1", "F1 table 0 in %s" % pos, rate, 1, 320)
        ch.tag = (list(F1_POSITIONS).index(pos), 0)
        grs = []
        for k in (0, 2):
            ix = np.zeros(576, np.int16)
            _fill(ix, rest, k)
            tables = [1, 1, 1]
            tables[reg] = 0
            if bt == 2:
                grs.append(granule(ix, 2, tables[:2], 288))
            elif reg < 2:
                behind = [(i, i + 1) for i in range(edges[reg + 1], edges[reg + 1] + 12, 2)]
                _fill(ix, behind, k + 1)
                grs.append(granule(ix, 0, tables, edges[reg + 1] // 2 + 6, 0, r0, r1))
            else:
                end = edges[reg] + 24  # twelve zero pairs of region 2, then two quadruples
                ix[end:end + 8] = (1, 0, -1, 1, 0, 0, 1, -1)
                grs.append(granule(ix, 0, tables, end // 2, 2, r0, r1, c1sel=k // 2))
        ch.frame(grs)
        out.append(ch.check())
        for t in TABLES:
            ch = Chain("F1", "F1 table %d in %s" % (t, pos), rate, 1, 320)
            ch.tag = (list(F1_POSITIONS).index(pos), ALL_TABLES.index(t))
            cells, grs, k = table_cells(t), [], 0
            lim = min(3900, 4 * ch.slot - 120)  # (two granules of a frame fit its slot, and each its 4095 bits)
            while k < len(cells):
                ix = np.zeros(576, np.int16)
                _fill(ix, rest, k)
                zero = sum(pair_bits(t, 0, 0)) if bt == 2 else 0  # (a short granule codes all 576 lines: the rest of the region as zeros)
                bits = 4 * len(rest) + zero * len(mine)
                used = 0
                for a, b in mine:
                    if k == len(cells) or bits > lim:
                        break
                    ix[a], ix[b] = cells[k]
                    bits += sum(pair_bits(t, *cells[k])) - zero
                    k += 1
                    used += 1
                tables = [1, 1, 1]
                tables[reg] = t
                if bt == 2:
                    grs.append(granule(ix, 2, tables[:2], 288))
                else:
                    grs.append(granule(ix, 0, tables, (mine[used - 1][1] + 1) // 2, 0, r0, r1))
                if len(grs) == 2:
                    ch.frame(grs)
                    grs = []
            if grs:
                ch.frame(grs + [granule()])
            out.append(ch.check())
    return out


def f2_chains(rate):
    out = []
    quads = []
    for p in range(16):
        mags = [(p >> k) & 1 for k in range(4)]
        nz = [k for k in range(4) if mags[k]]
        for s in range(1 << len(nz)):
            q = list(mags)
            for j, k in enumerate(nz):
                if (s >> j) & 1:
                    q[k] = -1
            quads.append(q)
    allq = np.array(quads, np.int16).reshape(-1)  # 81 quadruples
    for sel in (0, 1):
        ch = Chain("F2", "F2 every quadruple, count1 table %d" % sel, rate)
        ix = np.zeros(576, np.int16)
        ix[:len(allq)] = allq
        ix2 = np.zeros(576, np.int16)
        ix2[:40] = [3, -2, 0, 1, 2, 2, -1, 0] * 5
        ix2[40:40 + len(allq)] = allq
        ch.frame([granule(ix, c1=81, c1sel=sel), granule(ix2, 0, (7, 7, 7), 20, 81, 3, 2, c1sel=sel)])
        one = np.zeros(576, np.int16)
        one[:4] = (0, -1, 1, 0)
        full = np.tile(np.array([1, 0, -1, 1, 0, 0, 0, -1], np.int16), 72)
        ch.frame([granule(one, c1=1, c1sel=sel), granule(full, c1=144, c1sel=sel)])
        ch.frame([granule(c1=0, c1sel=sel), granule(full, 3, c1=144, c1sel=sel)])
        # 2 big_values + 4 count1 == 576 exactly, on every block type that has a count1 region
        ix3 = full.copy()
        ix3[:200] = np.tile(np.array([5, -3, 0, 2], np.int16), 50)
        for bt in (0, 1, 3):
            ch.frame([granule(ix3, bt, (9, 8, 7), 100, 94, 4, 3, c1sel=sel), granule(ix3, bt, (9, 8, 0) if bt else (9, 8, 9), 100, 94, 15, 5, c1sel=sel)])
        out.append(ch.check())
    ch = Chain("F2", "F2 region boundaries", rate)
    big = np.tile(np.array([2, -1, 0, 3, 1, 1], np.int16), 96)
    cases = [(0, 0, 288), (15, 5, 288), (14, 6, 288), (15, 4, 288), (15, 5, 5), (7, 7, 18), (0, 7, 2), (15, 0, 81), (3, 3, 1)]
    e = SFB_L[rate]
    cases += [(r0, r1, e[r0 + 1] // 2 + d) for r0, r1 in ((2, 3), (9, 5)) for d in (-1, 0, 1)]          # big_values around region 1's start
    cases += [(r0, r1, e[r0 + r1 + 2] // 2 + d) for r0, r1 in ((2, 3), (9, 5)) for d in (-1, 0, 1)]    # ... and region 2's
    grs = []
    for r0, r1, bv in cases:
        ix = big.copy()
        ix[2 * bv:] = 0
        ix[2 * bv:min(2 * bv + 8, 576)] = np.array([1, 0, 0, -1, 0, 1, 1, 1], np.int16)[:min(8, 576 - 2 * bv)]
        grs.append(granule(ix, 0, (5, 6, 7), bv, min(2, (576 - 2 * bv) // 4), r0, r1, c1sel=len(grs) & 1))
    for bt in (1, 3):  # region counts 7 / 13: region 1 runs to the end
        for bv in (e[8] // 2 - 1, e[8] // 2, e[8] // 2 + 1, 288):
            ix = big.copy()
            ix[2 * bv:] = 0
            grs.append(granule(ix, bt, (5, 6), bv))
    if len(grs) & 1:
        grs.append(granule())
    for k in range(0, len(grs), 2):
        ch.frame(grs[k:k + 2])
    out.append(ch.check())
    return out


def f3_chains(rate):
    out = []
    body = np.zeros(576, np.int16)
    body[:12] = (1, -2, 0, 3, 1, 1, 0, -1, 2, 0, 0, 1)

    def sf_long(sfc, phase):
        s = np.zeros(39, np.int32)
        for i in range(21):
            s[i] = ((1 << (SLEN1[sfc] if i < 11 else SLEN2[sfc])) - 1) * ((i + phase) & 1)
        return s

    def sf_short(sfc, phase):
        s = np.zeros(39, np.int32)
        for i in range(36):
            s[i] = ((1 << (SLEN1[sfc] if i < 18 else SLEN2[sfc])) - 1) * ((i // 3 + i + phase) & 1)
        return s

    ch = Chain("F3", "F3 scalefac_compress x scfsi, long", rate)
    for sfc in range(16):
        for pat in range(16):
            scfsi = [[(pat >> b) & 1 for b in range(4)], [0] * 4]
            # (scfsi is set in granule 0's frame too: it must be ignored there)
            ch.frame([granule(body, 0, (5, 0, 0), 6, 0, 7, 7, sfc=sfc, sf=sf_long(sfc, pat & 1)),
                      granule(body, 3 if pat == 5 else 0, (5, 0, 0), 6, 0, 7, 7, sfc=sfc, sf=sf_long(sfc, 1 - (pat & 1)))], scfsi=scfsi)
    out.append(ch.check())
    ch = Chain("F3", "F3 scalefac_compress, short and stereo scfsi", rate, 2, 320)
    sb = np.zeros(576, np.int16)
    sb[:9] = (1, 0, -1, 2, 0, 0, 1, 1, -2)
    for sfc in range(16):
        scfsi = [[sfc & 1, (sfc >> 1) & 1, (sfc >> 2) & 1, (sfc >> 3) & 1], [1 - (sfc & 1), 1, 0, (sfc >> 2) & 1]]
        ch.frame([granule(sb, 2, (7, 7), 288, sfc=sfc, sf=sf_short(sfc, 0)), granule(body, 0, (5, 0, 0), 6, 0, 7, 7, sfc=15 - sfc, sf=sf_long(15 - sfc, 0)),
                  granule(body, 0, (5, 0, 0), 6, 0, 7, 7, sfc=sfc, sf=sf_long(sfc, 1)), granule(sb, 2, (7, 7), 288, sfc=15 - sfc, sf=sf_short(15 - sfc, 1))],
                 scfsi=scfsi)
    out.append(ch.check())
    return out


def pairs_by_length():
    """total length (code + extension bits) -> (table, x, y): one pair for every total length that exists.  The tables give 1 .. 26,
    28, 30, 32 and 36: the 19-bit code words are in tables 13 and 15, which have no linbits (19 + 2 signs), and the corner cell of
    the tables with 13 linbits is 8 bits long (8 + 28)"""
    best = {}
    for t in TABLES:
        lm = int(HT.linmax[t])
        for x in range(HT.xlen[t]):
            for y in range(HT.ylen[t]):
                xv, yv = (x + lm if t > 15 and x == 15 else x), (y + lm if t > 15 and y == 15 else y)
                best.setdefault(sum(pair_bits(t, xv, yv)), (t, -xv, yv))
    return best


def f4_chains(rate):
    out = []
    by_len = pairs_by_length()
    assert set(by_len) >= set(range(1, 27)) | {28, 30, 32, 36} and max(by_len) == 36, sorted(by_len)
    # the longest code word (19 bits, with both signs 21) and the longest extension (13 + 1 + 13 + 1 = 28 bits behind 8): every offset
    n19, t19, x19, y19 = max((HT.cell(t, x, y)[1], t, x, y) for t in TABLES for x in range(HT.xlen[t]) for y in range(HT.ylen[t]))
    assert n19 == 19 and sum(pair_bits(31, 8206, 8206)) == HT.cell(31, 15, 15)[1] + 28
    sweep = [(by_len[n], (0, 17, 31, 32 - (n + 1) // 2)) for n in sorted(by_len)]
    sweep += [((t19, -x19, y19), tuple(range(32))), ((23, -8206, 8206), tuple(range(32))), ((31, 8206, -8206), tuple(range(32)))]
    ch = Chain("F4", "F4 code words across word edges", rate)
    for (t, x, y), offs in sweep:
        for off in offs:
            # granule 0 is `off` bits of stuffing (mod 32) behind a quadruple; granule 1's region 0 is table 1's (0, 0) twice,
            # the pair under test the first of region 1 behind two 1-bit pairs: the frame's image starts on a word edge, so its bit position is known
            g0 = granule(np.array([1, -1, 0, 1] + [0] * 572, np.int16), c1=1)
            ix = np.zeros(576, np.int16)
            ix[4], ix[5] = x, y
            ix[6], ix[7] = 1, -1
            g1 = granule(ix, 0, (1, t, 1), 4, 0, 0, 0)
            b0 = count1_bits(0, g0["ix"][:4])
            g0["stuff"] = (off - b0 - 2) % 32 + 32 * (off & 1)  # (two pairs of region 0 precede the pair under test)
            ch.frame([g0, g1], spill="drain")
    out.append(ch.check())
    ch = Chain("F4", "F4 granule starts at every word offset", rate, 2, 320)
    body = np.zeros(576, np.int16)
    body[:16] = (17, -3, 0, 40, 1, 1, -15, 16, 1, 0, 0, -1, 1, 0, 1, -1)
    for off in range(32):
        sf = np.zeros(39, np.int32)
        sf[:21] = [(i * 5 + off) % 8 if i < 11 else (i + off) % 4 for i in range(21)]
        grs = [granule(body, 0, (26, 0, 0), 4, 2, 15, 5, sfc=12, sf=sf, stuff=(off - k) % 32 + 32 * k) for k in range(4)]
        ch.frame(grs, spill="drain")
    out.append(ch.check())
    ch = Chain("F4", "F4 stuffing runs", rate)
    for n in (0, 1, 31, 32, 33, 63, 64, 65):
        for lead in (0, 5, 31):
            g0 = granule(body, 0, (26, 0, 0), 4, 2, 15, 5, stuff=lead)
            g1 = granule(body, 0, (26, 0, 0), 4, 2, 15, 5, stuff=n)
            ch.frame([g0, g1], spill="drain")
    g1 = granule(body, 0, (26, 0, 0), 4, 2, 15, 5)
    g1["stuff"] = 4095 - sum(k for _, k in granule_puts(rate, g1, g1["ix"], 1, [0] * 4))  # the largest a granule allows
    ch.frame([granule(stuff=4095), g1])  # (what the slot holds beyond 2 * 4095 bits is drained)
    out.append(ch.check())
    return out


def f5_chains(rate):
    out = []
    body = np.zeros(576, np.int16)
    body[:20] = (3, -3, 0, 7, 1, 1, -5, 6, 1, 0, 0, -1, 1, 0, 1, -1, 0, 0, 1, 0)

    def gb(**kw):
        return granule(body, 0, (12, 0, 0), 4, 3, 15, 5, **kw)

    ch = Chain("F5", "F5 part2_3_length 4095", rate)
    ch.frame([granule(), gb()], spill="drain")
    g = gb()
    g["stuff"] = 4095 - sum(k for _, k in granule_puts(rate, g, g["ix"], 0, [0] * 4))
    ch.frame([g, granule(stuff=4095)])                            # 4095 + 4095 bits, the rest of the frame's share is drained
    ch.frame([gb(), granule()], spill="drain")
    out.append(ch.check())
    ch = Chain("F5", "F5 part2_3_length 0, resvDrain values", rate, 1, 96)
    ch.frame([granule(), granule()], take=0)                      # an empty frame: both lengths 0
    for drain in (0, 8, 858, 3162, 1024):
        ch.frame([granule(), granule()], take=0 if ch.room() <= 511 else None)  # (room for the drain)
        g0, g1 = gb(), gb(sfc=5, sf=[1] * 11 + [1] * 10 + [0] * 18)
        bits = sum(sum(k for _, k in granule_puts(rate, g, g["ix"], gr, [0] * 4)) for gr, g in enumerate((g0, g1)))
        g1["stuff"] = (-(bits + drain)) % 8
        ch.frame([g0, g1], drain=drain)
    out.append(ch.check())
    # every bitrate, mono and stereo in turn; header fields
    for k, kbps in enumerate(BITRATES):
        C = 1 + (k & 1)
        ch = Chain("F5", "F5 %d kbps, %d channel(s)" % (kbps, C), rate, C, kbps)
        for _ in range(3):
            ch.frame([gb() if (j + _) & 1 else granule() for j in range(2 * C)])
        out.append(ch.check())
    for mode, mode_ext in ((3, 0), (0, 0), (2, 0), (1, 0), (1, 1), (1, 2), (1, 3), (0, 3)):
        for crc in (0, 1):
            C = 1 if mode == 3 else 2
            ch = Chain("F5", "F5 mode %d mode_ext %d crc %d" % (mode, mode_ext, crc), rate, C, 128, mode=mode, mode_ext=mode_ext, crc=crc)
            for _ in range(3):
                ch.frame([gb(sfc=9, sf=[3, 0] * 5 + [3] + [0, 3] * 5 + [0] * 18) for _j in range(2 * C)], scfsi=[[1, 0, 1, 0], [0, 1, 1, 0]])
            out.append(ch.check())
    for flags in range(16):
        ch = Chain("F5", "F5 copyright / original / emphasis %d" % flags, rate, 2 - (flags & 1), 96, copyright=flags >> 3, original=(flags >> 2) & 1,
                   emphasis=flags & 3, crc=(flags >> 1) & 1)
        ch.frame([gb() for _j in range(2 * ch.channels)])
        ch.frame([gb() for _j in range(2 * ch.channels)])
        out.append(ch.check())
    return out


def _pad_granules(C, bits):
    """2 * C granules of stuffing and quadruples that hold `bits` bits between them"""
    grs = []
    for k in range(2 * C):
        n = min(bits, 4095)
        bits -= n
        if n >= 32:
            ix = np.zeros(576, np.int16)
            ix[:8] = (1, 0, -1, 0, 0, 1, 1, -1)
            g = granule(ix, c1=2, c1sel=k & 1)
            g["stuff"] = n - sum(count1_bits(k & 1, ix[i:i + 4]) for i in (0, 4))
        else:
            g = granule(stuff=n)
        grs.append(g)
    assert bits == 0
    return grs


def f6_chain(name, rate, C, kbps, takes, crc=0):
    """a chain whose frames consume exactly takes[n] bytes"""
    ch = Chain("F6", name, rate, C, kbps, crc=crc)
    for t in takes:
        ch.frame(_pad_granules(C, 8 * t), take=t, drain=0)
    return ch.check()


def f6_chains(rate):
    out = []
    # the smallest slot: 32 kbps stereo (at 48 kHz 60 bytes: main_data_begin 511 reaches nine frames back)
    slot = frame_bytes_of(rate, 32) - 36
    up = []  # frames that take nothing until the reservoir is full, then exactly to 511
    m = 0
    while m + slot <= 511:
        up.append(0)
        m += slot
    up.append(m + slot - 511)
    reach = -(-511 // slot)
    out.append(f6_chain("F6 main_data_begin 0, 1 and 511, reach back %d frames" % reach, rate, 2, 32,
                        up + [511 + slot, slot - 1, slot + 1, slot, 0, slot - 1, 7, 2 * slot - 7]))
    out.append(f6_chain("F6 reach back 1 and 2 frames", rate, 2, 32, [slot - 5, slot + 5, 0, slot - 9, 2 * slot + 9, slot]))
    out.append(f6_chain("F6 one frame", rate, 2, 32, [slot - 3]))
    out.append(f6_chain("F6 one frame, mono, full slot", rate, 1, 64, [frame_bytes_of(rate, 64) - 21]))
    out.append(Chain("F6", "F6 no frames", rate, 2, 32).check())
    # the flush: the data ends exactly on a slot boundary with k = 1, 2 slots unwritten
    for C, kbps, crc in ((2, 32, 0), (2, 128, 0), (1, 64, 0), (2, 128, 1), (1, 40, 1), (2, 320, 0)):
        s = frame_bytes_of(rate, kbps) - (4 + 2 * crc + (32 if C == 2 else 17))
        tag = "%d ch %d kbps crc %d (slot %d)" % (C, kbps, crc, s)
        for k in (1, 2):
            if k * s > 511:
                continue
            base = [s] * 2
            out.append(f6_chain("F6 flush: ends on a boundary, %d queued, %s" % (k, tag), rate, C, kbps, base + [0] * k, crc))
            out.append(f6_chain("F6 flush: one byte before the boundary, %d queued, %s" % (k, tag), rate, C, kbps, base + [0] * (k - 1) + [1], crc))
            out.append(f6_chain("F6 flush: one byte past the boundary, %d queued, %s" % (k, tag), rate, C, kbps, [s, s - 1] + [0] * k, crc))
        out.append(f6_chain("F6 flush: ends on a boundary, nothing queued, %s" % tag, rate, C, kbps, [s] * 3, crc))
        out.append(f6_chain("F6 flush: a single frame that takes nothing, %s" % tag, rate, C, kbps, [0], crc))
    return out


def f7_chains(rate, n_chains=6, n_frames=16):
    out = []
    rng = np.random.default_rng(0xF7 + rate)
    for c in range(n_chains):
        C = 1 + (c & 1)
        kbps = (64, 128, 320, 96, 192, 48)[c % 6]
        ch = Chain("F7", "F7 random chain %d" % c, rate, C, kbps, crc=(c >> 1) & 1, mode=(3 if C == 1 else (0, 2, 1)[c % 3]))
        for _ in range(n_frames):
            budget = 8 * ch.room()
            scale = float(rng.choice([0.3, 1.0, 3.0, 12.0, 80.0]))
            while True:
                scfsi = rng.integers(0, 2, (2, 4))
                grs = [_random_granule(rng, rate, scale) for _k in range(2 * C)]
                bits = 0
                for k, g in enumerate(grs):
                    gr, chn = divmod(k, C)
                    own = sum(n for _, n in granule_puts(rate, g, g["ix"], gr, scfsi[chn]))
                    bits += own
                    g["fits"] = own <= 4095
                if bits + 8 <= budget and all(g["fits"] for g in grs):
                    break
                scale *= 0.5
            lo = max((bits + 7) // 8, ch.room() - 511)
            take = int(rng.integers(lo, min(ch.room(), lo + 2 * ch.slot) + 1))
            nxt = ch.room() - take
            if nxt > 0 and nxt % ch.slot == 0:
                take += 1
            drain = int(rng.integers(0, 4)) * 8 + (-bits) % 8
            if rng.random() < 0.3 or not 0 <= 8 * take - bits - drain <= 4095 * 2 * C - bits:
                drain = None  # (stuffing first, what it cannot hold is drained)
            ch.frame(grs, scfsi=scfsi, take=take, drain=drain)
        out.append(ch.check())
    return out


def _random_granule(rng, rate, scale):
    bt = int(rng.choice([0, 0, 1, 2, 3]))
    decay = np.exp(-np.arange(576) / float(rng.choice([20, 80, 300])))
    mag = np.trunc(rng.laplace(0, scale, 576) * decay)
    ix = np.clip(np.abs(mag), 0, 8206).astype(np.int64) * rng.choice([-1, 1], 576)
    sfc = int(rng.integers(0, 16))
    sf = np.zeros(39, np.int32)
    if bt == 2:
        sf[:18] = rng.integers(0, 1 << SLEN1[sfc], 18)
        sf[18:36] = rng.integers(0, 1 << SLEN2[sfc], 18)
        if not ix.any():
            return granule(None, 2, (0, 0), 0, sfc=sfc, sf=sf, gain=int(rng.integers(0, 256)))
        g = granule(ix, 2, (0, 0), 288, sfc=sfc, sf=sf, gain=int(rng.integers(0, 256)), preflag=0)
    else:
        sf[:11] = rng.integers(0, 1 << SLEN1[sfc], 11)
        sf[11:21] = rng.integers(0, 1 << SLEN2[sfc], 10)
        nz = np.flatnonzero(ix)
        end = int(nz[-1]) + 1 if nz.size else 0
        big = np.flatnonzero(np.abs(ix) > 1)
        bv = (int(big[-1]) + 2) // 2 if big.size else 0
        bv = min(288, bv + int(rng.integers(0, 3)))
        c1 = max(0, -(-(end - 2 * bv) // 4))
        if 2 * bv + 4 * c1 > 576:
            bv, c1 = 288, 0
        r0 = int(rng.integers(0, 16))
        r1 = int(rng.integers(0, min(7, 20 - r0) + 1))
        g = granule(ix, bt, (0, 0, 0), bv, c1, r0, r1, sfc=sfc, sf=sf, c1sel=int(rng.integers(0, 2)), gain=int(rng.integers(0, 256)),
                    preflag=int(rng.integers(0, 2)))
    m = region_maxima(rate, g, g["ix"])
    g["table_select"] = [int(rng.choice(legal_tables(v))) if v or rng.random() < 0.5 else 0 for v in m]
    if bt:
        g["table_select"][2] = 0
    return g


SET_NAMES = ("F1", "F2", "F3", "F4", "F5", "F6", "F7")
_cache = {}


def chains(rate):
    """every chain of every set at `rate`"""
    if rate not in _cache:
        _cache[rate] = f1_chains(rate) + f2_chains(rate) + f3_chains(rate) + f4_chains(rate) + f5_chains(rate) + f6_chains(rate) + f7_chains(rate)
    return _cache[rate]


def subset(all_chains, stride):
    """of F1 the chains whose position index + table index is a multiple of stride (stride 5: every table once, every position six
    times), every stride-th chain of F7, and every chain of the other sets: still contains every set"""
    n = {}
    out = []
    for c in all_chains:
        k = n[c.set] = n.get(c.set, -1) + 1
        if c.set == "F1":
            if sum(c.tag) % stride == 0:
                out.append(c)
        elif c.set != "F7" or k % stride == 0:
            out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the three implementations
# ---------------------------------------------------------------------------------------------------------------------
def run_oracle(lib, ch):
    """(bytes, main_data_begin after every frame, abort code | frames << 8)"""
    lib.mp3o_format_frames.restype = ctypes.c_size_t
    lib.mp3o_format_frames.argtypes = [ctypes.c_int] * 10 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p,
                                                               ctypes.POINTER(ctypes.c_int)]
    side, ix = np.ascontiguousarray(ch.side_array()), np.ascontiguousarray(ch.ix_array())
    after = np.zeros(max(ch.n_frames, 1), np.int32)
    out, ab = ctypes.c_void_p(), ctypes.c_int(0)
    n = lib.mp3o_format_frames(ch.rate, ch.channels, ch.kbps, ch.mode, ch.mode_ext, ch.crc, ch.copyright, ch.original, ch.emphasis, ch.n_frames,
                               side.ctypes.data, ix.ctypes.data, ctypes.byref(out), after.ctypes.data, ctypes.byref(ab))
    assert out.value, "the oracle refused %s" % ch.name
    data = ctypes.string_at(out.value, n)
    libc = ctypes.CDLL("libc.so.6")
    libc.free.argtypes = [ctypes.c_void_p]
    libc.free(out)
    return data, after[:ch.n_frames], ab.value


def write_chain(ch, path):
    with open(path, "wb") as f:
        f.write(np.array([ch.rate, ch.channels, ch.kbps, ch.mode, ch.mode_ext, ch.crc, ch.copyright, ch.original, ch.emphasis, ch.n_frames, 0, 0],
                         "<i4").tobytes())
        f.write(ch.side_array().tobytes())
        f.write(ch.ix_array().tobytes())


def run_probe(exe, ch, workdir, timeout=60):
    """one child process per chain: (exit status, bytes, main_data_begin after every frame the probe got through)"""
    cf, mp3, mdb = (os.path.join(workdir, n) for n in ("chain.bin", "out.mp3", "mdb.bin"))
    for p in (mp3, mdb):
        if os.path.exists(p):
            os.remove(p)
    write_chain(ch, cf)
    r = subprocess.run([exe, cf, mp3, mdb], capture_output=True, cwd=workdir, timeout=timeout)
    data = open(mp3, "rb").read() if os.path.exists(mp3) else b""
    after = np.fromfile(mdb, "<i4") if os.path.exists(mdb) else np.zeros(0, np.int32)
    return r.returncode, data, after, r.stderr[-300:]


def run_hook(lib, group):
    """chains of one format through mp3mi_debug_format_frames: (rc, [bytes per chain], status per chain)"""
    lib.mp3mi_debug_format_frames.argtypes = [ctypes.c_int] * 8 + [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    c0 = group[0]
    assert all(c.format_key() == c0.format_key() for c in group)
    S, nf, C = len(group), max(c.n_frames for c in group), c0.channels
    side = np.zeros((S, max(nf, 1)), SIDE_DT)
    ix = np.zeros((S, max(nf, 1), 2, C, 576), np.int16)
    for s, c in enumerate(group):
        side[s, :c.n_frames] = c.side_array()
        ix[s, :c.n_frames] = c.ix_array()
    counts = np.array([c.n_frames for c in group], np.int32)
    stride = (nf * c0.frame_bytes + 1 + 255) // 256 * 256
    out = np.zeros((S, stride), np.uint8)
    lens, status = np.zeros(S, np.uint32), np.zeros(S, np.int32)
    rc = lib.mp3mi_debug_format_frames(c0.rate, C, c0.kbps, c0.mode, c0.hdr_flags, c0.crc, S, nf, counts.ctypes.data, ix.ctypes.data,
                                       side.ctypes.data, out.ctypes.data, stride, lens.ctypes.data, status.ctypes.data)
    return rc, [out[s, :lens[s]].tobytes() for s in range(S)], status


def by_format(all_chains):
    groups = {}
    for c in all_chains:
        groups.setdefault(c.format_key(), []).append(c)
    return list(groups.values())


# ---------------------------------------------------------------------------------------------------------------------
# the decoder (ISO 11172-3, 2.4.1 - 2.4.3): shares nothing with the bit counter above or with the product
# ---------------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self, data):
        self.b = np.unpackbits(np.frombuffer(data, np.uint8)).tolist()
        self.p = 0

    def get(self, n):
        v = 0
        for bit in self.b[self.p:self.p + n]:
            v = v << 1 | bit
        assert self.p + n <= len(self.b), "the stream ends inside a field"
        self.p += n
        return v


class Decoder:
    def __init__(self, huff=None):
        h = huff or Huff()
        self.trees = {}
        for t in list(TABLES) + [32, 33]:
            d = {}
            for x in range(h.xlen[t]):
                for y in range(h.ylen[t]):
                    code, n = h.cell(t, x, y)
                    assert (n, code) not in d
                    d[(n, code)] = (x, y)
            self.trees[t] = d
        self.linbits = {t: int(h.linbits[t]) for t in TABLES}

    def _sym(self, r, t):
        d, code, b, p = self.trees[t], 0, r.b, r.p
        for n in range(1, min(20, len(b) - p + 1)):
            code = code << 1 | b[p + n - 1]
            if (n, code) in d:
                r.p = p + n
                return d[(n, code)]
        raise AssertionError("no code word of table %d matches" % t)

    def _value(self, r, t, v):
        if t > 15 and v == 15:
            v += r.get(self.linbits[t])
        return -v if v and r.get(1) else v

    def decode(self, data, n_frames):
        """-> list of frames: dict(header fields, main_data_begin, scfsi, gr[gr][ch] = dict(fields, scalefac, sent, ix), drain)"""
        hd = Bits(data[:4])
        assert hd.get(12) == 0xfff and hd.get(1) == 1 and hd.get(2) == 1
        crc = 1 - hd.get(1)
        kbps = (0,) + BITRATES
        kbps = kbps[hd.get(4)]
        rate = RATES[hd.get(2)]
        hd.get(2)
        C = 1 if hd.get(2) == 3 else 2
        fb = 144000 * kbps // rate
        si = 4 + 2 * crc + (32 if C == 2 else 17)
        main = b"".join(data[n * fb + si:(n + 1) * fb] for n in range(n_frames))
        md = Bits(main)
        frames = []
        for n in range(n_frames):
            r = Bits(data[n * fb:n * fb + si])
            f = {}
            assert r.get(12) == 0xfff
            f["version"], f["layer"], f["crc"], f["bitrate_index"], f["rate_index"] = r.get(1), 4 - r.get(2), 1 - r.get(1), r.get(4), r.get(2)
            f["padding"], f["extension"], f["mode"], f["mode_ext"] = r.get(1), r.get(1), r.get(2), r.get(2)
            f["copyright"], f["original"], f["emphasis"] = r.get(1), r.get(1), r.get(2)
            if f["crc"]:
                f["crc_word"] = r.get(16)
            f["main_data_begin"] = r.get(9)
            f["private_bits"] = r.get(3 if C == 2 else 5)
            f["scfsi"] = [[r.get(1) for _ in range(4)] for _ in range(C)]
            f["gr"] = [[None] * C for _ in range(2)]
            for gr in range(2):
                for ch in range(C):
                    g = dict(part2_3_length=r.get(12), big_values=r.get(9), global_gain=r.get(8), scalefac_compress=r.get(4),
                             window_switching_flag=r.get(1), block_type=0, mixed_block_flag=0, subblock_gain=[0, 0, 0])
                    if g["window_switching_flag"]:
                        g["block_type"], g["mixed_block_flag"] = r.get(2), r.get(1)
                        g["table_select"] = [r.get(5), r.get(5)]
                        g["subblock_gain"] = [r.get(3) for _ in range(3)]
                        g["region0_count"], g["region1_count"] = (8, 36) if g["block_type"] == 2 else (7, 13)
                    else:
                        g["table_select"] = [r.get(5) for _ in range(3)]
                        g["region0_count"], g["region1_count"] = r.get(4), r.get(3)
                    g["preflag"], g["scalefac_scale"], g["count1table_select"] = r.get(1), r.get(1), r.get(1)
                    f["gr"][gr][ch] = g
            assert r.p == 8 * si
            start = 8 * (n * (fb - si) - f["main_data_begin"])
            if frames:  # what lies between the frame before and this one: the drained bits, zeros
                gap = md.b[md.p:start]
                assert start >= md.p and not any(gap), "frame %d: main data overlaps, or ones in the drain" % n
                frames[-1]["drain"] = len(gap)
            md.p = start
            for gr in range(2):
                for ch in range(C):
                    self._granule(md, rate, f, gr, ch, frames)
            frames.append(f)
        if frames:
            frames[-1]["drain"] = None  # (the flush's zeros follow: not told apart)
        return frames

    def _granule(self, md, rate, f, gr, ch, frames):
        g = f["gr"][gr][ch]
        end = md.p + g["part2_3_length"]
        s1, s2 = SLEN1[g["scalefac_compress"]], SLEN2[g["scalefac_compress"]]
        sf, sent = [0] * 39, [False] * 39
        shortb = g["window_switching_flag"] and g["block_type"] == 2
        if shortb:
            for i in range(36):
                sf[i], sent[i] = md.get(s1 if i < 18 else s2), True
        else:
            for b, (lo, hi) in enumerate(((0, 6), (6, 11), (11, 16), (16, 21))):
                for i in range(lo, hi):
                    if gr == 0 or not f["scfsi"][ch][b]:
                        sf[i], sent[i] = md.get(s1 if i < 11 else s2), True
                    else:
                        sf[i] = f["gr"][0][ch]["scalefac"][i]  # shared with granule 0
        g["scalefac"], g["sent"] = sf, sent
        ix = [0] * 576
        bv2 = 2 * g["big_values"]
        assert bv2 <= 576
        ts = g["table_select"]
        if shortb:
            e = SFB_S[rate]
            k = 0
            for sfb in range(13):
                t = ts[0] if e[sfb] < 12 else ts[1]  # region 0 = the first 36 values = bands below line 12 (region0_count 8)
                for w in range(3):
                    for line in range(e[sfb], e[sfb + 1], 2):
                        if k < bv2:
                            x, y = self._sym(md, t) if t else (0, 0)
                            ix[line * 3 + w], ix[(line + 1) * 3 + w] = self._value(md, t, x), self._value(md, t, y)
                            k += 2
        else:
            r1 = SFB_L[rate][g["region0_count"] + 1]
            r2 = SFB_L[rate][min(g["region0_count"] + g["region1_count"] + 2, 22)]
            for i in range(0, bv2, 2):
                t = ts[0] if i < r1 else (ts[1] if i < r2 else ts[2])
                x, y = self._sym(md, t) if t else (0, 0)
                ix[i], ix[i + 1] = self._value(md, t, x), self._value(md, t, y)
        assert md.p <= end, "big values run past part2_3_length"
        i = bv2
        t = 32 + g["count1table_select"]
        while md.p < end and i + 4 <= 576:
            save = md.p
            try:
                _, p = self._sym(md, t)
                q = [self._value(md, 0, (p >> k) & 1) for k in range(4)]
            except AssertionError:
                md.p = save
                break
            if md.p > end:  # a quadruple that runs past the granule's end is stuffing, not data
                md.p = save
                break
            ix[i:i + 4] = q
            i += 4
        rest = md.b[md.p:end]
        assert all(rest), "stuffing that is not ones"
        md.p = end
        g["ix"] = ix


# ---------------------------------------------------------------------------------------------------------------------
# checks shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def roundtrip_mismatch(dec, ch, data):
    """None where the decoder reads back exactly what the chain holds: every header and side-info field, every scalefactor that was
    transmitted, every signed line, the drained zeros; else what differs first"""
    if not ch.n_frames:
        return None if data == b"" else "bytes for a chain of no frames"
    try:
        frames = dec.decode(data, ch.n_frames)
    except AssertionError as e:
        return "%s: the decoder stops: %s" % (ch.name, e)
    want_hdr = dict(version=1, layer=3, crc=ch.crc, bitrate_index=BITRATES.index(ch.kbps) + 1, rate_index=RATES.index(ch.rate), padding=0,
                    extension=0, mode=ch.mode, mode_ext=ch.mode_ext, copyright=ch.copyright, original=ch.original, emphasis=ch.emphasis,
                    private_bits=0)
    for n, (f, sd, ix) in enumerate(zip(frames, ch.sides, ch.ixs)):
        for k, v in want_hdr.items():
            if f[k] != v:
                return "%s frame %d: header %s %d, not %d" % (ch.name, n, k, f[k], v)
        if f.get("crc_word", 0) != 0 or f["main_data_begin"] != sd["main_data_begin"] or f["scfsi"] != sd["scfsi"][:ch.channels].tolist():
            return "%s frame %d: crc word, main_data_begin or scfsi" % (ch.name, n)
        if f["drain"] is not None and f["drain"] != sd["resvDrain"]:
            return "%s frame %d: %d drained bits, not %d" % (ch.name, n, f["drain"], sd["resvDrain"])
        for gr in range(2):
            for c in range(ch.channels):
                g, q = f["gr"][gr][c], sd["gr"][gr][c]
                names = ["part2_3_length", "big_values", "global_gain", "scalefac_compress", "window_switching_flag", "block_type", "preflag",
                         "count1table_select"] + ([] if q["window_switching_flag"] else ["region0_count", "region1_count"])
                for k in names:
                    if g[k] != q[k]:
                        return "%s frame %d gr %d ch %d: %s %d, not %d" % (ch.name, n, gr, c, k, g[k], q[k])
                nt = len(g["table_select"])
                if g["table_select"] != q["table_select"][:nt].tolist() or g["mixed_block_flag"] or g["scalefac_scale"] or any(g["subblock_gain"]):
                    return "%s frame %d gr %d ch %d: table_select or a field that is always 0" % (ch.name, n, gr, c)
                for i in range(39):
                    if g["sent"][i] and g["scalefac"][i] != q["scalefac"][i]:
                        return "%s frame %d gr %d ch %d: scalefactor %d is %d, not %d" % (ch.name, n, gr, c, i, g["scalefac"][i], q["scalefac"][i])
                if g["ix"] != ix[gr, c].tolist():
                    i = int(np.flatnonzero(np.array(g["ix"]) != ix[gr, c])[0])
                    return "%s frame %d gr %d ch %d: line %d is %d, not %d" % (ch.name, n, gr, c, i, g["ix"][i], ix[gr, c, i])
    return None


class Coverage:
    """what the chains reach, from their inputs: (table, position) pairs (table 0 included), cells, linbits values, the offsets of
    the puts and of those that span two words (scalefactors, code words, extensions and quadruples), reach-back"""

    def __init__(self):
        self.positions, self.cells, self.lin, self.offsets, self.two_word, self.stuff_two_word, self.reach = set(), set(), set(), set(), set(), set(), 0

    def add(self, ch):
        for n, (sd, ix, grs) in enumerate(zip(ch.sides, ch.ixs, ch.grs)):
            self.reach = max(self.reach, -(-ch.mdb[n] // ch.slot))
            pos = 0
            for k, g in enumerate(grs):
                gr, c = divmod(k, ch.channels)
                v = g["ix"]
                shortb = g["block_type"] == 2
                if 2 * g["big_values"]:
                    if shortb:
                        pairs, region = short_order(ch.rate)
                    else:
                        e = SFB_L[ch.rate]
                        r1, r2 = e[g["region0_count"] + 1], e[g["region0_count"] + g["region1_count"] + 2]
                        pairs = [(i, i + 1) for i in range(0, 2 * g["big_values"], 2)]
                        region = [0 if i < r1 else (1 if i < r2 else 2) for i, _ in pairs]
                    for (a, b), r in zip(pairs, region):
                        t = g["table_select"][r]
                        self.positions.add((t, ("short%d" if shortb else "long%d") % r))  # (table 0 too: a region of zeros)
                        if not t:
                            continue
                        x, y = abs(int(v[a])), abs(int(v[b]))
                        self.cells.add((t, min(x, 15), min(y, 15)))
                        if t > 15:
                            self.lin |= {(t, w - 15) for w in (x, y) if w > 14}
                for kind, nb in granule_puts(ch.rate, g, v, gr, sd["scfsi"][c]):
                    self.offsets.add(pos & 31)
                    if (pos & 31) + nb > 32:  # (stuffing is not counted: all ones look the same however they are shifted)
                        self.two_word.add(pos & 31)
                    pos += nb
                end = pos + g["stuff"]
                while pos < end:  # stuffing goes out in words of 32 and a rest
                    nb = min(32, end - pos)
                    if (pos & 31) + nb > 32:
                        self.stuff_two_word.add(pos & 31)
                    pos += nb
                assert pos - sum(int(sd["gr"][j // ch.channels][j % ch.channels]["part2_3_length"]) for j in range(k + 1)) == 0

    def missing(self):
        """what the sets were built to reach and did not (empty: complete)"""
        out = []
        out += [("position", t, p) for t in ALL_TABLES for p in F1_POSITIONS if (t, p) not in self.positions]
        out += [("cell", t, x, y) for t in TABLES for x in range(HT.xlen[t]) for y in range(HT.ylen[t]) if (t, x, y) not in self.cells]
        out += [("linbits", t, w) for t in TABLES if t > 15 for w in (0, HT.linmax[t]) if (t, w) not in self.lin]
        out += [("offset", o) for o in range(32) if o not in self.offsets] + [("two-word put at", o) for o in range(5, 32) if o not in self.two_word]
        # (the longest put that is not stuffing is the 28-bit extension of two 13-linbits escapes: it spans two words from offset 5 on;
        # a stuffing word of 32 ones does from offset 1 on -- a half that is not written shows as zeros)
        out += [("two-word stuffing at", o) for o in range(1, 32) if o not in self.stuff_two_word]
        return out
