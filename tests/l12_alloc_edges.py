"""Frames built to sit on the decisions of k12_alloc (csrc/k_l12.hip), the Layer I / II frame encoder behind the filterbank and the
model, and the three implementations that take them: the product's self-test hook mp3mi_debug_l12_alloc (csrc/l12_alloc_debug.cpp:
the device, or the emulated CPU build), the oracle's mp3o_l12_alloc_frames, which also says what the allocation reached (its
trace), and the unmodified reference's own functions (oracle/_ref/ref_harness_l12_alloc, a process per format).  Everything is
generated here, deterministically, the cases that need a particular outcome by search with the oracle; nothing is read from files.

A case is ONE frame: a format (layer, rate, the driver's mode letter with e / c / o behind it, a bitrate), subband samples
sb[C][parts][12][32] and signal-to-mask ratios ratio[passes][C][32].  The hook runs every case as frames 0, 1 and 2 of a stream, the
streams of a launch at their own bitrates.  The sets:
  A1  scale index: the peak of a band on every multiple[j], j = 0..62, and on its two neighbouring doubles, 0 and 2.0, at each of
      the 12 positions and negative; joint stereo with L = R (the mean is the value), L = -R (the mean is exactly 0) and
      L = m + e, R = m - e (the mean exactly on a table value)
  A2  transmission pattern (Layer II): all 49 pairs of scalefactor differences in -3..3 -- the 25 classes, 0x444 both ways round --
      with the scalefactors in the middle, down at 0 and up at 62, in stereo and in joint stereo
  A3  quantiser: every Layer I allocation 1..14 and every (subband, allocation) cell of the four Layer II tables, the allocation
      pinned by the band's ratio; in each band d = +1, d = -1, +-0, the smallest magnitudes, adjacent doubles either side of the
      sign change and of two quantisation boundaries; grouped triples with all three values at steps - 1, at d = +1 and at d = -1
  A4  allocation order: equal ratios everywhere, neighbouring floats (keys that share an upper half), random ratios chosen by their
      trace: a step that uses all that is left, one that misses by the smallest amount there is, a band closed for lack of room
      while cheaper steps still fit, what is left equal to an open step; Layer I's start at mnr[0][0] + 1 with band (0, 0) open,
      full, and closed for lack of room, a band on it and just below; Layer II's -999999.0f and its neighbour; loud bands at and
      above sblimit
  A5  joint stereo: each mode_ext, and 0 still over budget; rq equal to the frame's bits and just above; above the bound both
      channels' ratios and transmission patterns differ, or tie; two-channel Layer I at 32 kbit/s, whose frame outgrows its slot
  A6  header and CRC: the four modes x -e -c -o; pairs of frames whose allocation differs in one bit
Parity: every cost of a step and every sum of allocation fields is even, but for Layer II's fields at a joint-stereo bound of 12 or
16 in the two large tables (135 and 147 bits).  So `one bit short` and `rq one above the frame` exist only there; everywhere else the
nearest miss is 2 bits, and that is what the sets hold."""
import ctypes
import os
import struct
import subprocess

import numpy as np

from mp3common import L12_BITRATES, L12_DT, L12_MODES, L12_SEAM_DT, L12_SEAMS, ROOT

REF_HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness_l12_alloc")
SET_NAMES = ("A1", "A2", "A3", "A4", "A5", "A6")
NF = 3          # frames of a stream in a launch of the hook: the same case three times
SLOT0 = (0, 16, 5)  # phases of the first slot: Layer I frames then start at 0 12 6, at 16 10 4 (the batch's) and at 5 17 11
OUT_STRIDE = 5376   # >= 3 * 1728 + 1
NEVER = -1000100.0  # a ratio whose band is never a candidate (Layer II: mnr >= 999999)
INT_MAX = 0x7fffffff
TRACE_DT = np.dtype([("frame_bits", "<i4"), ("n_rq", "<i4"), ("rq", "<i4", (5,)), ("steps", "<i4"), ("closed_no_room", "<i4"),
                     ("granted_after_close", "<i4"), ("min_slack", "<i4"), ("min_short", "<i4"), ("exact_after_close", "<i4"),
                     ("min_short_after_close", "<i4"), ("pad", "<i4")])
assert TRACE_DT.itemsize == 60
MISSING = []  # what a search of the generator did not find (asserted empty by the tests)


class Tables:
    def __init__(self, lib):
        self.multiple, self.alloc, self.sblimit = np.zeros(64), np.zeros((4, 32, 16, 4), np.uint16), np.zeros(4, np.int32)
        self.snr, self.qa, self.qb = np.zeros(18), np.zeros(17), np.zeros(17)
        lib.mp3o_l12_tables.argtypes = [ctypes.c_void_p] * 6
        lib.mp3o_l12_tables.restype = None
        lib.mp3o_l12_tables(*(a.ctypes.data for a in (self.multiple, self.alloc, self.sblimit, self.snr, self.qa, self.qb)))
        # Layer I's own, as its first frame leaves them (src/encode.c:900-905, 1226-1231)
        self.snr1 = np.concatenate([self.snr[[0, 1, 3]], self.snr[5:18]])
        self.qa1 = np.concatenate([self.qa[[0, 2]], self.qa[4:17]])
        self.qb1 = np.concatenate([self.qb[[0, 2]], self.qb[4:17]])

    def max_alloc(self, table, sb):
        return (1 << int(self.alloc[table, sb, 0, 1])) - 1

    def snr2(self, table, sb, ba):
        """the signal-to-noise ratio of allocation ba in Layer II"""
        return float(self.snr[int(self.alloc[table, sb, ba, 3]) + 1]) if ba else 0.0


def frame_bits_of(layer, rate, kbps):
    spf, slot = (384, 32) if layer == 1 else (1152, 8)
    return int((spf / (rate / 1000.0)) * (kbps / float(slot))) * slot  # src/musicin.c:561-567


def table_of(rate, kbps, C):
    per, sf = kbps // C, rate // 1000  # pick_table, src/common.c:291-318
    if (sf == 48 and per >= 56) or 56 <= per <= 80:
        return 0
    if sf != 48 and per >= 96:
        return 1
    if sf != 32 and per <= 48:
        return 2
    return 3


class Case:
    def __init__(self, set_, name, layer, rate, mode, kbps, sb, ratio, emu=False, **expect):
        self.set, self.layer, self.rate, self.mode, self.kbps, self.emu, self.expect = set_, layer, rate, mode, kbps, emu, expect
        self.name = "%s L%d %d %s %dk %s" % (set_, layer, rate, mode, kbps, name)
        self.C = 1 if mode[0] == "m" else 2
        self.parts = 1 if layer == 1 else 3
        self.sb = np.ascontiguousarray(sb, np.float64).reshape(self.C, self.parts, 12, 32)
        r = np.asarray(ratio, np.float32)
        if layer == 2 and r.shape == (self.C, 32):  # one value a band: Layer II keeps the larger of two passes; the other lies below
            hi = ((np.arange(32)[None, :] + np.arange(self.C)[:, None]) & 1).astype(bool)
            r = np.stack([np.where(hi, r - np.float32(3.0), r), np.where(hi, r, r - np.float32(3.0))])
        self.ratio = np.ascontiguousarray(r, np.float32).reshape(layer, self.C, 32)
        assert kbps in L12_BITRATES[layer] and np.all(np.abs(self.sb) <= 2.0) and np.all(np.isfinite(self.ratio)), self.name

    @property
    def key(self):
        return (self.layer, self.rate, self.mode)

    @property
    def table(self):
        return table_of(self.rate, self.kbps, self.C)

    def smr(self):
        """[C][32] what the allocation sees"""
        return self.ratio.max(axis=0).astype(np.float64)


class Result:
    def __init__(self, data, dump, trace=None):
        self.bytes, self.dump, self.trace = data, dump, trace


def by_key(cases):
    groups = {}
    for c in cases:
        groups.setdefault(c.key, []).append(c)
    return [groups[k] for k in sorted(groups)]


def _pack(cases):
    kbps = np.array([c.kbps for c in cases], np.int32)
    sb = np.ascontiguousarray(np.stack([c.sb for c in cases]))
    ratio = np.ascontiguousarray(np.stack([c.ratio for c in cases]))
    return kbps, sb, ratio


def run_oracle(lib, cases):
    """cases of one key -> [Result]"""
    lib.mp3o_l12_alloc_frames.argtypes = [ctypes.c_int] * 3 + [ctypes.c_char_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_size_t] + [ctypes.c_void_p] * 3
    c0, n = cases[0], len(cases)
    kbps, sb, ratio = _pack(cases)
    out, lens = np.zeros((n, 2048), np.uint8), np.zeros(n, np.uint32)
    dumps, trace = np.zeros(n, L12_DT), np.zeros(n, TRACE_DT)
    rc = lib.mp3o_l12_alloc_frames(c0.layer, c0.rate, c0.C, c0.mode.encode(), n, kbps.ctypes.data, sb.ctypes.data, ratio.ctypes.data,
                                   out.ctypes.data, 2048, lens.ctypes.data, dumps.ctypes.data, trace.ctypes.data)
    assert rc == 0, (rc, c0.name)
    return [Result(out[i, :lens[i]].tobytes(), dumps[i], trace[i]) for i in range(n)]


def hook_call(lib, layer, rate, C, mode, crc, flags, slot0, kbps, sb, ratio, nf, stride=OUT_STRIDE):
    """mp3mi_debug_l12_alloc as it is: kbps[S], sb[S][nf][C][parts][12][32], ratio[S][nf][passes][C][32] -> (rc, out, lens, seams)"""
    lib.mp3mi_debug_l12_alloc.argtypes = [ctypes.c_int] * 9 + [ctypes.c_void_p] * 4 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
    kbps, sb, ratio = np.ascontiguousarray(kbps, np.int32), np.ascontiguousarray(sb, np.float64), np.ascontiguousarray(ratio, np.float32)
    S = len(kbps)
    out, lens, seams = np.zeros((S, max(stride, 1)), np.uint8), np.zeros(S, np.uint32), np.zeros((S, max(nf, 1)), L12_SEAM_DT)
    rc = lib.mp3mi_debug_l12_alloc(layer, rate, C, mode, crc, flags, slot0, S, nf, kbps.ctypes.data, sb.ctypes.data, ratio.ctypes.data,
                                   out.ctypes.data, stride, lens.ctypes.data, seams.ctypes.data)
    return rc, out, lens, seams


def run_hook(lib, cases, slot0=0, nf=NF):
    """cases of one key as the streams of ONE launch, each case nf times -> (rc, [(bytes, seams[nf])])"""
    c0, S = cases[0], len(cases)
    kbps, sb, ratio = _pack(cases)
    sb, ratio = np.repeat(sb[:, None], nf, axis=1), np.repeat(ratio[:, None], nf, axis=1)
    flags = 8 * ("c" in c0.mode[1:]) + 4 * ("o" in c0.mode[1:])
    stride = max(OUT_STRIDE, (nf * 1728 + 1 + 255) // 256 * 256)
    rc, out, lens, seams = hook_call(lib, c0.layer, c0.rate, c0.C, L12_MODES[c0.mode[0]], int("e" in c0.mode[1:]), flags, slot0, kbps, sb, ratio, nf, stride)
    return rc, [(out[s, :lens[s]].tobytes(), seams[s]) for s in range(S)]


def run_reference(cases, workdir):
    """cases of one key through oracle/_ref/ref_harness_l12_alloc, one process -> [Result]"""
    c0 = cases[0]
    fin, mpg, fout = (os.path.join(workdir, n) for n in ("cases.bin", "out.mpg", "out.bin"))
    flags = 1 * ("e" in c0.mode[1:]) + 2 * ("c" in c0.mode[1:]) + 4 * ("o" in c0.mode[1:])
    with open(fin, "wb") as f:
        f.write(np.array([c0.layer, c0.rate, c0.C, L12_MODES[c0.mode[0]], flags, len(cases), 0, 0], np.int32).tobytes())
        for c in cases:
            f.write(np.array([c.kbps, 0], np.int32).tobytes() + c.sb.tobytes() + c.ratio.tobytes())
    r = subprocess.run([REF_HARNESS, fin, mpg, fout], capture_output=True, cwd=workdir)
    assert r.returncode == 0, (r.returncode, r.stderr[-300:], c0.name)
    rec = np.fromfile(fout, np.dtype([("bits", "<i4"), ("pad", "<i4"), ("dump", L12_DT)]))
    data, pos, res = open(mpg, "rb").read(), 0, []
    assert len(rec) == len(cases) and len(data) == sum(int(b) for b in rec["bits"]) // 8 + 1
    for i in range(len(cases)):
        assert rec["bits"][i] % 8 == 0
        res.append(Result(data[pos:pos + rec["bits"][i] // 8], rec["dump"][i]))
        pos += rec["bits"][i] // 8
    return res


def mismatch_dump(c, got, want):
    """a reference or oracle Result against another: bytes and every member of the stage dump"""
    if got.bytes != want.bytes:
        return "%s: bytes differ (%d / %d)" % (c.name, len(got.bytes), len(want.bytes))
    for name in ["sb"] + L12_SEAMS:
        if not np.array_equal(got.dump[name], want.dump[name]):
            return "%s: %s differs" % (c.name, name)
    return None


def mismatch_hook(c, got, want, nf=NF):
    """what the hook returned for a stream -- nf frames and the file's last byte -- against the oracle's Result"""
    data, seams = got
    if data != want.bytes * nf + b"\0":
        return "%s: bytes differ (%d, wanted %d x %d + 1)" % (c.name, len(data), nf, len(want.bytes))
    for f in range(nf):
        for name in L12_SEAMS:
            if not np.array_equal(seams[f][name], want.dump[name]):
                return "%s: frame %d, %s differs" % (c.name, f, name)
    return None


# ---------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------
def _ord(x):
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b if b >= 0 else -(b & 0x7fffffffffffffff)


def _unord(i):
    return struct.unpack("<d", struct.pack("<q", i if i >= 0 else (-i) | -0x8000000000000000))[0]


def quant(x, div, qa, qb, qn):
    """src/encode.c:1245-1262, 1296-1320 on one sample"""
    d = x / div
    d = d * qa + qb
    sig = d >= 0
    if not sig:
        d += 1.0
    q = int(d * float(1 << qn))
    return q | (1 << qn) if sig else q


def boundary(div, qa, qb, qn, target):
    """adjacent doubles lo < hi in [-div, div] with quant(lo) < target <= quant(hi) (quant rises with x)"""
    lo, hi = _ord(-div), _ord(div)
    assert quant(-div, div, qa, qb, qn) < target <= quant(div, div, qa, qb, qn)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if quant(_unord(mid), div, qa, qb, qn) >= target:
            hi = mid
        else:
            lo = mid
    return _unord(lo), _unord(hi)


def edge_samples(rng, div, qa, qb, qn, n):
    """n >= 12 samples of a band whose scalefactor is div: the quantiser's edges first, the rest random inside (-div, div)"""
    top = quant(div, div, qa, qb, qn)  # (d = +1)
    t1, t2 = int(rng.integers(1, 1 << qn)), int(rng.integers((1 << qn) + 1, top + 1)) if top > (1 << qn) else top
    s = [div, -div, 0.0, -0.0, 5e-324, -5e-324]
    for t in (1 << qn, t1, t2):  # the sign change, a boundary below it and one above
        s += list(boundary(div, qa, qb, qn, t))
    s += list(rng.uniform(-div, div, n - len(s)))
    return np.array(s[:n])


def loud_band(rng, peak, pos=None, sign=1.0, n=12):
    """n samples below peak / 2 and the peak itself at pos"""
    x = rng.uniform(-0.5, 0.5, n) * peak
    x[int(rng.integers(n)) if pos is None else pos] = sign * peak
    return x


def random_sb(rng, layer, C, T, lo=0, hi=40):
    """random samples with a scalefactor index in lo..hi per (channel, part, band)"""
    parts = 1 if layer == 1 else 3
    sb = np.zeros((C, parts, 12, 32))
    for ch in range(C):
        for i in range(32):
            base = int(rng.integers(lo, hi))
            for t in range(parts):
                j = min(62, max(0, base + int(rng.integers(-3, 4)) * int(rng.integers(0, 2))))
                sb[ch, t, :, i] = loud_band(rng, T.multiple[j] * rng.uniform(0.8, 1.0), sign=rng.choice([-1.0, 1.0]))
    return sb


def scale_values(T):
    v = []
    for j in range(63):
        m = float(T.multiple[j])
        v += [np.nextafter(m, 0.0), m] + ([np.nextafter(m, 4.0)] if j else [])
    return v + [0.0]


def index_of(T, v):
    """the scalefactor just above the peak v (src/encode.c:529-534)"""
    for j in range(62, -1, -1):
        if v <= T.multiple[j]:
            return j
    return 0


# ---------------------------------------------------------------------------------------------------------------------
# the sets
# ---------------------------------------------------------------------------------------------------------------------
def set_a1(T):
    out, vals = [], scale_values(T)
    rng = np.random.default_rng(101)
    for layer, rate, kbps, nb in ((1, 44100, 448, 32), (2, 32000, 384, 30)):
        parts = 1 if layer == 1 else 3
        per = 2 * parts * nb
        for mode, kb in (("s", kbps), ("j", 128 if layer == 1 else 192)):
            per = (2 if mode == "s" else 1) * parts * nb
            for k in range((len(vals) + per - 1) // per):
                sb, want = np.zeros((2, parts, 12, 32)), np.full((2, 3, 32), -1)
                for n in range(min(per, len(vals) - k * per)):
                    idx = k * per + n
                    x = loud_band(rng, vals[idx], pos=idx % 12, sign=-1.0 if (idx // 12) & 1 else 1.0)
                    if mode == "s":
                        ch, t, i = n % 2, (n // 2) % parts, n // (2 * parts)
                        sb[ch, t, :, i] = x
                    else:
                        ch, t, i = 0, n % parts, n // parts
                        sb[:, t, :, i] = x  # L = R: the mean is the value
                    want[ch, t, i] = index_of(T, vals[idx])
                out.append(Case("A1", "peaks %d" % k, layer, rate, mode, kb, sb, np.full((2, 32), 15.0), emu=k == 0,
                                peaks=want if layer == 1 or mode == "j" else None))
        # L = -R: the mean is exactly 0; L = m + e, R = m - e: exactly m
        sb = random_sb(rng, layer, 2, T)
        sb[1] = -sb[0]
        out.append(Case("A1", "L = -R", layer, rate, "j", 128 if layer == 1 else 192, sb, np.full((2, 32), 15.0), emu=True, j_all=62))
        for k in range((63 + nb * parts - 1) // (nb * parts)):
            sb, want = np.zeros((2, parts, 12, 32)), np.full((3, 32), -1)
            for n in range(min(nb * parts, 63 - k * nb * parts)):
                j = k * nb * parts + n
                t, i = n % parts, n // parts
                m = float(T.multiple[j])
                e = 2.0 ** (np.frexp(m)[1] - 11)
                if 0.5 * ((m + e) + (m - e)) != m or m + e > 2.0:  # (2.0 + e is outside the domain, and next to a power of two m + e rounds)
                    e = 0.0
                x = loud_band(rng, m, pos=j % 12)
                sb[0, t, :, i], sb[1, t, :, i] = x, x
                sb[0, t, j % 12, i], sb[1, t, j % 12, i] = m + e, m - e
                want[t, i] = j
            out.append(Case("A1", "mean on the table %d" % k, layer, rate, "j", 128 if layer == 1 else 192, sb, np.full((2, 32), 15.0),
                            emu=k == 0, j_peaks=want))
    return out


def set_a2(T):
    out = []
    rng = np.random.default_rng(202)
    pairs = [(d0, d1) for d0 in range(-3, 4) for d1 in range(-3, 4)]
    for where in ("middle", "bottom", "top"):
        sb, pre = np.zeros((2, 3, 12, 32)), np.full((2, 3, 32), -1)
        for lane in range(60):
            d0, d1 = pairs[lane] if lane < 49 else pairs[int(rng.integers(49))]
            rel = np.array([0, -d0, -d0 - d1])  # scalar[1] = scalar[0] - d0, scalar[2] = scalar[1] - d1
            s = rel + {"middle": 30, "bottom": -rel.min(), "top": 62 - rel.max()}[where]
            i, ch = lane // 2, lane % 2
            for t in range(3):
                sb[ch, t, :, i] = loud_band(rng, T.multiple[s[t]] * 0.9, sign=rng.choice([-1.0, 1.0]))
            pre[ch, :, i] = s
        ratio = rng.uniform(5, 30, (2, 32)).astype(np.float32)
        out.append(Case("A2", where, 2, 32000, "s", 384, sb, ratio, emu=where == "middle", pre=pre))
        out.append(Case("A2", where, 2, 44100, "j", 192, sb, ratio + np.float32(10), emu=where == "top", pre=pre))
    return out


def _pin1(T, r0, k):
    """Layer I: the ratio of a band that ends with allocation k when band (0, 0), of ratio r0, ends full"""
    if k >= 14:
        return r0
    lim = (-r0 + T.snr1[14]) + 1
    return np.float32(0.5 * (T.snr1[k - 1] + T.snr1[k]) - lim) if k else np.float32(-lim - 50)


def _pin2(T, table, sb, k):
    """Layer II: the ratio of a band that ends with allocation k, given the room"""
    if k == 0:
        return np.float32(NEVER)
    top = T.max_alloc(table, sb)
    return np.float32(-999999.0 + (T.snr2(table, sb, k - 1) + 2.0 if k == top else 0.5 * (T.snr2(table, sb, k - 1) + T.snr2(table, sb, k))))


def set_a3(T):
    out = []
    rng = np.random.default_rng(303)
    for n, sf0 in enumerate((0, 1, 2, 29, 48, 61)):  # Layer I: band b of channel 0 ends with allocation b, of channel 1 with 15 - b
        for mode in ("m", "s"):
            C = 1 if mode == "m" else 2
            sb, ratio, want = np.zeros((C, 1, 12, 32)), np.full((C, 32), -1000.0, np.float32), np.zeros((2, 32), int)
            for ch in range(C):
                for b in range(15):
                    k = 14 if b == 0 else (b if ch == 0 else 15 - b)
                    sf = min(62, sf0 + (b % 2) * (b + ch))
                    sb[ch, 0, :, b] = rng.permutation(edge_samples(rng, float(T.multiple[sf]), float(T.qa1[k - 1]), float(T.qb1[k - 1]), k, 12))
                    ratio[ch, b] = _pin1(T, np.float32(20.0), k)
                    want[ch, b] = k
            out.append(Case("A3", "allocations 1..14, sf %d" % sf0, 1, 44100, mode, 448, sb, ratio, emu=n == 1, alloc=want))
    for rate, kbps in ((48000, 384), (32000, 384), (44100, 96), (32000, 96)):  # Layer II: every cell of the table, packed into frames
        table = table_of(rate, kbps, 2)
        nb = int(T.sblimit[table])
        lanes = [(ch, i) for i in range(nb) for ch in range(2)]
        nxt = {l: 1 for l in lanes}
        room0 = frame_bits_of(2, rate, kbps) - 32 - 2 * sum(int(T.alloc[table, i, 0, 1]) for i in range(nb))
        n = 0
        while any(nxt[l] <= T.max_alloc(table, l[1]) for l in lanes):
            room, sb, ratio, want = room0, np.zeros((2, 3, 12, 32)), np.full((2, 32), NEVER, np.float32), np.zeros((2, 32), int)
            for l in lanes[n % len(lanes):] + lanes[:n % len(lanes)]:
                ch, i = l
                k = nxt[l]
                if k > T.max_alloc(table, i):
                    continue
                steps, bits, grp, qnt = (int(v) for v in T.alloc[table, i, k])
                cost = 12 * grp * bits + 8
                if cost > room:
                    continue
                room -= cost
                nxt[l] = k + 1
                qn = (steps - 1).bit_length() - 1  # while ((1L << n) < steps) n++; n--;
                sf = (3 * i + k + n) % 63
                div, qa, qb = float(T.multiple[sf]), float(T.qa[qnt]), float(T.qb[qnt])
                x = edge_samples(rng, div, qa, qb, qn, 36)
                below = np.nextafter(div, 0.0)
                x[12:21] = [below] * 3 + [div] * 3 + [-div] * 3  # triples all at steps - 1, at d = +1 and at d = -1
                x[:12], x[21:] = rng.permutation(x[:12]), rng.permutation(x[21:])
                x[24] = -div  # (every part has the peak: one scalefactor, scfsi 2)
                sb[ch, :, :, i] = x.reshape(3, 12)
                ratio[ch, i] = _pin2(T, table, i, k)
                want[ch, i] = k
            out.append(Case("A3", "table %d frame %d" % (table, n), 2, rate, "s", kbps, sb, ratio, emu=n in (0, 7), alloc=want))
            n += 1
    return out


_WANTED, _SEEN = set(), set()  # (set, layer, name) the searches were asked for, and found in at least one format


def _searched(lib, cands, wanted):
    """run the candidates through the oracle; for every (name, predicate on the result) keep the first that satisfies it.  A format
    need not have every one of them (a residue may rule it out); a layer must: MISSING says which it has not"""
    res = []
    for g in by_key(cands):
        res += list(zip(g, run_oracle(lib, g)))
    keep = []
    for name, pred in wanted:
        hit = [c for c, r in res if pred(r)]
        _WANTED.add((cands[0].set, cands[0].layer, name))
        if not hit:
            continue
        c = hit[0]
        _SEEN.add((c.set, c.layer, name))
        c.name += " [" + name + "]"
        c.expect["found"] = c.expect.get("found", ()) + (name,)
        if c not in keep:
            keep.append(c)
    return keep


def set_a4(T, lib):
    out = []
    rng = np.random.default_rng(404)
    formats = ((1, 44100, "m"), (1, 44100, "s"), (1, 48000, "d"), (2, 44100, "m"), (2, 48000, "s"), (2, 32000, "d"))
    for layer, rate, mode in formats:
        C = 1 if mode == "m" else 2
        rates = L12_BITRATES[layer]
        for kbps in (rates[1], rates[6], rates[13]):  # equal ratios everywhere
            out.append(Case("A4", "equal ratios", layer, rate, mode, kbps, random_sb(rng, layer, C, T), np.full((C, 32), 20.0), emu=kbps == rates[6]))
        for kbps in (rates[3], rates[10]):  # neighbouring floats: every key in one upper half
            r = np.float32(20.0) + np.arange(32 * C, dtype=np.float32) * np.spacing(np.float32(20.0))
            out.append(Case("A4", "neighbouring floats", layer, rate, mode, kbps, random_sb(rng, layer, C, T), rng.permutation(r).reshape(C, 32),
                            emu=kbps == rates[3]))
        sbs = [random_sb(rng, layer, C, T) for _ in range(8)]
        cands = [Case("A4", "random %d" % n, layer, rate, mode, rates[int(rng.integers(14))], sbs[n % 8],
                      rng.uniform(-10, 40, (C, 32)).astype(np.float32)) for n in range(240)]
        wanted = [("a step that uses all that is left", lambda r: r.trace["min_slack"] == 0),
                  ("a step 2 bits short", lambda r: r.trace["min_short"] == 2),
                  ("closed while cheaper steps fit", lambda r: r.trace["granted_after_close"] > 0),
                  ("what is left equal to an open step", lambda r: r.trace["exact_after_close"] > 0),
                  ("what is left 2 bits below a step", lambda r: r.trace["min_short_after_close"] == 2)]
        found = _searched(lib, cands, wanted)
        for c in found[:2]:
            c.emu = True
        out += found + [c for c in cands[:3] if c not in found]
        sb = random_sb(rng, layer, C, T, 0, 6)  # loud everywhere, at and above sblimit too
        out.append(Case("A4", "loud above sblimit", layer, rate, mode, rates[8], sb, np.full((C, 32), 90.0), emu=True, nothing_above_sblimit=True))
    # Layer I: small starts at mnr[0][0] + 1.  Band 5 on it and just below (a ratio one float up), with band (0, 0) ...
    up = lambda v: np.nextafter(np.float32(v), np.float32(1e9))
    for mode in ("m", "s"):
        C = 1 if mode == "m" else 2
        for below in (False, True):
            # ... open: band 5 at mnr[0][0] + 1 from the start (nothing rides on it: band (0, 0) itself is smaller and goes first)
            r = np.full((C, 32), -1000.0, np.float32)
            r[0, 0], r[0, 5] = 10.0, up(9.0) if below else 9.0
            out.append(Case("A4", "start rule, (0,0) open%s" % (", below" if below else ""), 1, 44100, mode, 64, random_sb(rng, 1, C, T), r,
                            emu=True, alloc_at=((0, 5), None)))
            # ... full: 74.01 - 1 == (92.01 - 20) + 1 exactly, so band 5 stops at allocation 11 -- and takes one more from just below
            r = np.full((C, 32), -1000.0, np.float32)
            r[0, 0], r[0, 5] = 20.0, up(1.0) if below else 1.0
            assert (T.snr1[11] - 1.0) == (-20.0 + T.snr1[14]) + 1
            out.append(Case("A4", "start rule, (0,0) full%s" % (", below" if below else ""), 1, 44100, mode, 448, random_sb(rng, 1, C, T), r,
                            emu=True, alloc_at=((0, 5), 12 if below else 11), alloc0=14))
        for below in (False, True):
            # ... closed for lack of room at allocation 0 (mono, -e, 80 bits): bands 5 and 9 take a first step each (60), band (0, 0)'s
            # own (30) does not fit into 20, and 7 - 6 == 0 + 1: band 5 stays at 1 -- or takes 12 of the 20 from just below
            if mode != "m":
                continue
            r = np.full((1, 32), -1000.0, np.float32)
            r[0, 0], r[0, 5], r[0, 9] = 0.0, up(6.0) if below else 6.0, 5.0
            for rate in (44100, 48000):
                out.append(Case("A4", "start rule, (0,0) closed%s" % (", below" if below else ""), 1, rate, "me", 32, random_sb(rng, 1, 1, T), r,
                                emu=True, alloc_at=((0, 5), 2 if below else 1), alloc0=0))
    # a round's edge: band 9 waits at mnr 17, exactly where band 3's first step takes band 3 (10 + 7) -- the key that equals T -- or one
    # float above it -- inside T's upper half.  The reference gives band 3 both its steps first (the earlier of equals) and band 9's
    # first no longer fits: 224 bits, 162 of them gone to bands 2, 4 and 6 (three steps each, then out of reach of band (0, 0)'s
    # 17.5 + 1), 62 left for 30 + 12 + 30
    for above in (False, True):
        r = np.full((1, 32), -1000.0, np.float32)
        r[0, 0], r[0, 3], r[0, 9] = -17.5, -10.0, np.nextafter(np.float32(-17.0), np.float32(-1e9)) if above else -17.0
        r[0, [2, 4, 6]] = 6.5
        want = np.zeros((2, 32), int)
        want[0, [2, 4, 6]], want[0, 3] = 3, 2
        out.append(Case("A4", "a round's edge%s" % (", one float above" if above else ""), 1, 32000, "m", 32, random_sb(rng, 1, 1, T), r, emu=True, alloc=want))
    # Layer II: small starts at 999999.0
    for mode, rate, kbps in (("m", 44100, 192), ("s", 48000, 256)):
        C = 1 if mode == "m" else 2
        for below in (False, True):
            r = np.full((C, 32), NEVER, np.float32)  # (the band is the last to be looked at: nothing else may want the room)
            table = table_of(rate, kbps, C)
            r[0, 1], r[C - 1, 6] = _pin2(T, table, 1, 4), _pin2(T, table, 6, 2)
            r[0, 3] = np.nextafter(np.float32(-999999.0), np.float32(0)) if below else -999999.0
            out.append(Case("A4", "999999%s" % (", below" if below else ""), 2, rate, mode, kbps, random_sb(rng, 2, C, T), r, emu=True,
                            alloc_at=((0, 3), 1 if below else 0), alloc0=0))
    return out


def set_a5(T, lib):
    out = []
    rng = np.random.default_rng(505)
    for layer, rate, kbps_list in ((1, 44100, (128, 256)), (2, 44100, (128, 192)), (2, 48000, (128, 192)), (2, 32000, (96,)), (2, 44100, (64,))):
        for kbps in kbps_list:
            fb = frame_bits_of(layer, rate, kbps)
            for crc in ("", "e"):
                wanted = [("mode_ext %d" % m, (lambda m: lambda r: r.dump["mode"] == 1 and r.dump["mode_ext"] == m and r.trace["rq"][r.trace["n_rq"] - 1] <= fb)(m)) for m in range(4)]
                wanted += [("plain stereo", lambda r: r.dump["mode"] == 0), ("mode_ext 0 still over", lambda r: r.trace["n_rq"] == 5 and r.trace["rq"][4] > fb),
                           ("rq on the frame", lambda r: any(r.trace["rq"][k] == fb for k in range(r.trace["n_rq"]))),
                           ("rq 2 above", lambda r: any(r.trace["rq"][k] == fb + 2 for k in range(r.trace["n_rq"])))]
                odd = layer == 2 and table_of(rate, kbps, 2) < 2
                if odd:
                    wanted += [("rq 1 above", lambda r: any(r.trace["rq"][k] == fb + 1 for k in range(r.trace["n_rq"]))),
                               ("a step 1 bit short", lambda r: r.trace["min_short"] == 1),
                               ("what is left 1 bit below a step", lambda r: r.trace["min_short_after_close"] == 1)]
                cands = []
                for seed in range(6):
                    base, sb = rng.uniform(-15, 25, (2, 32)), random_sb(rng, layer, 2, T)
                    if seed % 3 == 0:
                        base[1] = base[0]  # ties between the channels
                    for off in np.arange(-30.0, 50.0, 0.5):
                        cands.append(Case("A5", "sweep %d %+.1f" % (seed, off), layer, rate, "j" + crc, kbps, sb, (base + off).astype(np.float32)))
                found = _searched(lib, cands, wanted)
                for c in found[:1] + [c for c in found if "rq on the frame" in c.expect["found"]]:
                    c.emu = True
                out += found
    # two-channel Layer I at 32 kbit/s: header and allocation fields alone pass the frame's 256 bits at 44.1 and 48 kHz
    for rate in (44100, 48000):
        for mode in ("s", "d", "j"):
            for crc in ("", "e"):
                out.append(Case("A5", "the frame outgrows its slot", 1, rate, mode + crc, 32, random_sb(rng, 1, 2, T), rng.uniform(0, 40, (2, 32)),
                                emu=True, frame_len=None if mode == "j" else (38 if crc else 36)))
    return out


def set_a6(T):
    out = []
    rng = np.random.default_rng(606)
    for layer in (1, 2):
        rates = L12_BITRATES[layer]
        for mode in "sjdm":
            C = 1 if mode == "m" else 2
            for f in range(8):
                flags = "".join(ch for b, ch in enumerate("eco") if (f >> b) & 1)
                for kbps in (rates[4 + f % 3], rates[9 + f % 4]):
                    out.append(Case("A6", "header", layer, (44100, 48000, 32000)[f % 3], mode + flags, kbps, random_sb(rng, layer, C, T),
                                    rng.uniform(-5, 35, (C, 32)), emu=kbps == rates[4 + f % 3] and f in (1, 6)))
    # an allocation that differs in ONE bit (band 2: 2 / 3, 6 / 7), everything else pinned: the CRC must differ
    for pair, (ka, kb) in enumerate(((2, 3), (6, 7))):
        for k in (ka, kb):
            sb, r = random_sb(rng, 1, 1, T), np.full((1, 32), -1000.0, np.float32)
            want = np.zeros((2, 32), int)
            for b, kk in ((0, 14), (1, 5), (2, k), (3, 9)):
                r[0, b], want[0, b] = _pin1(T, np.float32(20.0), kk), kk
            out.append(Case("A6", "one bit of the allocation", 1, 44100, "me", 448, sb, r, emu=True, alloc=want, crc_pair=(1, pair)))
            sb, r = random_sb(rng, 2, 1, T), np.full((1, 32), NEVER, np.float32)
            want = np.zeros((2, 32), int)
            for b, kk in ((0, 4), (1, 5), (2, k), (3, 1)):
                r[0, b], want[0, b] = _pin2(T, 1, b, kk), kk
            out.append(Case("A6", "one bit of the allocation", 2, 32000, "me", 384, sb, r, emu=True, alloc=want, crc_pair=(2, pair)))
    return out


_CACHE = {}
COUNTS = {"A1": 19, "A2": 6, "A3": 85, "A4": 87, "A5": 119, "A6": 136}


def cases(lib):
    """every case of every set, in a fixed order (generated once a process)"""
    if "all" not in _CACHE:
        T = Tables(lib)
        _CACHE["all"] = set_a1(T) + set_a2(T) + set_a3(T) + set_a4(T, lib) + set_a5(T, lib) + set_a6(T)
        _CACHE["T"] = T
        MISSING.extend("%s Layer %d: %s" % k for k in sorted(_WANTED - _SEEN))
    return _CACHE["all"]


def tables(lib):
    cases(lib)
    return _CACHE["T"]


# ---------------------------------------------------------------------------------------------------------------------
# what the oracle's outputs must show
# ---------------------------------------------------------------------------------------------------------------------
def check_expectations(c, r):
    """None, or what the oracle's result for c lacks of what c was built for"""
    e, d = c.expect, r.dump
    if e.get("peaks") is not None and c.layer == 1 and c.mode[0] == "s":
        w = e["peaks"]
        if not np.array_equal(d["scalar"][w >= 0], w[w >= 0]):
            return c.name + ": a scale index is not the peak's"
    if e.get("peaks") is not None and c.mode[0] == "j":  # L = R: the mean's index is the value's
        w = e["peaks"].max(axis=0)
        if not np.array_equal(d["j_scale"][w >= 0], w[w >= 0]):
            return c.name + ": a joint scale index is not the value's"
    if "j_all" in e and not np.all(d["j_scale"][:c.parts, :d["sblimit"]] == e["j_all"]):
        return c.name + ": the mean of L and -L is not 0"
    if "j_peaks" in e and not np.array_equal(d["j_scale"][e["j_peaks"] >= 0], e["j_peaks"][e["j_peaks"] >= 0]):
        return c.name + ": a joint scale index is not the mean's"
    if "alloc" in e and not np.array_equal(d["bit_alloc"], e["alloc"]):
        return c.name + ": the pinned allocation was not reached"
    if "alloc_at" in e and e["alloc_at"][1] is not None and d["bit_alloc"][e["alloc_at"][0]] != e["alloc_at"][1]:
        return c.name + ": allocation %d, built for %d" % (d["bit_alloc"][e["alloc_at"][0]], e["alloc_at"][1])
    if "alloc0" in e and d["bit_alloc"][0, 0] != e["alloc0"]:
        return c.name + ": band (0, 0) at %d, built for %d" % (d["bit_alloc"][0, 0], e["alloc0"])
    if e.get("nothing_above_sblimit") and np.any(d["bit_alloc"][:, d["sblimit"]:]):
        return c.name + ": bits above sblimit"
    if e.get("frame_len") is not None and len(r.bytes) != e["frame_len"]:
        return c.name + ": frame of %d bytes" % len(r.bytes)
    return None


def pattern_class(d):
    return 0 if d <= -3 else 1 if d < 0 else 2 if d == 0 else 3 if d < 3 else 4


def reached(pairs, T):
    """pairs: [(case, oracle Result)] -> what the sets reached between them"""
    got = {"scalar": set(), "j_scale": set(), "classes": set(), "p444": set(), "scfsi": set(), "scalar_ends": set(), "alloc1": set(), "cells": set(),
           "found": set(), "mode_ext": set(), "joint_scfsi_differs": 0, "joint_ties": 0, "joint_ratios_differ": 0, "overlong": set(),
           "modes_flags": set(), "crc_pairs": 0, "start_rule": set(), "l2_start": set(), "peak_pos": set()}
    crc_of = {}
    for c, r in pairs:
        d, e = r.dump, c.expect
        if c.set == "A1":
            got["scalar"] |= set(int(v) for v in d["scalar"][:c.C, :c.parts, :d["sblimit"]].ravel())
            got["j_scale"] |= set(int(v) for v in d["j_scale"][:c.parts, :d["sblimit"]].ravel())
            peak = np.abs(c.sb).argmax(axis=2)
            got["peak_pos"] |= set((int(p), bool(c.sb[ch, t, p, i] < 0)) for ch in range(c.C) for t in range(c.parts) for i in range(32)
                                   for p in [peak[ch, t, i]] if c.sb[ch, t, p, i] != 0)
        if "pre" in e:
            pre = e["pre"]
            for ch in range(2):
                for i in range(d["sblimit"]):
                    s = pre[ch, :, i]
                    if s[0] < 0:
                        continue
                    cl = (pattern_class(s[0] - s[1]), pattern_class(s[1] - s[2]))
                    got["classes"].add(cl)
                    if cl in ((1, 3),):
                        got["p444"].add(bool(s[0] > s[2]))
                    got["scalar_ends"] |= {int(s.min()), int(s.max())} & {0, 62}
            got["scfsi"] |= set(int(v) for v in d["scfsi"][:, :d["sblimit"]].ravel())
        if c.set == "A3":
            for ch in range(c.C):
                for i in range(32):
                    k = int(d["bit_alloc"][ch, i])
                    if k and c.layer == 1:
                        got["alloc1"].add(k)
                    elif k:
                        got["cells"].add((c.table, ch, i, k))
        got["found"] |= set((c.set, c.layer, n) for n in e.get("found", ()))
        if c.set == "A4" and "alloc_at" in e:
            (got["start_rule"] if c.layer == 1 else got["l2_start"]).add((int(d["bit_alloc"][0, 0]), int(d["bit_alloc"][e["alloc_at"][0]])))
        if c.set == "A5" and d["mode"] == 1:
            got["mode_ext"].add((c.layer, int(d["mode_ext"])))
            for i in range(d["jsbound"], d["sblimit"]):
                if d["bit_alloc"][0, i]:
                    got["joint_scfsi_differs"] += int(d["scfsi"][0, i] != d["scfsi"][1, i])
                    got["joint_ties"] += int(d["ltmin"][0, i] == d["ltmin"][1, i])
                    got["joint_ratios_differ"] += int(d["ltmin"][0, i] != d["ltmin"][1, i])
        if e.get("frame_len") is not None or (c.set == "A5" and c.kbps == 32 and c.layer == 1):
            got["overlong"].add((c.rate, c.mode, len(r.bytes)))
        if c.set == "A6" and "crc_pair" not in e:
            got["modes_flags"].add((c.layer, c.mode[0], "".join(sorted(c.mode[1:]))))
        if "crc_pair" in e:
            other = crc_of.get(e["crc_pair"])
            if other is None:
                crc_of[e["crc_pair"]] = (d["bit_alloc"].copy(), int(d["crc"]))
            else:
                diff = other[0] ^ d["bit_alloc"]
                got["crc_pairs"] += int(np.count_nonzero(diff) == 1 and bin(int(diff.max())).count("1") == 1 and other[1] != int(d["crc"]))
    return got


def assert_reached(got, T):
    """what every run of all cases must show (the CPU and the GPU test both call it)"""
    assert MISSING == [], MISSING  # (every search of the generator found its case: none of the named cases is silently absent)
    assert got["scalar"] >= set(range(63)) and got["j_scale"] >= set(range(63))
    assert got["peak_pos"] == {(p, s) for p in range(12) for s in (False, True)}
    assert got["classes"] == {(a, b) for a in range(5) for b in range(5)} and got["p444"] == {False, True}
    assert got["scfsi"] == {0, 1, 2, 3} and got["scalar_ends"] == {0, 62}
    assert got["alloc1"] == set(range(1, 15))
    cells = {(t, ch, i, k) for t in range(4) for ch in range(2) for i in range(int(T.sblimit[t])) for k in range(1, T.max_alloc(t, i) + 1)}
    assert got["cells"] == cells, (len(got["cells"]), len(cells))
    for layer in (1, 2):
        for name in ("a step that uses all that is left", "a step 2 bits short", "closed while cheaper steps fit", "what is left equal to an open step",
                     "what is left 2 bits below a step"):
            assert ("A4", layer, name) in got["found"], (layer, name)
        for name in ["mode_ext %d" % m for m in range(4)] + ["plain stereo", "mode_ext 0 still over", "rq on the frame", "rq 2 above"]:
            assert ("A5", layer, name) in got["found"], (layer, name)
    for name in ("rq 1 above", "a step 1 bit short", "what is left 1 bit below a step"):
        assert ("A5", 2, name) in got["found"], name
    assert got["mode_ext"] == {(l, m) for l in (1, 2) for m in range(4)}
    assert got["joint_scfsi_differs"] and got["joint_ties"] and got["joint_ratios_differ"]
    assert {(r, m, n) for r, m, n in got["overlong"] if m[0] != "j"} == {(r, m + e, 36 + 2 * bool(e)) for r in (44100, 48000) for m in "sd" for e in ("", "e")}
    assert len({(r, m) for r, m, n in got["overlong"] if m[0] == "j"}) == 4
    assert got["modes_flags"] == {(l, m, "".join(sorted(f))) for l in (1, 2) for m in "sjdm" for f in ("", "e", "c", "o", "ec", "eo", "co", "eco")}
    assert got["crc_pairs"] == 4
    # the start rules: band (0, 0) open / full / closed x the other band on the limit / below it, as (allocation of (0, 0), of the band)
    assert {(14, 11), (14, 12), (0, 1), (0, 2)} <= got["start_rule"] and got["l2_start"] == {(0, 0), (0, 1)}
