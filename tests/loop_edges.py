"""Chains of frames built to sit on the decisions of k_loop's SEARCH (csrc/k_loop.hip, loop_stream: everything around the
quantise+count pass that tests/quant_edges.py pins), and the three implementations that take them: the product's self-test hook
mp3mi_debug_iteration_loop (csrc/loop_debug.cpp: the device, or the emulated CPU build), the oracle's mp3o_iteration_loop, which
also says what the search reached (its trace), and the unmodified reference's iteration_loop (oracle/_ref/ref_harness_loop, a
process per chain, fresh-start chains only).  Everything is generated here, deterministically, the crafted values by search
with the oracle; nothing is read from files.

A chain is a format (rate, channels, kbps, crc), an optional initial loop state and N <= 6 frames of records: per (granule,
channel) 576 xr, pe, ratio_l[21], ratio_s[12][3] and a block type.  The sets:
  L1  a band's noise on its allowed distortion: the ratio of one band (each of the 21 long ones, 12 of the 36 short lanes), or of
      all at once, set so that xmin lands 0, +-1, +-2, +-4 ulps and +-5e-13, +-2e-12 relative from the noise xfsf the oracle's
      first pass found -- inside and outside loop_noise_close's 1e-12 --, in iteration 1, in iteration 2 (the bands whose noise
      grew from iteration 1 to 2, so that they did not violate before) and against the threshold BEHIND pre-emphasis'
      multiplication (sfb 11..20, the bands it moves); bands with xmin == 0 and bands without energy beside them
  L2  scalefactor limits: ratios 0 (a band that always violates) and ratios found by bisection that let a band be amplified n
      times, on bands either side of the split (sfb 11, lane 18): the two maxima on every cell of the (bit length <= 4, bit
      length <= 3) table, 15 / 16 and 7 / 8, the three ways out of the distortion loop
  L3  pre-emphasis: all four of sfb 17..20 violating against each three of four, block types 0, 1, 3 (fire) and 2 (never), and a
      granule 1 that shares scalefactors (scfsi) and inherits granule 0's preflag, set and clear
  L4  scfsi: pairs of spectra whose stored integer log-energies differ by 9 / 10 per group and 99 / 100 in all, likewise the
      stored log-xmin, every mask, short blocks and silence in either place, mono chains (whose second column only an initial
      state fills), several frames (stale values behind short blocks), granule 1 amplifying beside shared groups
  L5  budgets: every bitrate x channels x crc; pe putting more_bits on 100 / 101 and pe * 3.1 - mean_bits one ulp either side of
      101; the reservoir at 0, 0.8 ResvMax +- 8 and ResvMax (initial state; leading silent frames for the reference); the
      4095 clamp; ResvMax == 0; stuffing that puts part2_3_length[0][0] on 4094 / 4095, spills and drains
  L6  bisection and inner loop: spectra scaled until a probe counts exactly max_bits; short blocks at 32 kbit/s stereo whose
      scalefactors alone exceed the budget (the reference dies in inner_loop)
  L7  start step: one line at either end of the domain, tiny lines with global_gain on 255 / 256 (the reference dies on 256), a
      flat spectrum, the -100 clamp, 8 ln sfm on a rounding boundary of nint (k_prep's list), -0.0, silence between sound
  L8  Laplacian spectra, log-uniform ratios, all block types, random pe, every format, 6 frames
mean_bits is even for every format ((8 n - 288) / 2 and its like), so ResvFrameEnd's odd-mean_bits bit cannot be reached."""
import ctypes
import math
import os
import subprocess

import numpy as np

from mp3common import PSY_DT, SIDE_DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_HARNESS_LOOP = os.path.join(ROOT, "oracle", "_ref", "ref_harness_loop")
RATES = (44100, 48000, 32000)
BITRATES = (32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320)
SFB_L = {44100: [0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 90, 110, 134, 162, 196, 238, 288, 342, 418, 576],
         48000: [0, 4, 8, 12, 16, 20, 24, 30, 36, 42, 50, 60, 72, 88, 106, 128, 156, 190, 230, 276, 330, 384, 576],
         32000: [0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 54, 66, 82, 102, 126, 156, 194, 240, 296, 364, 448, 550, 576]}
SFB_S = {44100: [0, 4, 8, 12, 16, 22, 30, 40, 52, 66, 84, 106, 136, 192],
         48000: [0, 4, 8, 12, 16, 22, 28, 38, 50, 64, 80, 100, 126, 192],
         32000: [0, 4, 8, 12, 16, 22, 30, 42, 58, 78, 104, 138, 180, 192]}
PRETAB = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 3, 2]
SCFSI_BAND = (0, 6, 11, 16, 21)
GLOBAL_GAIN, HUFF_BITS = 1, 2  # MP3MI_STREAM_ABORT_* / MP3O_ABORT_*
EXIT_NO_OVER, EXIT_LOOP_BREAK, EXIT_SCALE_BITCOUNT = 1, 2, 3
XR_MAX, XR_MIN, STEP_MAX = 2.0 ** 64, 2.0 ** -500, 400  # the hook's domain (csrc/loop_debug.cpp)
BIG = 1e12  # a ratio no band's noise reaches: the band never violates

# mp3mi_loop_state (csrc/mp3mi_host.h) as the hook and the oracle exchange it, and the oracle's trace (oracle/mp3_oracle.h)
STATE_DT = np.dtype([("ResvSize", "<i4"), ("sc_en_tot", "<i4", (2, 2)), ("sc_en", "<i4", (2, 2, 21)), ("sc_xm", "<i4", (2, 2, 21)),
                     ("sc_xrmax", "<i4", (2, 2)), ("addr", "<i4", (2, 2, 3)), ("status", "<i4")])
TRACE_DT = np.dtype([("q0", "<i4"), ("q_final", "<i4"), ("n_outer", "<i4"), ("n_passes", "<i4"), ("n_probes", "<i4"), ("exit_how", "<i4"),
                     ("pre_iter", "<i4"), ("scfsi_mask", "<i4"), ("max_bits", "<i4"), ("more_bits", "<i4"), ("add_bits", "<i4"),
                     ("add_branch", "<i4"), ("bisect_equal", "<i4"), ("kept_iter", "<i4"), ("part2_3_length", "<i4"), ("resv_before", "<i4"),
                     ("probe_last", "<i4"), ("probe_prev", "<i4"), ("xfsf", "<f8", (36,)), ("xmin", "<f8", (36,)),
                     ("xmin_pre", "<f8", (36,)), ("closest", "<f8")])
assert STATE_DT.itemsize == 4 * 190 and TRACE_DT.itemsize == 72 + 8 * 109 and PSY_DT.itemsize == 472


def frame_bits_of(rate, kbps):
    return 8 * int((1152 / (rate / 1000.0)) * (kbps / 8.0))  # src/musicin.c:561-567


def mean_bits_of(rate, C, kbps, crc):
    return (frame_bits_of(rate, kbps) - (32 + (136 if C == 1 else 256) + 16 * crc)) // 2  # src/musicin.c:728-746


def resv_max_of(rate, kbps):
    b = frame_bits_of(rate, kbps)
    return 0 if b > 7680 else min(7680 - b, 4088)  # src/reservoir.c:81-92


class Chain:
    def __init__(self, set_, name, rate, C=1, kbps=128, crc=0, state=None, **expect):
        self.set, self.name, self.rate, self.channels, self.kbps, self.crc = set_, "%s %d %s" % (set_, rate, name), rate, C, kbps, crc
        self.state = state  # None (a fresh stream: what the reference can run), or a STATE_DT record
        self.expect = expect  # what the oracle's trace must show (tests/test_loop_edges.py, check_expectations)
        self.xr, self.psy = [], []

    @property
    def n_frames(self):
        return len(self.xr)

    def format_key(self):
        # (a chain that is to show up in k_prep's list gets a launch of its own: the count is the launch's)
        return (self.rate, self.channels, self.crc, self.n_frames, self.state is not None, self.name if self.expect.get("listed") else None)

    def frame(self, granules):
        """granules: [gr][ch] of (xr[576], pe, ratio_l[21] or scalar, ratio_s[12][3] or scalar, block type)"""
        x = np.zeros((2, self.channels, 576))
        p = np.zeros((2, self.channels), PSY_DT)
        for gr in range(2):
            for ch in range(self.channels):
                xr, pe, rl, rs, bt = granules[gr][ch]
                x[gr, ch] = xr
                p[gr, ch]["pe"], p[gr, ch]["ratio_l"], p[gr, ch]["ratio_s"], p[gr, ch]["block_type"] = pe, rl, rs, bt
        self.xr.append(x)
        self.psy.append(p)
        return self

    def mono(self, g0, g1=None):
        return self.frame([[g0], [g1 if g1 is not None else silent()]])

    def copy(self, name=None, **expect):
        c = Chain(self.set, "", self.rate, self.channels, self.kbps, self.crc, self.state, **(expect or self.expect))
        c.name = self.name if name is None else "%s %d %s" % (self.set, self.rate, name)
        c.xr, c.psy = [a.copy() for a in self.xr], [a.copy() for a in self.psy]
        return c

    def xr_array(self):
        return np.ascontiguousarray(np.stack(self.xr))  # [nf][2][C][576]

    def psy_array(self):
        return np.ascontiguousarray(np.stack(self.psy))


def silent(bt=0, pe=0.0):
    return (np.zeros(576), pe, 1.0, 1.0, bt)


def spectrum(rng, scale=300.0, decay=140.0, n=576):
    """a Laplacian spectrum with a tilt, as an MDCT of music has one"""
    x = rng.laplace(0.0, 1.0, 576) * scale * np.exp(-np.arange(576) / decay)
    x[n:] = 0.0
    return x


def band_energy(rate, xr, shortb):
    """calc_xmin's band energies: sequential double sums (np.cumsum adds in index order), long [21] or short [12][3]"""
    sq = xr * xr
    if not shortb:
        return np.array([np.cumsum(sq[a:b])[-1] for a, b in zip(SFB_L[rate][:21], SFB_L[rate][1:22])])
    return np.array([[np.cumsum(sq[3 * a + w:3 * b:3])[-1] for w in range(3)] for a, b in zip(SFB_S[rate][:12], SFB_S[rate][1:13])])


def band_width(rate, shortb):
    t = SFB_S[rate][:13] if shortb else SFB_L[rate][:22]
    return np.array([float(b - a) for a, b in zip(t[:-1], t[1:])])


# ---------------------------------------------------------------------------------------------------------------------
# the three implementations
# ---------------------------------------------------------------------------------------------------------------------
class Result:
    """ix [nf][2][C][576] int16, side [nf] SIDE_DT, state STATE_DT, trace [nf][2][C] TRACE_DT or None"""

    def __init__(self, ix, side, state, trace=None):
        self.ix, self.side, self.state, self.trace = ix, side, state, trace

    @property
    def status(self):
        return int(self.state["status"])


def run_oracle(lib, c, trace_iter=None):
    """trace_iter None: the iteration the chain was built for -- L1's chains put a threshold on the noise of iteration 1, or 2
    (expect["it"]), and the trace is to keep THAT comparison --, the last one for the other sets"""
    if trace_iter is None:
        trace_iter = c.expect.get("it", 1 if c.set == "L1" else 0)
    lib.mp3o_iteration_loop.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 4
    nf, C = c.n_frames, c.channels
    xr, psy = c.xr_array(), c.psy_array()
    ix, side = np.zeros((nf, 2, C, 576), np.int16), np.zeros(nf, SIDE_DT)
    state, trace = np.zeros((), STATE_DT), np.zeros((nf, 2, C), TRACE_DT)
    st_in = np.ascontiguousarray(c.state) if c.state is not None else None
    rc = lib.mp3o_iteration_loop(c.rate, C, c.kbps, c.crc, nf, xr.ctypes.data, psy.ctypes.data, st_in.ctypes.data if st_in is not None else None,
                                 trace_iter, ix.ctypes.data, side.ctypes.data, state.ctypes.data, trace.ctypes.data)
    assert rc == 0, "the oracle refused %s" % c.name
    return Result(ix, side, state, trace)


def run_hook(lib, group):
    """chains of one format_key() through mp3mi_debug_iteration_loop in ONE launch: (rc, [Result per chain], records k_prep redid)"""
    lib.mp3mi_debug_iteration_loop.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 8
    c0 = group[0]
    assert all(c.format_key() == c0.format_key() for c in group)
    S, nf, C = len(group), c0.n_frames, c0.channels
    kbps = np.array([c.kbps for c in group], np.int32)
    xr = np.ascontiguousarray(np.stack([c.xr_array() for c in group]))
    psy = np.ascontiguousarray(np.stack([c.psy_array() for c in group]))
    st_in = np.ascontiguousarray(np.stack([c.state for c in group])) if c0.state is not None else None
    ix, side, state = np.zeros((S, nf, 2, C, 576), np.int16), np.zeros((S, nf), SIDE_DT), np.zeros(S, STATE_DT)
    listed = np.zeros(1, np.int32)
    rc = lib.mp3mi_debug_iteration_loop(c0.rate, C, c0.crc, S, nf, kbps.ctypes.data, xr.ctypes.data, psy.ctypes.data,
                                        st_in.ctypes.data if st_in is not None else None, ix.ctypes.data, side.ctypes.data, state.ctypes.data,
                                        listed.ctypes.data)
    return rc, [Result(ix[s], side[s], state[s]) for s in range(S)], int(listed[0])


def run_reference(c, workdir, timeout=60):
    """a child process: (exit status, Result of the frames it got through -- state: ResvSize and addresses only --, stderr's end)"""
    assert c.state is None
    cf, of = os.path.join(workdir, "loop_chain.bin"), os.path.join(workdir, "loop_out.bin")
    if os.path.exists(of):
        os.remove(of)
    with open(cf, "wb") as f:
        f.write(np.array([c.rate, c.channels, c.kbps, c.crc, c.n_frames, 0, 0, 0], "<i4").tobytes())
        f.write(c.xr_array().tobytes())
        f.write(c.psy_array().tobytes())
    r = subprocess.run([REF_HARNESS_LOOP, cf, of], capture_output=True, cwd=workdir, timeout=timeout)
    raw = open(of, "rb").read() if os.path.exists(of) else b""
    C, per = c.channels, SIDE_DT.itemsize + 2 * c.channels * 576 * 2
    n = min(len(raw) // per, c.n_frames)
    side, ix = np.zeros(n, SIDE_DT), np.zeros((n, 2, C, 576), np.int16)
    for f in range(n):
        side[f] = np.frombuffer(raw, SIDE_DT, 1, f * per)[0]
        ix[f] = np.frombuffer(raw, "<i2", 2 * C * 576, f * per + SIDE_DT.itemsize).reshape(2, C, 576)
    state = np.zeros((), STATE_DT)
    if r.returncode == 0:
        tail = np.frombuffer(raw, "<i4", 13, c.n_frames * per)
        state["ResvSize"], state["addr"] = tail[0], tail[1:].reshape(2, 2, 3)
    return r.returncode, Result(ix, side, state), r.stderr[-300:]


GR_FIELDS = [n for n in SIDE_DT["gr"].base.names if n != "scalefac"]


def mismatch(c, got, want, with_state=True, frames=None):
    """None, or what differs first: every field of the side information, the scalefactors, the signed quantised values over the
    lines the side information declares (2 big_values + 4 count1: behind them a granule's ix keeps what the last pass of the
    search left, which no decoder reads -- tests/stage_check.py), the final ResvSize and addresses, the status word.  After an
    assertion of the reference's only the status word means anything."""
    if with_state and got.status != want.status:
        return "%s: status %#x against %#x" % (c.name, got.status, want.status)
    if want.status:
        return None
    for f in range(c.n_frames if frames is None else frames):
        for k in ("main_data_begin", "resvDrain"):
            if got.side[f][k] != want.side[f][k]:
                return "%s: frame %d %s %d against %d" % (c.name, f, k, got.side[f][k], want.side[f][k])
        if not np.array_equal(got.side[f]["scfsi"][:c.channels], want.side[f]["scfsi"][:c.channels]):
            return "%s: frame %d scfsi %s against %s" % (c.name, f, got.side[f]["scfsi"].tolist(), want.side[f]["scfsi"].tolist())
        for gr in range(2):
            for ch in range(c.channels):
                g, w = got.side[f]["gr"][gr][ch], want.side[f]["gr"][gr][ch]
                for k in GR_FIELDS:
                    if not np.array_equal(g[k], w[k]):
                        return "%s: frame %d gr %d ch %d %s %s against %s" % (c.name, f, gr, ch, k, g[k], w[k])
                if not np.array_equal(g["scalefac"][:36], w["scalefac"][:36]):
                    return "%s: frame %d gr %d ch %d scalefactors %s against %s" % (c.name, f, gr, ch, g["scalefac"].tolist(), w["scalefac"].tolist())
                n = 2 * int(w["big_values"]) + 4 * int(w["count1"])
                if not np.array_equal(got.ix[f, gr, ch, :n], want.ix[f, gr, ch, :n]):
                    k = int(np.argmax(got.ix[f, gr, ch, :n] != want.ix[f, gr, ch, :n]))
                    return "%s: frame %d gr %d ch %d ix[%d] %d against %d" % (c.name, f, gr, ch, k, got.ix[f, gr, ch, k], want.ix[f, gr, ch, k])
    if with_state:
        for k in ("ResvSize", "addr"):
            if not np.array_equal(got.state[k][..., :c.channels, :] if k == "addr" else got.state[k], want.state[k][..., :c.channels, :] if k == "addr" else want.state[k]):
                return "%s: final %s %s against %s" % (c.name, k, got.state[k].tolist(), want.state[k].tolist())
    return None


def by_format(all_chains):
    groups = {}
    for c in all_chains:
        groups.setdefault(c.format_key(), []).append(c)
    return list(groups.values())


# ---------------------------------------------------------------------------------------------------------------------
# the sets
# ---------------------------------------------------------------------------------------------------------------------
def _seed(rate, k):
    return np.random.default_rng([0x4C4F4F50, rate, k])


def _ulps(x, n):
    for _ in range(abs(n)):
        x = np.nextafter(x, math.inf if n > 0 else -math.inf)
    return float(x)


OFFSETS = [("0 ulp", 0, 0.0), ("+1 ulp", 1, 0.0), ("-1 ulp", -1, 0.0), ("+2 ulp", 2, 0.0), ("-2 ulp", -2, 0.0), ("+4 ulp", 4, 0.0), ("-4 ulp", -4, 0.0),
           ("+5e-13", 0, 5e-13), ("-5e-13", 0, -5e-13), ("+2e-12", 0, 2e-12), ("-2e-12", 0, -2e-12)]


def _target(xfsf, off):
    """where xmin is to land: `off` away from the noise"""
    _, n, rel = off
    return _ulps(xfsf, n) if rel == 0.0 else xfsf * (1.0 + rel)


def _ratio_for(target, en, bw, post=1.0):
    """the ratio r for which calc_xmin's r * en / bw (src/loop.c:1085-1118), times `post` (pre-emphasis' factor), is `target`, or
    comes nearest to it: the quotient's neighbourhood is searched ulp by ulp, with the arithmetic of the code"""
    r0 = target / post * bw / en
    best = None
    for k in range(-12, 13):
        r = _ulps(r0, k)
        v = r * en / bw * post
        if best is None or abs(v - target) < abs(best[1] - target):
            best = (r, v)
    return best[0]


def _base(rate, k, bt=0, scale=0.6):
    rng = _seed(rate, k)
    return spectrum(rng, scale, 160.0)


def _granule(xr, bt=0, pe=0.0, rl=BIG, rs=BIG):
    return (xr, pe, np.full(21, rl) if np.isscalar(rl) else np.array(rl, float), np.full((12, 3), rs) if np.isscalar(rs) else np.array(rs, float), bt)


def l1_chains(rate, lib):
    out = []
    bw_l, bw_s = band_width(rate, False), band_width(rate, True)
    # -- iteration 1, long: one pass with every ratio BIG gives the noise of the first iteration, which no ratio changes
    xr = _base(rate, 100)
    en = band_energy(rate, xr, False)
    t = run_oracle(lib, Chain("L1", "probe", rate).mono(_granule(xr)), 1).trace[0, 0, 0]
    assert t["kept_iter"] == 1
    x1 = t["xfsf"][:21].copy()
    for off in OFFSETS:
        inside = abs(off[2]) < 1e-12
        for b in range(21):
            rl = np.full(21, BIG)
            rl[b] = _ratio_for(_target(x1[b], off), en[b], bw_l[b])
            out.append(Chain("L1", "long sfb %d %s" % (b, off[0]), rate, close=inside, band=b, emu=(b % 7 == 3 and off[1] in (0, 1, -1) and off[2] == 0.0)).mono(_granule(xr, rl=rl)))
        rl = np.array([_ratio_for(_target(x1[b], off), en[b], bw_l[b]) for b in range(21)])
        out.append(Chain("L1", "long all bands %s" % off[0], rate, close=inside, band=-1, emu=True).mono(_granule(xr, rl=rl)))
    rl = np.array([_ratio_for(_target(x1[b], OFFSETS[b % 7]), en[b], bw_l[b]) for b in range(21)])
    out.append(Chain("L1", "long all bands, mixed offsets", rate, close=True, band=-1, emu=True).mono(_granule(xr, rl=rl)))
    # -- bands with xmin == 0 (ratio 0: they violate for ever) and a band without energy (noise 0 against xmin 0) beside crafted ones
    xz = xr.copy()
    xz[SFB_L[rate][9]:SFB_L[rate][10]] = 0.0
    xz[SFB_L[rate][4]:SFB_L[rate][5]] = -0.0
    rl = np.array([_ratio_for(_target(x1[b], OFFSETS[1 + b % 2]), en[b], bw_l[b]) for b in range(21)])
    rl[[1, 9, 12, 19]] = 0.0
    out.append(Chain("L1", "long xmin == 0 and empty bands", rate, close=None, band=-1, emu=True).mono(_granule(xz, rl=rl)))
    # -- iteration 1, short: 12 of the 36 lanes
    xs = _base(rate, 101)
    ens = band_energy(rate, xs, True)
    t = run_oracle(lib, Chain("L1", "probe", rate).mono(_granule(xs, bt=2)), 1).trace[0, 0, 0]
    s1 = t["xfsf"].copy()
    for off in OFFSETS:
        inside = abs(off[2]) < 1e-12
        for lane in (0, 1, 2, 7, 11, 16, 18, 19, 23, 27, 34, 35):
            rs = np.full((12, 3), BIG)
            rs[lane // 3, lane % 3] = _ratio_for(_target(s1[lane], off), ens[lane // 3, lane % 3], bw_s[lane // 3])
            out.append(Chain("L1", "short lane %d %s" % (lane, off[0]), rate, close=inside, band=lane, emu=(lane in (7, 34) and off[1] in (0, -1) and off[2] == 0.0)).mono(_granule(xs, bt=2, rs=rs)))
        rs = np.array([[_ratio_for(_target(s1[3 * b + w], off), ens[b, w], bw_s[b]) for w in range(3)] for b in range(12)])
        out.append(Chain("L1", "short all lanes %s" % off[0], rate, close=inside, band=-1, emu=off[2] == 0.0 and abs(off[1]) < 2).mono(_granule(xs, bt=2, rs=rs)))
    # -- iteration 2: sfb 0..19 violate in iteration 1 and are amplified (sfb 20 never: no loop_break, no pre-emphasis), and their
    #    doubled thresholds land on the second iteration's noise.  That noise depends on all of it, so the ratios are a fixed point,
    #    found by iteration; the last step, the offset, moves a ratio by parts in 1e12 and no decision with it.
    IFQ2 = math.sqrt(2.0) * math.sqrt(2.0)  # amp_scalefac_bands' ifqstep2 (src/loop.c:1243): not quite 2
    live = list(range(20))
    for _ in range(6):  # (a band that does not settle, or is not amplified for certain, leaves -- and the others settle again)
        rl = np.full(21, BIG)
        rl[live] = (x1 / 3.0 * bw_l / en)[live]
        for _ in range(40):
            t2 = run_oracle(lib, Chain("L1", "probe", rate).mono(_granule(xr, rl=rl)), 2).trace[0, 0, 0]
            if t2["kept_iter"] != 2 or max(abs(t2["xfsf"][b] / t2["xmin"][b] - 1.0) for b in live) < 1e-13:
                break
            for b in live:
                rl[b] *= t2["xfsf"][b] / t2["xmin"][b]
        t1 = run_oracle(lib, Chain("L1", "probe", rate).mono(_granule(xr, rl=rl)), 1).trace[0, 0, 0]
        keep = [b for b in live if t2["kept_iter"] == 2 and t1["xfsf"][b] > 1.5 * t1["xmin"][b] and abs(t2["xfsf"][b] / t2["xmin"][b] - 1.0) < 1e-9]
        if keep == live:
            break
        live = keep
    for off in OFFSETS:
        r2 = rl.copy()
        for b in live:
            r2[b] = _ratio_for(_target(t2["xfsf"][b], off), en[b], bw_l[b], IFQ2)
        out.append(Chain("L1", "iteration 2, %d bands %s" % (len(live), off[0]), rate, close=abs(off[2]) < 1e-12, band=-2, it=2, bands=list(live), n_bands=len(live), emu=off[2] == 0.0 and abs(off[1]) < 2).mono(_granule(xr, rl=r2)))
    # -- the second comparison: sfb 17..20 violate (ratio 0), pre-emphasis multiplies every threshold by sqrt(2)^(2 pretab), and
    #    the band's moved threshold lands on its noise
    for off in OFFSETS:
        for b in range(11, 21):
            rl = np.full(21, BIG)
            rl[17:21] = 0.0
            rl[b] = _ratio_for(_target(x1[b], off), en[b], bw_l[b], math.pow(math.sqrt(2.0), 2.0 * PRETAB[b]))
            out.append(Chain("L1", "behind pre-emphasis sfb %d %s" % (b, off[0]), rate, close=abs(off[2]) < 1e-12, band=b, pre=True, emu=(b in (11, 12) and off[1] in (0, 1) and off[2] == 0.0)).mono(_granule(xr, rl=rl)))
        rl = np.array([BIG] * 11 + [_ratio_for(_target(x1[b], off), en[b], bw_l[b], math.pow(math.sqrt(2.0), 2.0 * PRETAB[b])) for b in range(11, 21)])
        # (not for the emulated build: behind this second check k_loop's lanes read their bands' lines for the exact sums and then
        # scale their own lines with no collective in between -- one instruction after the other for a wavefront in lock-step, but
        # the emulator's lanes are fibers that run alone between collectives, in lane order, and a band lane would read lines that
        # a lane before it has scaled already.  Of the chains above the emulated build takes sfb 11 and 12: their lines, 62..102
        # at the three rates, belong to lanes 31..50, which run behind band lanes 11 and 12.)
        out.append(Chain("L1", "behind pre-emphasis sfb 11..20 %s" % off[0], rate, close=abs(off[2]) < 1e-12, band=-1, pre=True, emu=False).mono(_granule(xr, rl=rl)))
    return out


def _amplified(lib, c, lane):
    r = run_oracle(lib, c)
    return int(r.side[0]["gr"][0][0]["scalefac"][lane]), r


def _set_ratio(c, shortb, lane, v):
    if shortb:
        c.psy[0][0, 0]["ratio_s"][lane // 3, lane % 3] = v
    else:
        c.psy[0][0, 0]["ratio_l"][lane] = v


def _tune(lib, c, shortb, lane, n):
    """the ratio of band `lane` that leaves it amplified n times: a ratio 2^-e, the least e that reaches n by bisection (the
    threshold doubles with every amplification: one more e, about one more amplification); True where it lands on n"""
    if n == 0:
        _set_ratio(c, shortb, lane, BIG)
        return True
    lo, hi = -40.0, 80.0
    for _ in range(9):
        mid = 0.5 * (lo + hi)
        _set_ratio(c, shortb, lane, 2.0 ** -mid)
        if _amplified(lib, c, lane)[0] >= n:
            hi = mid
        else:
            lo = mid
    for k in range(25):  # (the noise moves with the step: the neighbourhood, outwards)
        e = hi + 0.125 * ((k + 1) // 2) * (1 if k % 2 else -1)
        _set_ratio(c, shortb, lane, 2.0 ** -e)
        if _amplified(lib, c, lane)[0] == n:
            return True
    return False


def l2_chains(rate, lib):
    out = []
    for shortb, (la, lb) in ((False, (3, 14)), (True, (7, 25))):
        xr = _base(rate, 200 + shortb)
        bt = 2 if shortb else 0
        what = "short" if shortb else "long"
        # the three ways out: nothing violates in iteration 1; every band is amplified (loop_break); a scalefactor passes its field
        out.append(Chain("L2", "%s over == 0 in iteration 1" % what, rate, exit=EXIT_NO_OVER, n_outer=1, emu=True).mono(_granule(xr, bt)))
        out.append(Chain("L2", "%s loop_break" % what, rate, exit=EXIT_LOOP_BREAK, emu=True).mono(_granule(xr, bt, rl=0.0, rs=0.0)))
        for lane, name in ((la, "first maximum to 16"), (lb, "second maximum to 8")):
            c = Chain("L2", "%s %s" % (what, name), rate, exit=EXIT_SCALE_BITCOUNT, emu=True).mono(_granule(xr, bt))
            _set_ratio(c, shortb, lane, 0.0)
            out.append(c)
        # every cell of the table: the largest value of each bit length, and the smallest of the longer ones
        cells = [(a, b) for a in (0, 1, 3, 7, 15) for b in (0, 1, 3, 7)] + [(2, 2), (4, 4), (8, 2), (8, 4), (4, 0), (2, 1), (4, 2), (6, 3), (5, 2)]
        for t1, t2 in (cells if not shortb else cells[::3]):
            for a, b in [(la + da, lb + db) for da, db in ((0, 0), (2, 2), (-2, -3), (4, 5), (1, 1), (-1, 3), (5, -2), (3, 4), (6, 6), (-3, -1), (2, -3), (7, 1))]:  # (another pair of bands where one does not settle)
                c = Chain("L2", "%s maxima %d / %d" % (what, t1, t2), rate, maxima=(t1, t2), emu=(not shortb and rate == 44100) or (t1 + 2 * t2) % 5 == 0).mono(_granule(xr, bt))
                ok = False
                for _ in range(3):
                    ok = _tune(lib, c, shortb, a, t1) and _tune(lib, c, shortb, b, t2) and _amplified(lib, c, a)[0] == t1
                    if ok:
                        break
                if ok:
                    out.append(c)
                    break
            else:
                MISSING.append("L2 %d %s maxima %d / %d" % (rate, what, t1, t2))
        # 15 against 16 and 7 against 8 with the other maximum at its end too
        for r1, r2, name in ((0.0, None, "16 / 7"), (None, 0.0, "15 / 8")):
            c = Chain("L2", "%s maxima %s" % (what, name), rate, exit=EXIT_SCALE_BITCOUNT, emu=True).mono(_granule(xr, bt))
            if r1 is None:
                _set_ratio(c, shortb, lb, 0.0)
                _tune(lib, c, shortb, la, 15)
            else:
                _set_ratio(c, shortb, la, 0.0)
                _tune(lib, c, shortb, lb, 7)
            out.append(c)
    return out


def l3_chains(rate, lib):
    out = []
    xr = _base(rate, 300)

    def rl_of(viol):
        rl = np.full(21, BIG)
        rl[list(viol)] = 0.0
        return rl
    for bt in (0, 1, 3, 2):
        out.append(Chain("L3", "all four, block type %d" % bt, rate, fired=bt != 2, emu=True).mono(_granule(xr, bt, rl=rl_of(range(17, 21)), rs=0.0 if bt == 2 else BIG)))
    for miss in range(17, 21):
        out.append(Chain("L3", "three of four, without sfb %d" % miss, rate, fired=False, emu=miss in (17, 20)).mono(_granule(xr, 0, rl=rl_of(b for b in range(17, 21) if b != miss))))
    # granule 1 shares scalefactors -- its two channels are alike but for group 0, as granule 0's are: calc_scfsi compares CHANNELS
    # (l4_chains) -- and inherits granule 0's preflag; sfb 2 violates in the group that is not shared, so that a second iteration
    # keeps what the first one inherited (outer_loop restores the preflag of before its last iteration)
    def other(x):
        y = x.copy()
        y[:SFB_L[rate][6]] *= 32.0
        return y
    for k, (v0, v1, name) in enumerate(((range(17, 21), (), "set"), (range(17, 20), range(17, 21), "clear"))):
        r0, r1 = rl_of(list(v0) + [2]), rl_of(list(v1) + [2])
        c = Chain("L3", "granule 1 inherits a preflag that is %s" % name, rate, 2, 192, inherit=1 - k, emu=True)
        out.append(c.frame([[_granule(xr, 0, rl=r0), _granule(other(xr), 0, rl=r0)], [_granule(xr * 0.9, 0, rl=r1), _granule(other(xr * 0.9), 0, rl=r1)]]))
    return out


def _coded(rate, k):
    """a spectrum whose band b holds 1.5 * 2^k[b] of energy in its first line: calc_scfsi stores (int) log2 = k[b] (k >= 0)"""
    x = np.zeros(576)
    for b in range(21):
        x[SFB_L[rate][b]] = math.sqrt(1.5 * 2.0 ** int(k[b])) * (-1.0 if b % 3 == 1 else 1.0)
    return x


def _coded_granule(rate, k, m, bt=0, pe=0.0):
    """... and whose stored log2 xmin is k[b] + m[b]: ratio = width * 2^m"""
    return _granule(_coded(rate, k), bt, pe, rl=band_width(rate, False) * 2.0 ** np.array(m, float))


def _spread(group, total):
    """a difference vector: `total` spread over the bands of scfsi group `group`"""
    d = np.zeros(21, int)
    lo, hi = SCFSI_BAND[group], SCFSI_BAND[group + 1]
    for i in range(total):
        d[lo + i % (hi - lo)] += 1
    return d


def l4_chains(rate, lib):
    """calc_scfsi compares sc_en[ch][0] with sc_en[ch][1] of arrays filled as [gr][ch] (sic): channel 0's mask comes from granule
    0's two CHANNELS, channel 1's from granule 1's; hence stereo, and mono only behind an initial state"""
    out = []
    k0, m0 = np.full(21, 6), np.full(21, 4)  # (thresholds 16 times the energy: no band violates unless a chain says so)

    def stereo(name, d_en0, d_xm0, d_en1, d_xm1, **kw):
        """granule 0: channel 1 differs from channel 0 by d_en0 (energies) and d_xm0 (xmin); granule 1 likewise"""
        c = Chain("L4", name, rate, 2, 192, **kw)
        g = [[_coded_granule(rate, k0 + gr, m0), _coded_granule(rate, k0 + gr + (d_en0, d_en1)[gr], m0 - (d_en0, d_en1)[gr] + (d_xm0, d_xm1)[gr])] for gr in range(2)]
        return c.frame(g)
    z = np.zeros(21, int)
    for g in range(4):
        for tot in (9, 10):
            out.append(stereo("energies differ by %d in group %d" % (tot, g), _spread(g, tot), z, z, _spread(g, tot), masks=((15 if tot == 9 else 15 - (1 << g)), ) * 2, emu=g == 0))
            out.append(stereo("xmin differs by %d in group %d" % (tot, g), z, _spread(g, tot), _spread(g, tot), z, masks=((15 if tot == 9 else 15 - (1 << g)), ) * 2, emu=g == 1 and tot == 10))
    rest = _spread(1, 30) + _spread(2, 30) + _spread(3, 30)
    out.append(stereo("99 in all", _spread(0, 9) + rest, z, z, z, masks=(1, 15), emu=True))
    out.append(stereo("100 in all", _spread(0, 10) + rest, z, z, z, masks=(0, 15), emu=True))
    out.append(stereo("100 in all, 9 in group 0", _spread(0, 9) + rest + _spread(1, 1), z, z, z, masks=(0, 15)))
    for mask in range(16):
        d0 = sum((_spread(g, 10) for g in range(4) if not mask >> g & 1), z)
        d1 = sum((_spread(g, 10) for g in range(4) if mask >> g & 1), z)
        out.append(stereo("masks %d and %d" % (mask, 15 - mask), d0 if mask else _spread(0, 10) + _spread(1, 10) + _spread(2, 10) + _spread(3, 9) + _spread(3, 1), z, d1, z,
                          masks=(mask, 15 - mask), emu=mask == 5))
    # short blocks and silence in either place; stale values behind a short block (frame 1 reads frame 0's)
    A, B = _coded_granule(rate, k0, m0), _coded_granule(rate, k0 + _spread(2, 10), m0)
    sh = _granule(_base(rate, 400, scale=8.0), 2, rs=1e-3)
    out.append(Chain("L4", "granule 1 channel 0 short", rate, 2, 192, masks=(0, 0)).frame([[A, A], [sh, A]]))
    out.append(Chain("L4", "granule 1 channel 1 short", rate, 2, 192, masks=(15, 0)).frame([[A, A], [A, sh]]))
    out.append(Chain("L4", "granule 0 channel 1 silent", rate, 2, 192, masks=(0, 15)).frame([[A, silent()], [A, A]]))
    out.append(Chain("L4", "granule 1 channel 0 silent", rate, 2, 192, masks=(15, 0), emu=True).frame([[A, A], [silent(), A]]))
    c = Chain("L4", "granule 0 channel 1 short behind a long one: stale energies", rate, 2, 192, masks=(15 - 4, 15), emu=True)
    c.frame([[A, B], [A, A]]).frame([[A, sh], [A, A]])
    c.expect["frame"] = 1
    out.append(c)
    c = Chain("L4", "three frames, short blocks wandering", rate, 2, 192, masks=None)
    c.frame([[A, A], [B, A]]).frame([[sh, A], [A, B]]).frame([[B, sh], [sh, A]])
    out.append(c)
    # granule 1 amplifies beside shared groups: copySF in iteration 1, preventSF behind it; granule 0 left scalefactors there
    mv = m0.copy()
    mv[2], mv[18], mv[19] = -30, -30, -30
    V = _coded_granule(rate, k0 + 3, mv)
    mw = mv.copy()
    mw[17:21] = -30
    W = _coded_granule(rate, k0 + 3 + _spread(3, 10), mw)
    out.append(Chain("L4", "granule 1 amplifies beside shared groups", rate, 2, 192, masks=(7, 15), more_iterations=True, emu=True).frame([[V, _coded_granule(rate, k0 + 3 + _spread(3, 10), mv)], [W, W]]))
    # mono: the second column is the initial state's
    for tot in (9, 10):
        st = np.zeros((), STATE_DT)
        st["sc_xrmax"][0][1], st["sc_en"][0][1], st["sc_xm"][0][1] = 3, k0 + _spread(1, tot), k0 + m0
        out.append(Chain("L4", "mono behind a state, %d in group 1" % tot, rate, 1, 128, state=st, masks=(15 if tot == 9 else 13,), emu=tot == 10).mono(A, _coded_granule(rate, k0 + 2, m0)))
    out.append(Chain("L4", "mono, fresh: never", rate, 1, 128, masks=(0,)).mono(A, A))
    return out


def _pe_for(mb, more):
    """pe with (int) (pe * 3.1 - mean_bits) == more, in the middle of its interval (src/reservoir.c:117)"""
    return (mb + more + 0.5) / 3.1


def _pe_edge(mb, t):
    """(below, on): neighbouring doubles whose pe * 3.1 - mean_bits lies just below t and on or just above it"""
    pe = (mb + t) / 3.1
    while pe * 3.1 - mb >= t:
        pe = _ulps(pe, -1)
    while _ulps(pe, 1) * 3.1 - mb < t:
        pe = _ulps(pe, 1)
    return pe, _ulps(pe, 1)


def l5_chains(rate, lib):
    out = []
    for k, (kbps, C, crc) in enumerate((b, C, crc) for b in BITRATES for C in (1, 2) for crc in (0, 1)):
        rng = _seed(rate, 5000 + k)
        mb = mean_bits_of(rate, C, kbps, crc) // C
        lo, on = _pe_edge(mb, 101.0)
        pes = [[_pe_for(mb, 100), lo], [_pe_for(mb, 101), on]]
        c = Chain("L5", "%d kbit/s %d ch crc %d: a silent frame, more_bits on 100 / 101" % (kbps, C, crc), rate, C, kbps, crc, emu=(k % 28 == 9))
        c.frame([[silent()] * C] * 2)
        gs = [[random_granule(rng, loud=0.3) for _ in range(C)] for _ in range(2)]
        c.frame([[(g[0], pes[gr][ch], g[2], g[3], g[4]) for ch, g in enumerate(gs[gr])] for gr in range(2)])
        c.frame([[random_granule(rng, loud=0.3) for _ in range(C)] for _ in range(2)])
        out.append(c)
    # pe * 3.1 - mean_bits one ulp below and on the integers 100, 101, 102 and 250 (more_bits 99 | 100, ... with the reservoir filled)
    for C in (1, 2):
        rng = _seed(rate, 5400 + C)
        mb = mean_bits_of(rate, C, 128, 0) // C
        edges = [v for t in (100.0, 101.0, 102.0, 250.0) for v in _pe_edge(mb, t)]
        c = Chain("L5", "%d ch: pe * 3.1 - mean_bits an ulp either side of 100, 101, 102, 250" % C, rate, C, 128, emu=C == 1)
        c.frame([[silent()] * C] * 2)
        nfr = len(edges) // (2 * C)
        for f in range(nfr):
            gs = [[random_granule(rng, loud=0.3) for _ in range(C)] for _ in range(2)]
            c.frame([[(g[0], edges[(f * 2 + gr) * C + ch]) + g[2:] for ch, g in enumerate(gs[gr])] for gr in range(2)])
        c.expect["more_bits"] = (slice(1, 1 + nfr), [99, 100, 100, 101, 101, 102, 249, 250])
        out.append(c)
    # the reservoir's levels, behind an initial state
    for C, kbps in ((1, 128), (2, 128), (1, 64)):
        rng = _seed(rate, 5500 + C)
        gs = [[random_granule(rng, loud=0.3) for _ in range(C)] for _ in range(2)]
        rmax = resv_max_of(rate, kbps)
        lvl = (rmax * 8 // 10) // 8 * 8
        for resv in (0, lvl - 8, lvl, lvl + 8, rmax):
            for pe in (0.0, 2500.0):
                st = np.zeros((), STATE_DT)
                st["ResvSize"] = resv
                c = Chain("L5", "%d kbit/s %d ch reservoir %d of %d, pe %g" % (kbps, C, resv, rmax, pe), rate, C, kbps, state=st, emu=(resv in (lvl, lvl + 8) and C == 1 and kbps == 128))
                out.append(c.frame([[(g[0], pe, g[2], g[3], g[4]) for g in row] for row in gs]))
    # the same levels as leading silent frames reach them (what the reference can run)
    for n in (1, 2, 3):
        rng = _seed(rate, 5600)
        c = Chain("L5", "%d silent frames first" % n, rate, 1, 64)
        for _ in range(n):
            c.mono(silent())
        g0, g1 = random_granule(rng, loud=0.3), random_granule(rng, loud=0.3)
        out.append(c.mono((g0[0], 2500.0) + g0[2:], (g1[0], 2500.0) + g1[2:]))
    # stuffing: silence at the highest bitrate drains (ResvMax is 0 or small), mono and stereo
    top = 320
    for C in (1, 2):
        c = Chain("L5", "silence at %d kbit/s, %d ch: stuffing spills and drains" % (top, C), rate, C, top, drain=(rate == 32000 and C == 1), emu=C == 1)
        out.append(c.frame([[silent()] * C] * 2).frame([[silent(bt=2)] * C] * 2))
    # part2_3_length[0][0] + stuffing on 4094 / 4095: granule 0 silent, granule 1's length found by search, the reservoir's
    # initial size (a multiple of 8) takes up the rest: the sum is ResvSize + 2 mean_bits - ResvMax - granule 1's length
    kbps = {44100: 256, 48000: 256, 32000: 192}[rate]
    mb, rmax = mean_bits_of(rate, 1, kbps, 0), resv_max_of(rate, kbps)
    found = {}
    for i in range(400):
        rng = _seed(rate, 5700 + i)
        x1 = np.zeros(576)  # (few lines, loud: its bits stay below every budget, so its length does not move with the reservoir)
        at = rng.choice(576, int(rng.integers(30, 130)), replace=False)
        x1[at] = rng.laplace(0.0, 30.0, len(at))
        g1 = _granule(x1, 0, rl=BIG)
        for want in (4094, 4095):
            if want in found:
                continue
            st = np.zeros((), STATE_DT)
            st["ResvSize"] = rmax
            c = Chain("L5", "part2_3_length[0][0] + stuffing = %d" % want, rate, 1, kbps, state=st, stuffed=want, emu=True).mono(silent(), g1)
            p1 = int(run_oracle(lib, c).trace[0, 1, 0]["part2_3_length"])  # (before ResvFrameEnd's stuffing)
            need = rmax + 2 * mb - rmax - p1 - want  # what the initial size has to lie below ResvMax
            if need >= 0 and need % 8 == 0 and need <= rmax:
                st["ResvSize"] = rmax - need
                r = run_oracle(lib, c)
                if int(r.side[0]["gr"][0][0]["part2_3_length"]) == want and int(r.trace[0, 1, 0]["part2_3_length"]) == p1:
                    found[want] = c
        if len(found) == 2:
            break
    out += [found[k] for k in sorted(found)]
    MISSING.extend("L5 %d stuffing on %d" % (rate, k) for k in (4094, 4095) if k not in found)
    return out


def l6_chains(rate, lib):
    out = []
    for bt in (0, 2):
        for i in range(6000):
            xr = _base(rate, 600 + bt + 10 * (i // 1500))
            c = Chain("L6", "a probe counts exactly max_bits, block type %d" % bt, rate, bisect_equal=True, emu=True).mono(_granule(xr * 1.003 ** (i % 1500), bt, rl=1e-2, rs=1e-2))
            if run_oracle(lib, c).trace[0, 0, 0]["bisect_equal"]:
                out.append(c)
                break
        else:
            MISSING.append("L6 %d a probe on max_bits, block type %d" % (rate, bt))
    out.append(Chain("L6", "the bisection ends on probes one step apart", rate, apart=True, emu=True).mono(_granule(_base(rate, 605), 0, rl=1e-2)))
    # many steps of inner_loop: the scalefactors of 16 amplifications of every band but one take their bits from the values
    xr = _base(rate, 610)
    rl = np.zeros(21)
    rl[20] = BIG
    out.append(Chain("L6", "scalefactors grow, the step follows", rate, 1, 64, steps=True, emu=True).mono(_granule(xr, 0, rl=rl)))
    # scalefactors alone above the budget: a short block at 32 kbit/s in stereo, 48 kHz -- 120 bits a granule against 18 * (4 + 3)
    # = 126, which takes lanes below 18 amplified 8 times and a lane from 18 on 4 to 7 times.  With 120 bits nothing behind line 36
    # is coded, so such a lane's noise IS its energy, amplified with it: it violates for ever or never -- unless its threshold sits
    # within ulps of its noise, where the roundings of the amplification decide anew each time.  Found by search.
    if rate == 48000:
        a, b = SFB_S[rate][6], SFB_S[rate][7]
        for crc in (0, 1):
            for i in range(3000):
                rng = _seed(rate, 6200 + i)
                x = np.zeros(576)
                x[0] = 1e-3
                x[3 * a:3 * b:3] = rng.uniform(0.5, 2.0, b - a)
                en = float(np.cumsum((x * x)[3 * a:3 * b:3])[-1])
                rs = np.full((12, 3), BIG)
                rs[:6] = 0.0
                rs[6, 0] = _ratio_for(_ulps(en / (b - a), -1 - i % 3), en, float(b - a))
                c = Chain("L6", "huff_bits < 0 in frame 1, crc %d" % crc, rate, 2, 32, crc, status=HUFF_BITS | 1 << 8, emu=crc == 0)
                c.frame([[silent()] * 2] * 2).frame([[_granule(x, 2, rs=rs), silent()], [silent(), silent()]])
                if run_oracle(lib, c).status == (HUFF_BITS | 1 << 8):
                    out.append(c)
                    break
            else:
                MISSING.append("L6 %d huff_bits < 0, crc %d" % (rate, crc))
    return out


def host_start_step(xr):
    """quantanf_init (src/loop.c:369-402) in double, as csrc/loop_debug.cpp restates it: (8 ln sfm, q0)"""
    nz = xr[xr != 0.0]
    t = nz * nz
    v = 8.0 * math.log(math.exp(float(np.cumsum(np.log(t))[-1]) / 576.0) / (float(np.cumsum(t)[-1]) / 576.0))
    tp = int(v - 0.5) if v < 0 else int(v + 0.5)
    return v, max(tp, -100) - 70


def _lines(pos, val):
    x = np.zeros(576)
    x[list(pos)] = val
    return x


def l7_chains(rate, lib):
    out = []
    out.append(Chain("L7", "one line of 2^64", rate, q0=-170, emu=True).mono(_granule(_lines([5], XR_MAX))))
    out.append(Chain("L7", "one line of -2^64 at the end, short", rate, q0=-170).mono(_granule(_lines([575], -XR_MAX), 2)))
    # the smallest single line whose start step stays in the table: 8 ln sfm = 8 (ln 576 - (575 / 576) ln xr^2) <= 470.4
    a = math.exp(-0.5 * (470.4 / 8.0 - math.log(576.0)) * 576.0 / 575.0)
    assert host_start_step(_lines([0], a))[1] == STEP_MAX
    out.append(Chain("L7", "one line at the table's end (q0 = 400)", rate, status=GLOBAL_GAIN, q0=STEP_MAX, emu=True).mono(_granule(_lines([0], a))))
    out.append(Chain("L7", "three lines, a start step above 200", rate, status=GLOBAL_GAIN, emu=False).mono(_granule(_lines([0, 300, 575], a * 3.4))))
    # a few tiny lines behind silence: global_gain 255 and 256
    found = {}
    for i in range(4000):
        v = 2.0 ** (-2.0 - i / 400.0)
        if host_start_step(_lines([3, 40, 41, 300], v))[1] not in range(42, 52):  # (the search ends a step above its start here)
            continue
        c = Chain("L7", "", rate).mono(silent(), _granule(_lines([3, 40, 41, 300], [v, -v, v, v]), rl=1.0))
        r = run_oracle(lib, c)
        gain = int(r.side[0]["gr"][1][0]["global_gain"])
        if gain in (255, 256) and gain not in found:
            c.name = "L7 %d tiny lines behind silence, global_gain %d" % (rate, gain)
            c.set, c.expect = "L7", dict(status=GLOBAL_GAIN if gain == 256 else 0, gain=gain, emu=True)
            found[gain] = c
        if len(found) == 2:
            break
    out += [found[k] for k in sorted(found)]
    MISSING.extend("L7 %d global_gain %d" % (rate, k) for k in (255, 256) if k not in found)
    out.append(Chain("L7", "a flat spectrum", rate, q0=-70, emu=True).mono(_granule(np.where(np.arange(576) % 2, -0.03125, 0.03125), rl=1e-3)))
    loud = _base(rate, 700, scale=1e-3)
    loud[17] = 40.0
    out.append(Chain("L7", "the -100 clamp", rate, q0=-170, emu=True).mono(_granule(loud, rl=1e-3)))
    # 8 ln sfm within k_prep's 2e-9 of a rounding boundary of nint: two levels, the upper one moved until v = -(n + 1/2)
    for n_hi, n in ((40, 12), (200, 3)):
        x = np.full(576, 0.01)
        lo, hi = 0.01, 10.0
        want = -(n + 0.5)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            x[:n_hi] = mid
            if host_start_step(x)[0] > want:
                lo = mid
            else:
                hi = mid
        best = min((abs(host_start_step(np.concatenate([np.full(n_hi, _ulps(lo, k)), x[n_hi:]]))[0] - want), k) for k in range(-40, 41))
        x[:n_hi] = _ulps(lo, best[1])
        x[1::2] *= -1.0
        out.append(Chain("L7", "8 ln sfm = %.1f: undecided by the first tier" % want, rate, listed=True, emu=True).mono(_granule(x, rl=1e-3), _granule(x[::-1].copy(), 2, rs=1e-3)))
    # -0.0, and silence between sound: the addresses of the frame before stay
    mz = _base(rate, 710)
    mz[100:] = -0.0
    mz[::5] = -0.0
    c = Chain("L7", "-0.0 lines, silence of -0.0 between sound", rate, 2, 128, emu=True)
    c.frame([[_granule(mz, 0, rl=1e-2), _granule(_base(rate, 711), 1, rl=1e-2)], [_granule(_base(rate, 712), 0, rl=1e-2), _granule(mz, 3, rl=1e-2)]])
    c.frame([[_granule(np.full(576, -0.0)), silent()], [silent(bt=1), _granule(np.full(576, -0.0), 3)]])
    c.frame([[_granule(_base(rate, 713), 0, rl=1e-2), silent()], [silent(), _granule(_base(rate, 714), 2, rs=1e-2)]])
    out.append(c)
    return out


def random_granule(rng, bt=None, loud=None):
    bt = int(rng.integers(0, 4)) if bt is None else bt
    loud = float(np.exp(rng.uniform(np.log(2e-3), np.log(2.0)))) if loud is None else loud
    x = spectrum(rng, loud, float(rng.uniform(40.0, 400.0)), int(rng.integers(60, 577)))
    return (x, float(rng.uniform(0.0, 2500.0)), np.exp(rng.uniform(np.log(1e-5), np.log(10.0), 21)),
            np.exp(rng.uniform(np.log(1e-5), np.log(10.0), (12, 3))), bt)


def l8_chains(rate, lib=None):
    """every format (bitrate x channels x crc), 6 frames of random granules"""
    out = []
    for k, (kbps, C, crc) in enumerate((b, C, crc) for b in BITRATES for C in (1, 2) for crc in (0, 1)):
        rng = _seed(rate, 8000 + k)
        c = Chain("L8", "%d kbit/s %d ch crc %d" % (kbps, C, crc), rate, C, kbps, crc, emu=(k == 20))
        for _ in range(6):
            c.frame([[random_granule(rng) for _ in range(C)] for _ in range(2)])
        out.append(c)
    return out


# chains per set at every rate (L6: two more at 48 kHz, the only rate at which a short block's scalefactors pass a granule's budget)
COUNTS = {"L1": 519, "L2": 51, "L3": 10, "L4": 45, "L5": 95, "L6": 4, "L7": 11, "L8": 56}
MISSING = []  # what a search of the generator did not find (tests assert that it is empty)
SET_NAMES = ("L1", "L2", "L3", "L4", "L5", "L6", "L7", "L8")
_cache = {}


def chains(rate, lib):
    """every chain of every set at `rate` (lib: the oracle's library, which the crafted values are searched with)"""
    if rate not in _cache:
        _cache[rate] = sum((f(rate, lib) for f in (l1_chains, l2_chains, l3_chains, l4_chains, l5_chains, l6_chains, l7_chains, l8_chains)), [])
    return _cache[rate]


def check_expectations(c, r):
    """None, or how the oracle's result r (with its trace) misses what chain c was built to reach"""
    e, t = c.expect, r.trace
    t0 = t[0, 0, 0]
    if "close" in e and e["close"] is not None:
        if e["close"] != bool(t0["closest"] <= 1e-12):
            return "%s: closeness %g" % (c.name, t0["closest"])
    if e.get("pre") and t0["pre_iter"] != 1:
        return "%s: pre-emphasis did not fire in iteration 1" % c.name
    if "n_bands" in e and e["n_bands"] < 4:
        return "%s: only %d bands" % (c.name, e["n_bands"])
    if "exit" in e and t0["exit_how"] != e["exit"]:
        return "%s: left the distortion loop by %d" % (c.name, t0["exit_how"])
    if "n_outer" in e and t0["n_outer"] != e["n_outer"]:
        return "%s: %d iterations" % (c.name, t0["n_outer"])
    if "maxima" in e:
        sf = r.side[0]["gr"][0][0]["scalefac"]
        short = r.side[0]["gr"][0][0]["block_type"] == 2
        got = (int(sf[:18].max()), int(sf[18:36].max())) if short else (int(sf[:11].max()), int(sf[11:21].max()))
        if got != tuple(e["maxima"]):
            return "%s: maxima %s" % (c.name, got)
    if "fired" in e and bool(t0["pre_iter"]) != e["fired"]:
        return "%s: pre-emphasis fired in iteration %d" % (c.name, t0["pre_iter"])
    if "inherit" in e:
        g = r.side[0]["gr"][1]
        for ch in range(2):
            if t[0, 1, ch]["scfsi_mask"] == 0 or t[0, 1, ch]["pre_iter"] or t[0, 1, ch]["n_outer"] < 2 or int(g[ch]["preflag"]) != e["inherit"]:
                return "%s: granule 1 channel %d mask %d, %d iterations, preflag %d" % (c.name, ch, t[0, 1, ch]["scfsi_mask"], t[0, 1, ch]["n_outer"], g[ch]["preflag"])
    if e.get("masks") is not None:
        f = e.get("frame", 0)
        got = tuple(int(t[f, 1, ch]["scfsi_mask"]) for ch in range(c.channels))
        if got != tuple(e["masks"]):
            return "%s: scfsi masks %s" % (c.name, got)
    if e.get("more_iterations") and not (t[0, 1, 0]["n_outer"] > 1 and t[0, 1, 0]["scfsi_mask"]):
        return "%s: granule 1 ran %d iterations" % (c.name, t[0, 1, 0]["n_outer"])
    if e.get("drain") and not r.side["resvDrain"].max() > 0:
        return "%s: nothing drained" % c.name
    if "stuffed" in e and int(r.side[0]["gr"][0][0]["part2_3_length"]) != min(e["stuffed"], 4095):
        return "%s: part2_3_length[0][0] %d" % (c.name, r.side[0]["gr"][0][0]["part2_3_length"])
    if e.get("apart") and (t0["bisect_equal"] or t0["n_probes"] < 3 or abs(int(t0["probe_last"]) - int(t0["probe_prev"])) != 1):
        return "%s: the bisection ended on probes %d, %d" % (c.name, t0["probe_prev"], t0["probe_last"])
    if "more_bits" in e:
        got = [int(x) for x in t[e["more_bits"][0]]["more_bits"].ravel()]
        if got != list(e["more_bits"][1]):
            return "%s: more_bits %s" % (c.name, got)
    if e.get("bisect_equal") and not t0["bisect_equal"]:
        return "%s: no probe counted max_bits" % c.name
    if e.get("steps") and not t0["n_passes"] - t0["n_probes"] > 2 * t0["n_outer"]:
        return "%s: %d passes in %d iterations" % (c.name, t0["n_passes"], t0["n_outer"])
    if "status" in e and (r.status & 255, r.status >> 8) != (e["status"] & 255, e["status"] >> 8):
        return "%s: status %#x" % (c.name, r.status)
    if "q0" in e and t0["q0"] != e["q0"]:
        return "%s: q0 %d" % (c.name, t0["q0"])
    if "gain" in e and int(r.side[0]["gr"][1][0]["global_gain"]) != e["gain"]:
        return "%s: global_gain" % c.name
    return None


def reached(pairs):
    """what the chains of `pairs` (chain, oracle's Result) reached between them, as the tests assert it: a dict of sets"""
    got = {"inside_violates": set(), "inside_violates_it2": set(), "inside_violates_pre": set(), "clamp_4095": False, "one_step_apart": False, "exits": set(), "compress": set(), "fired": set(), "mask_bits": set(), "add_branch": set(), "drain": False,
           "bisect_equal": False, "aborts": set(), "more_iterations": False}
    for c, r in pairs:
        t0 = r.trace[0, 0, 0]
        # (the decision of the iteration the chain was built for: run_oracle keeps that one's noise and thresholds)
        if c.set == "L1" and c.expect.get("close") and c.expect["band"] >= 0:
            b = c.expect["band"]
            assert t0["kept_iter"] == 1, c.name
            if c.expect.get("pre"):
                got["inside_violates_pre"].add(bool(t0["xfsf"][b] > t0["xmin_pre"][b]))
            else:
                got["inside_violates"].add(bool(t0["xfsf"][b] > t0["xmin"][b]))
        if c.set == "L1" and c.expect.get("close") and c.expect["band"] == -2:
            assert t0["kept_iter"] == 2, c.name
            got["inside_violates_it2"] |= {bool(t0["xfsf"][b] > t0["xmin"][b]) for b in c.expect["bands"]}
        if c.set == "L2":
            got["exits"].add(int(t0["exit_how"]))
            got["compress"].add(int(r.side[0]["gr"][0][0]["scalefac_compress"]))
        if c.set == "L3":
            got["fired"].add(bool(t0["pre_iter"]))
        if c.set == "L4":
            for t in r.trace[:, 1].ravel():
                got["mask_bits"] |= {(b, int(t["scfsi_mask"]) >> b & 1) for b in range(4)}
                got["more_iterations"] |= bool(t["scfsi_mask"] and t["n_outer"] > 1)
        if c.set == "L5":
            got["add_branch"] |= {int(x) & 3 for x in r.trace["add_branch"].ravel()}
            got["clamp_4095"] |= bool((r.trace["add_branch"] & 4).any())
            got["drain"] |= bool(r.side["resvDrain"].max() > 0)
        if c.set in ("L6", "L7"):
            got["bisect_equal"] |= bool(r.trace["bisect_equal"].max())
            got["one_step_apart"] |= bool(c.expect.get("apart") and not t0["bisect_equal"] and abs(int(t0["probe_last"]) - int(t0["probe_prev"])) == 1)
            if r.status:
                got["aborts"].add(r.status & 255)
    return got
