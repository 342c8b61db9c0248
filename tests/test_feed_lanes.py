"""A feeder with more lanes than slots (mp3mi_feed_create_lanes / mp3mi_feed_tick_lanes, include/mp3mi.h): a lane owns its FIFO and
its parked record, a slot is lent to a lane for the ticks in which it encodes; with more ready lanes than slots those that have been
ready for longest encode.  The judge is the oracle, as in test_feed.py: the bytes a LANE delivered from its stream's START through
the tick that closed it -- gathered slot by slot through the tick's slot_lane_host -- concatenated, are the oracle's file of the
stream's samples at its bitrate, exactly.  A Python model of the rules (Model) runs beside the library: after every tick
mp3mi_feed_lanes, mp3mi_batch_slot_frames, mp3mi_batch_slot_kbps and slot_lane_host must say what it says."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from golden_util import aborting_cases, case_pcm
from mp3common import ERR_REFERENCE_ABORT, ROOT
from test_feed import FeedRun
from test_feed import bind as bind_feed
from test_slot_park import Stream, attacks_pcm, chunked, oracle_exact
from test_stream_slots import END, START, SlotRun

ERR_ARG = -1
PARKED, DRAINING, WAITING, WAIT_SLOT = 1, 2, 4, 8  # mp3mi_feed_lanes flags
SIZES = (1, 7, 959, 960, 1152, 2303)  # push sizes, and max_push


def bind(mp):
    L = bind_feed(mp)
    L.mp3mi_feed_create_lanes.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p] + [ctypes.c_int] * 5
    L.mp3mi_feed_n_lanes.argtypes = [ctypes.c_void_p]
    L.mp3mi_feed_tick_lanes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    return L


class MLane:
    def __init__(self):
        self.open, self.pending, self.frames, self.kbps = False, 0, -1, 0
        self.parked = self.draining = self.waiting = self.wait_slot = False
        self.slot, self.since = -1, -1


class Model:
    """what mp3mi.h says of lanes and slots; no library involved.  tick() returns [(lane, slot, closes, started)] of the lanes that
    encode and keeps the history the tests ask about"""

    def __init__(self, S, L, tick_frames, cap, slot_kbps):
        self.S, self.L, self.tick_frames, self.full, self.cap, self.slot_kbps = S, L, tick_frames, tick_frames * 1152, cap, list(slot_kbps)
        self.lane = [MLane() for _ in range(L)]
        self.slot_lane = [-1] * S
        self.t = 0
        # history: ticks with more ready lanes than slots; lanes that waited for a slot while ready; slots a lane's current stream
        # encoded in; slots vacated and refilled in one tick, by an import and by a START
        self.over, self.waited, self.slots_of = 0, set(), [set() for _ in range(L)]
        self.refill_import = self.refill_start = self.parks = self.resumes = 0
        self.moved = False  # some stream encoded in two different slots
        self.log = []       # per tick ({ready lane: the tick its spell began}, the lanes that encode)

    def tick(self, feeds):
        """feeds: {lane: (ctl, n, kbps)}"""
        ln_ready = []
        closes = {}
        for i, l in enumerate(self.lane):
            c, n, k = feeds.get(i, (0, 0, 0))
            if c & START:
                l.open, l.pending, l.frames, l.kbps = True, 0, 0, k
                l.parked = l.draining = False
                l.waiting = True
                self.slots_of[i] = set()
            if not l.open:
                assert n == 0 and not c & END
                continue
            l.pending += n
            assert l.pending <= self.cap, "the plan overruns lane %d's ring" % i
            l.draining |= bool(c & END)
            closes[i] = l.draining and l.pending <= self.full
            if closes[i] or l.pending >= self.full:
                if l.since < 0:
                    l.since = self.t
                ln_ready.append(i)
            else:
                l.since = -1
                l.wait_slot = False
        self.over += len(ln_ready) > self.S
        chosen = sorted(sorted(ln_ready, key=lambda i: (self.lane[i].since, i))[:self.S])
        self.log.append(({i: self.lane[i].since for i in ln_ready}, chosen))
        vacated = set()
        for s in range(self.S):  # every stream in a slot whose lane does not encode leaves
            i = self.slot_lane[s]
            if i >= 0 and i not in chosen:
                l = self.lane[i]
                l.parked, l.slot, self.slot_lane[s] = not l.waiting, -1, -1
                vacated.add(s)
                self.parks += 1
        free = [s for s in range(self.S) if self.slot_lane[s] < 0]
        out = []
        for i in ln_ready:
            l = self.lane[i]
            if i not in chosen:
                l.wait_slot = True
                self.waited.add(i)
                continue
            if l.slot < 0:
                l.slot = free.pop(0)
                self.resumes += l.parked
                if l.slot in vacated:
                    self.refill_import += l.parked
                    self.refill_start += l.waiting
            s, started = l.slot, l.waiting
            if started and l.kbps == 0:
                l.kbps = self.slot_kbps[s]
            take = l.pending if closes[i] else self.full
            l.pending -= take
            l.frames += (take + 1151) // 1152 if closes[i] else self.tick_frames
            l.parked = l.waiting = l.wait_slot = False
            l.since = -1
            self.slots_of[i].add(s)
            self.moved |= len(self.slots_of[i]) > 1
            self.slot_lane[s] = i
            out.append((i, s, closes[i], started))
        for i, s, c, _ in out:
            if c:
                l = self.lane[i]
                l.open, l.frames, l.slot, self.slot_lane[s] = False, -1, -1, -1
        self.t += 1
        return out

    def flags(self):
        return [(PARKED * l.parked | DRAINING * l.draining | WAITING * l.waiting | WAIT_SLOT * l.wait_slot) if l.open else 0 for l in self.lane]


class LaneRun(SlotRun):
    """a slot batch with a feeder of n_lanes lanes, driven tick by tick beside the Model"""

    def __init__(self, mp, S, n_lanes, rate, ch, kbps, tick, max_push, max_rows=None, ring=0, **kw):
        SlotRun.__init__(self, mp, S, rate, ch, kbps, tick, **kw)
        bind(mp)
        self.n_lanes, self.tick_frames, self.full, self.max_push = n_lanes, tick, tick * 1152, max_push
        self.max_rows = n_lanes if max_rows is None else max_rows
        self.f = ctypes.c_void_p()
        assert self.L.mp3mi_feed_create_lanes(ctypes.byref(self.f), self.b, n_lanes, self.max_rows, tick, max_push, ring) == 0
        self.cap = ring if ring else self.full + max_push
        assert self.L.mp3mi_feed_capacity(self.f) == self.cap and self.L.mp3mi_feed_n_lanes(self.f) == n_lanes
        self.pitch = max_push + 3  # (rows that begin at every alignment)
        self.d_push = self.mem.alloc(self.max_rows * self.pitch * ch * 2)
        self.m = Model(S, n_lanes, tick, self.cap, self.kbps)
        self.st = [None] * n_lanes  # the Stream in each lane
        self.ticks, self.aborts, self.order = 0, [], []

    def lanes(self):
        n = self.n_lanes
        p, f, g = np.full(n, -7, np.int32), np.full(n, -7, np.int64), np.full(n, 77, np.uint8)
        k = self.L.mp3mi_feed_lanes(self.f, p.ctypes.data, f.ctypes.data, g.ctypes.data)
        return list(p), list(f), list(g), k

    def check_books(self):
        ml = self.m.lane
        p, f, g, n = self.lanes()
        assert n == sum(l.open for l in ml)
        assert p == [l.pending if l.open else 0 for l in ml], p
        assert f == [l.frames for l in ml], f
        assert g == self.m.flags(), (g, self.m.flags())
        sl = self.m.slot_lane
        assert list(self.frames()) == [ml[i].frames if i >= 0 else -1 for i in sl], (list(self.frames()), sl)
        k = np.full(self.S, -7, np.int32)
        assert self.L.mp3mi_batch_slot_kbps(self.b, k.ctypes.data) == max(self.kbps)
        assert list(k) == [ml[i].kbps if i >= 0 else self.kbps[s] for s, i in enumerate(sl)], list(k)

    def raw_tick(self, rows=(), ctl=(), n_push=(), kbps=(), pcm=True, out=True, out_len=True, sl=True, stride=None, pitch=None, f=True,
                 null=(), n_rows=None):
        """one mp3mi_feed_tick_lanes call as given; null: names of row arrays to pass as NULL.  Returns (rc, slot_lane)"""
        arr = dict(rows=np.ascontiguousarray(rows, np.int32), ctl=np.ascontiguousarray(ctl, np.uint8),
                   n_push=np.ascontiguousarray(n_push, np.int32), kbps=np.ascontiguousarray(kbps, np.int32))
        R = len(arr["rows"]) if n_rows is None else n_rows
        ptr = {k: (None if k in null or (R == 0 and n_rows is None) else a.ctypes.data) for k, a in arr.items()}
        slot_lane = np.full(self.S, -9, np.int32)
        rc = self.L.mp3mi_feed_tick_lanes(self.f if f else None, R, ptr["rows"], self.d_push if pcm else None,
                                          self.pitch if pitch is None else pitch, ptr["ctl"], ptr["n_push"], ptr["kbps"],
                                          self.d_out if out else None, self.stride if stride is None else stride,
                                          self.d_len if out_len else None, slot_lane.ctypes.data if sl else None)
        for a in arr.values():
            a[...] = 99  # (the library has copied them)
        return rc, slot_lane

    def tick(self, feeds, kbps0=False, sync=True):
        """feeds: {lane: (stream, ctl, n)} -- stream: the lane's (a new one with START).  Books the bytes every lane delivered and
        returns [(lane, slot)] of the lanes that encoded.  A sync that reports an abort is booked in self.aborts."""
        ch = self.ch
        rows = sorted(feeds)
        assert len(rows) <= self.max_rows
        pcm = np.full((self.max_rows, self.pitch * ch), 0x5A5A, np.int16)
        ctl, ns, kb, mfeeds = [], [], [], {}
        for r, i in enumerate(rows):
            st, c, n = feeds[i]
            assert (c & START) or self.st[i] is st
            if c & START:
                self.st[i] = st
            k = st.kbps if (c & START) and not kbps0 else 0
            ctl.append(c), ns.append(n), kb.append(k)
            mfeeds[i] = (c, n, k)
            pcm[r, :n * ch] = st.take(n)
        self.mem.upload(self.d_push, pcm)
        rc, slot_lane = self.raw_tick(rows, ctl, ns, kb)
        assert rc == 0, rc
        enc = self.m.tick(mfeeds)
        self.ticks += 1
        want = [-1] * self.S
        for i, s, closes, started in enc:
            want[s] = i
            self.st[i].frames = self.m.lane[i].frames
            if started:
                self.st[i].kbps = self.m.lane[i].kbps  # (kbps 0: the create-time bitrate of the slot it first encodes in)
        assert list(slot_lane) == want, (list(slot_lane), want)
        self.order.append(sorted(i for i, _, _, _ in enc))
        if not sync:
            return enc
        rc = self.L.mp3mi_batch_sync(self.b)
        assert rc in (0, ERR_REFERENCE_ABORT), rc
        if rc:
            self.aborts.append((self.ticks - 1, list(slot_lane)))
        outs, lens = self.outputs()
        for i, s, closes, _ in enc:
            self.st[i].calls.append(outs[s])
        assert all(lens[s] == 0 for s in range(self.S) if want[s] < 0), list(lens)
        self.check_books()
        for i, s, closes, _ in enc:
            if closes:
                self.st[i] = None
        return [(i, s) for i, s, _, _ in enc]

    def close(self, feeder_first=True):
        if self.f and feeder_first:
            self.L.mp3mi_feed_destroy(self.f)
        self.f = ctypes.c_void_p()
        SlotRun.close(self)


def cuts(n, sizes, max_push):
    """n samples cut into pushes that walk through `sizes`"""
    out, k = [], 0
    while n > 0:
        out.append(min(n, max_push, sizes[k % len(sizes)]))
        n -= out[-1]
        k += 1
    return out


def churn(run, plans, limit=90):
    """plans: {lane: (first tick, stream, [pushes])}: from its first tick on a lane pushes its next piece in every tick in which its
    ring has room for it (a waiting lane's ring fills up: the server holds the packet back), the first with START, the last with END.
    A first tick of None: the stream is open in the lane already, no START.  Ticks until every lane has closed."""
    todo = {i: [t0 or 0, st, list(p), t0 is not None] for i, (t0, st, p) in plans.items()}
    while todo or any(l.open for l in run.m.lane):
        feeds = {}
        for i in sorted(todo):
            t0, st, p, first = todo[i]
            if run.ticks < t0 or (not first and run.m.lane[i].pending + p[0] > run.cap):
                continue
            n = p.pop(0)
            feeds[i] = (st, (START if first else 0) | (0 if p else END), n)
            todo[i][3] = False
            if not p:
                del todo[i]
        run.tick(feeds)
        assert run.ticks < limit


def stream(mp, run, seed, frames, odd, kbps=None, pcm=None):
    """a stream of `frames` frames less `odd` samples: its length is no multiple of 1152"""
    n = frames * 1152 - odd
    assert n % 1152 != 0
    pcm = mp.synth(frames * 1152, run.ch, run.rate, seed) if pcm is None else pcm
    return Stream(pcm[:n * run.ch], run.ch, run.kbps[0] if kbps is None else kbps), n


# ---- 1. oversubscribed cuts ----
def oversubscribed_case(mp, oracle):
    max_push = 2304
    run = LaneRun(mp, 2, 7, 44100, 2, 128, 1, max_push, ring=1152 + max_push + 1000)
    try:
        sizes = SIZES + (max_push,)
        plans, streams = {}, []
        for i, (t0, frames, odd) in enumerate([(0, 5, 37), (0, 4, 1), (0, 6, 500), (1, 3, 1151), (1, 9, 7), (2, 4, 333), (3, 5, 960)]):
            st, n = stream(mp, run, 700 + i, frames, odd, pcm=attacks_pcm(mp) if i == 0 else None)
            rot = sizes[i:] + sizes[:i]
            plans[i] = (t0, st, [1152] + cuts(n - 1152, rot, max_push))  # (a whole tick at START: ready at once, more lanes than slots)
            streams.append(st)
        churn(run, plans)
        m = run.m
        # the schedule exercises the feature: conditions on the input, from the model alone
        assert m.over > 0, "no tick with more ready lanes than slots"
        assert m.waited == set(range(7)), m.waited
        assert m.moved, "no stream encoded in two different slots"
        assert m.refill_import > 0 and m.refill_start > 0, (m.refill_import, m.refill_start)
        assert all(st.pos * 2 == len(st.pcm) for st in streams)
        oracle_exact(oracle, run, streams)
    finally:
        run.close()


def test_oversubscribed_cuts_emulated(emu, oracle):
    oversubscribed_case(emu, oracle)


# ---- 2. fairness ----
def fairness_case(mp, oracle):
    """five lanes that always have a tick pending, two slots.  Tick 0: all begin their spell, 0 and 1 encode (the lower lanes).  Tick 1:
    0 and 1 begin a new spell, 2 and 3 encode.  Tick 2: 4 (spell 0) and, of 0 and 1 (spell 1), 0.  Tick 3: 1 (spell 1) and, of 2 and 3
    (spell 2), 2.  Tick 4: 3 (spell 2) and, of 0 and 4 (spell 3), 0: the round robin the rule gives -- by spell, ties to the lower
    lane.  Throughout, no lane encodes while a lane whose spell began earlier waits."""
    run = LaneRun(mp, 2, 5, 44100, 2, 128, 1, 1152)
    try:
        plans, streams = {}, []
        for i in range(5):
            st, n = stream(mp, run, 720 + i, 5, 100 + i)
            plans[i] = (0, st, cuts(n, (1152,), 1152))
            streams.append(st)
        churn(run, plans)
        assert run.order[:5] == [[0, 1], [2, 3], [0, 4], [1, 2], [0, 3]], run.order[:5]
        assert all(len(ready) == 5 for ready, _ in run.m.log[:8])  # every lane ready in every tick
        for ready, chosen in run.m.log:
            assert all(ready[j] >= ready[i] for i in chosen for j in ready if j not in chosen), (ready, chosen)
        served = [i for t in run.order for i in t]
        for i in range(5):  # between two services of a lane, every lane that waited all the while is served
            t = [k for k, o in enumerate(run.order[:8]) if i in o]
            assert all(t2 - t1 <= 3 for t1, t2 in zip(t, t[1:])) and t[0] <= 2, (i, t)
        assert all(served.count(i) == 5 for i in range(5)), served  # four frames and a partial one each
        oracle_exact(oracle, run, streams)
    finally:
        run.close()


def test_fairness_emulated(emu, oracle):
    fairness_case(emu, oracle)


# ---- 3. formats and bitrates ----
def format_case(mp, oracle, rate, ch, kbps, mode=None, crc=False, omode=None):
    run = LaneRun(mp, 2, 5, rate, ch, kbps, 2, 2304, mode=mode, crc=crc)
    try:
        plans, streams = {}, []
        for i, (t0, frames, odd) in enumerate([(0, 5, 3), (0, 4, 959), (0, 3, 1), (1, 6, 77), (2, 4, 1000)]):
            st, n = stream(mp, run, 740 + i, frames, odd)
            plans[i] = (t0, st, [2304] + cuts(n - 2304, (960, 2303, 7, 2304, 1), 2304))
            streams.append(st)
        churn(run, plans)
        assert run.m.over > 0 and run.m.moved and run.m.resumes > 0
        oracle_exact(oracle, run, streams, mode=omode)
    finally:
        run.close()


def bitrates_case(mp, oracle):
    """a batch with ceiling 320 whose slots were created at 320, 96 and 160; lanes START at 64 / 128 / 192 / 320 -- and one at kbps 0,
    the create-time bitrate of the slot it first encodes in -- and migrate between the slots"""
    run = LaneRun(mp, 3, 7, 44100, 2, [320, 96, 160], 1, 2304)
    try:
        plans, streams = {}, []
        for i, (t0, frames, odd, kbps) in enumerate([(0, 5, 3, 64), (0, 4, 959, 128), (0, 3, 1, 192), (0, 6, 77, 320), (1, 4, 1000, 64),
                                                     (1, 5, 576, 320), (2, 4, 11, 128)]):
            st, n = stream(mp, run, 760 + i, frames, odd, kbps=kbps)
            plans[i] = (t0, st, [1152] + cuts(n - 1152, (960, 1152, 2303, 7), 2304))
            streams.append(st)
        churn(run, plans)
        m = run.m
        assert m.over > 0 and m.moved and m.refill_import > 0
        oracle_exact(oracle, run, streams)
        # kbps 0: lanes 0 and 1 take slots 0 and 1 and with them 320 and 96
        a, _ = stream(mp, run, 770, 3, 5)
        b, _ = stream(mp, run, 771, 3, 6)
        assert run.tick({0: (a, START, 1152), 1: (b, START, 1152)}, kbps0=True) == [(0, 0), (1, 1)]
        assert (a.kbps, b.kbps) == (320, 96)
        churn(run, {0: (None, a, [2 * 1152 - 5]), 1: (None, b, [2 * 1152 - 6])})
        oracle_exact(oracle, run, [a, b])
    finally:
        run.close()


def test_formats_and_bitrates_emulated(emu, oracle):
    format_case(emu, oracle, 32000, 1, 56)
    format_case(emu, oracle, 48000, 2, 192, mode=2, crc=True, omode="de")
    bitrates_case(emu, oracle)


# ---- 4. sticky slots ----
def sticky_case(mp, oracle):
    """as many lanes as slots push exactly a tick every tick and one more lane is never ready: nobody moves"""
    run = LaneRun(mp, 2, 3, 44100, 2, 128, 1, 1152)
    try:
        a, na = stream(mp, run, 780, 5, 100)
        b, nb = stream(mp, run, 781, 5, 200)
        c, _ = stream(mp, run, 782, 1, 500)
        for t in range(4):
            first = START if t == 0 else 0
            feeds = {0: (a, first, 1152), 2: (b, first, 1152)}
            if t in (0, 2):
                feeds[1] = (c, first, 7 if t == 0 else 645 - 7)
            assert run.tick(feeds) == [(0, 0), (2, 1)]
            assert not any(g & (PARKED | WAIT_SLOT) for g in run.lanes()[2])
        assert run.m.parks == 0 and run.m.resumes == 0 and run.lanes()[2][1] == WAITING
        assert run.tick({0: (a, END, na - 4 * 1152), 2: (b, END, nb - 4 * 1152)}) == [(0, 0), (2, 1)]
        assert run.tick({1: (c, END, 0)}) == [(1, 0)]
        assert run.lanes()[3] == 0 and run.m.parks == 0
        oracle_exact(oracle, run, [a, b, c])
    finally:
        run.close()


def test_sticky_slots_emulated(emu, oracle):
    sticky_case(emu, oracle)


# ---- 5. draining, one-call files, abandoned streams ----
def draining_case(mp, oracle):
    """one slot, three lanes.  Lanes 0 and 1 END with several ticks pending and take turns in the slot while they drain; lane 2
    delivers one-call files, one of no samples at all"""
    run = LaneRun(mp, 1, 3, 48000, 2, 192, 1, 2400, ring=1152 + 2400 + 2304)
    try:
        a, na = stream(mp, run, 790, 5, 1147)  # 2304 + 2309
        b, nb = stream(mp, run, 791, 3, 152)   # 2304 + 1000
        one, n1 = stream(mp, run, 792, 1, 452)
        none = Stream(np.zeros(0, np.int16), 2, 192)
        assert run.tick({0: (a, START, 2304), 1: (b, START, 2304)}) == [(0, 0)]
        assert run.lanes()[2] == [0, WAITING | WAIT_SLOT, 0]
        assert run.tick({0: (a, END, na - 2304)}) == [(1, 0)]  # lane 1 was ready first; lane 0 drains, parked and waiting
        assert run.lanes()[:3] == ([3461, 1152, 0], [1, 1, -1], [PARKED | DRAINING | WAIT_SLOT, 0, 0])
        assert run.tick({1: (b, END, nb - 2304), 2: (one, START | END, n1)}) == [(0, 0)]
        assert run.lanes()[2] == [DRAINING, PARKED | DRAINING | WAIT_SLOT, DRAINING | WAITING | WAIT_SLOT]
        assert run.tick({}) == [(1, 0)]
        assert run.tick({}) == [(2, 0)]  # the one-call file waited two ticks for the slot
        assert run.tick({2: (none, START | END, 0)}) == [(0, 0)]
        assert run.lanes()[2][2] == DRAINING | WAITING | WAIT_SLOT
        churn(run, {})
        assert (a.pos, b.pos, one.pos) == (na, nb, n1) and run.lanes()[3] == 0
        oracle_exact(oracle, run, [a, b, one])
        # a stream without samples is an EMPTY file in this library (mp3mi.h: mp3mi_batch_encode_ragged, "0 for a stream without samples",
        # and the per-slot call's START | END with 0 samples), where the oracle writes the reference's closing byte
        assert len(none.calls) == 1 and none.data() == b"" and oracle.encode(none.fed(), run.rate, 192, 2)[0] == b"\x00"
    finally:
        run.close()


def abandoned_case(mp, oracle):
    """a lane's stream abandoned by a new START while it waits for a slot, while it is parked and while it sits in a slot -- with the
    new stream ready at once (the START goes to that slot) and not ready (the slot is vacated)"""
    run = LaneRun(mp, 2, 4, 44100, 2, 128, 1, 1152)
    try:
        def s(seed, frames=3, odd=9):
            return stream(mp, run, seed, frames, odd)[0]

        a, b, c, c2, a2, a3, a4 = s(800), s(801, 6), s(802), s(803, 4), s(804), s(805), s(806, 2)
        assert run.tick({0: (a, START, 1152), 1: (b, START, 1152), 2: (c, START, 1152)}) == [(0, 0), (1, 1)]
        assert run.lanes()[2][2] == WAITING | WAIT_SLOT
        # c is abandoned while it waits for a slot; lane 0 sits out, and lane 2 STARTs in the slot it leaves
        assert run.tick({0: (a, 0, 100), 1: (b, 0, 1152), 2: (c2, START, 1152)}) == [(1, 1), (2, 0)]
        assert run.lanes()[2][0] == PARKED and run.m.refill_start == 1
        # a is abandoned while it is parked
        assert run.tick({0: (a2, START, 1152), 1: (b, 0, 1152), 2: (c2, 0, 1152)}) == [(0, 0), (1, 1)]
        assert run.lanes()[2][2] == PARKED | WAIT_SLOT
        # a2 is abandoned in its slot for a stream that is ready: the START goes there; lane 1 sits out and lane 2 resumes in its slot
        assert run.tick({0: (a3, START, 1152)}) == [(0, 0), (2, 1)]
        assert run.m.refill_import == 1 and run.lanes()[2][1] == PARKED
        # a3 is abandoned in its slot for a stream that is not ready: the slot is vacated, the lane waits for samples
        assert run.tick({0: (a4, START, 10), 1: (b, 0, 1152), 2: (c2, 0, 1152)}) == [(1, 0), (2, 1)]
        assert run.lanes()[2][0] == WAITING and list(run.frames()) == [4, 3]
        churn(run, {0: (None, a4, [1142, 1143]), 1: (None, b, [1152, 1143]), 2: (None, c2, [1143])})
        assert (len(a.calls), len(c.calls), len(a2.calls), len(a3.calls)) == (1, 0, 1, 1)  # nothing of them after their lanes' next START
        oracle_exact(oracle, run, [b, c2, a4])
    finally:
        run.close()


def test_draining_emulated(emu, oracle):
    draining_case(emu, oracle)


def test_abandoned_streams_emulated(emu, oracle):
    abandoned_case(emu, oracle)


# ---- 6. a void stream ----
def void_case(mp, oracle):
    """abort_global_gain dies in frame 4.  It sits in lane 1 of four lanes on two slots, all of which push a tick every tick and so
    migrate: one sync reports the abort, the status of that tick's slot names lane 1, the lane delivers nothing afterwards, and the
    good lanes are the oracle's"""
    case = [c for c in aborting_cases() if c["name"] == "abort_global_gain"][0]
    bad_pcm = np.concatenate([case_pcm(case, mp.synth), np.zeros(2 * 1152 * 2, np.int16)])  # 6 frames, then silence
    run = LaneRun(mp, 2, 4, 44100, 2, 128, 2, 2304)
    try:
        good = [stream(mp, run, 810 + i, 8, 10 + i) for i in range(3)]
        bad = Stream(bad_pcm, 2, 128)
        plans = {0: (0, good[0][0], cuts(good[0][1], (2304,), 2304)), 1: (0, bad, [2304, 2304, 2304, 2304 - 99]),
                 2: (0, good[1][0], cuts(good[1][1], (2304,), 2304)), 3: (1, good[2][0], cuts(good[2][1], (2304,), 2304))}
        frame = case["reference_aborts"]["frame"]
        want = case["reference_aborts"]["status"] | frame << 8
        status_seen = []
        tick = run.tick

        def watched(feeds, **kw):
            before = run.m.lane[1].frames
            enc = tick(feeds, **kw)
            if run.aborts and not status_seen:
                status_seen.append((before, dict(enc), list(run.status())))
            return enc

        run.tick = watched
        churn(run, plans)
        assert run.m.moved and run.m.resumes > 0
        assert len(run.aborts) == 1, run.aborts  # one sync, however often the void stream moved afterwards
        before, enc, status = status_seen[0]
        t, slot_lane = run.aborts[0]
        assert 1 in enc and before <= frame < before + 2  # the tick in which lane 1 encoded the frame the reference dies in
        assert status[enc[1]] == want and slot_lane[enc[1]] == 1
        n_before = (frame // 2) + 1
        assert len(bad.calls) == 4 and all(c == b"" for c in bad.calls[n_before - 1:]), [len(c) for c in bad.calls]
        oracle_exact(oracle, run, [g[0] for g in good])
    finally:
        run.close()


def test_void_stream_emulated(emu, oracle):
    void_case(emu, oracle)


# ---- 7. rules ----
def rules_case(mp, oracle):
    L = bind(mp)
    probe = SlotRun(mp, 2, 44100, 2, 128, 2)
    try:
        f = ctypes.c_void_p()
        #                 n_lanes, max_rows, tick_frames, max_push, ring_samples
        for args in [(0, 1, 1, 100, 0), (5, 0, 1, 100, 0), (5, 6, 1, 100, 0), (5, 5, 0, 100, 0), (5, 5, 3, 100, 0), (5, 5, 1, 0, 0),
                     (5, 5, 1, 100, 1251), (5, 5, 1, 100, -1), (5, 5, 1, 100, 2 ** 31 - 1), (-1, 1, 1, 100, 0)]:
            assert L.mp3mi_feed_create_lanes(ctypes.byref(f), probe.b, *args) == ERR_ARG and not f.value, args
        assert L.mp3mi_feed_create_lanes(None, probe.b, 5, 5, 1, 100, 0) == ERR_ARG
        assert L.mp3mi_feed_create_lanes(ctypes.byref(f), None, 5, 5, 1, 100, 0) == ERR_ARG
        pcm = np.zeros((2, probe.row), np.int16)
        assert probe.call(pcm, [START, 0], [2304, 0]) == 0  # a stream is open
        assert L.mp3mi_feed_create_lanes(ctypes.byref(f), probe.b, 5, 5, 1, 100, 0) == ERR_ARG
        assert L.mp3mi_batch_reset(probe.b) == 0
        assert L.mp3mi_feed_create_lanes(ctypes.byref(f), probe.b, 1, 1, 2, 100, 2404) == 0  # fewer lanes than slots, the least ring given
        g = ctypes.c_void_p()
        assert L.mp3mi_feed_create_lanes(ctypes.byref(g), probe.b, 5, 5, 1, 100, 0) == ERR_ARG  # one feeder per batch
        assert L.mp3mi_feed_create(ctypes.byref(g), probe.b, 1, 100) == ERR_ARG
        assert L.mp3mi_feed_n_lanes(f) == 1 and L.mp3mi_feed_n_lanes(None) == 0 and L.mp3mi_feed_capacity(f) == 2404
        L.mp3mi_feed_destroy(f)
        # each kind of feeder has its own tick
        assert L.mp3mi_feed_create(ctypes.byref(f), probe.b, 1, 100) == 0 and L.mp3mi_feed_n_lanes(f) == 2
        z8, z32, sl = np.zeros(2, np.uint8), np.zeros(2, np.int32), np.zeros(2, np.int32)
        d = probe.mem.alloc(2 * 103 * 2 * 2)
        assert L.mp3mi_feed_tick_lanes(f, 0, None, None, 0, None, None, None, probe.d_out, probe.stride, probe.d_len, sl.ctypes.data) == ERR_ARG
        assert L.mp3mi_feed_tick(f, d, 103, z8.ctypes.data, z32.ctypes.data, None, probe.d_out, probe.stride, probe.d_len) == 0
    finally:
        probe.close()  # (the batch goes with the feeder attached)

    run = LaneRun(mp, 1, 4, 44100, 2, 128, 1, 2400, max_rows=3)
    try:
        (a, na), (d, nd), (w, nw) = (stream(mp, run, 820 + i, 4, 3 + 2 * i) for i in range(3))
        # lane 0 parked and waiting for the slot with 2400 pending, lane 1 in the slot with 2400 pending, lane 2 closed, lane 3 not
        # yet in the batch, waiting for the slot with a full ring
        assert run.tick({0: (a, START, 1152), 1: (d, START, 1152), 3: (w, START, 1152)}) == [(0, 0)]
        assert run.tick({0: (a, 0, 2400), 1: (d, 0, 2400), 3: (w, 0, 2400)}) == [(1, 0)]
        assert run.lanes()[:3] == ([2400, 2400, 0, 3552], [1, 1, -1, 0], [PARKED | WAIT_SLOT, 0, 0, WAITING | WAIT_SLOT])
        assert L.mp3mi_feed_tick(run.f, run.d_push, run.pitch, np.zeros(4, np.uint8).ctypes.data, None, None, run.d_out, run.stride, run.d_len) == ERR_ARG

        def tick(rows=(0, 2, 3), ctl=(0, 0, 0), n=(0, 0, 0), kbps=(0, 0, 0), **kw):
            return run.raw_tick(rows, ctl, n, kbps, **kw)[0]

        def refused(calls):
            for k, call in enumerate(calls):
                assert call() == ERR_ARG, k
                run.check_books()

        refused([
            lambda: tick(ctl=(0, 4, 0)), lambda: tick(ctl=(8, 0, 0)),                    # unknown ctl bits
            lambda: tick(n=(0, 5, 0)), lambda: tick(ctl=(0, END, 0)),                    # a closed lane without START
            lambda: tick(n=(-1, 0, 0)), lambda: tick(n=(0, 2401, 0), ctl=(0, START, 0)),
            lambda: tick(n=(1153, 0, 0)),                                                # 2400 + 1153 > 1152 + 2400
            lambda: tick(n=(0, 0, 1)),                                                   # the waiting lane's ring is full
            lambda: tick(pcm=False), lambda: tick(out=False), lambda: tick(out_len=False), lambda: tick(sl=False), lambda: tick(f=False),
            lambda: tick(null=("rows",)), lambda: tick(null=("ctl",)), lambda: tick(null=("n_push",)), lambda: tick(null=("kbps",)),
            lambda: tick(stride=run.stride - 1), lambda: tick(pitch=2399),
            lambda: tick(ctl=(0, START, 0), kbps=(0, 100, 0)),                           # no Layer III bitrate
            lambda: tick(ctl=(0, START, 0), kbps=(0, 160, 0)),                           # above the ceiling of a batch created at 128
            lambda: tick(kbps=(64, 0, 0)), lambda: tick(kbps=(0, 128, 0)),               # not the open stream's / nothing open
            lambda: tick(rows=(0, 3, 2)), lambda: tick(rows=(0, 2, 2)), lambda: tick(rows=(0, 2, 4)), lambda: tick(rows=(-1, 2, 3)),  # the row map
            lambda: tick(rows=(0, 1, 2, 3), ctl=(0,) * 4, n=(0,) * 4, kbps=(0,) * 4),    # more rows than max_rows
            lambda: tick(n_rows=-1),
            lambda: tick(ctl=(START, 4, 0), n=(5, 0, 0)),                                # a good row beside a bad one: nothing changes
        ])
        # no rows, every row array NULL -- and no pcm either: lane 3, ready for longest, gets the slot
        rc, slot_lane = run.raw_tick(pcm=False)
        assert rc == 0 and list(slot_lane) == [3] and L.mp3mi_batch_sync(run.b) == 0
        assert [(i, s) for i, s, _, _ in run.m.tick({})] == [(3, 0)]
        w.calls.append(run.outputs()[0][0])
        w.frames = 1
        run.check_books()
        # lane 1 drains, parked and waiting for the slot: START, END or a push on it are refused; its own bitrate may be passed on
        assert run.tick({1: (d, END, 0)}) == [(0, 0)]
        assert run.lanes()[2][1] == PARKED | DRAINING | WAIT_SLOT
        refused([lambda: tick(rows=(1,), ctl=(START,), n=(0,), kbps=(0,)), lambda: tick(rows=(1,), ctl=(END,), n=(0,), kbps=(0,)),
                 lambda: tick(rows=(1,), ctl=(0,), n=(1,), kbps=(0,)), lambda: tick(rows=(0, 1), ctl=(0, 0), n=(0, 0), kbps=(128, 64))])
        rc, slot_lane = run.raw_tick((0, 1), (0, 0), (0, 0), (128, 128))
        assert rc == 0 and list(slot_lane) == [1] and L.mp3mi_batch_sync(run.b) == 0
        assert [(i, s) for i, s, _, _ in run.m.tick({})] == [(1, 0)]
        d.calls.append(run.outputs()[0][0])
        d.frames = 2
        run.check_books()
        # after every refusal the next ticks' bytes are what they would have been
        churn(run, {0: (None, a, [na - 3552]), 3: (None, w, [nw - 3552])})
        assert d.pos == 3552
        oracle_exact(oracle, run, [a, d, w])
        # detached, the batch is the caller's again
        L.mp3mi_feed_destroy(run.f)
        run.f = ctypes.c_void_p()
        assert L.mp3mi_batch_reset(run.b) == 0
    finally:
        run.close(feeder_first=False)


def test_rules_emulated(emu, oracle):
    rules_case(emu, oracle)


# ---- 8. equal to the old feeder ----
def sit_out_plan(mp):
    """the ticks of test_feed.py's sitting-out case"""
    a, b = Stream(attacks_pcm(mp), 2, 128), Stream(mp.synth(4 * 1152, 2, 44100, 312), 2, 128)
    return (a, b), [{0: (a, START, 2304)}, {0: (a, 0, 2304)}, {0: (a, 0, 100), 1: (b, START, 2304)}, {0: (a, 0, 0), 1: (b, END, 501)},
                    {0: (a, 0, 100)}, {0: (a, 0, 2104)}, {0: (a, 0, 2304)}, {0: (a, END, 999)}]


def same_as_old_case(mp, oracle):
    old = FeedRun(mp, 3, 44100, 2, 128, 2, 2304)
    try:
        (a0, b0), plan = sit_out_plan(mp)
        for feeds in plan:
            old.tick(feeds)
    finally:
        old.close()
    run = LaneRun(mp, 3, 3, 44100, 2, 128, 2, 2304)
    try:
        (a, b), plan = sit_out_plan(mp)
        encoded = [run.tick(feeds) for feeds in plan]
        assert encoded[4] == [] and run.lanes()[3] == 0
        assert run.m.parks > 0 and run.m.resumes > 0
        assert a.calls == a0.calls and b.calls == b0.calls
        oracle_exact(oracle, run, [a, b])
    finally:
        run.close()


def test_same_as_the_old_feeder_emulated(emu, oracle):
    same_as_old_case(emu, oracle)


# ---- 9. fewer lanes than slots ----
def few_lanes_case(mp, oracle):
    run = LaneRun(mp, 3, 2, 44100, 2, 128, 1, 2304)
    try:
        a, na = stream(mp, run, 850, 5, 41)
        b, nb = stream(mp, run, 851, 4, 700)
        churn(run, {0: (0, a, cuts(na, (959, 2303, 1, 1152, 7), 2304)), 1: (1, b, cuts(nb, (2304, 960), 2304))})
        assert run.m.over == 0 and not run.m.waited and run.m.parks > 0
        oracle_exact(oracle, run, [a, b])
    finally:
        run.close()


def test_fewer_lanes_than_slots_emulated(emu, oracle):
    few_lanes_case(emu, oracle)


# ---- 11. the sanitizer program ----
def test_sanitized_lifecycle_program():
    """tests/hipemu/feed_lanes_main.cpp under AddressSanitizer, UndefinedBehaviorSanitizer and LeakSanitizer on the emulator: create with
    fewer, as many and more lanes than slots, ticks with waits, migrations and same-tick refills, every refused call, destroy in both
    orders.  Passes when the program exits 0 without a report."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "hipemu"), "-f", "feed_lanes.mk", "feed_lanes"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------- device

CASES = dict(oversubscribed=oversubscribed_case, fairness=fairness_case, bitrates=bitrates_case, sticky=sticky_case, draining=draining_case,
             abandoned=abandoned_case, void=void_case, rules=rules_case, same_as_old=same_as_old_case,
             few_lanes=few_lanes_case, mono32=lambda mp, oracle: format_case(mp, oracle, 32000, 1, 56),
             crc_dual48=lambda mp, oracle: format_case(mp, oracle, 48000, 2, 192, mode=2, crc=True, omode="de"))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_lanes_gpu(product, oracle, monkeypatch, chunk, case):
    chunked(monkeypatch, chunk)
    CASES[case](product, oracle)


# ---- 10. wider ----
WIDE = dict(S=64, L=512, T=12, tick=2, max_push=2304, rate=44100, ch=2, kbps=128)


def wide_plan():
    """a seeded random churn: every lane runs one stream of 1 .. 3 frames less an odd count, STARTed in one of ticks 0 .. 4 and cut into
    pushes of the awkward sizes, the last piece whatever is left.  Returns per tick {lane: (ctl, n)} and the streams' lengths; the
    Model says that every stream closes inside the 12 ticks, that lanes wait, park and resume, and which lane encodes in which slot"""
    W = WIDE
    rng = np.random.default_rng(20241)
    plan, length = [dict() for _ in range(W["T"])], []
    for i in range(W["L"]):
        n = int(rng.integers(1, 4)) * 1152 - int(rng.integers(1, 1152))
        length.append(n)
        pieces, left = [], n
        while left > W["max_push"] or (left > 0 and len(pieces) < 2 and rng.integers(0, 2)):
            pieces.append(min(left, int(rng.choice(SIZES + (W["max_push"],)))))
            left -= pieces[-1]
        if left or not pieces:
            pieces.append(left)
        t = int(rng.integers(0, 5))
        for k, p in enumerate(pieces):
            plan[t + k][i] = ((START if k == 0 else 0) | (END if k == len(pieces) - 1 else 0), p)
    return plan, length


def test_wide_plan_exercises_the_scheduler():
    """the input of the device-only case, judged by the Model alone (no library, no device)"""
    W = WIDE
    plan, length = wide_plan()
    m = Model(W["S"], W["L"], W["tick"], W["tick"] * 1152 + W["max_push"] + 2304, [W["kbps"]] * W["S"])
    for feeds in plan:
        m.tick({i: (c, n, 0) for i, (c, n) in feeds.items()})
    assert not any(l.open for l in m.lane), sum(l.open for l in m.lane)
    assert m.over >= 4 and len(m.waited) > 100 and m.parks > 30 and m.resumes > 30 and m.refill_import > 0 and m.refill_start > 0 and m.moved
    assert max(len(f) for f in plan) <= 512 and all(sum(n for _, n in (f.get(i, (0, 0)) for f in plan)) == length[i] for i in range(W["L"]))


def wide_run(sync_each):
    import importlib
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    W = WIDE
    S, L, T, ch = W["S"], W["L"], W["T"], W["ch"]
    dev = torch.device("cuda:0")
    plan, length = wide_plan()
    n_src = 4 * 1152
    src = torch.empty((L, n_src * ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    mp3.synth_pcm_device(src, n_src, ch, W["rate"], 4000)
    b = mp3.Batch(S, W["rate"], ch, W["kbps"], W["tick"])
    feed = b.feeder(W["tick"], W["max_push"], lanes=L, ring_samples=W["tick"] * 1152 + W["max_push"] + 2304)
    assert feed.n_lanes == L and feed.capacity == W["tick"] * 1152 + W["max_push"] + 2304
    stride = b.out_stride(W["tick"])
    m = Model(S, L, W["tick"], feed.capacity, [W["kbps"]] * S)
    pos = [0] * L
    pcms, rows = [], []
    for t in range(T):
        rl = sorted(plan[t])
        p = torch.zeros((max(len(rl), 1), W["max_push"] * ch), dtype=torch.int16, device=dev)
        for r, i in enumerate(rl):
            n = plan[t][i][1]
            p[r, :n * ch] = src[i, pos[i] * ch:(pos[i] + n) * ch]
            pos[i] += n
        pcms.append(p), rows.append(rl)
    outs = [torch.zeros((S, stride), dtype=torch.uint8, device=dev) for _ in range(T)]
    lens = [torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(T)]
    torch.cuda.synchronize()
    slot_lanes = []
    for t in range(T):
        rl = rows[t]
        sl = feed.tick_lanes(pcms[t] if rl else None, outs[t], lens[t], rl, start=[plan[t][i][0] & START for i in rl],
                             end=[plan[t][i][0] & END for i in rl], n_push=[plan[t][i][1] for i in rl])
        enc = m.tick({i: (c, n, 0) for i, (c, n) in plan[t].items()})
        want = [-1] * S
        for i, s, _, _ in enc:
            want[s] = i
        assert list(sl) == want, t
        assert list(feed.lanes()[2]) == m.flags(), t
        slot_lanes.append(want)
        if sync_each:
            b.sync()
    b.sync()
    assert feed.lanes()[3] == 0
    feed.close()
    b.close()
    got = [b""] * L
    for o, n, sl in zip(outs, lens, slot_lanes):
        o, n = o.cpu().numpy(), n.cpu().numpy()
        for s, i in enumerate(sl):
            if i >= 0:
                got[i] += o[s, :int(n[s])].tobytes()
            else:
                assert n[s] == 0
    return got, src.cpu().numpy(), length


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [None, "0"])
def test_wide_back_to_back_gpu(product, oracle, monkeypatch, hold):
    """64 slots, 512 lanes, twelve ticks issued without a sync in between -- with the call hold at its default and switched off -- give
    the bytes of the same ticks synchronised one by one, and every 8th lane's are the oracle's"""
    if hold is not None:
        monkeypatch.setenv("MP3MI_CALL_HOLD", hold)
    a, src, length = wide_run(sync_each=True)
    b, _, _ = wide_run(sync_each=False)
    assert a == b
    for i in range(0, WIDE["L"], 8):
        assert b[i] == oracle.encode(src[i, :length[i] * 2], WIDE["rate"], WIDE["kbps"], 2)[0], i
