"""Ticks on host buffers (mp3mi_feed_tick_lanes_host_async, mp3mi_feed_host_wait, mp3mi_feed_host_io_stats; include/mp3mi.h): the tick
of a feeder with lanes, fed from PACKED packets in host memory and delivering dense rows by encoding lane into host memory.  The
judge is that of test_feed_lanes.py -- its Model, its LaneRun, its plans: the bytes a lane delivers from START through the tick that
closes it, concatenated, are the oracle's file, exactly, and after every tick out_lane_host, out_slot_host, n_out, mp3mi_feed_lanes,
slot_frames and slot_kbps say what the Model says.  HostRun is a LaneRun whose ticks go through the host call; the plans of
test_feed_lanes.CASES run on it unchanged (their case functions build a `LaneRun`, which the tests here replace by HostRun).
Every run checks, in every tick, that rows and lengths from n_out on keep their canary and that a row is zero behind its length, and
at its end that the statistics are exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_feed_lanes as lanes_mod
from mp3common import ERR_REFERENCE_ABORT, ROOT
from test_feed_lanes import CASES, ERR_ARG, PARKED, WAIT_SLOT, WAITING, LaneRun, Model, churn, cuts, stream
from test_slot_park import Stream, chunked, oracle_exact
from test_stream_slots import END, START

ROW_CANARY, LEN_CANARY = 0xA5, 0xDEADBEEF


def bind(mp):
    L = lanes_mod.bind(mp)
    L.mp3mi_feed_tick_lanes_host_async.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_size_t] + [ctypes.c_void_p] * 4
    L.mp3mi_feed_host_wait.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.mp3mi_feed_host_io_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return L


class IoStats(ctypes.Structure):
    _fields_ = [("h2d_bytes", ctypes.c_double), ("d2h_bytes", ctypes.c_double), ("h2d_ms", ctypes.c_double), ("d2h_ms", ctypes.c_double),
                ("calls", ctypes.c_long)]


class HostBufs:
    """the host buffers of one tick: packed PCM, out rows [S, stride], lengths [S] -- numpy arrays of exactly the stated sizes, or
    page-locked memory of the library (mp3mi_host_alloc) seen through numpy"""

    def __init__(self, L, pinned, n_pcm, S, stride):
        self.L, self.ptrs = L, []
        self.pcm = self.array(pinned, max(n_pcm, 1), np.int16)
        self.out = self.array(pinned, S * stride, np.uint8).reshape(S, stride)
        self.len = self.array(pinned, S, np.uint32)

    def array(self, pinned, n, dtype):
        if not pinned:
            return np.zeros(n, dtype)
        nbytes = n * np.dtype(dtype).itemsize
        p = self.L.mp3mi_host_alloc(nbytes)
        assert p
        self.ptrs.append(p)
        return np.frombuffer((ctypes.c_uint8 * nbytes).from_address(p), dtype=dtype)

    def free(self):
        for p in self.ptrs:
            self.L.mp3mi_host_free(p)
        self.ptrs = []


class HostRun(LaneRun):
    """a LaneRun whose ticks are host ticks (which="host"), or alternate with device ticks (which="alternate": even ticks on host
    buffers).  pinned: page-locked host buffers.  A pool of four buffer sets, taken in turn: up to three ticks may be uncollected."""
    pinned, which, device_tick = False, "host", False

    def __init__(self, *a, **kw):
        LaneRun.__init__(self, *a, **kw)
        bind(self.mp)
        self.pool = [HostBufs(self.L, self.pinned, self.max_rows * self.max_push * self.ch, self.S, self.stride) for _ in range(4)]
        self.host_ticks, self.inflight, self.last = 0, [], None
        self.up_bytes = self.dn_bytes = 0
        self.by_slot = ([b""] * self.S, np.zeros(self.S, np.uint32))

    def raw_tick(self, rows=(), ctl=(), n_push=(), kbps=(), pcm=True, out=True, out_len=True, sl=True, stride=None, pitch=None, f=True, null=(),
                 n_rows=None, lists=(True, True, True), bufs=None):
        """one mp3mi_feed_tick_lanes_host_async call as given (LaneRun.raw_tick's arguments; pitch has no meaning here, sl=False
        drops all three lists, lists= each of them).  Returns (rc, the lane per slot as slot_lane_host would say it)"""
        if self.device_tick:
            return LaneRun.raw_tick(self, rows, ctl, n_push, kbps, pcm=pcm, out=out, out_len=out_len, sl=sl, stride=stride, pitch=pitch, f=f,
                                    null=null, n_rows=n_rows)
        arr = dict(rows=np.ascontiguousarray(rows, np.int32), ctl=np.ascontiguousarray(ctl, np.uint8),
                   n_push=np.ascontiguousarray(n_push, np.int32), kbps=np.ascontiguousarray(kbps, np.int32))
        R = len(arr["rows"]) if n_rows is None else n_rows
        ptr = {k: (None if k in null or (R == 0 and n_rows is None) else a.ctypes.data) for k, a in arr.items()}
        hb = self.pool[self.host_ticks % 4] if bufs is None else bufs
        hb.out[...] = ROW_CANARY
        hb.len[...] = LEN_CANARY
        ol, os_, no = np.full(self.S, -9, np.int32), np.full(self.S, -9, np.int32), np.full(1, -9, np.int32)
        want = [x and sl for x in lists]
        rc = self.L.mp3mi_feed_tick_lanes_host_async(self.f if f else None, R, ptr["rows"], hb.pcm.ctypes.data if pcm else None, ptr["ctl"],
                                                     ptr["n_push"], ptr["kbps"], hb.out.ctypes.data if out else None,
                                                     self.stride if stride is None else stride, hb.len.ctypes.data if out_len else None,
                                                     ol.ctypes.data if want[0] else None, os_.ctypes.data if want[1] else None,
                                                     no.ctypes.data if want[2] else None)
        for a in arr.values():
            a[...] = 99  # (the library has copied them)
        slot_lane = np.full(self.S, -1, np.int32)
        if rc == 0:
            n = int(no[0])
            assert 0 <= n <= self.S and (ol[n:] == -9).all() and (os_[n:] == -9).all()
            assert list(ol[:n]) == sorted(ol[:n]) and len(set(os_[:n])) == n
            slot_lane[os_[:n]] = ol[:n]
            self.last = (hb, list(ol[:n]), list(os_[:n]))
            self.host_ticks += 1
        else:
            assert (ol == -9).all() and (os_ == -9).all() and no[0] == -9  # nothing is told of a refused tick
            assert (hb.out == ROW_CANARY).all() and (hb.len == LEN_CANARY).all()
        return rc, slot_lane

    def outputs(self):
        """by slot, as SlotRun.outputs: of the latest host tick (which must be through), or of a device tick"""
        return self.by_slot if self.by_slot is not None else LaneRun.outputs(self)

    def rows_of(self, hb, n_out):
        """the tick's rows, checked: zero behind the length, canaries from n_out on"""
        assert (hb.out[n_out:] == ROW_CANARY).all() and (hb.len[n_out:] == LEN_CANARY).all(), "rows from n_out on were written"
        got = []
        for i in range(n_out):
            n = int(hb.len[i])
            assert n <= self.stride and not hb.out[i, n:].any(), "row %d is not zero behind its %d bytes" % (i, n)
            got.append(hb.out[i, :n].tobytes())
        return got

    def collect(self):
        """books the bytes of the oldest uncollected host tick (the caller has waited for it)"""
        hb, enc = self.inflight.pop(0)
        got = self.rows_of(hb, len(enc))
        outs, lens = [b""] * self.S, np.zeros(self.S, np.uint32)
        for (i, s, closes, _, st), data in zip(enc, got):
            st.calls.append(data)
            outs[s], lens[s] = data, len(data)
        self.by_slot = (outs, lens)

    def tick(self, feeds, kbps0=False, sync=True):
        if self.which == "alternate" and self.ticks % 2 == 1:
            self.by_slot, self.device_tick = None, True
            try:
                return LaneRun.tick(self, feeds, kbps0=kbps0, sync=sync)
            finally:
                self.device_tick = False
        ch = self.ch
        rows = sorted(feeds)
        assert len(rows) <= self.max_rows
        hb = self.pool[self.host_ticks % 4]
        hb.pcm[...] = 0x5A5A
        ctl, ns, kb, mfeeds, at = [], [], [], {}, 0
        for i in rows:
            st, c, n = feeds[i]
            assert (c & START) or self.st[i] is st
            if c & START:
                self.st[i] = st
            k = st.kbps if (c & START) and not kbps0 else 0
            ctl.append(c), ns.append(n), kb.append(k)
            mfeeds[i] = (c, n, k)
            hb.pcm[at:at + n * ch] = st.take(n)  # PACKED: behind the row before
            at += n * ch
        rc, slot_lane = self.raw_tick(rows, ctl, ns, kb, pcm=at > 0 or self.ticks % 3 != 0)  # (nothing pushed: with and without a buffer)
        assert rc == 0, rc
        self.up_bytes += 2 * at
        enc = self.m.tick(mfeeds)
        self.ticks += 1
        _, got_lanes, got_slots = self.last
        assert (got_lanes, got_slots) == ([i for i, _, _, _ in enc], [s for _, s, _, _ in enc]), (got_lanes, got_slots, enc)
        self.dn_bytes += len(enc) * (self.stride + 4)
        for i, s, closes, started in enc:
            self.st[i].frames = self.m.lane[i].frames
            if started:
                self.st[i].kbps = self.m.lane[i].kbps
        self.order.append(sorted(i for i, _, _, _ in enc))
        self.inflight.append((hb, [(i, s, c, b, self.st[i]) for i, s, c, b in enc]))
        if not sync:
            return enc
        assert self.L.mp3mi_feed_host_wait(self.f, 0) == 0
        while self.inflight:
            self.collect()
        rc = self.L.mp3mi_batch_sync(self.b)
        assert rc in (0, ERR_REFERENCE_ABORT), rc
        if rc:
            self.aborts.append((self.ticks - 1, list(slot_lane)))
        self.check_books()
        for i, s, closes, _ in enc:
            if closes:
                self.st[i] = None
        return [(i, s) for i, s, _, _ in enc]

    def stats(self):
        st = IoStats()
        assert self.L.mp3mi_feed_host_io_stats(self.f, ctypes.byref(st)) == 0
        return st

    def close(self, feeder_first=True):
        try:
            if self.f:
                st = self.stats()  # exact, whatever the plan was
                assert (st.calls, st.h2d_bytes, st.d2h_bytes) == (self.host_ticks, self.up_bytes, self.dn_bytes), \
                    (st.calls, st.h2d_bytes, st.d2h_bytes, self.host_ticks, self.up_bytes, self.dn_bytes)
        finally:
            LaneRun.close(self, feeder_first)
            for hb in self.pool:
                hb.free()


class PinnedRun(HostRun):
    pinned = True


class AlternateRun(HostRun):
    which = "alternate"


def through(monkeypatch, cls, case, mp, oracle):
    """a case of test_feed_lanes.py with its LaneRun replaced"""
    monkeypatch.setattr(lanes_mod, "LaneRun", cls)
    CASES[case](mp, oracle)


# the rules case drives the device call's own arguments (a pitch, a NULL pcm_dev with rows): the host call's are in rules_host_case
PLANS = sorted(set(CASES) - {"rules"})


# ---- 1. the plans of test_feed_lanes.py through host ticks; alternation ----
PINNED = ("abandoned", "draining", "fairness", "few_lanes", "mono32", "sticky")  # on page-locked buffers; the others on pageable ones


@pytest.mark.parametrize("case", PLANS)
def test_plans_emulated(emu, oracle, monkeypatch, case):
    through(monkeypatch, PinnedRun if case in PINNED else HostRun, case, emu, oracle)


@pytest.mark.parametrize("case", ["draining"])
def test_device_and_host_ticks_alternate_emulated(emu, oracle, monkeypatch, case):
    through(monkeypatch, AlternateRun, case, emu, oracle)


# ---- 2. a plan of this file: what the plans above leave out ----
EXTRA = dict(S=2, L=5, tick=1, max_push=1152, kbps=128, rate=44100, ch=2)
EXTRA_PLAN = [
    {0: (START, 100)},                                   # nobody is ready: n_out == 0
    {0: (0, 1052), 1: (START, 1152), 2: (START, 1152)},  # three ready lanes on two slots: n_out == S, lane 2 waits while ready
    {0: (0, 500), 1: (0, 0), 2: (0, 600)},               # a row of no samples between two that push; lane 2 STARTs in the slot lane 0 leaves
    {0: (0, 652), 1: (0, 1152)},                         # lane 0 resumes in the slot lane 2 leaves in this tick
    {2: (0, 552), 3: (START, 1152)},
    {1: (0, 1152), 3: (0, 1152)},                        # lane 1, which ran in slot 1, resumes in slot 0
    {0: (END, 7), 1: (END, 300), 2: (END, 5), 3: (END, 20)},
    {}, {},
]


def extra_model():
    """the Model through EXTRA_PLAN, and what each tick showed: (n_out, whether a row of no samples lay between two that push)"""
    E = EXTRA
    m = Model(E["S"], E["L"], E["tick"], E["tick"] * 1152 + E["max_push"], [E["kbps"]] * E["S"])
    seen = []
    for feeds in EXTRA_PLAN:
        enc = m.tick({i: (c, n, 0) for i, (c, n) in feeds.items()})
        ns = [feeds[i][1] for i in sorted(feeds)]
        seen.append((len(enc), any(ns[k] == 0 and any(ns[:k]) and any(ns[k + 1:]) for k in range(len(ns)))))
    return m, seen


def test_the_plans_exercise_the_host_tick():
    """the input of the cases here, judged by the Model alone (no library, no device): EXTRA_PLAN holds everything a host tick does
    differently, whatever the plans of test_feed_lanes.py hold"""
    m, seen = extra_model()
    assert not any(l.open for l in m.lane)
    assert any(n == 0 for n, _ in seen[:7]), "no tick with n_out == 0 while lanes are open"
    assert any(n == EXTRA["S"] for n, _ in seen), "no tick with n_out == n_streams"
    assert any(z for _, z in seen), "no row of no samples between two that push"
    assert m.refill_import > 0 and m.refill_start > 0, "no slot vacated and refilled in one tick, by import and by START"
    assert m.waited, "no lane that waits for a slot while ready"
    assert m.moved, "no stream that encodes in two different slots"


def extra_case(mp, oracle, cls, sync_every=1):
    E = EXTRA
    run = cls(mp, E["S"], E["L"], E["rate"], E["ch"], E["kbps"], E["tick"], E["max_push"])
    try:
        total = [sum(f.get(i, (0, 0))[1] for f in EXTRA_PLAN) for i in range(E["L"])]
        sts = [Stream(mp.synth(4 * 1152, E["ch"], E["rate"], 900 + i), E["ch"], E["kbps"]) for i in range(E["L"])]
        for t, feeds in enumerate(EXTRA_PLAN):
            run.tick({i: (sts[i], c, n) for i, (c, n) in feeds.items()})
        assert run.lanes()[3] == 0 and [st.pos for st in sts] == total
        oracle_exact(oracle, run, [st for st, n in zip(sts, total) if n])
        return [st.calls for st in sts]
    finally:
        run.close()


EXTRA_DONE = {}


def extra_once(mp, oracle, cls):
    """a run of EXTRA_PLAN per library and kind of tick, shared by the tests that compare them"""
    key = (id(mp), cls.__name__)
    if key not in EXTRA_DONE:
        EXTRA_DONE[key] = extra_case(mp, oracle, cls)
    return EXTRA_DONE[key]


def test_extra_plan_emulated(emu, oracle):
    assert all(len(calls) >= 2 for calls in extra_once(emu, oracle, HostRun)[:4])


# ---- 3. the same plan through device ticks, through host ticks and through both in turn ----
def test_host_ticks_equal_device_ticks_emulated(emu, oracle):
    """per lane and tick the same bytes and lengths (Stream.calls: the bytes of every tick in which the lane encoded)"""
    host = extra_once(emu, oracle, HostRun)
    assert extra_once(emu, oracle, LaneRun) == host and extra_once(emu, oracle, AlternateRun) == host


# ---- 4. waits and statistics ----
def waits_case(mp, oracle, cls=HostRun):
    """three host ticks without a wait in between (the third waits for the first by itself), then host_wait(1) and host_wait(0)"""
    run = cls(mp, 2, 3, 44100, 2, 128, 1, 1152)
    try:
        L, f = run.L, run.f
        assert L.mp3mi_feed_host_wait(f, 0) == ERR_ARG and L.mp3mi_feed_host_wait(f, 1) == ERR_ARG  # no host tick yet
        assert L.mp3mi_feed_host_wait(None, 0) == ERR_ARG and L.mp3mi_feed_host_io_stats(f, None) == ERR_ARG
        st0 = run.stats()
        assert (st0.calls, st0.h2d_bytes, st0.d2h_bytes) == (0, 0, 0)
        a, na = stream(mp, run, 930, 4, 100)
        b, nb = stream(mp, run, 931, 4, 200)
        run.tick({0: (a, START, 1152), 2: (b, START, 1152)}, sync=False)
        assert L.mp3mi_feed_host_wait(f, 1) == ERR_ARG  # one host tick: none before it
        for bad in (-1, 2):
            assert L.mp3mi_feed_host_wait(f, bad) == ERR_ARG
        run.tick({0: (a, 0, 1152), 2: (b, 0, 1152)}, sync=False)
        run.tick({0: (a, 0, 1152), 2: (b, 0, 1152)}, sync=False)
        run.collect()  # tick 0: the third tick took its slot, and waited for it
        assert L.mp3mi_feed_host_wait(f, 1) == 0
        run.collect()
        assert L.mp3mi_feed_host_wait(f, 0) == 0
        run.collect()
        assert L.mp3mi_feed_host_wait(f, 0) == 0 and L.mp3mi_feed_host_wait(f, 1) == 0  # again: at once
        assert [len(a.calls), len(b.calls)] == [3, 3]
        # a tick of rows that push nothing uploads nothing; a tick in which nothing encodes downloads nothing
        before = run.stats()
        assert run.tick({0: (a, 0, 0), 2: (b, 0, 0)}) == []
        after = run.stats()
        assert (after.calls, after.h2d_bytes, after.d2h_bytes) == (before.calls + 1, before.h2d_bytes, before.d2h_bytes)
        assert before.h2d_bytes == 3 * 2 * 1152 * 4 and before.d2h_bytes == 6 * (run.stride + 4)
        churn(run, {0: (None, a, [na - 3 * 1152]), 2: (None, b, [nb - 3 * 1152])})
        oracle_exact(oracle, run, [a, b])
    finally:
        run.close()


def test_waits_and_statistics_emulated(emu, oracle):
    waits_case(emu, oracle)


# ---- 5. a larger stride: the dense rows grow ----
def test_a_larger_stride_emulated(emu, oracle):
    run = HostRun(emu, 2, 3, 44100, 2, 128, 1, 1152)
    try:
        a, na = stream(emu, run, 940, 3, 77)
        run.tick({1: (a, START, 1152)})
        wide = HostBufs(run.L, False, 1152 * 2, 2, run.stride + 40)
        wide.pcm[:1152 * 2] = a.take(1152)
        rc, slot_lane = run.raw_tick([1], [0], [1152], [0], stride=run.stride + 40, bufs=wide)
        assert rc == 0 and list(slot_lane) == [1, -1] and run.L.mp3mi_feed_host_wait(run.f, 0) == 0
        run.up_bytes += 1152 * 4
        run.dn_bytes += run.stride + 40 + 4
        assert (wide.out[1:] == ROW_CANARY).all() and (wide.len[1:] == LEN_CANARY).all() and not wide.out[0, int(wide.len[0]):].any()
        a.calls.append(wide.out[0, :int(wide.len[0])].tobytes())
        run.m.tick({1: (0, 1152, 0)})
        run.ticks += 1
        run.check_books()
        churn(run, {1: (None, a, [na - 2304])})
        oracle_exact(oracle, run, [a])
    finally:
        run.close()


# ---- 6. refusals ----
def rules_host_case(mp, oracle):
    L = bind(mp)
    # the host call on a feeder made by mp3mi_feed_create
    probe = lanes_mod.SlotRun(mp, 2, 44100, 2, 128, 2)
    try:
        f = ctypes.c_void_p()
        assert L.mp3mi_feed_create(ctypes.byref(f), probe.b, 1, 100) == 0
        out, ln, lst, n = np.zeros((2, probe.stride), np.uint8), np.zeros(2, np.uint32), np.zeros((2, 2), np.int32), np.zeros(1, np.int32)
        assert L.mp3mi_feed_tick_lanes_host_async(f, 0, None, None, None, None, None, out.ctypes.data, probe.stride, ln.ctypes.data, lst[0].ctypes.data,
                                                  lst[1].ctypes.data, n.ctypes.data) == ERR_ARG
        assert L.mp3mi_feed_host_wait(f, 0) == ERR_ARG
        st = IoStats()
        assert L.mp3mi_feed_host_io_stats(f, ctypes.byref(st)) == 0 and st.calls == 0
    finally:
        probe.close()  # (the batch goes with the feeder attached)

    run = HostRun(mp, 1, 4, 44100, 2, 128, 1, 2400, max_rows=3)
    try:
        (a, na), (d, nd), (w, nw) = (stream(mp, run, 820 + i, 4, 3 + 2 * i) for i in range(3))
        # as in test_feed_lanes.py: lane 0 parked and waiting for the slot with 2400 pending, lane 1 in the slot with 2400 pending, lane 2
        # closed, lane 3 not yet in the batch, waiting for the slot with a full ring
        assert run.tick({0: (a, START, 1152), 1: (d, START, 1152), 3: (w, START, 1152)}) == [(0, 0)]
        assert run.tick({0: (a, 0, 2400), 1: (d, 0, 2400), 3: (w, 0, 2400)}) == [(1, 0)]
        assert run.lanes()[:3] == ([2400, 2400, 0, 3552], [1, 1, -1, 0], [PARKED | WAIT_SLOT, 0, 0, WAITING | WAIT_SLOT])

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
            lambda: tick(out=False), lambda: tick(out_len=False), lambda: tick(f=False),
            lambda: tick(lists=(False, True, True)), lambda: tick(lists=(True, False, True)), lambda: tick(lists=(True, True, False)),  # each new NULL
            lambda: tick(ctl=(0, START, 0), n=(0, 7, 0), pcm=False),                     # no pcm_host, and a push
            lambda: tick(null=("rows",)), lambda: tick(null=("ctl",)), lambda: tick(null=("n_push",)), lambda: tick(null=("kbps",)),
            lambda: tick(stride=run.stride - 1),
            lambda: tick(ctl=(0, START, 0), kbps=(0, 100, 0)),                           # no Layer III bitrate
            lambda: tick(ctl=(0, START, 0), kbps=(0, 160, 0)),                           # above the ceiling of a batch created at 128
            lambda: tick(kbps=(64, 0, 0)), lambda: tick(kbps=(0, 128, 0)),               # not the open stream's / nothing open
            lambda: tick(rows=(0, 3, 2)), lambda: tick(rows=(0, 2, 2)), lambda: tick(rows=(0, 2, 4)), lambda: tick(rows=(-1, 2, 3)),  # the row map
            lambda: tick(rows=(0, 1, 2, 3), ctl=(0,) * 4, n=(0,) * 4, kbps=(0,) * 4),    # more rows than max_rows
            lambda: tick(n_rows=-1),
            lambda: tick(ctl=(START, 4, 0), n=(5, 0, 0)),                                # a good row beside a bad one: nothing changes
        ])
        assert run.stats().calls == 2  # a refused call is no tick
        assert L.mp3mi_feed_tick(run.f, run.d_push, run.pitch, np.zeros(4, np.uint8).ctypes.data, None, None, run.d_out, run.stride, run.d_len) == ERR_ARG
        # rows that push nothing and no pcm_host: lane 3, ready for longest, gets the slot
        assert run.tick({}) == [(3, 0)]
        w.frames = 1
        # lane 1 drains, parked and waiting for the slot: START, END or a push on it are refused; its own bitrate may be passed on
        assert run.tick({1: (d, END, 0)}) == [(0, 0)]
        assert run.lanes()[2][1] == PARKED | lanes_mod.DRAINING | WAIT_SLOT
        refused([lambda: tick(rows=(1,), ctl=(START,), n=(0,), kbps=(0,)), lambda: tick(rows=(1,), ctl=(END,), n=(0,), kbps=(0,)),
                 lambda: tick(rows=(1,), ctl=(0,), n=(1,), kbps=(0,)), lambda: tick(rows=(0, 1), ctl=(0, 0), n=(0, 0), kbps=(128, 64))])
        rc, slot_lane = run.raw_tick((0, 1), (0, 0), (0, 0), (128, 128), pcm=False)
        assert rc == 0 and list(slot_lane) == [1] and L.mp3mi_feed_host_wait(run.f, 0) == 0 and L.mp3mi_batch_sync(run.b) == 0
        assert [(i, s) for i, s, _, _ in run.m.tick({})] == [(1, 0)]
        hb, got_lanes, got_slots = run.last
        d.calls.append(run.rows_of(hb, 1)[0])
        run.dn_bytes += run.stride + 4
        run.ticks += 1
        d.frames = 2
        run.check_books()
        # after every refusal the next ticks' bytes are what they would have been
        churn(run, {0: (None, a, [na - 3552]), 3: (None, w, [nw - 3552])})
        assert d.pos == 3552
        oracle_exact(oracle, run, [a, d, w])
    finally:
        run.close()


def test_refusals_emulated(emu, oracle):
    rules_host_case(emu, oracle)


# ---- 7. the sanitizer program ----
def test_sanitized_lifecycle_program():
    """tests/hipemu/feed_host_main.cpp under AddressSanitizer, UndefinedBehaviorSanitizer and LeakSanitizer on the emulator: host ticks
    on staging, rows and lists of exactly the stated sizes, a regrow of the dense rows, a failed call, alternation with device ticks,
    destroy with ticks in flight, mp3mi_batch_destroy with the feeder attached.  Passes when the program exits 0 without a report."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "hipemu"), "-f", "feed_host.mk", "feed_host"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------- device

@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
@pytest.mark.parametrize("case", PLANS)
def test_plans_gpu(product, oracle, monkeypatch, chunk, case):
    chunked(monkeypatch, chunk)
    through(monkeypatch, PinnedRun if chunk else HostRun, case, product, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_extra_waits_refusals_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    host = extra_case(product, oracle, PinnedRun)
    assert extra_case(product, oracle, AlternateRun) == host and extra_case(product, oracle, LaneRun) == host and extra_case(product, oracle, HostRun) == host
    waits_case(product, oracle, PinnedRun)
    rules_host_case(product, oracle)


# ---- 8. wider, back to back, through the Python binding ----
WIDE = dict(S=64, L=256, T=12, tick=2, max_push=2304, rate=44100, ch=2, kbps=128)


def wide_plan():
    """a seeded random churn as test_feed_lanes.wide_plan: every lane runs one stream of 1 .. 3 frames less an odd count, STARTed in one
    of ticks 0 .. 4 and cut into pushes of the awkward sizes.  Returns per tick {lane: (ctl, n)} and the streams' lengths"""
    W = WIDE
    rng = np.random.default_rng(20251)
    plan, length = [dict() for _ in range(W["T"])], []
    for i in range(W["L"]):
        n = int(rng.integers(1, 4)) * 1152 - int(rng.integers(1, 1152))
        length.append(n)
        pieces, left = [], n
        while left > W["max_push"] or (left > 0 and len(pieces) < 2 and rng.integers(0, 2)):
            pieces.append(min(left, int(rng.choice(lanes_mod.SIZES + (W["max_push"],)))))
            left -= pieces[-1]
        if left or not pieces:
            pieces.append(left)
        t = int(rng.integers(0, 5))
        for k, p in enumerate(pieces):
            plan[t + k][i] = ((START if k == 0 else 0) | (END if k == len(pieces) - 1 else 0), p)
    return plan, length


def test_wide_plan_closes_and_oversubscribes():
    """the input of the wide device case, judged by the Model alone"""
    W = WIDE
    plan, length = wide_plan()
    m = Model(W["S"], W["L"], W["tick"], W["tick"] * 1152 + W["max_push"] + 2304, [W["kbps"]] * W["S"])
    n_outs = [len(m.tick({i: (c, n, 0) for i, (c, n) in feeds.items()})) for feeds in plan]
    assert not any(l.open for l in m.lane), sum(l.open for l in m.lane)
    assert m.over >= 1 and m.waited and m.parks > 10 and m.resumes > 10 and max(n_outs) == W["S"] and min(n_outs) < W["S"], (m.over, n_outs)


def wide_host_run():
    """twelve host ticks from page-locked buffers, issued back to back; tick t is collected with host_wait(1) behind tick t + 1's issue"""
    import importlib
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    W = WIDE
    S, L, T, ch = W["S"], W["L"], W["T"], W["ch"]
    plan, length = wide_plan()
    src = np.zeros((L, 3 * 1152 * ch), np.int16)
    for i in range(L):
        mp3.lib().mp3mi_synth_pcm(src[i].ctypes.data, 3 * 1152, ch, W["rate"], 5000 + i, 0x6D70336D)
    b = mp3.Batch(S, W["rate"], ch, W["kbps"], W["tick"])
    feed = b.feeder(W["tick"], W["max_push"], lanes=L, ring_samples=W["tick"] * 1152 + W["max_push"] + 2304)
    stride = b.out_stride(W["tick"])
    m = Model(S, L, W["tick"], feed.capacity, [W["kbps"]] * S)
    pos = [0] * L
    pcms, outs, lens = [], [], []
    for t in range(T):
        rl = sorted(plan[t])
        n_all = sum(plan[t][i][1] for i in rl)
        p = torch.zeros(max(n_all * ch, 1), dtype=torch.int16).pin_memory()
        at = 0
        for i in rl:
            n = plan[t][i][1]
            p[at:at + n * ch] = torch.from_numpy(src[i, pos[i] * ch:(pos[i] + n) * ch])
            pos[i] += n
            at += n * ch
        pcms.append(p)
        outs.append(torch.full((S, stride), ROW_CANARY, dtype=torch.uint8).pin_memory())
        lens.append(torch.full((S,), -7, dtype=torch.int32).pin_memory())
    got = [b""] * L
    told = []

    def collect(t):
        lanes_t, slots_t = told[t]
        o, n = outs[t].numpy(), lens[t].numpy()
        assert (o[len(lanes_t):] == ROW_CANARY).all() and (n[len(lanes_t):] == -7).all(), t
        for k, i in enumerate(lanes_t):
            assert not o[k, int(n[k]):].any()
            got[i] += o[k, :int(n[k])].tobytes()

    up = dn = 0
    for t in range(T):
        rl = sorted(plan[t])
        lanes_t, slots_t = feed.tick_lanes_host(pcms[t], outs[t], lens[t], rl, start=[plan[t][i][0] & START for i in rl],
                                                end=[plan[t][i][0] & END for i in rl], n_push=[plan[t][i][1] for i in rl])
        enc = m.tick({i: (c, n, 0) for i, (c, n) in plan[t].items()})
        assert (list(lanes_t), list(slots_t)) == ([i for i, _, _, _ in enc], [s for _, s, _, _ in enc]), t
        assert list(feed.lanes()[2]) == m.flags(), t
        told.append((list(lanes_t), list(slots_t)))
        up += sum(plan[t][i][1] for i in rl) * ch * 2
        dn += len(lanes_t) * (stride + 4)
        if t > 0:
            feed.host_wait(1)
            collect(t - 1)
    feed.host_wait(0)
    collect(T - 1)
    b.sync()
    st = feed.host_io_stats()
    assert (st["calls"], st["h2d_bytes"], st["d2h_bytes"]) == (T, up, dn), st
    assert feed.lanes()[3] == 0
    feed.close()
    b.close()
    return got, src, length


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [None, "0"])
def test_wide_back_to_back_gpu(product, oracle, monkeypatch, hold):
    """64 slots, 256 lanes, twelve host ticks from page-locked buffers with no wait in between but host_wait(1) behind the next issue --
    with the call hold at its default and switched off: every lane's file is the oracle's"""
    if hold is not None:
        monkeypatch.setenv("MP3MI_CALL_HOLD", hold)
    got, src, length = wide_host_run()
    for i in range(WIDE["L"]):
        assert got[i] == oracle.encode(src[i, :length[i] * 2], WIDE["rate"], WIDE["kbps"], 2)[0], i
