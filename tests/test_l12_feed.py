"""The feeder of Layers I and II on the emulated build (mp3mi_l12_feed_*, include/mp3mi_l12.h): lanes in front of three slots at
44.1 kHz.  The judge is byte equality: the bytes a lane delivers from a stream's START through the tick that closes it, gathered slot
by slot through slot_lane_host, are the CPU oracle's file of the stream's samples at its bitrate and the library's own ragged
whole-file call's.  After every tick the books -- slot_lane_host, mp3mi_l12_feed_lanes, mp3mi_l12_batch_slot_frames, _slot_kbps --
are compared with a Python model of the contract (tests/l12_feed.py).  No scenario skips a stream: check() wants every stream that was
started, fed to its last sample and closed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from l12_feed import (DRAINING, END, ERR_ARG, PARKED, START, WAIT_SLOT, WAITING, FeedRun, bind, check, churn, cuts, more_lanes_case)
from l12_park import Ticket, aligned
from l12_slots import SlotRun, ragged_whole_file
from mp3common import ROOT, l12_signal, oracle_l12

SPF = {1: 384, 2: 1152}
KBPS = {1: 192, 2: 128}


# ---- 1. any cut is the same file ----
@pytest.mark.parametrize("layer,tick,mode", [(1, 1, "m"), (1, 2, "s"), (2, 1, "s"), (2, 2, "m"), (2, 1, "je"), (2, 2, "je"), (1, 1, "s"), (1, 2, "m")])
def test_any_cut_is_the_same_file(emu, oracle, layer, tick, mode):
    """one stream in five lanes over three slots: one push per tick, packets of 160, 960 and 1000 samples, and irregular seeded cuts"""
    full = tick * SPF[layer]
    max_push = max(full, 1000)
    run = FeedRun(emu, layer, 3, 5, 44100, mode, KBPS[layer], tick, max_push)
    try:
        n = 4 * full + 3 * SPF[layer] // 2 - 11
        rng = np.random.default_rng(layer * 10 + tick)
        irregular = [int(x) for x in rng.integers(1, max_push + 1, 64)]
        streams = [run.stream(500, n, kbps=KBPS[layer]) for _ in range(5)]
        plans = {i: (0, streams[i], cuts(n, sizes, max_push)) for i, sizes in enumerate([(full,), (160,), (960,), (1000,), irregular])}
        churn(run, plans)
        check(run, oracle, streams)
        assert all(st.got == streams[0].got for st in streams) and len(streams[0].got) > 1
        assert run.m.over > 0 or tick * SPF[layer] > 1000  # (lanes with small packets are seldom ready together)
    finally:
        run.close()


# ---- 2. more lanes than slots ----
@pytest.mark.parametrize("layer,tick", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_more_lanes_than_slots(emu, oracle, layer, tick):
    more_lanes_case(emu, oracle, layer, tick)


# ---- 3. migration through resume; 4. young streams ----
@pytest.mark.parametrize("layer,k", [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (1, 4), (1, 5)])
def test_migration_through_resume(emu, oracle, layer, k):
    """a stream encodes k ticks of one frame in slot 0, sits out a tick in which two other lanes take slots 0 and 1, and goes on in slot
    2: the resume at every phase case_phase of tests/l12_park.py distinguishes (Layer I: a frame is 12 filterbank slots against
    granules of 18; Layer II: the two warm-up passes).  Layer I after 1 .. 4 frames and Layer II after one are YOUNGER than the 1792
    samples of a history row, which then begins with zeros; a stream has encoded whole frames when it is resumed, never exactly 1792
    samples, so the first resume whose history fills the row exactly -- n_hist == 1792, nothing in front -- is Layer I after 5 frames
    (1920 samples) and Layer II after two (n_hist 1792 itself: tests/test_l12_feed_kernel.py)."""
    spf = SPF[layer]
    run = FeedRun(emu, layer, 3, 3, 44100, "s", KBPS[layer], 1, spf)
    try:
        a = run.stream(510 + k, (k + 3) * spf - 5, kbps=KBPS[layer])
        b, c = run.stream(520, 3 * spf, kbps=KBPS[layer], noise=True), run.stream(521, 3 * spf, kbps=KBPS[layer], noise=True)
        for t in range(k):
            assert run.tick({0: (a, START if t == 0 else 0, spf)}) == [(0, 0)]
        assert run.tick({1: (b, START, spf), 2: (c, START, spf)}) == [(1, 0), (2, 1)]  # full-scale noise where the stream was
        assert run.lanes()[2][0] == PARKED and run.frames()[0] == 1
        assert run.tick({0: (a, 0, spf), 1: (b, 0, spf), 2: (c, 0, spf)}) == [(0, 2), (1, 0), (2, 1)]
        assert run.m.resumed_at == [k * spf] and (k * spf < 1792) == ((layer, k) not in ((1, 5), (2, 2)))
        assert run.tick({0: (a, 0, spf), 1: (b, END, spf), 2: (c, END, spf)}) == [(0, 2), (1, 0), (2, 1)]
        assert run.tick({0: (a, END, spf - 5)}) == [(0, 2)]
        assert run.m.slots_of[0] == [0] * k + [2, 2, 2]
        check(run, oracle, [a, b, c])
    finally:
        run.close()


# ---- 5. other relations ----
@pytest.mark.parametrize("layer,n_lanes", [(1, 2), (2, 3), (2, 2), (1, 3)])
def test_fewer_and_as_many_lanes_as_slots(emu, oracle, layer, n_lanes):
    spf = SPF[layer]
    run = FeedRun(emu, layer, 3, n_lanes, 44100, "j", KBPS[layer], 2, 2 * spf)
    try:
        streams = [run.stream(530 + i, (5 + i) * spf - 7 * (i + 1), kbps=KBPS[layer]) for i in range(n_lanes)]
        churn(run, {i: (i, st, cuts(len(st.pcm) // 2, (959, 2 * spf, 1, 160, 7), 2 * spf)) for i, st in enumerate(streams)})
        assert run.m.over == 0 and not run.m.waited and run.m.parks > 0 and run.m.resumes > 0
        check(run, oracle, streams)
    finally:
        run.close()


# ---- 6. END ----
@pytest.mark.parametrize("layer", [1, 2])
def test_drain_one_call_files_and_abandoned_streams(emu, oracle, layer):
    """one slot, three lanes.  Lanes 0 and 1 END with several ticks pending and take turns in the slot while they drain; a stream ENDs
    with 0 pending; lane 2 delivers one-call files of 0, 1, frame - 1, frame and frame + 1 samples; a START on an open lane abandons
    the stream there -- while it waits for a slot, while it is parked and while it sits in the slot"""
    spf = SPF[layer]
    run = FeedRun(emu, layer, 1, 3, 44100, "s", KBPS[layer], 1, spf + 1, ring=4 * spf)
    try:
        k = KBPS[layer]
        a, b = run.stream(540, 4 * spf - 9, kbps=k), run.stream(541, 3 * spf, kbps=k)
        assert run.tick({0: (a, START, spf), 1: (b, START, spf)}) == [(0, 0)]
        assert run.lanes()[2] == [0, WAITING | WAIT_SLOT, 0]
        assert run.tick({0: (a, 0, spf + 1), 1: (b, 0, spf)}) == [(1, 0)]          # lane 1 was ready first
        assert run.tick({0: (a, 0, spf), 1: (b, 0, spf)}) == [(0, 0)]
        assert run.tick({0: (a, END, spf - 10), 1: (b, END, 0)}) == [(1, 0)]       # both drain from here: a has 2 * frame - 9 pending, b a frame
        assert run.lanes()[2][:2] == [PARKED | DRAINING | WAIT_SLOT, DRAINING]
        assert run.tick({}) == [(0, 0)]
        assert run.tick({}) == [(1, 0)] and run.lanes()[1][1] == -1                # b closed on exactly a frame
        assert run.tick({}) == [(0, 0)] and run.lanes()[3] == 0
        # END with 0 pending on a stream that is in the slot, and on one that is parked
        c, d = run.stream(542, spf, kbps=k), run.stream(543, spf, kbps=k)
        assert run.tick({0: (c, START, spf)}) == [(0, 0)]
        assert run.tick({0: (c, END, 0), 1: (d, START, spf)}) == [(0, 0)]
        assert run.tick({}) == [(1, 0)]
        assert run.tick({2: (run.stream(544, spf, kbps=k), START, spf)}) == [(2, 0)]   # d is parked
        e = run.st[2]
        assert run.tick({1: (d, END, 0), 2: (e, END, 0)}) == [(1, 0)] and run.lanes()[2][2] == PARKED | DRAINING | WAIT_SLOT
        assert run.tick({}) == [(2, 0)]
        files = []
        for n in (0, 1, spf - 1, spf, spf + 1):  # (frame + 1: a tick, and the last sample in the tick behind it)
            f = run.stream(545 + n % 7, n, kbps=k)
            files.append(f)
            assert run.tick({2: (f, START | END, n)}) == [(2, 0)]
            if n > spf:
                assert run.lanes()[2][2] == DRAINING and run.tick({}) == [(2, 0)]
            assert run.lanes()[3] == 0
        assert [len(f.got) for f in files[:2]] == [1, len(files[1].got)] and len(files[4].got) > len(files[3].got)
        check(run, oracle, [a, b, c, d, e] + files)
        # abandoned: waiting for a slot (w), parked (p), in the slot (q)
        n_done = len(run.done)
        p, w, w2, p2, q, q2 = (run.stream(550 + i, 4 * spf, kbps=k) for i in range(6))
        q3 = run.stream(556, 2 * spf - 7, kbps=k)
        assert run.tick({0: (p, START, spf), 1: (w, START, spf)}) == [(0, 0)]
        assert run.tick({1: (w2, START, spf)}) == [(1, 0)] and run.lanes()[2][0] == PARKED        # w is gone before the batch saw it
        assert run.tick({0: (p2, START, spf), 1: (w2, 0, spf)}) == [(0, 0)]                        # p is gone while parked
        assert run.tick({0: (p2, 0, spf), 1: (w2, 0, spf)}) == [(1, 0)]
        assert run.tick({0: (p2, 0, spf), 1: (w2, END, spf)}) == [(0, 0)]
        assert run.tick({0: (q, START, 5)}) == [(1, 0)]                                            # p2 is gone from its slot; q is not ready
        assert run.lanes()[2][0] == WAITING and run.tick({}) == [(1, 0)]
        assert run.tick({0: (q2, START, spf)}) == [(0, 0)]                                         # q is gone before the batch saw it
        assert run.tick({0: (q3, START, spf)}) == [(0, 0)]                                         # q2 is gone from the slot, to q3's START
        assert run.tick({0: (q3, END, spf - 7)}) == [(0, 0)]
        assert len(run.done) == n_done + 2 and not any(st in run.done for st in (p, w, p2, q, q2))
        check(run, oracle, [w2, q3])
    finally:
        run.close()


# ---- 7. bitrates ----
@pytest.mark.parametrize("layer", [1, 2])
def test_bitrates_per_lane(emu, oracle, layer):
    """a batch created at three bitrates; lanes START at others -- in Layer II 64, 128 and 192 kbps at 44.1 kHz stereo select allocation
    tables 2, 0 and 1 (src/common.c:291-318) -- and at kbps 0, the create-time bitrate of the slot a stream first encodes in; the
    streams migrate, so cfg of a slot follows the stream that resumes there.  A bitrate above the ceiling is refused."""
    spf = SPF[layer]
    create = [320, 96, 160] if layer == 2 else [320, 96, 160]
    rates = [64, 128, 192, 0, 96] if layer == 2 else [64, 128, 192, 0, 96]
    run = FeedRun(emu, layer, 3, 5, 44100, "s", create, 1, spf, ring=3 * spf)
    try:
        streams = [run.stream(560 + i, (3 + i % 2) * spf - 3 - i, kbps=rates[i] or None) for i in range(5)]
        plans = {i: (0, st, [spf] + cuts(len(st.pcm) // 2 - spf, (160, spf, 959), spf)) for i, st in enumerate(streams)}
        churn(run, plans)
        assert run.m.over > 0 and run.m.moved and run.m.resumes > 0
        assert streams[3].kbps in create and sorted(set(st.kbps for st in streams)) == sorted(set([64, 128, 192, 96, streams[3].kbps]))
        check(run, oracle, streams)
        # kbps 0 again, on a quiet feeder: lanes 0 and 1 take slots 0 and 1 and with them 320 and 96
        a, b = run.stream(570, 2 * spf - 5), run.stream(571, 2 * spf - 6)
        assert run.tick({0: (a, START, spf), 1: (b, START, spf)}) == [(0, 0), (1, 1)]
        assert (a.kbps, b.kbps) == (320, 96)
        # until the bitrate is known only 0 may be passed; from then on the stream's own; above the ceiling: refused
        assert run.raw_tick((0,), (0,), (0,), (96,))[0] == ERR_ARG and run.raw_tick((2,), (START,), (5,), (352 if layer == 1 else 384,))[0] == ERR_ARG
        run.check_books()
        churn(run, {0: (None, a, [spf - 5]), 1: (None, b, [spf - 6])})
        check(run, oracle, [a, b])
    finally:
        run.close()


# ---- 8. refusals ----
def test_refusals(emu, oracle):
    """each refusal once: MP3MI_ERR_ARG and feeder and batch as they were -- the books after every refused call, and the files of the
    correct ticks that follow"""
    L = bind(emu)
    probe = SlotRun(emu, 2, 2, 44100, "s", 128, 2)
    try:
        f = ctypes.c_void_p()
        #            n_lanes, max_rows, tick_frames, max_push, ring_samples
        for args in [(0, 1, 1, 100, 0), (5, 0, 1, 100, 0), (5, 6, 1, 100, 0), (5, 5, 0, 100, 0), (5, 5, 3, 100, 0), (5, 5, 1, 0, 0),
                     (5, 5, 1, 100, 1251), (5, 5, 1, 100, -1), (5, 5, 1, 100, 2 ** 31 - 1), (-1, 1, 1, 100, 0)]:
            assert L.mp3mi_l12_feed_create(ctypes.byref(f), probe.b, *args) == ERR_ARG and not f.value, args
        assert L.mp3mi_l12_feed_create(None, probe.b, 5, 5, 1, 100, 0) == ERR_ARG
        assert L.mp3mi_l12_feed_create(ctypes.byref(f), None, 5, 5, 1, 100, 0) == ERR_ARG
        pcm = np.zeros((2, 2 * 1152 * 2), np.int16)
        assert probe.call(pcm, [START, 0], [2304, 0]) == 0  # a stream is open
        assert L.mp3mi_l12_feed_create(ctypes.byref(f), probe.b, 5, 5, 1, 100, 0) == ERR_ARG
        assert L.mp3mi_l12_batch_reset(probe.b) == 0
        assert L.mp3mi_l12_feed_create(ctypes.byref(f), probe.b, 1, 1, 2, 100, 2404) == 0  # fewer lanes than slots, the least ring given
        g = ctypes.c_void_p()
        assert L.mp3mi_l12_feed_create(ctypes.byref(g), probe.b, 5, 5, 1, 100, 0) == ERR_ARG and not g.value  # one feeder per batch
        assert L.mp3mi_l12_feed_n_lanes(f) == 1 and L.mp3mi_l12_feed_n_lanes(None) == 0
        assert L.mp3mi_l12_feed_capacity(f) == 2404 and L.mp3mi_l12_feed_capacity(None) == 0
        assert L.mp3mi_l12_feed_lanes(f, None, None, None) == ERR_ARG and L.mp3mi_l12_feed_lanes(None, None, None, None) == ERR_ARG
    finally:
        probe.close()  # (the batch goes with the feeder attached)

    spf = 384
    run = FeedRun(emu, 1, 1, 4, 44100, "s", 192, 1, 800, max_rows=3)
    try:
        a, d, w = (run.stream(580 + i, 4 * spf - 3 - 2 * i, kbps=192) for i in range(3))
        # lane 0 parked and waiting for the slot with 800 pending, lane 1 in the slot with 800 pending, lane 2 closed, lane 3 not yet
        # in the batch, waiting for the slot with a full FIFO
        assert run.tick({0: (a, START, spf), 1: (d, START, spf), 3: (w, START, spf)}) == [(0, 0)]
        assert run.tick({0: (a, 0, 800), 1: (d, 0, 800), 3: (w, 0, 800)}) == [(1, 0)]
        assert run.lanes()[:3] == ([800, 800, 0, 1184], [1, 1, -1, 0], [PARKED | WAIT_SLOT, 0, 0, WAITING | WAIT_SLOT])
        books = run.books()

        def tick(rows=(0, 2, 3), ctl=(0, 0, 0), n=(0, 0, 0), kbps=(0, 0, 0), **kw):
            return run.raw_tick(rows, ctl, n, kbps, **kw)[0]

        def refused(calls):
            for k, call in enumerate(calls):
                assert call() == ERR_ARG, k
                assert run.books() == books, k
                run.check_books()

        refused([
            lambda: tick(ctl=(0, 4, 0)), lambda: tick(ctl=(8, 0, 0)),                    # unknown ctl bits
            lambda: tick(n=(0, 5, 0)), lambda: tick(ctl=(0, END, 0)),                    # a closed lane without START
            lambda: tick(n=(-1, 0, 0)), lambda: tick(n=(0, 801, 0), ctl=(0, START, 0)),
            lambda: tick(n=(385, 0, 0)),                                                 # 800 + 385 > 384 + 800
            lambda: tick(n=(0, 0, 1)),                                                   # the waiting lane's FIFO is full
            lambda: tick(pcm=False), lambda: tick(out=False), lambda: tick(out_len=False), lambda: tick(sl=False), lambda: tick(f=False),
            lambda: tick(null=("rows",)), lambda: tick(null=("ctl",)), lambda: tick(null=("n_push",)), lambda: tick(null=("kbps",)),
            lambda: tick(stride=run.stride - 1), lambda: tick(pitch=799),
            lambda: tick(ctl=(0, START, 0), kbps=(0, 100, 0)),                           # no Layer I bitrate
            lambda: tick(ctl=(0, START, 0), kbps=(0, 224, 0)),                           # above the ceiling of a batch created at 192
            lambda: tick(kbps=(64, 0, 0)), lambda: tick(kbps=(0, 192, 0)),               # not the open stream's / nothing open
            lambda: tick(rows=(0, 3, 2)), lambda: tick(rows=(0, 2, 2)), lambda: tick(rows=(0, 2, 4)), lambda: tick(rows=(-1, 2, 3)),  # the row map
            lambda: tick(rows=(0, 1, 2, 3), ctl=(0,) * 4, n=(0,) * 4, kbps=(0,) * 4),    # more rows than max_rows
            lambda: tick(n_rows=-1),
            lambda: tick(ctl=(START, 4, 0), n=(5, 0, 0)),                                # a good row beside a bad one: nothing changes
        ])
        # the batch's calls while the feeder is attached: the streams are the feeder's
        vp = ctypes.c_void_p
        z8, z32 = np.zeros(1, np.uint8), np.zeros(1, np.int32)
        state = aligned(run.mem, run.ch * 5696 + 16)
        refused([
            lambda: L.mp3mi_l12_batch_encode(run.b, run.d_pcm, None, 1, run.d_out, run.stride, run.d_len),
            lambda: L.mp3mi_l12_batch_encode_next(run.b, run.d_pcm, 1, run.d_out, run.stride, run.d_len),
            lambda: L.mp3mi_l12_batch_encode_slots(run.b, run.d_pcm, 1, z8.ctypes.data, None, run.d_out, run.stride, run.d_len),
            lambda: L.mp3mi_l12_batch_encode_slots_kbps(run.b, run.d_pcm, 1, z8.ctypes.data, None, z32.ctypes.data, run.d_out, run.stride, run.d_len),
            lambda: L.mp3mi_l12_batch_flush(run.b, run.d_out, run.stride, run.d_len),
            lambda: L.mp3mi_l12_batch_reset(run.b),
            lambda: L.mp3mi_l12_batch_slots_export(run.b, 1, z32.ctypes.data, 0, state, run.ch * 5696, (Ticket * 1)()),
            lambda: L.mp3mi_l12_batch_slots_import(run.b, 1, z32.ctypes.data, state, run.ch * 5696, (Ticket * 1)()),
            lambda: L.mp3mi_l12_batch_set_mode(run.b, 1),
            lambda: L.mp3mi_l12_batch_set_error_protection(run.b, 1),
            lambda: L.mp3mi_l12_batch_set_header(run.b, 1, 1, 0),
        ])
        assert L.mp3mi_l12_batch_sync(run.b) == 0
        # no rows, every row array NULL -- and no pcm either: lane 3, ready for longest, gets the slot
        run.mem.upload(run.d_out, np.full(run.S * run.stride, 0xA5, np.uint8))
        rc, slot_lane = run.raw_tick(pcm=False)
        assert rc == 0 and slot_lane == [3]
        assert [(i, s) for i, s, _, _, _ in run.m.tick({})] == [(3, 0)]
        w.got += run.outputs()[0][0]
        run.check_books()
        # lane 1 drains, parked and waiting for the slot: START, END or a push on it are refused; its own bitrate may be passed on
        assert run.tick({1: (d, END, 0)}) == [(0, 0)]
        assert run.lanes()[2][1] == PARKED | DRAINING | WAIT_SLOT
        books = run.books()
        refused([lambda: tick(rows=(1,), ctl=(START,), n=(0,), kbps=(0,)), lambda: tick(rows=(1,), ctl=(END,), n=(0,), kbps=(0,)),
                 lambda: tick(rows=(1,), ctl=(0,), n=(1,), kbps=(0,)), lambda: tick(rows=(0, 1), ctl=(0, 0), n=(0, 0), kbps=(192, 64))])
        rc, slot_lane = run.raw_tick((0, 1), (0, 0), (0, 0), (192, 192))
        assert rc == 0 and slot_lane == [1]
        assert [(i, s) for i, s, _, _, _ in run.m.tick({})] == [(1, 0)]
        d.got += run.outputs()[0][0]
        run.check_books()
        # after every refusal the next ticks' bytes are what they would have been
        churn(run, {0: (None, a, [len(a.pcm) // 2 - 1184]), 3: (None, w, [len(w.pcm) // 2 - 1184])})
        assert d.pos == 1184
        d.pcm = d.pcm[:1184 * 2]
        run.done.append(d)
        check(run, oracle, [a, d, w])
    finally:
        run.close()


# ---- 9. attach and detach ----
@pytest.mark.parametrize("layer", [1, 2])
def test_after_the_feeder_the_batch_is_the_callers_again(emu, oracle, layer):
    spf = SPF[layer]
    run = FeedRun(emu, layer, 3, 4, 44100, "s", KBPS[layer], 2, 2 * spf)
    try:
        L = run.L
        streams = [run.stream(590 + i, 5 * spf, kbps=KBPS[layer]) for i in range(4)]
        for t in range(2):  # streams in slots, parked and waiting when the feeder goes
            run.tick({i: (st, START if t == 0 else 0, 2 * spf) for i, st in enumerate(streams)})
        assert L.mp3mi_l12_batch_set_mode(run.b, 1) == ERR_ARG
        L.mp3mi_l12_feed_destroy(run.f)
        run.f = ctypes.c_void_p()
        assert run.frames() == [-1] * 3
        assert L.mp3mi_l12_batch_set_mode(run.b, 1) == 0 and L.mp3mi_l12_batch_set_mode(run.b, 0) == 0
        pcm = [l12_signal(2 * spf - 9 * s, 2, 600 + s) for s in range(3)]
        rows, ns = np.zeros((3, 2 * spf * 2), np.int16), np.zeros(3, np.int32)
        for s, p in enumerate(pcm):
            rows[s, :len(p)], ns[s] = p, len(p) // 2
        run.put(rows)
        d_ns = run.mem.alloc(12)
        run.mem.upload(d_ns, ns)
        assert L.mp3mi_l12_batch_encode(run.b, run.d_pcm, d_ns, 2, run.d_out, run.stride, run.d_len) == 0
        got = run.outputs()[0]
        for s, p in enumerate(pcm):
            assert got[s] == oracle_l12(oracle, layer, 44100, KBPS[layer], "s", p)[0], s
        # ... and takes a feeder again
        assert L.mp3mi_l12_feed_create(ctypes.byref(run.f), run.b, 4, 4, 2, 2 * spf, 0) == 0
        run.m = type(run.m)(3, 4, 2, spf, run.capacity, run.kbps)
        run.st = [None] * 4
        a = run.stream(610, 3 * spf + 1, kbps=KBPS[layer])
        churn(run, {2: (0, a, cuts(3 * spf + 1, (1000, 160), 2 * spf))})
        check(run, oracle, [a])
    finally:
        run.close(feeder_first=False)  # (the batch goes with the feeder attached)


# ---- 10. the sanitizer program ----
def test_sanitized_feed_program():
    """tests/hipemu/l12_feed_main.cpp under AddressSanitizer, UndefinedBehaviorSanitizer and LeakSanitizer on the emulator: create, ticks
    with waiting, resume and drain, one refusal, destroy in both orders.  Passes when the program exits 0 without a report."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "hipemu"), "-f", "l12_feed.mk", "l12_feed"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
