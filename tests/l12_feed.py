"""The feeder of Layers I and II (mp3mi_l12_feed_*, include/mp3mi_l12.h): helpers shared by the CPU tests (tests/test_l12_feed.py and
tests/test_l12_feed_kernel.py, on the emulated build) and the GPU tests (tests/test_gpu_l12_feed.py).

kernel_case() runs k12_feed alone through mp3mi_debug_l12_feed against a numpy model of ring, rows and history rows.  Model is the
scheduler as the header states it -- who is ready, who encodes, who keeps, leaves and takes which slot, what the flags say -- with no
library involved; a FeedRun drives a batch with a feeder tick by tick beside it and compares, after EVERY tick, slot_lane_host,
mp3mi_l12_feed_lanes, mp3mi_l12_batch_slot_frames and _slot_kbps with the model, and out_len 0 and an untouched output row for the
slots in which nothing encodes.  The judge of the bytes is check_streams() of tests/l12_park.py: the CPU oracle and the library's own
ragged whole-file call, at each stream's bitrate."""
import ctypes

import numpy as np

from l12_park import Stream, bind as bind_park, check_streams
from l12_slots import END, FILL, START, SlotRun
from mp3common import l12_signal

ERR_ARG = -1
HIST, FB = 1792, 1056      # the two history rows of a slot, samples per channel
RESUME = 0x80000000        # word 7 of a descriptor: resume, n_hist below
PARKED, DRAINING, WAITING, WAIT_SLOT = 1, 2, 4, 8  # mp3mi_l12_feed_lanes flags
CANARY = 0x5A5A


def bind(mp):
    L = bind_park(mp)
    vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.mp3mi_l12_feed_create.argtypes = [ctypes.POINTER(vp), vp] + [ci] * 5  # (AttributeError without the feature)
    L.mp3mi_l12_feed_destroy.argtypes = [vp]
    L.mp3mi_l12_feed_destroy.restype = None
    L.mp3mi_l12_feed_capacity.argtypes = [vp]
    L.mp3mi_l12_feed_capacity.restype = sz
    L.mp3mi_l12_feed_n_lanes.argtypes = [vp]
    L.mp3mi_l12_feed_tick.argtypes = [vp, ci, vp, vp, sz, vp, vp, vp, vp, sz, vp, vp]
    L.mp3mi_l12_feed_lanes.argtypes = [vp, vp, vp, vp]
    L.mp3mi_debug_l12_feed.argtypes = [ci] * 7 + [vp, vp, sz, vp, sz, vp, sz, vp, vp]
    L.mp3mi_l12_batch_set_header.argtypes = [vp, ci, ci, ci]
    return L


# ------------------------------------------------------------------------------------------------------------------ the kernel
N_LANES, N_SLOTS, N_PROWS = 5, 3, 6
N_HIST = (384, 1055, 1056, 1057, 1791, 1792)


def kernel_model(desc, cap, ring, push, rows, hist, fb):
    """what the five arrays hold after one launch: everything is read from the arrays as they were before it"""
    ring0 = ring
    ring, rows, hist, fb = ring.copy(), rows.copy(), hist.copy(), fb.copy()
    for head, pending, n, take, ln, pr, sl, w7 in desc:
        stream = np.concatenate([ring0[ln, (head + np.arange(pending)) % cap], push[pr, :n]])
        if take:
            rows[sl, :take] = stream[:take]
        ring[ln, (head + pending + np.arange(n)) % cap] = push[pr, :n]  # ALL pushed samples: those the row took are later history
        if w7 & RESUME:
            nh = w7 & 0x7FFFFFFF
            h = np.concatenate([np.zeros((HIST - nh,) + ring.shape[2:], np.int16), ring0[ln, (head - nh + np.arange(nh)) % cap]])
            hist[sl], fb[sl] = h, h[-FB:]
    return ring, rows, hist, fb


def kernel_descriptors(cap, R):
    """(head, pending, n_push, take, resume word) at which the history span, the pending span and the append wrap at the ring's end,
    each on its own, or end exactly there; take 0 (push only), push 0 (drain), both; every head at eight consecutive samples -- with
    samples of 2 and 4 bytes every misalignment of source against destination from 2 to 14 bytes"""
    scen = [(100, 50, 30, 60),                  # the history wraps; the row takes from ring and push
            (cap - 20, 60, 10, 60),             # the pending span wraps; the push is only appended
            (cap - 100, 90, 40, 0),             # the append wraps; take 0: push only
            (cap - 300, R, 0, R),               # push 0: drain
            (500, 0, R, R),                     # the row straight from the push
            (0, 0, 7, 0),                       # the history ends at the ring's end (and wraps from the second head on)
            (cap - 64, 64, 33, 80),             # the pending span ends at the ring's end
            (200, cap - HIST - 100, 100, R)]    # a full ring: history, pending and append fill it exactly
    out = []
    for k, (head, pending, n, take) in enumerate(scen):
        for off in range(8):
            w7 = (RESUME | N_HIST[(off + k) % 6]) if off != 7 else 0  # a flagged descriptor beside unflagged ones
            out.append(((head + off) % cap, pending, n, take, w7))
    return out


def kernel_call(L, ch, desc, cap, ring, push, rows, hist, fb, row_samples, ring_pitch=None):
    d = np.ascontiguousarray(desc, dtype=np.uint32).reshape(-1, 8)
    return L.mp3mi_debug_l12_feed(ch, len(d), ring.shape[0], push.shape[0], rows.shape[0], cap, row_samples, d.ctypes.data, ring.ctypes.data,
                                  ring.shape[1] if ring_pitch is None else ring_pitch, push.ctypes.data, push.shape[1], rows.ctypes.data,
                                  rows.shape[1], hist.ctypes.data, fb.ctypes.data)


def kernel_case(mp, ch, R):
    """R: samples of a row (a tick of one frame of Layer I or II).  Launch after launch on the same five rings, three slots and their
    history rows; after each the WHOLE ring, the rows, both history rows and the push rows are compared with the model"""
    L = bind(mp)
    cap = HIST + R + 1000 + 3
    assert cap % 8 != 0
    ring_pitch, row_pitch, push_pitch = (cap + 8 + 7) // 8 * 8, R + 16, R + 7
    rng = np.random.default_rng(7 + ch + R)
    ring = np.full((N_LANES, ring_pitch, ch), CANARY, np.int16)
    ring[:, :cap] = rng.integers(1, 10000, (N_LANES, cap, ch))
    push = np.full((N_PROWS, push_pitch, ch), CANARY, np.int16)
    rows = np.full((N_SLOTS, row_pitch, ch), CANARY, np.int16)
    rows[:, :R] = 30000
    hist = np.full((N_SLOTS, HIST, ch), 31000, np.int16)
    fb = np.full((N_SLOTS, FB, ch), 32000, np.int16)
    todo = kernel_descriptors(cap, R)
    launches, seen_nh = 0, set()
    while todo:
        lanes, prows, slots = list(rng.permutation(N_LANES)), list(rng.permutation(N_PROWS)), list(rng.permutation(N_SLOTS))
        desc = []
        for d in list(todo):  # up to five descriptors a launch, three of which may take or resume
            head, pending, n, take, w7 = d
            uses_slot = bool(take or w7)
            if not lanes or (uses_slot and not slots):
                continue
            desc.append((head, pending, n, take, int(lanes.pop()), int(prows.pop()) if n else 0, int(slots.pop()) if uses_slot else 0, w7))
            todo.remove(d)
            if w7:
                seen_nh.add(w7 & 0x7FFFFFFF)
        push[:, :R + 7 - 1] = -rng.integers(1, 10000, (N_PROWS, R + 6, ch))  # negative: never a ring sample
        want = kernel_model(desc, cap, ring, push, rows, hist, fb)
        got = [a.copy() for a in (ring, rows, hist, fb)]
        p2 = push.copy()
        assert kernel_call(L, ch, desc, cap, got[0], p2, got[1], got[2], got[3], R) == 0, desc
        for name, g, w in zip(("ring", "rows", "hist", "fb_hist"), got, want):
            assert np.array_equal(g, w), (name, launches, desc, np.argwhere(g != w)[:4])
        assert np.array_equal(p2, push)
        assert (want[0][:, cap:] == CANARY).all() and (want[1][:, R:] == CANARY).all()  # (the model keeps inside its records)
        ring, rows, hist, fb = want
        launches += 1
    assert seen_nh == set(N_HIST) and launches >= 13
    # each descriptor rule broken once: MP3MI_ERR_ARG, and the buffers are untouched
    ok = (0, 8, 8, 16)
    bad_sets = [
        [(cap, 0, 0, 0, 0, 0, 0, 0)],                                  # head outside the ring
        [(0, cap - HIST, 1, 0, 0, 0, 0, 0)],                           # 1792 + pending + push > cap
        [(0, 5, 5, 11, 0, 0, 0, 0)],                                   # take above what there is
        [(0, R, 100, R + 1, 0, 0, 0, 0)],                              # take above the row
        [(0, 0, push_pitch + 1, 0, 0, 0, 0, 0)],                       # a push beyond its row
        [ok + (N_LANES, 0, 0, 0)], [ok + (0, N_PROWS, 0, 0)], [ok + (0, 0, N_SLOTS, 0)],  # an index out of range
        [ok + (0, 0, 0, RESUME | (HIST + 1))],                         # more history than a row holds
        [ok + (0, 0, 0, 5)], [ok + (0, 0, 0, RESUME | 0x40000000)],    # word 7: a count without the flag, another bit
        [ok + (1, 0, 0, 0), ok + (1, 1, 1, 0)],                        # a lane twice
        [ok + (1, 3, 0, 0), ok + (2, 3, 1, 0)],                        # a push row twice
        [ok + (1, 0, 2, 0), ok + (2, 1, 2, 0)],                        # a slot twice: two that take
        [ok + (1, 0, 2, 0), (0, 8, 0, 0, 2, 0, 2, RESUME | 384)],      # ... one that takes, one that only resumes
    ]
    before = [a.copy() for a in (ring, push, rows, hist, fb)]
    for bad in bad_sets:
        assert kernel_call(L, ch, bad, cap, ring, push, rows, hist, fb, R) == ERR_ARG, bad
    odd_pitch = [q for q in range(cap, cap + 4) if q % 4 == 1][0]  # no multiple of 16 bytes at 2 or 4 bytes a sample
    assert kernel_call(L, ch, [ok + (0, 0, 0, 0)], cap, ring, push, rows, hist, fb, R, ring_pitch=odd_pitch) == ERR_ARG
    for a, b in zip((ring, push, rows, hist, fb), before):
        assert np.array_equal(a, b)
    # the same slot and push row may be named by descriptors that do not use them
    quiet = [(0, 8, 0, 8, 1, 0, 1, 0), (0, 0, 8, 0, 2, 0, 1, 0), (0, 8, 0, 0, 3, 0, 1, 0)]
    want = kernel_model(quiet, cap, ring, push, rows, hist, fb)
    assert kernel_call(L, ch, quiet, cap, ring, push, rows, hist, fb, R) == 0
    for g, w in zip((ring, rows, hist, fb), want):
        assert np.array_equal(g, w)


# --------------------------------------------------------------------------------------------------------------- the scheduler
class MLane:
    def __init__(self):
        self.open, self.pending, self.frames, self.kbps = False, 0, -1, 0
        self.parked = self.draining = self.waiting = self.wait_slot = False
        self.slot, self.since = -1, -1


class Model:
    """Lanes and slots as include/mp3mi_l12.h states them; no library involved.  tick() returns [(lane, slot, closes, started,
    resumed)] of the lanes that encode, ascending by lane, and keeps the history the tests ask about."""

    def __init__(self, S, n_lanes, tick_frames, spf, capacity, slot_kbps):
        self.S, self.spf, self.tick_frames, self.full, self.capacity = S, spf, tick_frames, tick_frames * spf, capacity
        self.slot_kbps = list(slot_kbps)
        self.lane = [MLane() for _ in range(n_lanes)]
        self.slot_lane = [-1] * S
        self.t = 0
        self.over, self.waited, self.parks, self.resumes, self.moved = 0, set(), 0, 0, False
        self.slots_of = [[] for _ in range(n_lanes)]  # the slots a lane's current stream encoded in, tick by tick
        self.resumed_at = []                           # samples a stream had encoded when it was resumed

    def tick(self, feeds):
        """feeds: {lane: (ctl, n, kbps)}"""
        ready, closes = [], {}
        for i, l in enumerate(self.lane):
            c, n, k = feeds.get(i, (0, 0, 0))
            if c & START:  # a new stream; one that is open in the lane is abandoned
                l.open, l.pending, l.frames, l.kbps = True, 0, 0, k
                l.parked = l.draining = False
                l.waiting = True
                self.slots_of[i] = []
            if not l.open:
                assert n == 0 and not c & END
                continue
            l.pending += n
            assert l.pending <= self.capacity, "the plan overruns lane %d's FIFO" % i
            l.draining |= bool(c & END)
            closes[i] = l.draining and l.pending <= self.full
            if closes[i] or l.pending >= self.full:
                if l.since < 0:
                    l.since = self.t  # the spell of being ready begins
                ready.append(i)
            else:
                l.since, l.wait_slot = -1, False
        self.over += len(ready) > self.S
        chosen = sorted(sorted(ready, key=lambda i: (self.lane[i].since, i))[:self.S])
        for s in range(self.S):  # every stream in a slot whose lane does not encode leaves it
            i = self.slot_lane[s]
            if i >= 0 and i not in chosen:
                l = self.lane[i]
                l.parked, l.slot, self.slot_lane[s] = not l.waiting, -1, -1
                self.parks += 1
        free = [s for s in range(self.S) if self.slot_lane[s] < 0]
        out = []
        for i in ready:
            l = self.lane[i]
            if i not in chosen:
                l.wait_slot = True
                self.waited.add(i)
                continue
            resumed = False
            if l.slot < 0:
                l.slot = free.pop(0)  # the lowest free slot to the lowest lane
                resumed = l.parked
                if resumed:
                    self.resumes += 1
                    self.resumed_at.append(l.frames * self.spf)
            s, started = l.slot, l.waiting
            if started and l.kbps == 0:
                l.kbps = self.slot_kbps[s]
            take = l.pending if closes[i] else self.full
            l.pending -= take
            l.frames += (take + self.spf - 1) // self.spf if closes[i] else self.tick_frames
            l.parked = l.waiting = l.wait_slot = False
            l.since = -1
            self.slots_of[i].append(s)
            self.moved |= len(set(self.slots_of[i])) > 1
            self.slot_lane[s] = i
            out.append((i, s, closes[i], started, resumed))
        for i, s, c, _, _ in out:
            if c:
                l = self.lane[i]
                l.open, l.frames, l.slot, self.slot_lane[s] = False, -1, -1, -1
        self.t += 1
        return out

    def flags(self):
        return [(PARKED * l.parked | DRAINING * l.draining | WAITING * l.waiting | WAIT_SLOT * l.wait_slot) if l.open else 0 for l in self.lane]


class FeedRun(SlotRun):
    """a Layer I / II slot batch with a feeder, driven tick by tick beside the Model.  mode, kbps: as SlotRun takes them"""

    def __init__(self, mp, layer, S, n_lanes, rate, mode, kbps, tick, max_push, max_rows=None, ring=0):
        SlotRun.__init__(self, mp, layer, S, rate, mode, kbps, tick)
        self.L = bind(mp)
        self.n_lanes, self.tick_frames, self.full, self.max_push = n_lanes, tick, tick * self.spf, max_push
        self.max_rows = n_lanes if max_rows is None else max_rows
        self.f = ctypes.c_void_p()
        assert self.L.mp3mi_l12_feed_create(ctypes.byref(self.f), self.b, n_lanes, self.max_rows, tick, max_push, ring) == 0
        self.capacity = ring if ring else self.full + max_push
        assert self.L.mp3mi_l12_feed_capacity(self.f) == self.capacity and self.L.mp3mi_l12_feed_n_lanes(self.f) == n_lanes
        self.pitch = max_push + 3  # (rows that begin at every alignment)
        self.d_push = self.mem.alloc(self.max_rows * self.pitch * self.ch * 2)
        self.m = Model(S, n_lanes, tick, self.spf, self.capacity, self.kbps)
        self.st = [None] * n_lanes  # the Stream in each lane
        self.ticks, self.order, self.done = 0, [], []

    def stream(self, seed, n_per_ch, kbps=None, noise=False):
        """kbps None: 0 at START, the create-time bitrate of the slot the stream first encodes in (booked in the Stream then)"""
        from l12_slots import loud
        pcm = loud(n_per_ch * self.ch, seed) if noise else l12_signal(max(n_per_ch, 1), self.ch, seed, self.rate)[:n_per_ch * self.ch]
        return Stream(pcm, 0 if kbps is None else kbps, self.ch)

    def lanes(self):
        n = self.n_lanes
        p, f, g = np.full(n, -7, np.int32), np.full(n, -7, np.int64), np.full(n, 77, np.uint8)
        k = self.L.mp3mi_l12_feed_lanes(self.f, p.ctypes.data, f.ctypes.data, g.ctypes.data)
        return [int(x) for x in p], [int(x) for x in f], [int(x) for x in g], k

    def books(self):
        k = np.full(self.S, -7, np.int32)
        assert self.L.mp3mi_l12_batch_slot_kbps(self.b, k.ctypes.data) == max(self.kbps)
        return self.lanes(), self.frames(), [int(x) for x in k]

    def check_books(self):
        ml, sl = self.m.lane, self.m.slot_lane
        (p, f, g, n), frames, kb = self.books()
        assert n == sum(l.open for l in ml)
        assert p == [l.pending if l.open else 0 for l in ml], p
        assert f == [l.frames for l in ml], f
        assert g == self.m.flags(), (g, self.m.flags())
        assert frames == [ml[i].frames if i >= 0 else -1 for i in sl], (frames, sl)  # a parked lane's slot reads as closed
        assert kb == [ml[i].kbps if i >= 0 else self.kbps[s] for s, i in enumerate(sl)], kb

    def raw_tick(self, rows=(), ctl=(), n_push=(), kbps=(), pcm=True, out=True, out_len=True, sl=True, stride=None, pitch=None, f=True,
                 null=(), n_rows=None):
        """one mp3mi_l12_feed_tick as given; null: names of row arrays to pass as NULL.  Returns (rc, slot_lane)"""
        arr = dict(rows=np.ascontiguousarray(rows, np.int32), ctl=np.ascontiguousarray(ctl, np.uint8),
                   n_push=np.ascontiguousarray(n_push, np.int32), kbps=np.ascontiguousarray(kbps, np.int32))
        R = len(arr["rows"]) if n_rows is None else n_rows
        ptr = {k: (None if k in null or (R == 0 and n_rows is None) else a.ctypes.data) for k, a in arr.items()}
        slot_lane = np.full(self.S, -9, np.int32)
        rc = self.L.mp3mi_l12_feed_tick(self.f if f else None, R, ptr["rows"], self.d_push if pcm else None,
                                        self.pitch if pitch is None else pitch, ptr["ctl"], ptr["n_push"], ptr["kbps"],
                                        self.d_out if out else None, self.stride if stride is None else stride,
                                        self.d_len if out_len else None, slot_lane.ctypes.data if sl else None)
        for a in arr.values():
            a[...] = 99  # (the library has copied them)
        return rc, [int(x) for x in slot_lane]

    def tick(self, feeds):
        """feeds: {lane: (stream, ctl, n)} -- stream: the lane's (a new one with START).  Books the bytes every lane delivered, checks
        the books against the model and returns [(lane, slot)] of the lanes that encoded"""
        ch = self.ch
        rows = sorted(feeds)
        assert len(rows) <= self.max_rows
        pcm = np.full((self.max_rows, self.pitch * ch), CANARY, np.int16)
        ctl, ns, kb, mfeeds = [], [], [], {}
        for r, i in enumerate(rows):
            st, c, n = feeds[i]
            assert (c & START) or self.st[i] is st
            if c & START:
                self.st[i] = st
                st.frames, st.got = 0, b""
            k = st.kbps if c & START else 0
            ctl.append(c), ns.append(n), kb.append(k)
            mfeeds[i] = (c, n, k)
            pcm[r, :n * ch] = st.take(n)
        self.mem.upload(self.d_push, pcm)
        self.mem.upload(self.d_out, np.full(self.S * self.stride, FILL, np.uint8))
        self.mem.upload(self.d_len, np.full(self.S, 0xFFFFFFFF, np.uint32))
        rc, slot_lane = self.raw_tick(rows, ctl, ns, kb)
        assert rc == 0, rc
        enc = self.m.tick(mfeeds)
        self.ticks += 1
        want = [-1] * self.S
        for i, s, closes, started, _ in enc:
            want[s] = i
            if started:
                self.st[i].kbps = self.m.lane[i].kbps  # (kbps 0: the create-time bitrate of the slot it first encodes in)
        assert slot_lane == want, (slot_lane, want)
        self.order.append(sorted(i for i, _, _, _, _ in enc))
        outs, lens, raw = self.outputs()
        for i, s, closes, _, _ in enc:
            self.st[i].got += outs[s]
        for s in range(self.S):
            if want[s] < 0:
                assert lens[s] == 0, (s, lens)
                assert (raw[s] == FILL).all(), "the tick wrote into the row of slot %d, in which nothing encodes" % s
        self.check_books()
        for i, s, closes, _, _ in enc:
            if closes:
                self.done.append(self.st[i])
                self.st[i] = None
        return [(i, s) for i, s, _, _, _ in enc]

    def close(self, feeder_first=True):
        if self.f and feeder_first:
            self.L.mp3mi_l12_feed_destroy(self.f)
        self.f = ctypes.c_void_p()
        SlotRun.close(self)


def cuts(n, sizes, max_push):
    """n samples cut into pushes that walk through `sizes`"""
    out, k = [], 0
    while n > 0:
        out.append(min(n, max_push, sizes[k % len(sizes)]))
        n -= out[-1]
        k += 1
    return out or [0]


def churn(run, plans, limit=400):
    """plans: {lane: (first tick, stream, [pushes])}: from its first tick on a lane pushes its next piece in every tick in which its FIFO
    has room for it (a waiting lane's FIFO fills up: the server holds the packet back), the first with START, the last with END.  A
    first tick of None: the stream is open in the lane already, no START.  Ticks until every lane has closed."""
    todo = {i: [t0 or 0, st, list(p), t0 is not None] for i, (t0, st, p) in plans.items()}
    t_first = run.ticks
    while todo or any(l.open for l in run.m.lane):
        feeds = {}
        for i in sorted(todo):
            t0, st, p, first = todo[i]
            if run.ticks - t_first < t0 or (not first and run.m.lane[i].pending + p[0] > run.capacity):
                continue
            n = p.pop(0)
            feeds[i] = (st, (START if first else 0) | (0 if p else END), n)
            todo[i][3] = False
            if not p:
                del todo[i]
        run.tick(feeds)
        assert run.ticks - t_first < limit


def check(run, oracle, streams):
    """every stream: fed to its last sample, closed, and its file the oracle's and the ragged whole-file call's"""
    assert streams and all(st.pos * st.ch == len(st.pcm) for st in streams), [(st.pos, len(st.pcm)) for st in streams]
    assert all(any(st is d for d in run.done) for st in streams)
    check_streams(run, oracle, streams, len(streams))


# ---------------------------------------------------------------------------------------------------------------- scenarios
def more_lanes_case(mp, oracle, layer, tick, S=3, n_lanes=5, seed=0, mode="s"):
    """seeded arrival over more lanes than slots: every lane runs one stream of a few ticks less an odd count, in awkward pushes"""
    spf = 384 if layer == 1 else 1152
    full = tick * spf
    run = FeedRun(mp, layer, S, n_lanes, 44100, mode, 192 if layer == 1 else 128, tick, full, ring=3 * full)
    try:
        rng = np.random.default_rng(100 * layer + 10 * tick + seed)
        plans, streams = {}, []
        for i in range(n_lanes):
            n = int(rng.integers(2, 5)) * full - int(rng.integers(1, spf))
            st = run.stream(400 + i, n, kbps=run.kbps[0])
            sizes = [int(x) for x in rng.choice([1, 7, 160, 959, 960, 1000, full], 5)]
            plans[i] = (0 if i < 4 else int(rng.integers(1, 3)), st, [full] + cuts(n - full, sizes, full))  # a whole tick at START: ready at once,
            # four lanes in the first tick: more than slots
            streams.append(st)
        churn(run, plans)
        m = run.m
        assert m.over > 0 and m.waited and m.parks > 0 and m.resumes > 0 and m.moved, (m.over, m.waited, m.parks, m.resumes, m.moved)
        check(run, oracle, streams)
    finally:
        run.close()


def back_to_back_case(mp, oracle, layer, n_ticks=8, S=4, n_lanes=6):
    """n_ticks ticks issued back to back with no sync until the end -- more than the upload ring has entries, so the host meets its
    fences --, every tick with push rows and output buffers of its own; the model alone says who encodes where.  Lane i STARTs in tick
    i % 3 with a tick of samples, pushes a tick more, then ENDs on a partial one: lanes wait, leave and resume on the way"""
    spf = 384 if layer == 1 else 1152
    run = FeedRun(mp, layer, S, n_lanes, 44100, "s", 192 if layer == 1 else 128, 1, spf, ring=3 * spf)
    try:
        mem, ch, stride = run.mem, run.ch, run.stride
        streams = [run.stream(700 + i, 3 * spf - 20 - i, kbps=run.kbps[0]) for i in range(n_lanes)]
        plan = [dict() for _ in range(n_ticks)]
        for i in range(n_lanes):
            for k, (c, n) in enumerate([(START, spf), (0, spf), (END, spf - 20 - i)]):
                plan[i % 3 + k][i] = (c, n)
        issued = []
        for t, feeds in enumerate(plan):
            rows = sorted(feeds)
            pcm = np.full((run.max_rows, run.pitch * ch), CANARY, np.int16)
            for r, i in enumerate(rows):
                pcm[r, :feeds[i][1] * ch] = streams[i].take(feeds[i][1])
            d_push, d_out, d_len = mem.alloc(pcm.nbytes), mem.alloc(S * stride), mem.alloc(4 * S)
            mem.upload(d_push, pcm)
            mem.upload(d_out, np.full(S * stride, FILL, np.uint8))
            mem.upload(d_len, np.full(S, 0xFFFFFFFF, np.uint32))
            issued.append((rows, d_push, d_out, d_len))
        wants = []
        for (rows, d_push, d_out, d_len), feeds in zip(issued, plan):  # no sync, no upload, no download in between
            a = lambda x, t: np.ascontiguousarray(x, dtype=t)
            rl, ctl, ns = a(rows, np.int32), a([feeds[i][0] for i in rows], np.uint8), a([feeds[i][1] for i in rows], np.int32)
            kb = a([run.kbps[0] if feeds[i][0] & START else 0 for i in rows], np.int32)
            sl = np.full(S, -9, np.int32)
            R = len(rows)
            p = lambda x: x.ctypes.data if R else None
            assert run.L.mp3mi_l12_feed_tick(run.f, R, p(rl), d_push if R else None, run.pitch, p(ctl), p(ns), p(kb), d_out, stride, d_len,
                                             sl.ctypes.data) == 0
            enc = run.m.tick({i: (feeds[i][0], feeds[i][1], run.kbps[0] if feeds[i][0] & START else 0) for i in rows})
            want = [-1] * S
            for i, s, _, _, _ in enc:
                want[s] = i
            assert [int(x) for x in sl] == want, (sl, want)
            wants.append(want)
        assert run.L.mp3mi_l12_batch_sync(run.b) == 0
        run.check_books()
        assert run.m.over > 0 and run.m.resumes > 0 and not any(l.open for l in run.m.lane)
        for (rows, d_push, d_out, d_len), want in zip(issued, wants):
            out, lens = mem.download(d_out, (S, stride), np.uint8), mem.download(d_len, (S,), np.uint32)
            for s, i in enumerate(want):
                if i >= 0:
                    streams[i].got += out[s, :lens[s]].tobytes()
                else:
                    assert lens[s] == 0 and (out[s] == FILL).all(), s
        run.done += streams
        check(run, oracle, streams)
    finally:
        run.close()
