"""Parking and resuming the streams of a slot batch (mp3mi_batch_slots_export / mp3mi_batch_slots_import, include/mp3mi.h): a
stream leaves its slot as a ticket and a device record and goes on later in any closed slot, of the same batch or of another
one of the same format.  The judge is the oracle: the bytes a stream delivered from its START through its END, concatenated
over every slot and batch it lived in, are the oracle's file of its samples at its bitrate -- exact equality throughout."""
import ctypes

import numpy as np
import pytest

from golden_util import aborting_cases, case_pcm, encoding_cases
from mp3common import ERR_REFERENCE_ABORT
from test_slots_host import HostRun
from test_stream_slots import END, START, SlotRun

ERR_ARG = -1
MAGIC, VERSION = 0x4B54334D, 1  # MP3MI_SLOT_TICKET_MAGIC, MP3MI_SLOT_TICKET_VERSION


class Ticket(ctypes.Structure):
    """include/mp3mi.h: mp3mi_slot_ticket"""
    _fields_ = [("magic", ctypes.c_uint32), ("version", ctypes.c_uint32), ("state_bytes", ctypes.c_uint64),
                ("rate_hz", ctypes.c_int32), ("channels", ctypes.c_int32), ("hdr_mode", ctypes.c_int32), ("hdr_flags", ctypes.c_int32),
                ("error_protection", ctypes.c_int32), ("kbps", ctypes.c_int32), ("frames", ctypes.c_int64)]


def bind(mp):
    L = mp.lib
    L.mp3mi_batch_slot_state_bytes.restype = ctypes.c_size_t
    L.mp3mi_batch_slot_state_bytes.argtypes = [ctypes.c_void_p]
    L.mp3mi_batch_slots_export.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                           ctypes.c_void_p]
    L.mp3mi_batch_slots_import.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.mp3mi_batch_encode_slots_kbps.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.mp3mi_batch_slot_kbps.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return L


class Stream:
    """one stream: its PCM (interleaved), its bitrate, how far it has been fed and the bytes every call delivered for it"""

    def __init__(self, pcm, ch, kbps):
        self.pcm, self.ch, self.kbps, self.pos, self.calls, self.frames = pcm, ch, kbps, 0, [], 0

    def take(self, n):
        piece = self.pcm[self.pos * self.ch:(self.pos + n) * self.ch]
        assert len(piece) == n * self.ch, "the stream's PCM is too short for the plan"
        self.pos += n
        return piece

    def data(self):
        return b"".join(self.calls)

    def fed(self):
        return self.pcm[:self.pos * self.ch]


class Parked:
    """streams out of their slots: the device records (d, stride apart), the tickets, the Stream objects"""

    def __init__(self, d, stride, tickets, streams):
        self.d, self.stride, self.tickets, self.streams = d, stride, tickets, streams


class ParkRun(SlotRun):
    """SlotRun that knows which Stream is open in which slot: step() feeds them a call and books the bytes, export() / import_()
    move them out of and into slots; after every accepted call mp3mi_batch_slot_frames and mp3mi_batch_slot_kbps must agree"""

    def __init__(self, mp, S, rate, ch, kbps, nf, **kw):
        SlotRun.__init__(self, mp, S, rate, ch, kbps, nf, **kw)
        bind(mp)
        self.state_bytes = self.L.mp3mi_batch_slot_state_bytes(self.b)
        assert self.state_bytes > 0 and self.state_bytes % 16 == 0
        self.open = {}

    def slot_kbps(self):
        k = np.full(self.S, -7, np.int32)
        return list(k), self.L.mp3mi_batch_slot_kbps(self.b, k.ctypes.data), k

    def check_books(self):
        assert list(self.frames()) == [self.open[s].frames if s in self.open else -1 for s in range(self.S)]
        _, ceil, k = self.slot_kbps()
        assert ceil == max(self.kbps)
        assert list(k) == [self.open[s].kbps if s in self.open else self.kbps[s] for s in range(self.S)], list(k)

    def step(self, feeds, nf=None, abort=False, kbps0=False):
        """feeds: {slot: (stream, ctl, n)} -- n: the samples of a stream that ENDs in the call.  Every open slot must be fed.
        kbps0: STARTs pass kbps 0 (the slot's create-time bitrate) and the stream's .kbps says what that is."""
        nf = self.nf if nf is None else nf
        full = nf * 1152
        assert set(self.open) <= set(feeds), "an open slot without samples"
        pcm = np.zeros((self.S, full * self.ch), np.int16)
        ctl, ns, kb = np.zeros(self.S, np.uint8), np.zeros(self.S, np.int32), np.zeros(self.S, np.int32)
        for s, (st, c, n) in feeds.items():
            assert (c & START) or self.open.get(s) is st
            ctl[s], ns[s] = c, (n if c & END else full)
            kb[s] = 0 if kbps0 or not (c & START) else st.kbps
            piece = st.take(ns[s])
            pcm[s, :len(piece)] = piece
        self.mem.upload(self.d_pcm, pcm)
        assert self.L.mp3mi_batch_encode_slots_kbps(self.b, self.d_pcm, nf, ctl.ctypes.data, ns.ctypes.data, kb.ctypes.data, self.d_out,
                                                    self.stride, self.d_len) == 0
        rc = self.L.mp3mi_batch_sync(self.b)
        assert rc == (ERR_REFERENCE_ABORT if abort else 0), rc
        outs, lens = self.outputs()
        for s in range(self.S):
            if s not in feeds:
                assert lens[s] == 0, s
                continue
            st, c, n = feeds[s]
            st.calls.append(outs[s])
            st.frames += (n + 1151) // 1152 if c & END else nf
            if c & END:
                self.open.pop(s, None)
            else:
                self.open[s] = st
        self.check_books()

    def export(self, slots, close=True, stride=None):
        n = len(slots)
        stride = self.state_bytes if stride is None else stride
        d = self.mem.alloc(n * stride)
        tickets = (Ticket * n)()
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        assert self.L.mp3mi_batch_slots_export(self.b, n, sl.ctypes.data, 1 if close else 0, d, stride, ctypes.addressof(tickets)) == 0
        sl[...] = -1  # (the library has copied the list)
        streams = [self.open[s] for s in slots]
        for t, st in zip(tickets, streams):
            assert (t.magic, t.version, t.state_bytes, t.rate_hz, t.channels) == (MAGIC, VERSION, self.state_bytes, self.rate, self.ch)
            assert (t.kbps, t.frames) == (st.kbps, st.frames), (t.kbps, t.frames)
        if close:
            for s in slots:
                del self.open[s]
        self.check_books()
        return Parked(d, stride, tickets, streams)

    def import_(self, slots, parked, streams=None):
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        assert self.L.mp3mi_batch_slots_import(self.b, len(slots), sl.ctypes.data, parked.d, parked.stride, ctypes.addressof(parked.tickets)) == 0
        sl[...] = -1
        for s, st in zip(slots, parked.streams if streams is None else streams):
            self.open[s] = st
        self.check_books()


def oracle_exact(oracle, run, streams, mode=None):
    for st in streams:
        ref = oracle.encode(st.fed(), run.rate, st.kbps, run.ch, mode=mode)[0]
        assert st.data() == ref, "%d samples at %d kbps: %d bytes vs the oracle's %d" % (st.pos, st.kbps, len(st.data()), len(ref))


def attacks_pcm(mp):
    """44.1 kHz stereo with attacks: block switching and pre-echo history, which a forgotten piece of the psy state changes"""
    case = [c for c in encoding_cases() if c["name"] == "s44_128_bursty"][0]
    return case_pcm(case, mp.synth)


def stream_of(mp, run, seed, kbps=None, frames=12, pcm=None):
    return Stream(mp.synth(frames * 1152, run.ch, run.rate, seed) if pcm is None else pcm, run.ch, run.kbps[0] if kbps is None else kbps)


# ---- 1 and 3: park, wait, resume in the same slot ----
def same_slot_case(mp, oracle, rate, ch, kbps, mode=None, crc=False, omode=None, golden=False):
    """slot 0 STARTs, runs two calls and is parked; two calls go by without it; it resumes in slot 0, runs two calls and ENDs on
    1000 samples.  Slot 1 runs throughout, slot 2 STARTs and ENDs while slot 0 is away.  Returns whether the call before the
    park left bytes behind (it delivered fewer than its frames hold: they travel in the record's carry)."""
    run = ParkRun(mp, 3, rate, ch, kbps, 2, mode=mode, crc=crc)
    try:
        a = stream_of(mp, run, 21, pcm=attacks_pcm(mp) if golden else None)
        b, c = stream_of(mp, run, 22, frames=16), stream_of(mp, run, 23)
        run.step({0: (a, START, 0), 1: (b, START, 0)})
        run.step({0: (a, 0, 0), 1: (b, 0, 0)})
        frame_bytes = int(1152 / (rate / 1000.0) * (kbps / 8.0))
        carried = len(a.calls[-1]) < 2 * frame_bytes
        parked = run.export([0])
        assert list(run.frames()) == [-1, 4, -1]
        run.step({1: (b, 0, 0), 2: (c, START, 0)})
        run.step({1: (b, 0, 0), 2: (c, END, 700)})
        run.import_([0], parked)
        assert list(run.frames()) == [4, 8, -1]
        run.step({0: (a, 0, 0), 1: (b, 0, 0)})
        run.step({0: (a, 0, 0), 1: (b, 0, 0)})
        run.step({0: (a, END, 1000), 1: (b, END, 5)})
        assert (a.pos, b.pos, c.pos) == (4 * 2304 + 1000, 6 * 2304 + 5, 2304 + 700)
        oracle_exact(oracle, run, [a, b, c], mode=omode)
        return carried
    finally:
        run.close()


FORMATS = [dict(rate=44100, ch=2, kbps=128, golden=True), dict(rate=48000, ch=2, kbps=192), dict(rate=32000, ch=1, kbps=56),
           dict(rate=44100, ch=1, kbps=320), dict(rate=44100, ch=2, kbps=128, crc=True, mode=0, omode="se"),
           dict(rate=44100, ch=2, kbps=128, mode=2, omode="d")]


def formats_case(mp, oracle):
    carried = [same_slot_case(mp, oracle, **f) for f in FORMATS]
    assert any(carried), "no park with bytes in the carry"


def test_park_and_resume_in_every_format_emulated(emu, oracle):
    formats_case(emu, oracle)


# ---- 2: resume in a different, dirty slot ----
def dirty_slot_case(mp, oracle):
    """the stream parked out of slot 0 resumes in slot 1, where another stream ran on and ENDed after the park; slot 0 takes a
    new stream meanwhile"""
    run = ParkRun(mp, 3, 44100, 2, 128, 2)
    try:
        a, b, d = stream_of(mp, run, 31, pcm=attacks_pcm(mp)), stream_of(mp, run, 32), stream_of(mp, run, 33)
        run.step({0: (a, START, 0), 1: (b, START, 0)})
        run.step({0: (a, 0, 0), 1: (b, 0, 0)})
        parked = run.export([0])
        run.step({1: (b, END, 1500)})
        run.import_([1], parked)
        assert list(run.frames()) == [-1, 4, -1]
        run.step({0: (d, START, 0), 1: (a, 0, 0)})
        run.step({0: (d, 0, 0), 1: (a, 0, 0)})
        run.step({0: (d, END, 2304), 1: (a, END, 1000)})
        oracle_exact(oracle, run, [a, b, d])
    finally:
        run.close()


def test_resume_in_a_dirty_slot_emulated(emu, oracle):
    dirty_slot_case(emu, oracle)


# ---- 4: migration to another batch ----
def migration_case(mp, oracle):
    """batch A (three slots at 128) parks a stream; batch B (four slots created at 320) imports it as its very first call, runs
    it at 128 to its END, and afterwards STARTs a stream with kbps 0 in the same slot, which encodes at 320"""
    A = ParkRun(mp, 3, 44100, 2, 128, 2)
    B = ParkRun(mp, 4, 44100, 2, 320, 2)
    try:
        a, n = stream_of(mp, A, 41, pcm=attacks_pcm(mp)), stream_of(mp, A, 42)
        A.step({0: (a, START, 0), 2: (n, START, 0)})
        A.step({0: (a, 0, 0), 2: (n, 0, 0)})
        parked = A.export([0])
        assert A.L.mp3mi_batch_sync(A.b) == 0  # the record is whole before another batch reads it
        A.step({2: (n, END, 900)})
        B.import_([2], parked)
        assert B.slot_kbps()[2].tolist() == [320, 320, 128, 320] and list(B.frames()) == [-1, -1, 4, -1]
        B.step({2: (a, 0, 0)})
        B.step({2: (a, 0, 0)})
        B.step({2: (a, END, 1000)})
        assert B.slot_kbps()[2].tolist() == [320] * 4
        z = stream_of(mp, B, 43, kbps=320)
        B.step({2: (z, START, 0)}, kbps0=True)
        B.step({2: (z, END, 2000)})
        oracle_exact(oracle, A, [a, n, z])
    finally:
        A.close()
        B.close()


def test_migration_to_another_batch_emulated(emu, oracle):
    migration_case(emu, oracle)


# ---- 5: snapshot and fork ----
def snapshot_case(mp, oracle):
    """export with close = 0 at frame 4: the stream runs on to its END (file F); the snapshot, imported into another slot
    afterwards and fed the same remaining PCM, delivers F's bytes from the snapshot on, call for call"""
    run = ParkRun(mp, 3, 44100, 2, 128, 2)
    try:
        pcm = attacks_pcm(mp)
        a = Stream(pcm, 2, 128)
        run.step({0: (a, START, 0)})
        run.step({0: (a, 0, 0)})
        snap = run.export([0], close=False)
        assert list(run.frames()) == [4, -1, -1]
        run.step({0: (a, 0, 0)})
        run.step({0: (a, 0, 0)})
        run.step({0: (a, END, 1000)})
        oracle_exact(oracle, run, [a])
        fork = Stream(pcm, 2, 128)
        fork.pos, fork.frames = 4 * 1152, 4
        run.import_([2], snap, streams=[fork])
        run.step({2: (fork, 0, 0)})
        run.step({2: (fork, 0, 0)})
        run.step({2: (fork, END, 1000)})
        assert fork.calls == a.calls[2:]
    finally:
        run.close()


def test_snapshot_and_fork_emulated(emu, oracle):
    snapshot_case(emu, oracle)


# ---- 6: whole-batch bookkeeping ----
def whole_batch_case(mp, oracle):
    """a batch driven by encode_next alone: a snapshot leaves the whole-batch bookkeeping in charge; slot 1 is parked for one
    call and resumes; the flush ends all three"""
    run = ParkRun(mp, 3, 44100, 2, 128, 2)
    try:
        L = run.L
        st = [stream_of(mp, run, 61 + s, pcm=attacks_pcm(mp) if s == 1 else None) for s in range(3)]

        def encode_next(slots):
            pcm = np.zeros((3, run.row), np.int16)
            for s in slots:
                pcm[s] = st[s].take(2304)
            run.mem.upload(run.d_pcm, pcm)
            assert L.mp3mi_batch_encode_next(run.b, run.d_pcm, 2, run.d_out, run.stride, run.d_len) == 0 and L.mp3mi_batch_sync(run.b) == 0
            outs, lens = run.outputs()
            for s in range(3):
                if s in slots:
                    st[s].calls.append(outs[s])
                    st[s].frames += 2
                else:
                    assert lens[s] == 0

        encode_next([0, 1, 2])
        run.open = {s: st[s] for s in range(3)}
        run.export([0], close=False)
        assert list(run.frames()) == [2, 2, 2]
        encode_next([0, 1, 2])
        parked = run.export([1])
        assert list(run.frames()) == [4, -1, 4]
        encode_next([0, 2])
        run.import_([1], parked)
        assert list(run.frames()) == [6, 4, 6]
        encode_next([0, 1, 2])
        assert list(run.frames()) == [8, 6, 8]
        assert L.mp3mi_batch_flush(run.b, run.d_out, run.stride, run.d_len) == 0 and L.mp3mi_batch_sync(run.b) == 0
        outs, _ = run.outputs()
        for s in range(3):
            st[s].calls.append(outs[s])
        assert list(run.frames()) == [-1, -1, -1]
        assert [x.pos for x in st] == [8 * 1152, 6 * 1152, 8 * 1152]
        oracle_exact(oracle, run, st)
    finally:
        run.close()


def test_whole_batch_bookkeeping_emulated(emu, oracle):
    whole_batch_case(emu, oracle)


# ---- 7: the status travels ----
def void_stream_case(mp, oracle):
    """abort_global_gain dies in frame 4, before the park: from its new slot it reports the same status, delivers nothing and is
    not reported a second time; the neighbour is the oracle's"""
    case = [c for c in aborting_cases() if c["name"] == "abort_global_gain"][0]
    bad_pcm = np.concatenate([case_pcm(case, mp.synth), np.zeros(6 * 1152 * 2, np.int16)])  # 6 frames, then silence
    run = ParkRun(mp, 3, 44100, 2, 128, 2)
    try:
        good, bad = stream_of(mp, run, 71), Stream(bad_pcm, 2, 128)
        run.step({0: (good, START, 0), 1: (bad, START, 0)})
        run.step({0: (good, 0, 0), 1: (bad, 0, 0)})
        run.step({0: (good, 0, 0), 1: (bad, 0, 0)}, abort=True)
        want = case["reference_aborts"]["status"] | case["reference_aborts"]["frame"] << 8
        assert run.status()[1] == want
        parked = run.export([1])
        run.import_([2], parked)
        assert run.status()[2] == want and run.status()[0] == 0
        run.step({0: (good, 0, 0), 2: (bad, 0, 0)})  # (the sync inside reports nothing: the abort was reported before the park)
        run.step({0: (good, END, 1000), 2: (bad, END, 100)})
        assert run.status()[2] == want and run.status()[0] == 0
        assert bad.calls[2:] == [b""] * 3  # nothing from the call it died in on
        oracle_exact(oracle, run, [good])
    finally:
        run.close()


def kept_status_case(mp, oracle):
    """a flush ends abort_flush_slot in slot 0 (the reference dies in its final flush) and keeps its status for the next call to
    put back; a healthy stream parked before the flush resumes in that very slot in between: its status stays 0, its bytes the
    oracle's"""
    case = [c for c in aborting_cases() if c["name"] == "abort_flush_slot"][0]
    run = ParkRun(mp, 2, 48000, 2, 64, 2)
    try:
        bad, good = Stream(case_pcm(case, mp.synth), 2, 64), stream_of(mp, run, 72)  # bad: 5 frames
        run.step({0: (bad, START, 0), 1: (good, START, 0)})
        run.step({0: (bad, 0, 0), 1: (good, 0, 0)})
        run.step({0: (bad, 0, 0), 1: (good, 0, 0)}, nf=1)
        parked = run.export([1])
        assert run.L.mp3mi_batch_flush(run.b, run.d_out, run.stride, run.d_len) == 0
        assert run.L.mp3mi_batch_sync(run.b) == ERR_REFERENCE_ABORT
        _, lens = run.outputs()
        assert list(lens) == [0, 0]
        run.open = {}
        want = case["reference_aborts"]["status"] | case["reference_aborts"]["frame"] << 8
        assert list(run.status()) == [want, 0]
        run.import_([0], parked)
        assert list(run.status()) == [0, 0]
        run.step({0: (good, 0, 0)})
        assert list(run.status()) == [0, 0]
        run.step({0: (good, 0, 0)})
        run.step({0: (good, END, 1000)})
        assert good.pos == 9 * 1152 + 1000
        oracle_exact(oracle, run, [good])
    finally:
        run.close()


def test_void_stream_stays_void_emulated(emu, oracle):
    void_stream_case(emu, oracle)


def test_kept_status_does_not_reach_a_resumed_stream_emulated(emu, oracle):
    kept_status_case(emu, oracle)


# ---- 8: host rows ----
def host_rows_case(mp, oracle):
    """per-slot calls on host buffers with a row map: a parked slot must not be given a row, a resumed one must"""
    run = ParkRun(mp, 3, 44100, 2, 128, 2)
    host = HostRun(mp, 3, 44100, 2, 128, 2, b=run.b)
    try:
        a, b = stream_of(mp, run, 81, pcm=attacks_pcm(mp)), stream_of(mp, run, 82)

        def tick(rows, feeds, want=0):
            """feeds: per row (stream, ctl, n)"""
            pcm = np.zeros((len(rows), run.row), np.int16)
            ns = np.array([n if c & END else 2304 for _, c, n in feeds], np.int32)
            pos = [st.pos for st, _, _ in feeds]
            for r, (st, c, n) in enumerate(feeds):
                piece = st.take(ns[r])
                pcm[r, :len(piece)] = piece
            rc, out, lens = host.tick(rows, pcm, [c for _, c, _ in feeds], ns)
            assert rc == want, rc
            if rc != 0:
                for (st, _, _), p in zip(feeds, pos):
                    st.pos = p
                return
            assert host.sync() == 0
            for r, (st, c, n) in enumerate(feeds):
                st.calls.append(out[r, :lens[r]].tobytes())
                st.frames += (n + 1151) // 1152 if c & END else 2
                if c & END:
                    del run.open[rows[r]]
                else:
                    run.open[rows[r]] = st
            run.check_books()

        tick([0, 1], [(a, START, 0), (b, START, 0)])
        tick([0, 1], [(a, 0, 0), (b, 0, 0)])
        parked = run.export([0])
        tick([0, 1], [(a, 0, 0), (b, 0, 0)], want=ERR_ARG)  # a row for the parked slot
        run.check_books()
        tick([1], [(b, 0, 0)])
        run.import_([2], parked)
        tick([1], [(b, 0, 0)], want=ERR_ARG)  # no row for the resumed slot
        run.check_books()
        tick([1, 2], [(b, 0, 0), (a, 0, 0)])
        tick([1, 2], [(b, 0, 0), (a, 0, 0)])
        tick([1, 2], [(b, END, 5), (a, END, 1000)])
        oracle_exact(oracle, run, [a, b])
    finally:
        host.close()
        run.close()


def test_host_rows_follow_park_and_resume_emulated(emu, oracle):
    host_rows_case(emu, oracle)


# ---- 9: argument errors ----
def test_argument_errors_emulated(emu, oracle):
    """every broken rule returns MP3MI_ERR_ARG and leaves the batch as it was: the books say so, and the streams finish
    oracle-exact afterwards"""
    run = ParkRun(emu, 3, 44100, 2, 128, 2)
    try:
        L, b, nb = run.L, run.b, run.state_bytes
        x, y = stream_of(emu, run, 91), stream_of(emu, run, 92)
        run.step({0: (x, START, 0), 1: (y, START, 0)})
        run.step({0: (x, 0, 0), 1: (y, 0, 0)})
        parked = run.export([1])  # slot 0 open at 4 frames, slots 1 and 2 closed, one good ticket
        d = run.mem.alloc(4 * (nb + 16))
        tk = (Ticket * 4)()
        tp = ctypes.addressof(tk)

        def arr(*v):
            return np.array(v, np.int32)

        def export(slots, n=None, close=1, state=d, stride=nb, tickets=tp):
            return L.mp3mi_batch_slots_export(b, len(slots) if n is None else n, None if slots is None else slots.ctypes.data, close, state,
                                              stride, tickets)

        def import_(slots, tickets, n=None, state=parked.d, stride=nb):
            return L.mp3mi_batch_slots_import(b, len(slots) if n is None else n, slots.ctypes.data, state, stride,
                                              None if tickets is None else ctypes.addressof(tickets))

        def ticket(**kw):
            t = (Ticket * 1)()
            ctypes.memmove(t, parked.tickets, ctypes.sizeof(Ticket))
            for k, v in kw.items():
                setattr(t[0], k, v)
            return t

        bad = [
            lambda: export(arr(1)),                        # a closed slot
            lambda: export(arr(0, 0)),                     # twice the same
            lambda: export(arr(3)), lambda: export(arr(-1)),
            lambda: export(arr(0), n=0), lambda: export(arr(0, 1, 2, 0), n=4),
            lambda: export(arr(0), state=None), lambda: export(arr(0), tickets=None),
            lambda: L.mp3mi_batch_slots_export(b, 1, None, 1, d, nb, tp), lambda: L.mp3mi_batch_slots_export(None, 1, arr(0).ctypes.data, 1, d, nb, tp),
            lambda: export(arr(0), stride=nb - 16), lambda: export(arr(0), stride=nb + 8), lambda: export(arr(0), state=d + 8),
            lambda: export(arr(0), close=0, stride=nb - 16),
            lambda: import_(arr(0), ticket()),             # an open slot
            lambda: import_(arr(1, 1), (Ticket * 2)(parked.tickets[0], parked.tickets[0])),
            lambda: import_(arr(3), ticket()), lambda: import_(arr(-1), ticket()),
            lambda: import_(arr(1), ticket(), n=0), lambda: import_(arr(1), ticket(), n=4),
            lambda: import_(arr(1), None), lambda: import_(arr(1), ticket(), state=None),
            lambda: import_(arr(1), ticket(), stride=nb - 16), lambda: import_(arr(1), ticket(), stride=nb + 4),
            lambda: import_(arr(1), ticket(magic=MAGIC + 1)), lambda: import_(arr(1), ticket(version=VERSION + 1)),
            lambda: import_(arr(1), ticket(state_bytes=nb + 16)),
            lambda: import_(arr(1), ticket(rate_hz=48000)), lambda: import_(arr(1), ticket(channels=1)), lambda: import_(arr(1), ticket(hdr_mode=2)),
            lambda: import_(arr(1), ticket(error_protection=1)), lambda: import_(arr(1), ticket(hdr_flags=4)),
            lambda: import_(arr(1), ticket(kbps=160)),     # above the ceiling of a batch created at 128
            lambda: import_(arr(1), ticket(kbps=100)), lambda: import_(arr(1), ticket(kbps=0)),  # no Layer III bitrate
            lambda: import_(arr(1), ticket(frames=-1)),
        ]
        for k, call in enumerate(bad):
            assert call() == ERR_ARG, k
            run.check_books()
        assert L.mp3mi_batch_slot_state_bytes(None) == 0
        run.step({0: (x, 0, 0)})
        run.import_([1], parked)
        run.step({0: (x, 0, 0), 1: (y, 0, 0)})
        run.step({0: (x, 0, 0), 1: (y, 0, 0)})
        run.step({0: (x, END, 300), 1: (y, END, 1000)})
        oracle_exact(oracle, run, [x, y])
    finally:
        run.close()


# ---------------------------------------------------------------------------------------------------------------------- device

def chunked(monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("MP3MI_CHUNK_FRAMES", str(chunk))  # a call's two frames in chunks of their own


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_park_and_resume_in_every_format_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    formats_case(product, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_resume_in_a_dirty_slot_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    dirty_slot_case(product, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_migration_to_another_batch_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    migration_case(product, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_snapshot_and_fork_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    snapshot_case(product, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_whole_batch_bookkeeping_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    whole_batch_case(product, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_status_travels_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    void_stream_case(product, oracle)
    kept_status_case(product, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_host_rows_follow_park_and_resume_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    host_rows_case(product, oracle)


def back_to_back(sync_each):
    """call, export(close), call, import, call, call through the Python binding, every call on buffers of its own: slot 0's stream
    is parked for one call and resumes in slot 2; slot 1 runs throughout.  Returns the bytes per call and slot."""
    import importlib
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    dev = torch.device("cuda:0")
    S, rate, ch, kbps, nf = 3, 44100, 2, 128, 2
    full = nf * 1152
    src = torch.empty((S, 4 * full * ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    mp3.synth_pcm_device(src, 4 * full, ch, rate, 950)
    b = mp3.Batch(S, rate, ch, kbps, nf)
    stride = b.out_stride(nf)
    # where each call's rows come from: (slot, source row, source call) -- the parked stream misses call 1
    feeds = [[(0, 0, 0), (1, 1, 0)], [(1, 1, 1)], [(2, 0, 1), (1, 1, 2)], [(2, 0, 2), (1, 1, 3)]]
    pcms = []
    for f in feeds:
        p = torch.zeros((S, full * ch), dtype=torch.int16, device=dev)
        for slot, row, k in f:
            p[slot] = src[row, k * full * ch:(k + 1) * full * ch]
        pcms.append(p)
    outs = [torch.zeros((S, stride), dtype=torch.uint8, device=dev) for _ in feeds]
    lens = [torch.zeros(S, dtype=torch.int32, device=dev) for _ in feeds]
    state = torch.zeros((1, b.slot_state_bytes()), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def step(fn):
        fn()
        if sync_each:
            b.sync()

    step(lambda: b.encode_slots(pcms[0], nf, outs[0], lens[0], start=[True, True, False]))
    tickets = []
    step(lambda: tickets.append(b.export_slots([0], state)))
    assert list(b.slot_frames()) == [-1, 2, -1] and tickets[0][0].frames == 2
    step(lambda: b.encode_slots(pcms[1], nf, outs[1], lens[1]))
    step(lambda: b.import_slots([2], state, tickets[0]))
    assert list(b.slot_frames()) == [-1, 4, 2]
    step(lambda: b.encode_slots(pcms[2], nf, outs[2], lens[2]))
    step(lambda: b.encode_slots(pcms[3], nf, outs[3], lens[3], end=[False, True, True]))
    b.sync()
    b.close()
    got = [[o.cpu().numpy()[s, :int(n.cpu().numpy()[s])].tobytes() for s in range(S)] for o, n in zip(outs, lens)]
    return got, src.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [None, "0"])
def test_back_to_back_without_sync_gpu(product, oracle, monkeypatch, hold):
    """the sequence issued without a sync in between -- with the call hold at its default and switched off -- gives the bytes of
    the same sequence synchronised after every step, and those are the oracle's"""
    if hold is not None:
        monkeypatch.setenv("MP3MI_CALL_HOLD", hold)
    a, src = back_to_back(sync_each=True)
    b, _ = back_to_back(sync_each=False)
    assert a == b
    full = 2 * 1152 * 2
    assert a[0][0] + a[2][2] + a[3][2] == oracle.encode(src[0, :3 * full], 44100, 128, 2)[0]
    assert a[0][1] + a[1][1] + a[2][1] + a[3][1] == oracle.encode(src[1, :4 * full], 44100, 128, 2)[0]
    assert [len(x) for x in (a[1][0], a[1][2], a[0][2], a[2][0], a[3][0])] == [0] * 5
