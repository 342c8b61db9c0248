"""A bitrate per stream at START, and park / resume, for Layers I and II (mp3mi_l12_batch_encode_slots_kbps, _slot_kbps,
_slots_export, _slots_import; include/mp3mi_l12.h): helpers shared by the CPU tests (tests/test_l12_slot_park.py, on the emulated
build) and the GPU tests (tests/test_gpu_l12_slot_park.py).  A Stream is one file in the making -- its samples, its bitrate, the
bytes it has delivered so far -- wherever it lives; a ParkRun is a batch driven call by call that keeps its own books of which
Stream sits in which slot and compares them, after EVERY accepted call, with mp3mi_l12_batch_slot_frames and _slot_kbps, and checks
out_len 0 and an untouched output row for the closed slots (whose PCM rows hold full-scale noise).  check_streams() compares
finished streams with the CPU oracle and with the library's own ragged whole-file call, each at its own bitrate."""
import copy
import ctypes

import numpy as np

from l12_slots import END, FILL, START, SlotRun, bind as bind_slots, loud, ragged_whole_file
from mp3common import l12_signal, oracle_l12

MAGIC = 0x4B54324D  # "M2TK"


class Ticket(ctypes.Structure):
    """mp3mi_l12_slot_ticket"""
    _fields_ = [("magic", ctypes.c_uint32), ("version", ctypes.c_uint32), ("state_bytes", ctypes.c_uint64), ("layer", ctypes.c_int32),
                ("rate_hz", ctypes.c_int32), ("channels", ctypes.c_int32), ("hdr_mode", ctypes.c_int32), ("hdr_flags", ctypes.c_int32),
                ("error_protection", ctypes.c_int32), ("kbps", ctypes.c_int32), ("reserved", ctypes.c_int32), ("frames", ctypes.c_int64)]


assert ctypes.sizeof(Ticket) == 56


def bind(mp):
    L = bind_slots(mp)
    vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.mp3mi_l12_batch_encode_slots_kbps.argtypes = [vp, vp, ci, vp, vp, vp, vp, sz, vp]  # (AttributeError without the feature)
    L.mp3mi_l12_batch_slot_kbps.argtypes = [vp, vp]
    L.mp3mi_l12_batch_slot_state_bytes.restype = sz
    L.mp3mi_l12_batch_slot_state_bytes.argtypes = [vp]
    L.mp3mi_l12_batch_slots_export.argtypes = [vp, ci, vp, ci, vp, sz, vp]
    L.mp3mi_l12_batch_slots_import.argtypes = [vp, ci, vp, vp, sz, vp]
    return L


def aligned(mem, nbytes):
    """nbytes of the memory the library computes on, at a multiple of 16"""
    return (mem.alloc(nbytes + 16) + 15) & ~15


def copy_dev(mem, dst, src, nbytes):
    if mem.emu:
        ctypes.memmove(dst, src, nbytes)
    else:
        assert mem.hip.hipMemcpy(dst, src, nbytes, 3) == 0


class Stream:
    """pcm: interleaved int16, everything the stream may ever be fed"""

    def __init__(self, pcm, kbps, ch):
        self.pcm, self.kbps, self.ch = pcm, kbps, ch
        self.pos, self.frames, self.got = 0, 0, b""

    def take(self, n):
        piece = self.pcm[self.pos * self.ch:(self.pos + n) * self.ch]
        assert len(piece) == n * self.ch, "source too short"
        self.pos += n
        return piece

    def fed(self):
        return self.pcm[:self.pos * self.ch]

    def clone(self):
        return copy.copy(self)  # (the samples are shared, the books are not)


class Parked:
    """a stream out of its slot: the books, the ticket, and where its state record lies"""

    def __init__(self, stream, ticket, ptr):
        self.stream, self.ticket, self.ptr = stream, ticket, ptr


class ParkRun(SlotRun):
    """kbps: the create-time bitrates, one or one per slot; pool: the DevMem the state records live in (default: the run's own --
    a record that outlives its run wants another)"""

    def __init__(self, mp, layer, S, rate, mode, kbps, nf, scratch_mb=0, pool=None):
        SlotRun.__init__(self, mp, layer, S, rate, mode, kbps, nf, scratch_mb=scratch_mb)
        self.L = bind(mp)
        self.pool = pool or self.mem
        self.cur = [None] * S
        self.calls = 0
        self.state_bytes = self.L.mp3mi_l12_batch_slot_state_bytes(self.b)
        assert self.state_bytes == self.ch * (1792 + 1056) * 2

    def stream(self, seed, n_per_ch, kbps=None, slot=0, noise=False):
        """a new Stream of this run's format; kbps None: the create-time bitrate of `slot`"""
        pcm = loud(n_per_ch * self.ch, seed) if noise else l12_signal(n_per_ch, self.ch, seed, self.rate)
        return Stream(pcm, self.kbps[slot] if kbps is None else kbps, self.ch)

    # ---- the books
    def slot_kbps(self):
        k = np.full(self.S, -7, np.int32)
        assert self.L.mp3mi_l12_batch_slot_kbps(self.b, k.ctypes.data) == max(self.kbps)  # the ceiling
        return [int(x) for x in k]

    def check_books(self):
        assert self.frames() == [-1 if st is None else st.frames for st in self.cur], (self.frames(), [st and st.frames for st in self.cur])
        assert self.slot_kbps() == [self.kbps[s] if st is None else st.kbps for s, st in enumerate(self.cur)], self.slot_kbps()

    def collect(self, nf, ctl, ns, flush=False):
        """the outputs of the last call into the streams' files; returns the streams it ended"""
        outs, lens, rows = self.outputs()
        done = []
        for s, st in enumerate(self.cur):
            if st is None:
                assert lens[s] == 0, (s, lens[s])
                assert (rows[s] == FILL).all(), "the call wrote into the row of closed slot %d" % s
                continue
            st.got += outs[s]
            if flush or ctl[s] & END:
                st.frames += 0 if flush else (int(ns[s]) + self.spf - 1) // self.spf
                done.append(st)
                self.cur[s] = None
            else:
                st.frames += nf
        self.check_books()
        return done

    # ---- the calls
    def pcm_for(self, nf, ends):
        full = nf * self.spf
        pcm = loud(self.S * full * self.ch, 1000 + self.calls).reshape(self.S, full * self.ch)  # closed slots, and behind a last sample
        self.calls += 1
        ns = np.zeros(self.S, np.int32)
        for s, st in enumerate(self.cur):
            if st is not None:
                ns[s] = ends[s] if s in ends else full
                piece = st.take(int(ns[s]))
                pcm[s, :len(piece)] = piece
        return pcm, ns

    def step(self, nf=None, starts=None, ends=None, kbps="start"):
        """one mp3mi_l12_batch_encode_slots_kbps: starts {slot: Stream}, ends {slot: samples of the call}; every other open stream
        goes on.  kbps: "start" -- the array names the STARTing streams' bitrates, 0 elsewhere; "all" -- every open stream's too (a
        persistent array); "zero" -- all 0; None -- no array.  Returns the streams that ended."""
        nf, starts, ends = nf or self.nf, starts or {}, ends or {}
        ctl, kb = np.zeros(self.S, np.uint8), np.zeros(self.S, np.int32)
        for s, st in starts.items():
            ctl[s] |= START
            self.cur[s], st.frames = st, 0  # (a stream still open there is abandoned)
        for s in ends:
            ctl[s] |= END
        pcm, ns = self.pcm_for(nf, ends)
        for s, st in enumerate(self.cur):
            if st is not None and (kbps == "all" or (kbps == "start" and s in starts)):
                kb[s] = st.kbps
        if kbps in (None, "zero"):
            assert all(st.kbps == self.kbps[s] for s, st in starts.items())
        self.put(pcm)
        rc = self.L.mp3mi_l12_batch_encode_slots_kbps(self.b, self.d_pcm, nf, ctl.ctypes.data, ns.ctypes.data, None if kbps is None else kb.ctypes.data,
                                                      self.d_out, self.stride, self.d_len)
        assert rc == 0, "call %d -> %d" % (self.calls - 1, rc)
        return self.collect(nf, ctl, ns)

    def next(self, nf=None, starts=None):
        """mp3mi_l12_batch_encode_next: the open streams go on; starts (a Stream per slot, every slot closed): they all begin"""
        nf = nf or self.nf
        if starts:
            assert all(st is None for st in self.cur)
            self.cur = list(starts)
            for st in starts:
                st.frames = 0
        pcm, ns = self.pcm_for(nf, {})
        assert self.encode_next(pcm, nf) == 0
        return self.collect(nf, np.zeros(self.S, np.uint8), ns)

    def flush_all(self):
        assert self.flush() == 0
        return self.collect(0, None, None, flush=True)

    def reset(self):
        assert self.L.mp3mi_l12_batch_reset(self.b) == 0
        self.cur = [None] * self.S
        self.check_books()

    def whole_file(self, streams, nf=None):
        """mp3mi_l12_batch_encode of a Stream per slot, all of each (ragged); every stream open before is over.  Returns the files."""
        nf = nf or self.nf
        pcm, ns = np.zeros((self.S, nf * self.spf * self.ch), np.int16), np.zeros(self.S, np.int32)
        for s, st in enumerate(streams):
            ns[s] = len(st.pcm) // self.ch
            pcm[s, :len(st.pcm)] = st.take(int(ns[s]))
        self.put(pcm)
        d_ns = self.mem.alloc(4 * self.S)
        self.mem.upload(d_ns, ns)
        assert self.L.mp3mi_l12_batch_encode(self.b, self.d_pcm, d_ns, nf, self.d_out, self.stride, self.d_len) == 0
        self.cur = [None] * self.S
        outs = self.outputs()[0]
        self.check_books()
        for st, o in zip(streams, outs):
            st.got = o
        return list(streams)

    def raw_step(self, ctl, ns=None, kb=None, nf=None):
        """the call's return code and nothing else (refusals)"""
        a = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=t)
        ctl, ns, kb = a(ctl, np.uint8), a(ns, np.int32), a(kb, np.int32)
        p = lambda x: None if x is None else x.ctypes.data
        return self.L.mp3mi_l12_batch_encode_slots_kbps(self.b, self.d_pcm, nf or self.nf, p(ctl), p(ns), p(kb), self.d_out, self.stride, self.d_len)

    def export(self, slots, close=True, stride=None, fill=None, sync=True):
        """mp3mi_l12_batch_slots_export; returns a Parked per slot (close=False: of a copy of the stream's books)"""
        n, stride = len(slots), stride or self.state_bytes
        p = aligned(self.pool, n * stride)
        if fill is not None:
            self.pool.upload(p, np.full(n * stride, fill, np.uint8))
        tk = (Ticket * n)()
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        assert self.L.mp3mi_l12_batch_slots_export(self.b, n, sl.ctypes.data, int(close), p, stride, tk) == 0
        parked = []
        for i, s in enumerate(slots):
            st, t = self.cur[s], tk[i]
            assert (t.magic, t.version, t.state_bytes, t.layer, t.rate_hz, t.channels) == (MAGIC, 1, self.state_bytes, self.layer, self.rate, self.ch)
            assert (t.hdr_mode, t.hdr_flags, t.error_protection, t.reserved) == ("sjdm".index(self.mode[0]), 0, int("e" in self.mode[1:]), 0)
            assert (t.kbps, t.frames) == (st.kbps, st.frames), (t.kbps, t.frames, st.kbps, st.frames)
            parked.append(Parked(st if close else st.clone(), Ticket.from_buffer_copy(t), p + i * stride))
            if close:
                self.cur[s] = None
        self.check_books()
        if sync:
            assert self.L.mp3mi_l12_batch_sync(self.b) == 0
        return parked

    def import_(self, slots, parked, stride=None):
        """mp3mi_l12_batch_slots_import of records gathered one behind the other (their exporters are synced: export()); the
        slots then hold COPIES of the parked streams' books, so a record may be imported again"""
        n, stride = len(slots), stride or self.state_bytes
        p = aligned(self.pool, n * stride)
        for i, pk in enumerate(parked):
            copy_dev(self.pool, p + i * stride, pk.ptr, self.state_bytes)
        tk = (Ticket * n)(*[pk.ticket for pk in parked])
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        assert self.L.mp3mi_l12_batch_slots_import(self.b, n, sl.ctypes.data, p, stride, tk) == 0
        for s, pk in zip(slots, parked):
            self.cur[s] = pk.stream.clone()
        self.check_books()
        return [self.cur[s] for s in slots]


def check_streams(run, orc, streams, n_least=1):
    """every finished stream: the oracle's bytes and the ragged whole-file call's, at the stream's bitrate"""
    assert len(streams) >= n_least, (len(streams), n_least)
    whole = ragged_whole_file(run.mp, run, [(st.kbps, st.fed()) for st in streams])
    for i, (st, w) in enumerate(zip(streams, whole)):
        ref = oracle_l12(orc, run.layer, run.rate, st.kbps, run.mode, st.fed())[0]
        what = "stream %d, %d kbps, %d samples: %d bytes" % (i, st.kbps, st.pos, len(st.got))
        assert st.got == ref, "%s vs the oracle's %d" % (what, len(ref))
        assert st.got == w, "%s vs the whole-file call's %d" % (what, len(w))


# ---- scenarios the CPU tests run over a few slots and the GPU tests over 64 ----
def l12_rates(layer, n):
    """n create-time bitrates that differ from slot to slot"""
    return [([192, 224, 256, 288] if layer == 1 else [128, 160, 192, 224])[s % 4] for s in range(n)]


def case_phase(mp, orc, layer, k, S=6):
    """Export with close after k calls of one frame; import into a higher slot, a lower slot and a second batch with other create-time
    bitrates, another n_streams and another max_frames.  Groups of six slots of batch A: 0 and 5 run full-scale noise and END in
    call k (the targets); 1 moves to 5, 2 to 0, 3 to batch B; 4 is a neighbour that goes on.  Between export and import the vacated
    slots START full-scale noise; B's target slots ended full-scale noise before, and B's last slot churns."""
    from mp3common import DevMem
    G = S // 6
    assert G >= 1
    pool = DevMem(mp)
    a = ParkRun(mp, layer, S, 44100, "s", l12_rates(layer, S), 2, pool=pool)
    b = ParkRun(mp, layer, G + 1, 44100, "s", [64] * G + [448 if layer == 1 else 384], 3, pool=pool)
    try:
        spf, done = a.spf, []
        grp = lambda j: [6 * g + j for g in range(G)]
        src = {s: a.stream(10 + s, 12 * spf, slot=s, noise=s % 6 in (0, 5)) for s in range(6 * G)}
        nb = b.stream(900, 12 * spf, slot=G)
        bl = [b.stream(910 + g, 4 * spf, slot=g, noise=True) for g in range(G)]
        done += b.step(1, starts=dict([(G, nb)] + [(g, bl[g]) for g in range(G)]), ends={g: spf - 3 for g in range(G)})
        for c in range(k):
            done += a.step(1, starts=src if c == 0 else None, ends={s: spf for s in grp(0) + grp(5)} if c == k - 1 else None)
        parked = a.export(grp(1) + grp(2) + grp(3))
        px, py, pz = parked[:G], parked[G:2 * G], parked[2 * G:]
        fill = {s: a.stream(50 + s, 6 * spf, slot=s, noise=True) for s in grp(1) + grp(2) + grp(3)}
        done += a.step(1, starts=fill)
        done += b.step(2)
        x = a.import_(grp(5) + grp(0), px + py)
        z = b.import_(list(range(G)), pz)
        done += a.step(1)
        done += b.step(1)
        done += a.step(2)
        done += b.step(3, ends={G: 2 * spf + 1})
        ends = {s: spf + 7 for s in grp(5)}
        ends.update({s: 0 for s in grp(0)})
        ends.update({s: 2 * spf for s in grp(1) + grp(2) + grp(3)})
        ends.update({s: 5 for s in grp(4)})
        done += a.step(2, ends=ends)
        done += b.step(1, ends={g: 100 for g in range(G)})
        assert a.frames() == [-1] * S and b.frames() == [-1] * (G + 1)
        assert all(st in done for st in x + z)
        check_streams(a, orc, done, 10 * G + 1)
    finally:
        a.close()
        b.close()
        pool.free()


def case_snapshot(mp, orc, layer, S=4):
    """close=0: the original goes on; the record is imported twice; three identical files.  Groups of four slots: 0 a neighbour, 1 the
    original, 2 and 3 the copies (which ended full-scale noise before)."""
    G = S // 4
    run = ParkRun(mp, layer, S, 48000, "j", l12_rates(layer, S), 2)
    try:
        spf, done = run.spf, []
        grp = lambda j: [4 * g + j for g in range(G)]
        src = {s: run.stream(20 + s, 10 * spf, slot=s, noise=s % 4 >= 2) for s in range(4 * G)}
        done += run.step(2, starts=src, ends={s: spf for s in grp(2) + grp(3)})
        done += run.step(1)
        snap = run.export(grp(1), close=False)
        done += run.step(1)  # the original is a call ahead of its snapshot now
        run.export(grp(1), close=True)  # ... and leaves; the snapshot of the call before comes back three times
        copies = run.import_(grp(1) + grp(2) + grp(3), snap + snap + snap)
        done += run.step(2)
        done += run.step(1, ends={s: (0 if s % 4 == 0 else 77) for s in range(4 * G)})
        assert all(st in done for st in copies)
        for g in range(G):
            files = [st.got for st in copies[g::G]]
            assert len(files) == 3 and files[0] == files[1] == files[2] and len(files[0]) > 1
        check_streams(run, orc, done, 6 * G)
    finally:
        run.close()


def case_rates(mp, orc, layer, rate, mode, create, rates, S=4):
    """a batch created at `create`; STARTs at `rates` in turn, staggered over the calls, END and START again in the same slots at the
    next bitrate: cfg is rewritten while the neighbours go on"""
    run = ParkRun(mp, layer, S, rate, mode, create, 2)
    try:
        spf, done, n = run.spf, [], 0
        for c in range(len(rates) + 3):
            starts, ends = {}, {}
            for s in range(S):
                if run.cur[s] is None and (c + s) % 2 == 0 and c < len(rates) + 1:
                    starts[s] = run.stream(30 + n, 6 * spf, kbps=rates[n % len(rates)])
                    n += 1
                elif run.cur[s] is not None and (run.cur[s].frames >= 3 or c == len(rates) + 2):
                    ends[s] = min([spf + 9, 0, 2 * spf, 1][(c + s) % 4], (2 if c % 2 else 1) * spf)
            done += run.step(2 if c % 2 else 1, starts=starts, ends=ends, kbps="all" if c % 2 else "start")
        assert run.frames() == [-1] * S
        assert {st.kbps for st in done} == set(rates), sorted({st.kbps for st in done})
        check_streams(run, orc, done, S)
    finally:
        run.close()


def case_travel(mp, orc, S=3):
    """Layer II: started at 96 kbps in a batch created at 384, exported, imported into slots created at 160: continues at 96; after its
    END the slot reports 160 again and encodes at 160"""
    from mp3common import DevMem
    pool = DevMem(mp)
    a = ParkRun(mp, 2, S, 44100, "s", 384, 2, pool=pool)
    b = ParkRun(mp, 2, S, 44100, "s", 160, 2, pool=pool)
    try:
        spf, done = a.spf, []
        slots = list(range(1, S))
        done += a.step(2, starts={s: a.stream(40 + s, 8 * spf, kbps=96) for s in slots})
        assert a.slot_kbps() == [384] + [96] * (S - 1)
        done += b.step(1, starts={0: b.stream(60, 8 * spf)})
        parked = a.export(slots)
        assert a.slot_kbps() == [384] * S
        moved = b.import_(slots, parked)
        assert b.slot_kbps() == [160] + [96] * (S - 1)
        done += b.step(2)
        done += b.step(1, ends={s: 500 for s in slots})
        assert b.slot_kbps() == [160] * S and all(st in done and st.kbps == 96 for st in moved)
        # the same slots at their own bitrate again, with no bitrate array; a's vacated slots at theirs
        done += b.step(1, starts={s: b.stream(70 + s, 4 * spf) for s in slots}, kbps=None)
        done += b.step(2, ends={s: spf + 1 for s in range(S)}, kbps=None)
        done += a.step(1, starts={s: a.stream(80 + s, 4 * spf) for s in slots}, ends={s: 700 for s in slots}, kbps=None)
        assert sorted(st.kbps for st in done) == sorted([96] * (S - 1) + [160] * S + [384] * (S - 1))
        check_streams(a, orc, done, 3 * S - 2)
    finally:
        a.close()
        b.close()
        pool.free()
