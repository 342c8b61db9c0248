"""A bitrate per STREAM of a slot batch, chosen at its START (mp3mi_batch_encode_slots_kbps, mp3mi_batch_encode_slots_kbps_host_async,
mp3mi_batch_slot_kbps; include/mp3mi.h): a batch created at a ceiling runs streams of any bitrate up to it, slot by slot and
stream after stream.  The bytes of every stream are the oracle's file of its samples at the stream's OWN bitrate, whatever the
slot was created with and whatever ran in it before; the calls that start every stream afresh are back at the create-time
bitrates."""
import ctypes

import numpy as np
import pytest

from golden_util import aborting_cases, case_pcm
from mp3common import DevMem, ReferenceAborts
from test_slots_host import HostRun
from test_stream_slots import END, START, SlotRun, churn_schedule, drive

ERR_ARG = -1


def bind(mp):
    L = mp.lib
    L.mp3mi_batch_encode_slots_kbps.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.mp3mi_batch_encode_slots_kbps_host_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                           ctypes.c_void_p]
    L.mp3mi_batch_slot_kbps.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return L


class KbpsRun(SlotRun):
    """SlotRun whose calls go through mp3mi_batch_encode_slots_kbps: call k of a drive() takes its kbps array from `per_call`
    (None: kbps_host NULL).  After every accepted call mp3mi_batch_slot_kbps must report the bitrates of the open streams and
    the create-time bitrate of every closed slot; `ended` lists (slot, kbps) of the streams the calls ENDed, in drive()'s order."""

    def __init__(self, mp, S, rate, ch, kbps, nf, per_call=(), **kw):
        SlotRun.__init__(self, mp, S, rate, ch, kbps, nf, **kw)
        bind(mp)
        self.per_call, self.n_call = list(per_call), 0
        self.live, self.open_, self.ended = list(self.kbps), [False] * S, []

    def slot_kbps(self):
        k = np.full(self.S, -7, np.int32)
        ceil = self.L.mp3mi_batch_slot_kbps(self.b, k.ctypes.data)
        return list(k), ceil

    def call(self, pcm, ctl, ns=None, kbps="plan", nf=None):
        if isinstance(kbps, str):
            kbps = self.per_call[self.n_call] if self.n_call < len(self.per_call) else None
            self.n_call += 1
        nf = self.nf if nf is None else nf
        self.mem.upload(self.d_pcm, np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.S, -1))
        ctl = np.ascontiguousarray(ctl, dtype=np.uint8)
        ns = None if ns is None else np.ascontiguousarray(ns, dtype=np.int32)
        kb = None if kbps is None else np.array(kbps, dtype=np.int32)
        rc = self.L.mp3mi_batch_encode_slots_kbps(self.b, self.d_pcm, nf, ctl.ctypes.data, None if ns is None else ns.ctypes.data,
                                                  None if kb is None else kb.ctypes.data, self.d_out, self.stride, self.d_len)
        if kb is not None:
            kb[...] = -1  # (the library has copied it)
        if rc != 0:
            return rc
        for s in range(self.S):
            if ctl[s] & START:
                self.live[s], self.open_[s] = (int(kbps[s]) if kbps is not None and kbps[s] else self.kbps[s]), True
            if ctl[s] & END:
                self.ended.append((s, self.live[s]))
                self.live[s], self.open_[s] = self.kbps[s], False
        assert self.slot_kbps() == (self.live, max(self.kbps)), (self.slot_kbps(), self.live)
        return rc

    def flushed(self):
        """after a flush: the streams it ended join `ended`, every slot reports its create-time bitrate again"""
        self.ended += [(s, self.live[s]) for s in range(self.S) if self.open_[s]]
        self.live, self.open_ = list(self.kbps), [False] * self.S
        assert self.slot_kbps() == (self.live, max(self.kbps))


def check_own_kbps(run, oracle, done, mode=None):
    """every finished stream is the oracle's file at the bitrate its START chose"""
    assert [s for s, _, _ in done] == [s for s, _ in run.ended], (done, run.ended)
    for (s, pcm, data), (_, k) in zip(done, run.ended):
        ref = oracle.encode(pcm, run.rate, k, run.ch, mode=mode)[0]
        assert data == ref, "slot %d at %d kbps, %d samples: %d bytes vs the oracle's %d" % (s, k, len(pcm) // run.ch, len(data), len(ref))


# ---- case 1: mixed bitrates, slot reuse (test_stream_slots.staggered's plan on a batch created at 320) ----
MIXED_PLAN = [
    [(START, 0), (0, 0), (0, 0)],
    [(0, 0), (START, 0), (0, 0)],
    [(0, 0), (END, 0), (START, 0)],
    [(END, 1000), (START | END, 2 * 1152 - 5), (0, 0)],
]
# slot 0: one stream at 128; slot 1: a stream at 32, then a one-call file at 320 in the same slot (a stale reservoir or bit budget
# would show); slot 2 STARTs with 0 and comes out at the create-time 320, which the flush ends it at
MIXED_KBPS = [[128, 0, 0], [128, 32, 0], [0, 32, 0], [128, 320, 320]]
MIXED_STREAMS = [(0, 128, 3 * 2304 + 1000), (1, 32, 2304), (1, 320, 2299), (2, 320, 2 * 2304)]  # (slot, kbps, samples) as they end


def mixed_sources(mp, rate=44100, ch=2):
    return [[mp.synth(8 * 1152, ch, rate, sd) for sd in seeds] for seeds in ([11], [12, 13], [14])]


def mixed_case(mp, oracle):
    run = KbpsRun(mp, 3, 44100, 2, 320, 2, per_call=MIXED_KBPS)
    try:
        assert run.slot_kbps() == ([320] * 3, 320)
        done = drive(run, MIXED_PLAN, mixed_sources(mp))
        run.flushed()
        assert sorted((s, k, len(p) // 2) for (s, p, _), (_, k) in zip(done, run.ended)) == sorted(MIXED_STREAMS)
        check_own_kbps(run, oracle, done)
    finally:
        run.close()


# ---- case 2: other formats ----
def other_formats_case(mp, oracle):
    """32 kHz mono created at 128: streams at 56 and 128; 48 kHz stereo, error protection on, created with [32, 320]: slot 0
    STARTs with 0 (32), slot 1 at 64"""
    plan = [[(START, 0), (0, 0)], [(0, 0), (START, 0)], [(END, 700), (0, 0)]]
    for rate, ch, kbps, mode, crc, omode, per_call, want in (
            (32000, 1, 128, None, False, None, [[56, 0], [56, 128], [56, 128]], [(0, 56), (1, 128)]),
            (48000, 2, [32, 320], 0, True, "se", [[0, 0], [0, 64], [32, 64]], [(0, 32), (1, 64)])):
        run = KbpsRun(mp, 2, rate, ch, kbps, 2, per_call=per_call, mode=mode, crc=crc)
        try:
            src = [[mp.synth(8 * 1152, ch, rate, 80 + s)] for s in range(2)]
            done = drive(run, plan, src)
            run.flushed()
            assert run.ended == want
            assert sorted((s, len(p) // ch) for s, p, _ in done) == [(0, 2 * 2304 + 700), (1, 2 * 2304)]
            check_own_kbps(run, oracle, done, mode=omode)
        finally:
            run.close()


# ---- case 3: the reference's flush abort at the stream's own bitrate ----
def flush_abort_case(mp, oracle):
    """abort_flush_slot (48 kHz, 64 kbps) in slot 0 of a batch created at 128, STARTed with kbps 64 and ENDed inside a call: the
    fixture's status and frame -- k_stream_tail settles the file's end with the stream's frame size --, the neighbour at 128"""
    case = [c for c in aborting_cases() if c["name"] == "abort_flush_slot"][0]
    bad = case_pcm(case, mp.synth)  # 5 frames: the reference dies in its final flush
    with pytest.raises(ReferenceAborts):
        oracle.encode(bad, 48000, 64, 2)
    run = KbpsRun(mp, 2, 48000, 2, 128, 2, per_call=[[64, 0], [64, 128], [64, 0]])
    try:
        good = mp.synth(8 * 1152, 2, 48000, 70)
        plan = [[(START, 0), (START, 0)], [(0, 0), (0, 0)], [(END, 1152), (END, 1000)]]
        done = drive(run, plan, [[bad], [good]], flush=False, aborts=(2,))
        st = run.status()
        assert (st[0] & 255) == case["reference_aborts"]["status"] and (st[0] >> 8) == case["reference_aborts"]["frame"], st[0]
        assert st[1] == 0
        assert run.ended == [(0, 64), (1, 128)]
        by = {s: (p, d) for s, p, d in done}
        assert by[1][1] == oracle.encode(by[1][0], 48000, 128, 2)[0]
        assert run.L.mp3mi_batch_sync(run.b) == 0
    finally:
        run.close()


# ---- case 4: rules ----
def rules_case(mp, oracle):
    """every broken bitrate rule returns MP3MI_ERR_ARG and leaves slot_frames and slot_kbps as they were; a continuing slot given
    its own bitrate, or 0, is accepted, and the streams of the valid calls are the oracle's"""
    rate, ch, S, nf = 44100, 2, 3, 2
    full = nf * 1152
    run = KbpsRun(mp, S, rate, ch, 128, nf)
    try:
        src = [mp.synth(4 * full, ch, rate, 50 + s) for s in range(S)]
        piece = lambda k: np.stack([x[k * full * ch:(k + 1) * full * ch] for x in src])
        got = [b""] * S

        def ok(pcm, ctl, ns, kbps):
            assert run.call(pcm, ctl, ns, kbps=kbps) == 0 and run.L.mp3mi_batch_sync(run.b) == 0
            outs, _ = run.outputs()
            for s in range(S):
                got[s] += outs[s]

        ok(piece(0), [START, 0, START], None, [64, 0, 0])  # slot 0 open at 64, slot 1 closed, slot 2 open at 128
        frames, kb = list(run.frames()), run.slot_kbps()
        assert frames == [2, -1, 2] and kb == ([64, 128, 128], 128)
        bad = [
            dict(ctl=[0, START, 0], kbps=[0, 192, 0]),       # above the ceiling
            dict(ctl=[0, START, 0], kbps=[0, 100, 0]),       # not a Layer III bitrate
            dict(ctl=[0, START, 0], kbps=[0, -64, 0]),       # negative
            dict(ctl=[START, 0, 0], kbps=[320, 0, 0]),       # above the ceiling, on a slot that abandons its stream
            dict(ctl=[0, 0, 0], kbps=[64, 128, 128]),        # a closed slot that does not START
            dict(ctl=[0, 0, 0], kbps=[128, 0, 128]),         # a continuing slot, not its stream's bitrate
            dict(ctl=[0, 0, END], kbps=[0, 0, 64]),          # ... nor an ending one
        ]
        for kw in bad:
            assert run.call(piece(1), kw["ctl"], None, kbps=kw["kbps"]) == ERR_ARG, kw
            assert list(run.frames()) == frames and run.slot_kbps() == kb, kw
        assert run.L.mp3mi_batch_slot_kbps(run.b, None) == ERR_ARG and run.L.mp3mi_batch_slot_kbps(None, None) == ERR_ARG
        assert run.L.mp3mi_batch_encode_slots_kbps(None, run.d_pcm, nf, np.zeros(S, np.uint8).ctypes.data, None, None, run.d_out, run.stride,
                                                   run.d_len) == ERR_ARG
        ok(piece(1), [0, 0, 0], None, [64, 0, 0])  # its own bitrate, and 0
        pcm = np.zeros((S, full * ch), np.int16)
        pcm[0, :100 * ch] = src[0][2 * full * ch:(2 * full + 100) * ch]
        pcm[1, :2000 * ch] = src[1][:2000 * ch]
        ok(pcm, [END, START | END, END], [100, 2000, 0], [0, 32, 128])
        assert run.ended == [(0, 64), (1, 32), (2, 128)] and list(run.frames()) == [-1] * S
        assert got[0] == oracle.encode(src[0][:(2 * full + 100) * ch], rate, 64, ch)[0]
        assert got[1] == oracle.encode(src[1][:2000 * ch], rate, 32, ch)[0]
        assert got[2] == oracle.encode(src[2][:2 * full * ch], rate, 128, ch)[0]
        # every slot is closed: encode_next starts them all, at the create-time bitrate (slot 1 has just run a stream at 32)
        L = run.L
        run.mem.upload(run.d_pcm, piece(0))
        assert L.mp3mi_batch_encode_next(run.b, run.d_pcm, nf, run.d_out, run.stride, run.d_len) == 0 and L.mp3mi_batch_sync(run.b) == 0
        got = run.outputs()[0]
        assert L.mp3mi_batch_flush(run.b, run.d_out, run.stride, run.d_len) == 0 and L.mp3mi_batch_sync(run.b) == 0
        assert got[1] + run.outputs()[0][1] == oracle.encode(src[1][:full * ch], rate, 128, ch)[0]
    finally:
        run.close()


# ---- case 5: back to the create-time bitrates ----
def back_to_create_case(mp, oracle):
    rate, ch, S, nf = 44100, 2, 3, 2
    full = nf * 1152
    create, own = [128, 64, 96], [32, 64, 64]  # (slot 1 STARTs with 0)
    src = [mp.synth(2 * full, ch, rate, 90 + s) for s in range(S)]
    first = np.stack([x[:full * ch] for x in src])
    second = np.stack([x[full * ch:] for x in src])
    ref_create = [oracle.encode(src[s][:full * ch], rate, create[s], ch)[0] for s in range(S)]
    run = KbpsRun(mp, S, rate, ch, create, nf)
    fresh = SlotRun(mp, S, rate, ch, create, nf)
    L = run.L

    def whole(r):
        r.mem.upload(r.d_pcm, first)
        assert L.mp3mi_batch_encode(r.b, r.d_pcm, nf, r.d_out, r.stride, r.d_len) == 0 and L.mp3mi_batch_sync(r.b) == 0
        return r.outputs()[0]

    def start_all():
        assert run.call(second, [START] * S, None, kbps=[32, 0, 64]) == 0
        assert run.slot_kbps() == (own, 128)

    try:
        # a whole-file call on a batch whose streams are open at bitrates of their own: a fresh batch's bytes
        start_all()
        assert run.call(second, [0, END, 0], [full, 7, full], kbps=None) == 0  # (not all at one frame: the per-slot bookkeeping stays)
        got = whole(run)
        assert got == whole(fresh) and got == ref_create
        assert run.slot_kbps() == (create, 128) and list(run.frames()) == [-1] * S
        # reset, then encode_next + flush
        start_all()
        assert L.mp3mi_batch_reset(run.b) == 0
        assert run.slot_kbps() == (create, 128)
        run.mem.upload(run.d_pcm, first)
        assert L.mp3mi_batch_encode_next(run.b, run.d_pcm, nf, run.d_out, run.stride, run.d_len) == 0 and L.mp3mi_batch_sync(run.b) == 0
        got = run.outputs()[0]
        assert L.mp3mi_batch_flush(run.b, run.d_out, run.stride, run.d_len) == 0 and L.mp3mi_batch_sync(run.b) == 0
        assert [a + b for a, b in zip(got, run.outputs()[0])] == ref_create
        # every slot STARTed at one frame (the whole-batch bookkeeping takes over), continued by encode_next, ended by the flush:
        # the streams keep their own bitrates
        assert run.call(first, [START] * S, None, kbps=[32, 0, 64]) == 0 and L.mp3mi_batch_sync(run.b) == 0
        got = run.outputs()[0]
        run.mem.upload(run.d_pcm, second)
        assert L.mp3mi_batch_encode_next(run.b, run.d_pcm, nf, run.d_out, run.stride, run.d_len) == 0 and L.mp3mi_batch_sync(run.b) == 0
        assert run.slot_kbps() == (own, 128) and list(run.frames()) == [4] * S
        got = [a + b for a, b in zip(got, run.outputs()[0])]
        assert L.mp3mi_batch_flush(run.b, run.d_out, run.stride, run.d_len) == 0 and L.mp3mi_batch_sync(run.b) == 0
        got = [a + b for a, b in zip(got, run.outputs()[0])]
        assert got == [oracle.encode(src[s], rate, own[s], ch)[0] for s in range(S)]
        assert run.slot_kbps() == (create, 128)
        # ... and an encode_next that starts every slot is back at the create-time bitrates
        run.mem.upload(run.d_pcm, first)
        assert L.mp3mi_batch_encode_next(run.b, run.d_pcm, nf, run.d_out, run.stride, run.d_len) == 0 and L.mp3mi_batch_sync(run.b) == 0
        got = run.outputs()[0]
        assert L.mp3mi_batch_flush(run.b, run.d_out, run.stride, run.d_len) == 0 and L.mp3mi_batch_sync(run.b) == 0
        assert [a + b for a, b in zip(got, run.outputs()[0])] == ref_create
    finally:
        run.close()
        fresh.close()


# ---- case 6: two calls in flight ----
CHURN = dict(S=64, rate=44100, ch=2, nf=2, n_calls=10, seed=20261018, ceil=320)


def churn_kbps(sched, S, seed):
    """a seeded bitrate per START out of {64, 128, 192, 320}; the other entries 0"""
    rng = np.random.default_rng(seed)
    return [np.where(ctl & START > 0, rng.choice([64, 128, 192, 320], S), 0).astype(np.int32) for ctl, _ in sched]


def churn_run(mp, sched, kbps, sync_each):
    """The schedule through mp3mi_batch_encode_slots_kbps, every call into an output buffer of its own, then a flush; the stream a
    slot STARTs in call k reads source row s from sample k * nf * 1152 on.  Returns the per-call (bytes per slot, lengths), the
    finished streams [(slot, first sample, samples, kbps, bytes)] and the source rows."""
    S, rate, ch, nf, n_calls = (CHURN[k] for k in ("S", "rate", "ch", "nf", "n_calls"))
    full = nf * 1152
    L = bind(mp)
    src = np.stack([mp.synth(n_calls * full, ch, rate, 900 + s) for s in range(S)])
    mem = DevMem(mp)
    b = ctypes.c_void_p()
    assert L.mp3mi_batch_create(ctypes.byref(b), S, rate, ch, None, CHURN["ceil"], nf) == 0
    try:
        stride = L.mp3mi_batch_out_stride(b, nf)
        d_pcm = [mem.alloc(S * full * ch * 2) for _ in range(n_calls)]
        d_out = [mem.alloc(S * stride) for _ in range(n_calls + 1)]
        d_len = [mem.alloc(4 * S) for _ in range(n_calls + 1)]
        for k in range(n_calls):
            mem.upload(d_pcm[k], np.ascontiguousarray(src[:, k * full * ch:(k + 1) * full * ch]))
        for k, (ctl, ns) in enumerate(sched):
            assert L.mp3mi_batch_encode_slots_kbps(b, d_pcm[k], nf, ctl.ctypes.data, ns.ctypes.data, kbps[k].ctypes.data, d_out[k], stride,
                                                   d_len[k]) == 0, k
            if sync_each:
                assert L.mp3mi_batch_sync(b) == 0
        assert L.mp3mi_batch_flush(b, d_out[n_calls], stride, d_len[n_calls]) == 0
        assert L.mp3mi_batch_sync(b) == 0
        lens = [mem.download(d, (S,), np.uint32) for d in d_len]
        outs = [mem.download(d, (S, stride), np.uint8) for d in d_out]
    finally:
        L.mp3mi_batch_destroy(b)
        mem.free()
    per_call = [([outs[k][s, :lens[k][s]].tobytes() for s in range(S)], list(lens[k])) for k in range(n_calls + 1)]
    first, rate_of, acc, done = [None] * S, [0] * S, [b""] * S, []
    for k in range(n_calls + 1):
        ctl, ns = sched[k] if k < n_calls else (np.full(S, END, np.uint8), np.zeros(S, np.int32))
        for s in range(S):
            if k < n_calls and ctl[s] & START:
                first[s], rate_of[s], acc[s] = k, int(kbps[k][s]), b""
            if first[s] is None:
                assert lens[k][s] == 0, (k, s)
                continue
            acc[s] += per_call[k][0][s]
            if ctl[s] & END:
                done.append((s, first[s] * full, (k - first[s]) * full + int(ns[s]), rate_of[s], acc[s]))
                first[s] = None
    return per_call, done, src


def churn_check(mp, oracle, done, src):
    """every finished stream equals the product's own ragged whole-file call on a batch created with the streams' bitrates; the
    shortest, the longest and two others the oracle.  mp None (the emulated build, where that ragged call -- 92 streams of up to
    20 frames -- takes as long again as the schedule, ten minutes): EVERY stream against the oracle instead."""
    rate, ch = CHURN["rate"], CHURN["ch"]
    assert len(done) > CHURN["S"] and len(set(d[3] for d in done)) == 4, len(done)
    if mp is None:
        for s, a, n, k, data in done:
            assert data == oracle.encode(src[s, a * ch:(a + n) * ch], rate, k, ch)[0], "slot %d, %d samples at %d kbps" % (s, n, k)
        return
    L = mp.lib
    L.mp3mi_batch_encode_ragged.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.c_void_p]
    N, max_nf = len(done), CHURN["n_calls"] * CHURN["nf"]
    pcm = np.zeros((N, max_nf * 1152 * ch), np.int16)
    for j, (s, a, n, _, _) in enumerate(done):
        pcm[j, :n * ch] = src[s, a * ch:(a + n) * ch]
    ns = np.array([d[2] for d in done], np.int32)
    karr = np.array([d[3] for d in done], np.int32)
    mem = DevMem(mp)
    b = ctypes.c_void_p()
    assert L.mp3mi_batch_create(ctypes.byref(b), N, rate, ch, karr.ctypes.data, 0, max_nf) == 0
    try:
        stride = L.mp3mi_batch_out_stride(b, max_nf)
        d_pcm, d_ns, d_out, d_len = mem.alloc(pcm.nbytes), mem.alloc(ns.nbytes), mem.alloc(N * stride), mem.alloc(4 * N)
        mem.upload(d_pcm, pcm)
        mem.upload(d_ns, ns)
        assert L.mp3mi_batch_encode_ragged(b, d_pcm, d_ns, max_nf, d_out, stride, d_len) == 0 and L.mp3mi_batch_sync(b) == 0
        out, ln = mem.download(d_out, (N, stride), np.uint8), mem.download(d_len, (N,), np.uint32)
    finally:
        L.mp3mi_batch_destroy(b)
        mem.free()
    bad = [j for j in range(N) if out[j, :ln[j]].tobytes() != done[j][4]]
    assert not bad, "%d of %d streams differ from the ragged call (first: slot %d, %d samples at %d kbps)" % (
        len(bad), N, done[bad[0]][0], done[bad[0]][2], done[bad[0]][3])
    order = sorted(range(N), key=lambda j: done[j][2])
    for j in sorted(set([order[0], order[-1], order[N // 3], order[2 * N // 3]])):
        s, a, n, k, data = done[j]
        assert data == oracle.encode(src[s, a * ch:(a + n) * ch], rate, k, ch)[0], "slot %d, %d samples at %d kbps" % (s, n, k)


def churn_setup(monkeypatch):
    monkeypatch.setenv("MP3MI_CALL_HOLD", "1")
    monkeypatch.setenv("MP3MI_CHUNK_FRAMES", "1")
    sched = churn_schedule(CHURN["S"], CHURN["n_calls"], CHURN["nf"], CHURN["seed"])
    return sched, churn_kbps(sched, CHURN["S"], CHURN["seed"] + 1)


# ---- case 7: host rows ----
def host_rows_case(mp, oracle):
    """4 slots, 2 rows, row_slot_host = [1, 3], kbps_host by row: the bytes of the device call for the same streams, tick by tick"""
    L = bind(mp)
    S, nf, rate, ch = 4, 2, 44100, 2
    full = nf * 1152
    pcms = [mp.synth(full + 700, ch, rate, 95), mp.synth(3 * full - 5, ch, rate, 96)]  # slot 1 at 64, slot 3 at 192
    ticks = [  # (rows, ctl, n_samples, kbps) by row
        ([1, 3], [START, START], [full, full], [64, 192]),
        ([1, 3], [END, 0], [700, full], [64, 0]),
        ([3], [END], [full - 5], [192]),
    ]
    host = HostRun(mp, S, rate, ch, 320, nf)
    dev = KbpsRun(mp, S, rate, ch, 320, nf)
    try:
        got, pos = {1: b"", 3: b""}, {1: 0, 3: 0}
        for t, (rows, ctl, ns, kb) in enumerate(ticks):
            R = len(rows)
            pcm = np.zeros((R, host.row), np.int16)
            for r, s in enumerate(rows):
                pcm[r, :ns[r] * ch] = pcms[s // 2][pos[s] * ch:(pos[s] + ns[r]) * ch]
                pos[s] += ns[r]
            out, lens = host.buf((R, host.stride), np.uint8, 0x5A), host.buf((R,), np.uint32, 0xDEADBEEF)
            h_pcm = host.buf((R, host.row), np.int16, 0)
            h_pcm[...] = pcm
            rows_a, ctl_a = np.array(rows, np.int32), np.array(ctl, np.uint8)
            ns_a, kb_a = np.array(ns, np.int32), np.array(kb, np.int32)
            assert L.mp3mi_batch_encode_slots_kbps_host_async(host.b, h_pcm.ctypes.data, nf, R, rows_a.ctypes.data, ctl_a.ctypes.data, ns_a.ctypes.data,
                                                              kb_a.ctypes.data, out.ctypes.data, host.stride, lens.ctypes.data) == 0, t
            for a in (rows_a, ns_a, kb_a):
                a[...] = -1  # (copied before the call returned)
            assert host.sync() == 0
            d_pcm, d_ctl, d_ns, d_kb = np.zeros((S, dev.row), np.int16), [0] * S, [0] * S, [0] * S
            for r, s in enumerate(rows):
                d_pcm[s], d_ctl[s], d_ns[s], d_kb[s] = pcm[r], ctl[r], ns[r], kb[r]
            assert dev.call(d_pcm, d_ctl, d_ns, kbps=d_kb) == 0 and dev.L.mp3mi_batch_sync(dev.b) == 0
            outs, dlens = dev.outputs()
            k_host = np.zeros(S, np.int32)
            assert L.mp3mi_batch_slot_kbps(host.b, k_host.ctypes.data) == 320 and (list(k_host), 320) == dev.slot_kbps()
            assert host.frames() == list(dev.frames())
            for r, s in enumerate(rows):
                assert out[r, :lens[r]].tobytes() == outs[s], (t, s)
                assert not out[r, lens[r]:].any()
                got[s] += outs[s]
            assert sum(dlens) == sum(lens)
        assert got[1] == oracle.encode(pcms[0], rate, 64, ch)[0] and got[3] == oracle.encode(pcms[1], rate, 192, ch)[0]
        # a row's bitrate rules are its slot's: not a Layer III bitrate, negative, above the ceiling
        z = host.buf((1, host.row), np.int16, 0)
        o, ln = host.buf((1, host.stride), np.uint8, 0), host.buf((1,), np.uint32, 0)
        row2, start1 = np.array([2], np.int32), np.array([START], np.uint8)
        for k in (100, -32, 384):
            bad_kb = np.array([k], np.int32)
            assert L.mp3mi_batch_encode_slots_kbps_host_async(host.b, z.ctypes.data, nf, 1, row2.ctypes.data, start1.ctypes.data, None, bad_kb.ctypes.data,
                                                              o.ctypes.data, host.stride, ln.ctypes.data) == ERR_ARG, k
        assert host.frames() == [-1] * S
    finally:
        host.close()
        dev.close()


# ------------------------------------------------------------------------------------------------------------------- emulator

def test_mixed_bitrates_slot_reuse_emulated(emu, oracle):
    mixed_case(emu, oracle)


def test_other_formats_emulated(emu, oracle):
    other_formats_case(emu, oracle)


def test_flush_abort_at_own_bitrate_emulated(emu, oracle):
    flush_abort_case(emu, oracle)


def test_bitrate_rules_emulated(emu, oracle):
    rules_case(emu, oracle)


def test_back_to_create_time_bitrates_emulated(emu, oracle):
    back_to_create_case(emu, oracle)


def test_churn_synchronised_emulated(emu, oracle, monkeypatch):
    """the synchronised half of test_churn_two_calls_in_flight_gpu's schedule (64 slots, 10 calls of 2 frames, the shape the two-calls-in-flight
    case is defined at: ten to twelve minutes on the emulator, which runs one workgroup at a time); every finished stream is the oracle's"""
    sched, kbps = churn_setup(monkeypatch)
    _, done, src = churn_run(emu, sched, kbps, sync_each=True)
    churn_check(None, oracle, done, src)


def test_host_rows_emulated(emu, oracle):
    host_rows_case(emu, oracle)


# ---------------------------------------------------------------------------------------------------------------------- device

def chunked(monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("MP3MI_CHUNK_FRAMES", str(chunk))  # starts and ends in different chunks


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_mixed_bitrates_slot_reuse_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    mixed_case(product, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_other_formats_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    other_formats_case(product, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_flush_abort_at_own_bitrate_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    flush_abort_case(product, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_bitrate_rules_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    rules_case(product, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_back_to_create_time_bitrates_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    back_to_create_case(product, oracle)


@pytest.mark.gpu
def test_churn_two_calls_in_flight_gpu(product, oracle, monkeypatch):
    """the schedule once with a sync after every call and once back to back (call hold on, one-frame chunks, another control block
    and other bitrates each call): the same bytes and lengths call for call -- a START's bitrate reaches the live arrays behind
    the kernels of the call before, which may still run, held even, and ahead of its own"""
    sched, kbps = churn_setup(monkeypatch)
    a_calls, a_done, src = churn_run(product, sched, kbps, sync_each=True)
    b_calls, b_done, _ = churn_run(product, sched, kbps, sync_each=False)
    for k, (a, b) in enumerate(zip(a_calls, b_calls)):
        assert a[1] == b[1], "call %d: lengths differ" % k
        assert a[0] == b[0], "call %d: bytes differ" % k
    assert a_done == b_done
    churn_check(product, oracle, a_done, src)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_host_rows_gpu(product, oracle, monkeypatch, chunk):
    chunked(monkeypatch, chunk)
    host_rows_case(product, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_python_binding_gpu(product, oracle, monkeypatch, chunk):
    """Batch.encode_slots(kbps=...) and Batch.slot_kbps() on the device: case 1's streams"""
    import importlib
    import torch
    chunked(monkeypatch, chunk)
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    dev = torch.device("cuda:0")
    S, nf, rate, ch = 3, 2, 44100, 2
    full = nf * 1152
    src = mixed_sources(product)
    b = mp3.Batch(S, rate, ch, 320, nf)
    try:
        stride = b.out_stride(nf)
        out = torch.zeros((S, stride), dtype=torch.uint8, device=dev)
        lens = torch.zeros(S, dtype=torch.int32, device=dev)
        nxt, cur, pos, acc, rate_of, done = [iter(x) for x in src], [None] * S, [0] * S, [b""] * S, [0] * S, []

        def collect(ending):
            torch.cuda.synchronize()
            o, n = out.cpu().numpy(), lens.cpu().numpy()
            for s in range(S):
                if cur[s] is None:
                    assert n[s] == 0
                    continue
                acc[s] += o[s, :n[s]].tobytes()
                if ending[s]:
                    done.append((s, rate_of[s], cur[s][:pos[s] * ch], acc[s]))
                    cur[s] = None

        assert b.slot_kbps()[1] == 320 and list(b.slot_kbps()[0]) == [320] * S
        for step, kb in zip(MIXED_PLAN, MIXED_KBPS):
            pcm = np.zeros((S, full * ch), np.int16)
            ns = np.zeros(S, np.int32)
            for s, (c, n) in enumerate(step):
                if c & START:
                    cur[s], pos[s], acc[s], rate_of[s] = next(nxt[s]), 0, b"", kb[s] or 320
                if cur[s] is None:
                    continue
                ns[s] = n if c & END else full
                pcm[s, :ns[s] * ch] = cur[s][pos[s] * ch:(pos[s] + ns[s]) * ch]
                pos[s] += ns[s]
            ending = [bool(c & END) for c, _ in step]
            d_pcm = torch.from_numpy(pcm).to(dev)
            b.encode_slots(d_pcm, nf, out, lens, start=[bool(c & START) for c, _ in step], end=ending, n_samples=ns, kbps=kb)
            b.sync()
            collect(ending)
            want = [rate_of[s] if cur[s] is not None else 320 for s in range(S)]
            assert list(b.slot_kbps()[0]) == want, (list(b.slot_kbps()[0]), want)
        with pytest.raises(mp3.Mp3miError):
            b.encode_slots(d_pcm, nf, out, lens, kbps=[64, 0, 0])  # slot 0 is closed
        b.flush(out, lens)
        b.sync()
        collect([True] * S)
        assert sorted((s, k, len(p) // ch) for s, k, p, _ in done) == sorted(MIXED_STREAMS)
        for s, k, p, data in done:
            assert data == oracle.encode(p, rate, k, ch)[0], (s, k)
    finally:
        b.close()
