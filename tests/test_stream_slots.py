"""Continuous batching (mp3mi_batch_encode_slots, include/mp3mi.h): every stream index of a batch is a slot through which
one stream after another passes, each beginning and ending in a call of its own -- on a partial frame too -- while the
other slots go on.  The bytes a slot delivers from a stream's START call through its END call, concatenated, must be the
stream's file: the oracle's, and the product's own ragged whole-file call's."""
import ctypes

import numpy as np
import pytest

from golden_util import aborting_cases, case_pcm
from mp3common import ERR_REFERENCE_ABORT, DevMem, ReferenceAborts

START, END = 1, 2  # MP3MI_SLOT_START, MP3MI_SLOT_END


def bind(mp):
    L = mp.lib
    L.mp3mi_batch_encode_slots.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.mp3mi_batch_slot_frames.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.mp3mi_batch_encode_ragged.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_size_t, ctypes.c_void_p]
    return L


class SlotRun:
    """A batch driven call by call through mp3mi_batch_encode_slots on memory of the library under test"""

    def __init__(self, mp, S, rate, ch, kbps, nf, mode=None, crc=False):
        self.mp, self.S, self.rate, self.ch, self.nf = mp, S, rate, ch, nf
        self.kbps = [kbps] * S if np.isscalar(kbps) else list(kbps)
        self.L = L = bind(mp)
        self.mem = DevMem(mp)
        self.b = ctypes.c_void_p()
        karr = None if np.isscalar(kbps) else np.ascontiguousarray(kbps, dtype=np.int32)
        assert L.mp3mi_batch_create(ctypes.byref(self.b), S, rate, ch, karr.ctypes.data if karr is not None else None,
                                    int(kbps) if karr is None else 0, nf) == 0
        if mode is not None:
            assert L.mp3mi_batch_set_mode(self.b, mode) == 0
        if crc:
            assert L.mp3mi_batch_set_error_protection(self.b, 1) == 0
        self.stride = L.mp3mi_batch_out_stride(self.b, nf)
        self.row = nf * 1152 * ch
        self.d_pcm = self.mem.alloc(S * self.row * 2)
        self.d_out = self.mem.alloc(S * self.stride)
        self.d_len = self.mem.alloc(4 * S)

    def call(self, pcm, ctl, ns=None, nf=None, stride=None, pcm_ptr=True):
        nf = self.nf if nf is None else nf
        pcm = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.S, -1)
        self.mem.upload(self.d_pcm, pcm)
        ctl = None if ctl is None else np.ascontiguousarray(ctl, dtype=np.uint8)
        ns = None if ns is None else np.ascontiguousarray(ns, dtype=np.int32)
        return self.L.mp3mi_batch_encode_slots(self.b, self.d_pcm if pcm_ptr else None, nf, None if ctl is None else ctl.ctypes.data,
                                               None if ns is None else ns.ctypes.data, self.d_out, self.stride if stride is None else stride,
                                               self.d_len)

    def outputs(self):
        out = self.mem.download(self.d_out, (self.S, self.stride), np.uint8)
        lens = self.mem.download(self.d_len, (self.S,), np.uint32)
        return [out[s, :lens[s]].tobytes() for s in range(self.S)], lens

    def frames(self):
        f = np.zeros(self.S, np.int64)
        n = self.L.mp3mi_batch_slot_frames(self.b, f.ctypes.data)
        assert n == int((f >= 0).sum())
        return f

    def status(self):
        st = np.zeros(self.S, np.int32)
        assert self.L.mp3mi_batch_stream_status(self.b, st.ctypes.data) >= 0
        return st

    def close(self):
        if self.b:
            self.L.mp3mi_batch_destroy(self.b)
            self.b = ctypes.c_void_p()
        self.mem.free()


def drive(run, plan, sources, flush=True, aborts=(), state=None):
    """plan: per call a list of (ctl, n) per slot (n: samples of an ENDing stream in the call, else ignored); sources[s]: the
    PCM of the streams slot s runs, in order (interleaved int16, long enough).  Checks out_len 0 for closed slots and
    mp3mi_batch_slot_frames after every call.  Returns [(slot, pcm, bytes)] of every stream that ended; `aborts`: indices of
    calls after which the sync is to report an abort.  With flush=False the slots' state is kept in `state` (a dict) for a
    further drive() over the same run."""
    S, ch, full = run.S, run.ch, run.nf * 1152
    if state is None or not state:
        st = dict(cur=[None] * S, pos=[0] * S, got=[b""] * S, frames=[-1] * S, nxt=[iter(sources[s]) for s in range(S)])
        if state is not None:
            state.update(st)
        state = st
    cur, pos, got, frames, nxt = state["cur"], state["pos"], state["got"], state["frames"], state["nxt"]
    done = []
    for k, step in enumerate(plan):
        pcm = np.zeros((S, run.row), np.int16)
        ctl = np.zeros(S, np.uint8)
        ns = np.zeros(S, np.int32)
        for s, (c, n) in enumerate(step):
            ctl[s] = c
            if c & START:
                cur[s], pos[s], got[s], frames[s] = next(nxt[s]), 0, b"", 0
            if cur[s] is None:
                continue
            ns[s] = n if c & END else full
            piece = cur[s][pos[s] * ch:(pos[s] + ns[s]) * ch]
            assert len(piece) == ns[s] * ch
            pcm[s, :len(piece)] = piece
            pos[s] += ns[s]
        assert run.call(pcm, ctl, ns) == 0, "call %d" % k
        rc = run.L.mp3mi_batch_sync(run.b)
        assert rc == (ERR_REFERENCE_ABORT if k in aborts else 0), (k, rc)
        outs, lens = run.outputs()
        for s in range(S):
            if cur[s] is None:
                assert lens[s] == 0, (k, s)
                continue
            got[s] += outs[s]
            frames[s] += (ns[s] + 1151) // 1152 if ctl[s] & END else run.nf
            if ctl[s] & END:
                done.append((s, cur[s][:pos[s] * ch], got[s]))
                cur[s], frames[s] = None, -1
        assert list(run.frames()) == frames, (k, list(run.frames()), frames)
    if flush:
        assert run.L.mp3mi_batch_flush(run.b, run.d_out, run.stride, run.d_len) == 0
        assert run.L.mp3mi_batch_sync(run.b) == 0
        outs, lens = run.outputs()
        for s in range(S):
            if cur[s] is None:
                assert lens[s] == 0, s
            else:
                done.append((s, cur[s][:pos[s] * ch], got[s] + outs[s]))
        assert list(run.frames()) == [-1] * S
    return done


def check_oracle(run, oracle, done, mode=None, skip=()):
    for s, pcm, data in done:
        if any(np.shares_memory(pcm, x) for x in skip):
            continue
        ref = oracle.encode(pcm, run.rate, run.kbps[s], run.ch, mode=mode)[0]
        assert data == ref, "slot %d, %d samples: %d bytes vs the oracle's %d" % (s, len(pcm) // run.ch, len(data), len(ref))


def synth_streams(mp, run, seeds, n_per_ch=None):
    n = n_per_ch or 8 * 1152
    return [mp.synth(n, run.ch, run.rate, sd) for sd in seeds]


def staggered(mp, oracle, rate, ch, kbps, mode=None, crc=False, oracle_mode=None):
    """case 1: slot 0 open through four calls and ENDing on 1000 samples; slot 1 STARTing in call 2, ENDing in call 3 with
    0 samples and then a one-call file of 2 * 1152 - 5 samples; slot 2 closed for two calls, STARTing in call 3 and ended
    by the flush"""
    run = SlotRun(mp, 3, rate, ch, kbps, 2, mode=mode, crc=crc)
    try:
        src = [synth_streams(mp, run, [11]), synth_streams(mp, run, [12, 13]), synth_streams(mp, run, [14])]
        plan = [
            [(START, 0), (0, 0), (0, 0)],
            [(0, 0), (START, 0), (0, 0)],
            [(0, 0), (END, 0), (START, 0)],
            [(END, 1000), (START | END, 2 * 1152 - 5), (0, 0)],
        ]
        done = drive(run, plan, src)
        assert sorted((s, len(p) // ch) for s, p, _ in done) == [(0, 3 * 2304 + 1000), (1, 2299), (1, 2304), (2, 2 * 2304)]
        check_oracle(run, oracle, done, mode=oracle_mode)
        # the slots are closed: encode_next starts every one of them again, as after a flush
        assert run.L.mp3mi_batch_encode_next(run.b, run.d_pcm, 2, run.d_out, run.stride, run.d_len) == 0
        assert list(run.frames()) == [2, 2, 2]
    finally:
        run.close()


def test_staggered_lifecycles_emulated(emu, oracle):
    staggered(emu, oracle, 44100, 2, 128)


def test_slots_against_encode_next_emulated(emu, oracle):
    """all slots STARTed, then continued with ctl 0: encode_next's bytes, call for call; encode_next after a slot ENDed goes
    on with the open slots only, and the flush delivers nothing for the closed one"""
    from mp3common import BatchRun
    rate, ch, kbps, S, nf = 44100, 2, 128, 3, 2
    ref = BatchRun(emu, S, rate, ch, kbps, 3 * nf, stream0=40)
    run = SlotRun(emu, S, rate, ch, kbps, nf)
    try:
        whole = ref.mem.download(ref.d_pcm, (S, ref.n_per_ch * ch), np.int16)
        row = nf * 1152 * ch
        ctl_first = np.full(S, START, np.uint8)
        for k in range(3):
            piece = np.ascontiguousarray(whole[:, k * row:(k + 1) * row])
            ref.mem.upload(run.d_pcm, piece)  # (scratch: the reference run's own buffer follows)
            d_piece = ref.mem.alloc(piece.nbytes)
            ref.mem.upload(d_piece, piece)
            assert emu.lib.mp3mi_batch_encode_next(ref.b, d_piece, nf, ref.d_out, ref.stride, ref.d_len) == 0
            a = [ref.mem.download(ref.d_out + s * ref.stride, (ref.stride,), np.uint8) for s in range(S)]
            la = ref.mem.download(ref.d_len, (S,), np.uint32)
            assert run.call(piece, ctl_first if k == 0 else np.zeros(S, np.uint8)) == 0
            outs, lens = run.outputs()
            assert [a[s][:la[s]].tobytes() for s in range(S)] == outs, "call %d" % k
        assert list(run.frames()) == [6, 6, 6]
        # slot 1 ENDs on 500 samples; encode_next continues slots 0 and 2
        tail = emu.synth(3 * 1152, ch, rate, 41)
        pcm = np.zeros((S, row), np.int16)
        ns = np.array([2304, 500, 2304], np.int32)
        for s in range(S):
            pcm[s, :ns[s] * ch] = tail[:ns[s] * ch]
        assert run.call(pcm, np.array([0, END, 0], np.uint8), ns) == 0
        assert list(run.frames()) == [8, -1, 8]
        assert run.L.mp3mi_batch_encode_next(run.b, run.d_pcm, nf, run.d_out, run.stride, run.d_len) == 0
        _, lens = run.outputs()
        assert lens[1] == 0 and list(run.frames()) == [10, -1, 10]
        assert run.L.mp3mi_batch_flush(run.b, run.d_out, run.stride, run.d_len) == 0 and run.L.mp3mi_batch_sync(run.b) == 0
        _, lens = run.outputs()
        assert lens[1] == 0 and lens[0] > 0 and lens[2] > 0 and list(run.frames()) == [-1, -1, -1]
    finally:
        run.close()
        ref.close()


def test_argument_errors_emulated(emu, oracle):
    """every broken rule returns MP3MI_ERR_ARG and leaves the batch as it was; the next valid call still gives oracle bytes"""
    rate, ch, kbps, S, nf = 44100, 2, 128, 2, 2
    run = SlotRun(emu, S, rate, ch, kbps, nf)
    try:
        full = nf * 1152
        src = [emu.synth(4 * full, ch, rate, 50 + s) for s in range(S)]
        pcm = np.stack([x[:full * ch] for x in src])
        assert run.call(pcm, [START, 0]) == 0  # slot 0 open at 2 frames, slot 1 closed
        first, _ = run.outputs()
        L = run.L
        before = list(run.frames())
        bad = [
            dict(ctl=[4, 0]),                                # unknown bit
            dict(ctl=[0, END], ns=[full, 0]),                # END on a closed slot
            dict(ctl=[0, 0], ns=[full - 1, 0]),              # a continuing stream short of a full call
            dict(ctl=[0, 0], ns=[full, 1]),                  # samples for a closed slot
            dict(ctl=[END, 0], ns=[full + 1, 0]),            # more than a call holds
            dict(ctl=[END, 0], ns=[-1, 0]),
            dict(ctl=[0, START], ns=[full, 7]),              # a starting stream that does not end gives a full call
            dict(ctl=None),                                  # NULL control
            dict(ctl=[0, 0], pcm_ptr=False),                 # NULL PCM
            dict(ctl=[0, 0], nf=0),
            dict(ctl=[0, 0], nf=nf + 1),
            dict(ctl=[0, 0], stride=nf * 417 + 1 + 2047),    # no room for the carried bytes
        ]
        for kw in bad:
            assert run.call(pcm, **kw) == -1, kw
            assert list(run.frames()) == before, kw
        assert L.mp3mi_batch_encode_slots(run.b, run.d_pcm, nf, np.zeros(S, np.uint8).ctypes.data, None, None, run.stride, run.d_len) == -1
        assert L.mp3mi_batch_encode_slots(run.b, run.d_pcm, nf, np.zeros(S, np.uint8).ctypes.data, None, run.d_out, run.stride, None) == -1
        assert L.mp3mi_batch_encode_slots(None, run.d_pcm, nf, np.zeros(S, np.uint8).ctypes.data, None, run.d_out, run.stride, run.d_len) == -1
        assert L.mp3mi_batch_slot_frames(run.b, None) == -1 and L.mp3mi_batch_slot_frames(None, None) == -1
        # valid: slot 0 ENDs on 100 samples, slot 1 is a one-call file of 2000
        pcm2 = np.zeros((S, full * ch), np.int16)
        pcm2[0, :100 * ch] = src[0][full * ch:(full + 100) * ch]
        pcm2[1, :2000 * ch] = src[1][:2000 * ch]
        assert run.call(pcm2, [END, START | END], [100, 2000]) == 0 and L.mp3mi_batch_sync(run.b) == 0
        second, _ = run.outputs()
        assert first[0] + second[0] == oracle.encode(src[0][:(full + 100) * ch], rate, kbps, ch)[0]
        assert second[1] == oracle.encode(src[1][:2000 * ch], rate, kbps, ch)[0]
        assert list(run.frames()) == [-1, -1]
    finally:
        run.close()


def aborts_case(mp, oracle):
    """abort_global_gain in slot 1: voided, reported once, cleared by the slot's next START, after which the slot's next
    stream is the oracle's; abort_flush_slot ENDed inside a call has the status a flush gives it; neighbours untouched"""
    case = [c for c in aborting_cases() if c["name"] == "abort_global_gain"][0]
    bad = case_pcm(case, mp.synth)  # 6 frames: the reference dies in frame 4
    run = SlotRun(mp, 3, 44100, 2, 128, 2)
    try:
        good = [mp.synth(10 * 1152, 2, 44100, 60 + k) for k in range(4)]
        n_bad = len(bad) // 2
        src = [[good[0]], [bad, good[1]], [good[2]]]
        plan = [
            [(START, 0), (START, 0), (START, 0)],
            [(0, 0), (0, 0), (0, 0)],
            [(0, 0), (END, n_bad - 4 * 1152), (0, 0)],  # the aborting frame is in this call
            [(0, 0), (START, 0), (0, 0)],
            [(END, 321), (0, 0), (0, 0)],
        ]
        state = {}
        done = drive(run, plan[:3], src, flush=False, aborts=(2,), state=state)
        assert run.L.mp3mi_batch_sync(run.b) == 0  # reported once
        st = run.status()
        assert st[0] == 0 and st[2] == 0 and (st[1] & 255) == case["reference_aborts"]["status"], st
        assert (st[1] >> 8) == case["reference_aborts"]["frame"], st[1] >> 8
        assert [s for s, _, _ in done] == [1]
        with pytest.raises(ReferenceAborts):
            oracle.encode(bad, 44100, 128, 2)
        done += drive(run, plan[3:], src, state=state)
        st = run.status()
        assert st[1] == 0, st  # START cleared it
        check_oracle(run, oracle, done, skip=(bad,))
        assert sorted((s, len(p) // 2) for s, p, _ in done) == sorted([(0, 4 * 2304 + 321), (1, n_bad), (1, 2 * 2304), (2, 5 * 2304)])
    finally:
        run.close()
    # abort_flush_slot, ENDed inside a call
    case = [c for c in aborting_cases() if c["name"] == "abort_flush_slot"][0]
    bad = case_pcm(case, mp.synth)  # 5 frames at 48 kHz, 64 kbps: the reference dies in its final flush
    run = SlotRun(mp, 2, 48000, 2, 64, 2)
    try:
        good = mp.synth(8 * 1152, 2, 48000, 70)
        plan = [[(START, 0), (START, 0)], [(0, 0), (0, 0)], [(END, 1152), (END, 1000)]]
        done = drive(run, plan, [[bad], [good]], flush=False, aborts=(2,))
        st = run.status()
        assert (st[0] & 255) == case["reference_aborts"]["status"] and (st[0] >> 8) == case["reference_aborts"]["frame"], st[0]
        assert st[1] == 0
        by = {s: (p, d) for s, p, d in done}
        assert by[1][1] == oracle.encode(by[1][0], 48000, 64, 2)[0]
        assert run.L.mp3mi_batch_sync(run.b) == 0
        assert run.status()[0] == st[0]  # kept until the slot STARTs again
    finally:
        run.close()


def other_formats(mp, oracle):
    """mono 32 kHz; 48 kHz with per-stream bitrates 32 and 320 and error protection on"""
    plan = [[(START, 0), (0, 0)], [(0, 0), (START, 0)], [(END, 700), (0, 0)]]
    for rate, ch, kbps, mode, crc, omode in ((32000, 1, 64, None, False, None), (48000, 2, [32, 320], 0, True, "se")):
        run = SlotRun(mp, 2, rate, ch, kbps, 2, mode=mode, crc=crc)
        try:
            src = [synth_streams(mp, run, [80 + s]) for s in range(2)]
            done = drive(run, plan, src)
            assert sorted((s, len(p) // ch) for s, p, _ in done) == [(0, 2 * 2304 + 700), (1, 2 * 2304)]
            check_oracle(run, oracle, done, mode=omode)
        finally:
            run.close()


def test_aborts_and_slot_reuse_emulated(emu, oracle):
    aborts_case(emu, oracle)


def test_other_formats_emulated(emu, oracle):
    other_formats(emu, oracle)


# ---------------------------------------------------------------------------------------------------------------------- device

@pytest.mark.gpu
@pytest.mark.parametrize("rate,ch,kbps,chunk", [(44100, 2, 128, None), (48000, 2, 192, 1), (32000, 1, 56, 1), (44100, 1, 320, 1)])
def test_staggered_lifecycles_gpu(product, oracle, monkeypatch, rate, ch, kbps, chunk):
    if chunk:
        monkeypatch.setenv("MP3MI_CHUNK_FRAMES", str(chunk))  # starts and ends in different chunks
    staggered(product, oracle, rate, ch, kbps)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_aborts_and_slot_reuse_gpu(product, oracle, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("MP3MI_CHUNK_FRAMES", str(chunk))
    aborts_case(product, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 1])
def test_other_formats_gpu(product, oracle, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("MP3MI_CHUNK_FRAMES", str(chunk))
    other_formats(product, oracle)


def churn_schedule(S, n_calls, nf, seed):
    """a seeded server loop: every slot STARTs in the first call; in every call ~1/16 of the open slots END (at a random
    length) and closed slots START.  Returns per call (ctl, n_samples) as host arrays."""
    rng = np.random.default_rng(seed)
    full = nf * 1152
    open_ = np.zeros(S, bool)
    out = []
    for k in range(n_calls):
        ctl = np.zeros(S, np.uint8)
        ctl[~open_] = START if k == 0 else 0
        if k > 0:
            closed = np.flatnonzero(~open_)
            ctl[closed[rng.random(len(closed)) < 0.5]] = START
        ending = open_ & (rng.random(S) < 1 / 16)
        ctl[ending] |= END
        ns = np.where(open_ | (ctl & START > 0), full, 0).astype(np.int32)
        ns[ending] = rng.integers(0, full + 1, int(ending.sum()))
        out.append((ctl, ns))
        open_ = (open_ | (ctl & START > 0)) & ~(ctl & END > 0)
    return out


def churn_run(product, S, rate, ch, kbps, nf, sched, sync_each):
    """Runs the schedule: the stream a slot STARTs in call k reads source row s from sample k * nf * 1152 on.  Returns the
    finished streams [(slot, first sample, samples, bytes)] and the per-call outputs."""
    import importlib
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    dev = torch.device("cuda:0")
    n_calls, full = len(sched), nf * 1152
    src = torch.empty((S, n_calls * full * ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    assert product.lib.mp3mi_synth_pcm_device(src.data_ptr(), S, n_calls * full, ch, rate, 900, 0x6D70336D) == 0
    b = mp3.Batch(S, rate, ch, kbps, nf)
    stride = b.out_stride(nf)
    pcms = [src[:, k * full * ch:(k + 1) * full * ch].contiguous() for k in range(n_calls)]
    outs = [torch.zeros((S, stride), dtype=torch.uint8, device=dev) for _ in range(n_calls + 1)]
    lens = [torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(n_calls + 1)]
    torch.cuda.synchronize()
    for k, (ctl, ns) in enumerate(sched):
        b.encode_slots(pcms[k], nf, outs[k], lens[k], start=ctl & START > 0, end=ctl & END > 0, n_samples=ns)
        if sync_each:
            b.sync()
    b.flush(outs[n_calls], lens[n_calls])
    b.sync()
    b.close()
    got_o = [o.cpu().numpy() for o in outs]
    got_l = [x.cpu().numpy() for x in lens]
    first, acc, done = [None] * S, [b""] * S, []
    for k in range(n_calls + 1):
        ctl, ns = sched[k] if k < n_calls else (np.full(S, END, np.uint8), None)
        for s in range(S):
            if k < n_calls and ctl[s] & START:
                first[s], acc[s] = k, b""
            if first[s] is None:
                assert got_l[k][s] == 0, (k, s)
                continue
            acc[s] += got_o[k][s, :got_l[k][s]].tobytes()
            if ctl[s] & END:
                n = (k - first[s]) * full + (int(ns[s]) if ns is not None else 0)
                done.append((s, first[s] * full, n, acc[s]))
                first[s] = None
    return done, (got_o, got_l), src


@pytest.mark.gpu
def test_full_chip_churn_gpu(product, oracle):
    """4096 slots, 12 calls of 16 frames, ~1/16 of the open slots ENDing per call at random lengths, closed slots STARTing,
    then a flush: every finished stream equals the product's own ragged whole-file call of its samples (one batch), 16 of
    them -- the shortest and the longest among them -- the oracle"""
    import torch
    S, rate, ch, kbps, nf, n_calls = 4096, 44100, 2, 128, 16, 12
    sched = churn_schedule(S, n_calls, nf, 20261016)
    done, _, src = churn_run(product, S, rate, ch, kbps, nf, sched, sync_each=True)
    assert len(done) > S + 1000, len(done)
    L = bind(product)
    N, max_nf = len(done), n_calls * nf
    full_all = max_nf * 1152
    pcm = torch.zeros((N, full_all * ch), dtype=torch.int16, device=src.device)
    for j, (s, a, n, _) in enumerate(done):
        pcm[j, :n * ch] = src[s, a * ch:(a + n) * ch]
    ns = torch.tensor([n for _, _, n, _ in done], dtype=torch.int32, device=src.device)
    b = ctypes.c_void_p()
    assert L.mp3mi_batch_create(ctypes.byref(b), N, rate, ch, None, kbps, max_nf) == 0
    try:
        stride = L.mp3mi_batch_out_stride(b, max_nf)
        out = torch.zeros((N, stride), dtype=torch.uint8, device=src.device)
        ln = torch.zeros(N, dtype=torch.int32, device=src.device)
        torch.cuda.synchronize()
        assert L.mp3mi_batch_encode_ragged(b, pcm.data_ptr(), ns.data_ptr(), max_nf, out.data_ptr(), stride, ln.data_ptr()) == 0
        assert L.mp3mi_batch_sync(b) == 0
        out_h, ln_h = out.cpu().numpy(), ln.cpu().numpy()
    finally:
        L.mp3mi_batch_destroy(b)
    bad = [j for j in range(N) if out_h[j, :ln_h[j]].tobytes() != done[j][3]]
    assert not bad, "%d of %d streams differ from the ragged call (first: slot %d, %d samples)" % (len(bad), N, done[bad[0]][0], done[bad[0]][2])
    order = sorted(range(N), key=lambda j: done[j][2])
    pick = sorted(set(order[:6] + order[-6:] + [order[len(order) * q // 5] for q in range(1, 5)]))
    for j in pick:
        s, a, n, data = done[j]
        ref = oracle.encode(src[s, a * ch:(a + n) * ch].cpu().numpy(), rate, kbps, ch)[0]
        assert data == ref, "slot %d, %d samples" % (s, n)


@pytest.mark.gpu
def test_back_to_back_without_sync_gpu(product, monkeypatch):
    """the churn schedule issued without a sync between the calls (call_hold on, a different control block each call) gives
    the bytes of the synchronised run: the control block's double buffering keeps a call's arrays from being overwritten
    while the kernels of the call before still read them"""
    monkeypatch.setenv("MP3MI_CALL_HOLD", "1")
    S, rate, ch, kbps, nf, n_calls = 1024, 44100, 2, 128, 8, 12
    sched = churn_schedule(S, n_calls, nf, 7)
    a_done, (a_o, a_l), _ = churn_run(product, S, rate, ch, kbps, nf, sched, sync_each=True)
    b_done, (b_o, b_l), _ = churn_run(product, S, rate, ch, kbps, nf, sched, sync_each=False)
    for k in range(n_calls + 1):
        assert (a_l[k] == b_l[k]).all(), "call %d: lengths differ" % k
        for s in range(S):
            assert a_o[k][s, :a_l[k][s]].tobytes() == b_o[k][s, :b_l[k][s]].tobytes(), (k, s)
    assert [d[3] for d in a_done] == [d[3] for d in b_done]
