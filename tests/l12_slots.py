"""Continuous batching for Layers I and II (mp3mi_l12_batch_encode_slots, include/mp3mi_l12.h): helpers shared by the CPU tests
(tests/test_l12_slots.py, on the emulated build) and the GPU tests (tests/test_gpu_l12_slots.py).  A SlotRun is a batch driven call
by call on memory of the library under test; drive() runs a plan over it and checks, after EVERY call, out_len 0 and an untouched
output row for the closed slots -- whose PCM rows hold full-scale noise -- and mp3mi_l12_batch_slot_frames against its own count;
check() compares EVERY ended stream with the CPU oracle and with the library's own ragged whole-file call."""
import ctypes

import numpy as np

from mp3common import DevMem, L12_MODES, L12Run, l12_signal, l12_spf, oracle_l12

START, END = 1, 2  # MP3MI_SLOT_START, MP3MI_SLOT_END
FILL = 0xA5        # what an output row holds before a call


def bind(mp):
    L = mp.lib
    vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.mp3mi_l12_batch_create.argtypes = [ctypes.POINTER(vp)] + [ci] * 4 + [vp, ci, ci, ctypes.c_uint]
    L.mp3mi_l12_batch_destroy.argtypes = [vp]
    L.mp3mi_l12_batch_set_mode.argtypes = [vp, ci]
    L.mp3mi_l12_batch_set_error_protection.argtypes = [vp, ci]
    L.mp3mi_l12_batch_out_stride.restype = sz
    L.mp3mi_l12_batch_out_stride.argtypes = [vp, ci]
    L.mp3mi_l12_batch_sync.argtypes = [vp]
    L.mp3mi_l12_batch_encode.argtypes = [vp] * 3 + [ci, vp, sz, vp]
    L.mp3mi_l12_batch_encode_next.argtypes = [vp, vp, ci, vp, sz, vp]
    L.mp3mi_l12_batch_flush.argtypes = [vp, vp, sz, vp]
    L.mp3mi_l12_batch_reset.argtypes = [vp]
    L.mp3mi_l12_batch_kernel_timing.argtypes = [vp, vp, vp]
    L.mp3mi_l12_batch_encode_slots.argtypes = [vp, vp, ci, vp, vp, vp, sz, vp]  # (AttributeError without the feature)
    L.mp3mi_l12_batch_slot_frames.argtypes = [vp, vp]
    return L


class SlotRun:
    """mode: the driver's -m letter (s / d / j / m), followed by e for error protection; kbps: one, or one per slot"""

    def __init__(self, mp, layer, S, rate, mode, kbps, nf, scratch_mb=0):
        self.mp, self.layer, self.S, self.rate, self.mode, self.nf = mp, layer, S, rate, mode, nf
        self.ch = 1 if mode[0] == "m" else 2
        self.spf = l12_spf(layer)
        self.kbps = [kbps] * S if np.isscalar(kbps) else list(kbps)
        self.L = L = bind(mp)
        self.mem = DevMem(mp)
        self.b = ctypes.c_void_p()
        karr = np.ascontiguousarray(self.kbps, dtype=np.int32)
        assert L.mp3mi_l12_batch_create(ctypes.byref(self.b), layer, S, rate, self.ch, karr.ctypes.data, 0, nf, scratch_mb) == 0
        assert L.mp3mi_l12_batch_set_mode(self.b, L12_MODES[mode[0]]) == 0
        assert L.mp3mi_l12_batch_set_error_protection(self.b, int("e" in mode[1:])) == 0
        self.stride = L.mp3mi_l12_batch_out_stride(self.b, nf)
        self.d_pcm = self.mem.alloc(S * nf * self.spf * self.ch * 2)
        self.d_out = self.mem.alloc(S * self.stride)
        self.d_len = self.mem.alloc(4 * S)

    def put(self, pcm):
        self.mem.upload(self.d_pcm, np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.S, -1))
        self.mem.upload(self.d_out, np.full(self.S * self.stride, FILL, np.uint8))
        self.mem.upload(self.d_len, np.full(self.S, 0xFFFFFFFF, np.uint32))

    def call(self, pcm, ctl, ns=None, nf=None, stride=None, pcm_ptr=True):
        """mp3mi_l12_batch_encode_slots on pcm [S][nf * frame * channels]; returns its code"""
        nf = self.nf if nf is None else nf
        self.put(pcm)
        ctl = None if ctl is None else np.ascontiguousarray(ctl, dtype=np.uint8)
        ns = None if ns is None else np.ascontiguousarray(ns, dtype=np.int32)
        return self.L.mp3mi_l12_batch_encode_slots(self.b, self.d_pcm if pcm_ptr else None, nf, None if ctl is None else ctl.ctypes.data,
                                                   None if ns is None else ns.ctypes.data, self.d_out, self.stride if stride is None else stride,
                                                   self.d_len)

    def encode_next(self, pcm, nf):
        self.put(pcm)
        return self.L.mp3mi_l12_batch_encode_next(self.b, self.d_pcm, nf, self.d_out, self.stride, self.d_len)

    def flush(self):
        self.mem.upload(self.d_out, np.full(self.S * self.stride, FILL, np.uint8))
        self.mem.upload(self.d_len, np.full(self.S, 0xFFFFFFFF, np.uint32))
        return self.L.mp3mi_l12_batch_flush(self.b, self.d_out, self.stride, self.d_len)

    def outputs(self):
        """(bytes per slot, lengths, the whole rows) of the last call, after a sync"""
        assert self.L.mp3mi_l12_batch_sync(self.b) == 0
        out = self.mem.download(self.d_out, (self.S, self.stride), np.uint8)
        lens = self.mem.download(self.d_len, (self.S,), np.uint32)
        assert (lens <= self.stride).all(), lens
        return [out[s, :lens[s]].tobytes() for s in range(self.S)], lens, out

    def frames(self):
        f = np.full(self.S, -7, np.int64)
        n = self.L.mp3mi_l12_batch_slot_frames(self.b, f.ctypes.data)
        assert n == int((f >= 0).sum())
        return [int(x) for x in f]

    def launches(self):
        ms, n = (ctypes.c_double * 4)(), (ctypes.c_long * 4)()
        assert self.L.mp3mi_l12_batch_kernel_timing(self.b, ms, n) == 0
        return list(n)

    def close(self):
        if self.b:
            self.L.mp3mi_l12_batch_destroy(self.b)
            self.b = ctypes.c_void_p()
        self.mem.free()


def loud(n, seed):
    """full-scale noise, n int16"""
    return np.random.default_rng(seed).choice(np.array([-32768, 32767], np.int16), n)


def plan_from(scripts, nfs):
    """scripts[s][k]: what slot s does in call k -- "S" START, "." go on (or stay closed), ("E", n) END on n samples, ("SE", n) a
    one-call file of n samples; nfs[k]: frames of call k.  Returns the plan of drive()."""
    tok = lambda t: (START, 0) if t == "S" else (0, 0) if t == "." else ({"E": END, "SE": START | END}[t[0]], t[1])
    assert all(len(sc) == len(nfs) for sc in scripts)
    return [(nf, [tok(sc[k]) for sc in scripts]) for k, nf in enumerate(nfs)]


def new_state(S, sources):
    return dict(cur=[None] * S, pos=[0] * S, got=[b""] * S, frames=[-1] * S, nxt=[iter(sources[s]) for s in range(S)], calls=0)


def drive(run, plan, sources, state=None):
    """plan: per call (n_frames, [(ctl, n) per slot]) (n: samples of an ENDing stream in the call, else ignored); sources[s]: the PCM
    of the streams slot s STARTs, in order (interleaved int16, long enough).  A START over an open stream abandons it.  Returns
    [(slot, pcm, bytes)] of every stream that ended.  state (new_state): kept for a further drive() over the same run."""
    S, ch, spf = run.S, run.ch, run.spf
    st = state if state is not None else new_state(S, sources)
    cur, pos, got, frames, nxt = st["cur"], st["pos"], st["got"], st["frames"], st["nxt"]
    done = []
    for nf, step in plan:
        k = st["calls"]
        st["calls"] += 1
        full = nf * spf
        pcm = loud(S * full * ch, 1000 + k).reshape(S, full * ch)  # closed slots, and what follows an ENDing stream's last sample
        ctl = np.zeros(S, np.uint8)
        ns = np.zeros(S, np.int32)
        for s, (c, n) in enumerate(step):
            ctl[s] = c
            if c & START:
                cur[s], pos[s], got[s], frames[s] = next(nxt[s]), 0, b"", 0
            if cur[s] is None:
                assert c == 0
                continue
            ns[s] = n if c & END else full
            piece = cur[s][pos[s] * ch:(pos[s] + ns[s]) * ch]
            assert len(piece) == ns[s] * ch, "source of slot %d too short" % s
            pcm[s, :len(piece)] = piece
            pos[s] += ns[s]
        assert run.call(pcm, ctl, ns, nf=nf) == 0, "call %d" % k
        outs, lens, rows = run.outputs()
        for s in range(S):
            if cur[s] is None:
                assert lens[s] == 0, (k, s, lens[s])
                assert (rows[s] == FILL).all(), "call %d wrote into the row of closed slot %d" % (k, s)
                continue
            got[s] += outs[s]
            frames[s] += (ns[s] + spf - 1) // spf if ctl[s] & END else nf
            if ctl[s] & END:
                done.append((s, cur[s][:pos[s] * ch], got[s]))
                cur[s], frames[s] = None, -1
        assert run.frames() == frames, (k, run.frames(), frames)
    return done


def ragged_whole_file(mp, run, streams):
    """the library's own whole-file call over [(kbps, pcm)] as one ragged batch"""
    n_frames = max(1, max((len(p) // run.ch + run.spf - 1) // run.spf for _, p in streams))
    ref = L12Run(mp, run.layer, run.rate, [k for k, _ in streams], run.mode, [p for _, p in streams], n_frames=n_frames)
    try:
        return ref.encode()
    finally:
        ref.close()


def check(run, orc, done, n_least):
    """every ended stream: the oracle's bytes, and the ragged whole-file call's"""
    assert len(done) >= n_least, (len(done), n_least)
    whole = ragged_whole_file(run.mp, run, [(run.kbps[s], p) for s, p, _ in done])
    for (s, pcm, data), w in zip(done, whole):
        ref = oracle_l12(orc, run.layer, run.rate, run.kbps[s], run.mode, pcm)[0]
        what = "slot %d, %d samples: %d bytes" % (s, len(pcm) // run.ch, len(data))
        assert data == ref, "%s vs the oracle's %d" % (what, len(ref))
        assert data == w, "%s vs the whole-file call's %d" % (what, len(w))


def sources_for(run, scripts, seed, n_per_ch):
    """a signal per START of every script"""
    return [[l12_signal(n_per_ch, run.ch, seed + 16 * s + j, run.rate) for j in range(sum(1 for t in sc if t == "S" or t[0] == "SE"))]
            for s, sc in enumerate(scripts)]


# ---- the churn plans at the smallest calls: STARTs in different calls, so that one call holds slots at frames 0, 1, 2 and >= 5 (Layer I
# needs 1792 samples = 4.7 frames of history: a stream's history spans five calls of one frame); ENDs on a partial frame, on a
# whole frame and with 0 samples; START | END, START | END with 0 samples; a START over an open stream (slot 2)
L1_NFS = [1] * 14
L1_SCRIPTS = [
    ["S", ".", ".", ".", ".", ".", ".", ".", ".", ".", ".", ".", ".", ("E", 100)],
    [".", "S", ".", ".", ".", ".", ".", ("E", 384), ".", "S", ".", ".", ".", ("E", 0)],
    [".", ".", "S", ".", ".", ".", ".", ".", ".", "S", ".", ".", ".", ("E", 1)],
    [("SE", 200), ".", ".", "S", ".", ".", ".", ".", ".", ".", ".", ("E", 383), ".", ("SE", 0)],
    [".", ".", ".", ".", "S", ".", ".", ".", ".", ".", ("E", 0), "S", ".", ("E", 384)],
    [".", ".", ".", ".", ".", "S", ".", ".", ".", ".", ".", ".", ".", ("E", 50)],
    [("SE", 0), "S", ".", ".", ".", ".", ".", ("E", 77), ("SE", 384), ".", ".", "S", ".", ("E", 300)],
    [".", ".", ".", ".", ".", ".", "S", ".", ("E", 10), ".", ".", ".", ("SE", 5), "."],
]
L2_NFS = [1, 2, 1, 1, 2, 1, 2, 1]
L2_SCRIPTS = [
    ["S", ".", ".", ".", ".", ".", ".", ("E", 700)],
    [".", "S", ".", ("E", 1152), ("SE", 0), "S", ".", ("E", 0)],
    [("SE", 1000), ".", "S", ".", ".", "S", ".", ("E", 1152)],
    [".", ".", ".", "S", ".", ".", ("E", 1153), ("SE", 0)],
    [".", ("SE", 2304), "S", ".", ("E", 0), ".", "S", ("E", 5)],
    [".", ".", ".", ".", "S", ".", ("E", 2000), "."],
]


def churn(mp, orc, layer, S, rate=44100, mode="s", kbps=None, seed=0):
    """the layer's churn plan over S slots (slot s runs script s modulo the scripts); every slot is closed at its end"""
    base, nfs = (L1_SCRIPTS, L1_NFS) if layer == 1 else (L2_SCRIPTS, L2_NFS)
    scripts = [base[s % len(base)] for s in range(S)]
    run = SlotRun(mp, layer, S, rate, mode, kbps or (192 if layer == 1 else 128), max(nfs))
    try:
        src = sources_for(run, scripts, 300 + seed, sum(nfs) * run.spf)
        done = drive(run, plan_from(scripts, nfs), src)
        assert run.frames() == [-1] * S
        check(run, orc, done, S)
        # nothing is open: the flush delivers nothing
        assert run.flush() == 0
        _, lens, rows = run.outputs()
        assert (lens == 0).all() and (rows == FILL).all()
    finally:
        run.close()
    return done


def history_cleared(mp, orc, layer, S=2):
    """a slot runs full-scale noise to its END; in the very next call a quiet stream STARTs there, beside a neighbour that goes on"""
    nf = 2 if layer == 1 else 1
    run = SlotRun(mp, layer, S, 44100, "s", 192 if layer == 1 else 128, nf)
    try:
        full = nf * run.spf
        quiet = lambda sd: (np.random.default_rng(sd).integers(-20, 21, 3 * full * run.ch)).astype(np.int16)
        scripts, src = [], []
        for s in range(S):
            if s % 2 == 0:
                scripts.append(["S", ".", ".", ("E", full), "S", ".", ("E", 100)])
                src.append([loud(4 * full * run.ch, 50 + s), quiet(60 + s)])
            else:
                scripts.append(["S", ".", ".", ".", ".", ".", ("E", 7)])
                src.append([l12_signal(7 * full, run.ch, 70 + s)])
        done = drive(run, plan_from(scripts, [nf] * 7), src)
        check(run, orc, done, S + (S + 1) // 2)
    finally:
        run.close()
