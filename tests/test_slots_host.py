"""Per-slot streaming on host buffers (mp3mi_batch_encode_slots_host_async, mp3mi_batch_host_wait; include/mp3mi.h): the
per-slot call with every array indexed by ROW -- one dense row per live slot, PCM from and bytes to host memory -- so that
closed slots cost no transfer.  Whichever rows a stream travelled in, its bytes from its START call through its END call
are its file: the oracle's, and those of the device call mp3mi_batch_encode_slots on the same schedule."""
import ctypes

import numpy as np
import pytest

from golden_util import aborting_cases, case_pcm
from mp3common import ERR_REFERENCE_ABORT, ReferenceAborts
from test_stream_slots import END, START, SlotRun


class IoStats(ctypes.Structure):
    _fields_ = [("h2d_bytes", ctypes.c_double), ("d2h_bytes", ctypes.c_double), ("h2d_ms", ctypes.c_double), ("d2h_ms", ctypes.c_double),
                ("calls", ctypes.c_long)]


def bind(mp):
    L = mp.lib
    L.mp3mi_batch_encode_slots_host_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.mp3mi_batch_host_wait.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.mp3mi_batch_slot_frames.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return L


class HostRun:
    """A batch driven tick by tick through mp3mi_batch_encode_slots_host_async.  Buffers: numpy arrays (pageable), or
    page-locked memory of the library when pinned=True; every tick's buffers stay alive until close()."""

    def __init__(self, mp, S, rate, ch, kbps, nf, pinned=False, stride=None, b=None):
        self.mp, self.S, self.rate, self.ch, self.nf, self.pinned = mp, S, rate, ch, nf, pinned
        self.kbps = [kbps] * S if np.isscalar(kbps) else list(kbps)
        self.L = L = bind(mp)
        self.own = b is None
        self.b = ctypes.c_void_p() if b is None else b
        if b is None:
            karr = None if np.isscalar(kbps) else np.ascontiguousarray(kbps, dtype=np.int32)
            assert L.mp3mi_batch_create(ctypes.byref(self.b), S, rate, ch, karr.ctypes.data if karr is not None else None,
                                        int(kbps) if karr is None else 0, nf) == 0
        self.stride = L.mp3mi_batch_out_stride(self.b, nf) if stride is None else stride
        self.row = nf * 1152 * ch
        self.keep, self.raw = [], []

    def buf(self, shape, dtype, fill):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if not self.pinned:
            a = np.empty(shape, dtype)
        else:
            p = self.L.mp3mi_host_alloc(max(n, 1))
            assert p
            self.raw.append(p)
            a = np.ctypeslib.as_array((ctypes.c_uint8 * max(n, 1)).from_address(p))[:n].view(dtype).reshape(shape)
        a[...] = fill
        self.keep.append(a)
        return a

    def tick(self, rows, pcm, ctl, ns=None, nf=None, n_rows=None, stride=None, null=()):
        """rows: the slots of the rows (None: no map); pcm [n_rows][row]; ctl / ns per row.  Returns (rc, out, lens)."""
        nf = self.nf if nf is None else nf
        R = len(pcm)
        h_pcm = self.buf((R, self.row), np.int16, 0)
        h_pcm[...] = np.asarray(pcm, dtype=np.int16).reshape(R, -1)
        out = self.buf((R, self.stride), np.uint8, 0x5A)
        lens = self.buf((R,), np.uint32, 0xDEADBEEF)
        rows_a = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        ctl_a = np.ascontiguousarray(ctl, dtype=np.uint8)
        ns_a = None if ns is None else np.ascontiguousarray(ns, dtype=np.int32)
        arg = dict(pcm=h_pcm.ctypes.data, ctl=ctl_a.ctypes.data, out=out.ctypes.data, len=lens.ctypes.data)
        for k in null:
            arg[k] = None
        rc = self.L.mp3mi_batch_encode_slots_host_async(self.b, arg["pcm"], nf, R if n_rows is None else n_rows,
                                                        None if rows_a is None else rows_a.ctypes.data, arg["ctl"],
                                                        None if ns_a is None else ns_a.ctypes.data, arg["out"],
                                                        self.stride if stride is None else stride, arg["len"])
        # (the control arrays may go now: the library has copied them)
        if rows_a is not None:
            rows_a[...] = -1
        ctl_a[...] = 0xFF
        if ns_a is not None:
            ns_a[...] = -1
        return rc, out, lens

    def sync(self):
        return self.L.mp3mi_batch_sync(self.b)

    def wait(self, k=0):
        return self.L.mp3mi_batch_host_wait(self.b, k)

    def frames(self):
        f = np.zeros(self.S, np.int64)
        n = self.L.mp3mi_batch_slot_frames(self.b, f.ctypes.data)
        assert n == int((f >= 0).sum())
        return list(f)

    def status(self):
        st = np.zeros(self.S, np.int32)
        assert self.L.mp3mi_batch_stream_status(self.b, st.ctypes.data) >= 0
        return st

    def stats(self):
        st = IoStats()
        assert self.L.mp3mi_batch_host_io_stats(self.b, ctypes.byref(st)) == 0
        return st

    def close(self):
        if self.own and self.b:
            self.L.mp3mi_batch_destroy(self.b)
            self.b = ctypes.c_void_p()
        for p in self.raw:
            self.L.mp3mi_host_free(p)
        self.raw, self.keep = [], []


# ---- schedules: a stream is (slot, first tick, samples per channel); it takes ceil(samples / tick) ticks (at least one) ----

def lifecycle_streams(nf):
    """six slots, eight streams of different lengths ending on partial frames (one on a full tick, one of a single sample);
    slots 0 and 2 are reused; at most four rows per tick, the row set changes from tick to tick"""
    full = nf * 1152
    return [(0, 0, 3 * full + 1000), (2, 0, full + 7), (3, 0, 500), (5, 1, 2 * full + 1151), (2, 2, 2 * full), (1, 3, full + 1153),
            (4, 4, 2 * full - 5), (0, 4, 1)]


def plan_ticks(streams, nf):
    """per tick the rows [(slot, stream index, ctl, samples, first sample)], by slot"""
    full = nf * 1152
    ticks = {}
    for j, (slot, t0, n) in enumerate(streams):
        T = max(1, -(-n // full))
        for k in range(T):
            last = k == T - 1
            ticks.setdefault(t0 + k, []).append((slot, j, (START if k == 0 else 0) | (END if last else 0), n - k * full if last else full, k * full))
    out = [sorted(ticks.get(t, [])) for t in range(max(ticks) + 1)]
    for rows in out:
        assert len(set(r[0] for r in rows)) == len(rows), "two streams in one slot"
    return out


def tick_rows(plan_t, pcms, ch, row):
    pcm = np.zeros((len(plan_t), row), np.int16)
    for r, (_, j, _, n, a) in enumerate(plan_t):
        pcm[r, :n * ch] = pcms[j][a * ch:(a + n) * ch]
    return [p[0] for p in plan_t], pcm, [p[2] for p in plan_t], [p[3] for p in plan_t]


def run_host(run, streams, pcms, sync_each=True, wait_prev=False):
    """The schedule through the host call.  Returns (per stream its bytes, per tick {slot: bytes}).  sync_each: a sync after
    every tick; wait_prev: no sync, tick t is collected with host_wait(1) after tick t + 1 has been issued."""
    plan = plan_ticks(streams, run.nf)
    got, per_tick, res, open_ = [b""] * len(streams), [], [], [-1] * run.S

    def collect(t):
        _, out, lens = res[t]
        d = {}
        for r, (slot, j, _, _, _) in enumerate(plan[t]):
            d[slot] = out[r, :lens[r]].tobytes()
            assert not out[r, lens[r]:].any(), "tick %d row %d: bytes behind the length" % (t, r)
            got[j] += d[slot]
        per_tick.append(d)

    for t, p in enumerate(plan):
        assert p, "a tick without a row"
        rows, pcm, ctl, ns = tick_rows(p, pcms, run.ch, run.row)
        res.append(run.tick(rows, pcm, ctl, ns))
        assert res[t][0] == 0, "tick %d: %d" % (t, res[t][0])
        for slot, _, c, n, _ in p:
            open_[slot] = -1 if c & END else (0 if c & START else open_[slot]) + run.nf
        assert run.frames() == open_, (t, run.frames(), open_)
        if sync_each:
            assert run.sync() == 0
            collect(t)
        elif wait_prev and t >= 1:
            assert run.wait(1) == 0
            collect(t - 1)
    if not sync_each:
        if wait_prev:
            assert run.wait(0) == 0
            collect(len(plan) - 1)
            assert run.sync() == 0
        else:
            assert run.sync() == 0
            for t in range(len(plan)):
                collect(t)
    assert not run.status().any(), run.status()  # no stream left out of the comparison
    return got, per_tick


def run_device(mp, S, rate, ch, kbps, nf, streams, pcms, mode=None, crc=False):
    """the same schedule through mp3mi_batch_encode_slots (rows per slot in device memory)"""
    run = SlotRun(mp, S, rate, ch, kbps, nf, mode=mode, crc=crc)
    try:
        plan = plan_ticks(streams, nf)
        got, per_tick = [b""] * len(streams), []
        for t, p in enumerate(plan):
            pcm, ctl, ns = np.zeros((S, run.row), np.int16), np.zeros(S, np.uint8), np.zeros(S, np.int32)
            for slot, j, c, n, a in p:
                pcm[slot, :n * ch] = pcms[j][a * ch:(a + n) * ch]
                ctl[slot], ns[slot] = c, n
            assert run.call(pcm, ctl, ns) == 0 and run.L.mp3mi_batch_sync(run.b) == 0
            outs, lens = run.outputs()
            named = {slot: j for slot, j, _, _, _ in p}
            for s in range(S):
                if s not in named:
                    assert lens[s] == 0
            per_tick.append({slot: outs[slot] for slot in named})
            for slot, j in named.items():
                got[j] += outs[slot]
        assert not run.status().any()
        return got, per_tick
    finally:
        run.close()


def stream_pcms(mp, streams, ch, rate, seed0):
    return [mp.synth(max(n, 1), ch, rate, seed0 + j) for j, (_, _, n) in enumerate(streams)]


def check_oracle(oracle, streams, pcms, got, rate, kbps_of_slot, ch, mode=None):
    for j, (slot, _, n) in enumerate(streams):
        ref = oracle.encode(pcms[j][:n * ch], rate, kbps_of_slot[slot], ch, mode=mode)[0]
        assert got[j] == ref, "stream %d (slot %d, %d samples): %d bytes vs the oracle's %d" % (j, slot, n, len(got[j]), len(ref))


def lifecycles(mp, oracle, rate, ch, kbps, pinned=False, device_too=False):
    S, nf = 6, 2
    streams = lifecycle_streams(nf)
    assert max(len(p) for p in plan_ticks(streams, nf)) == 4 and len(set(tuple(r[0] for r in p) for p in plan_ticks(streams, nf))) >= 5
    pcms = stream_pcms(mp, streams, ch, rate, 300)
    run = HostRun(mp, S, rate, ch, kbps, nf, pinned=pinned)
    try:
        got, per_tick = run_host(run, streams, pcms)
        check_oracle(oracle, streams, pcms, got, rate, run.kbps, ch)
        assert run.frames() == [-1] * S
    finally:
        run.close()
    if device_too:
        dgot, dper = run_device(mp, S, rate, ch, kbps, nf, streams, pcms)
        assert dper == per_tick and dgot == got


# ------------------------------------------------------------------------------------------------------------------- emulator

def test_staggered_lifecycles_through_rows_emulated(emu, oracle):
    """case 1: every stream's concatenated bytes are the oracle's file of its samples"""
    lifecycles(emu, oracle, 44100, 2, 128)


def test_rows_equal_device_slots_emulated(emu, oracle):
    """case 2: the schedule through mp3mi_batch_encode_slots gives the same bytes per tick and per slot (mixed bitrates)"""
    lifecycles(emu, oracle, 48000, 2, [64, 128, 320, 96, 192, 56], device_too=True)


def test_null_map_equals_identity_map_emulated(emu, oracle):
    """case 3: row_slot_host == NULL is the identity map over all slots"""
    S, nf, rate, ch, kbps = 3, 2, 44100, 2, 128
    full = nf * 1152
    src = [emu.synth(3 * full, ch, rate, 320 + s) for s in range(S)]
    a, b = HostRun(emu, S, rate, ch, kbps, nf), HostRun(emu, S, rate, ch, kbps, nf)
    try:
        acc = [b""] * S
        for t, (ctl, ns) in enumerate((([START] * 3, [full] * 3), ([0, END, 0], [full, 1000, full]), ([END, START | END, END], [full, 77, 0]))):
            pcm = np.zeros((S, a.row), np.int16)
            for s in range(S):
                off = 0 if (ctl[s] & START and t > 0) else t * full
                pcm[s, :ns[s] * ch] = src[s][off * ch:(off + ns[s]) * ch]
            ra, rb = a.tick(None, pcm, ctl, ns), b.tick([0, 1, 2], pcm, ctl, ns)
            assert ra[0] == 0 and rb[0] == 0 and a.sync() == 0 and b.sync() == 0
            assert list(ra[2]) == list(rb[2]) and a.frames() == b.frames()
            for s in range(S):
                assert ra[1][s, :ra[2][s]].tobytes() == rb[1][s, :rb[2][s]].tobytes(), (t, s)
                acc[s] += ra[1][s, :ra[2][s]].tobytes()
            if t == 1:
                assert acc[1] == oracle.encode(src[1][:(full + 1000) * ch], rate, kbps, ch)[0]
                acc[1] = b""
        assert acc[0] == oracle.encode(src[0][:3 * full * ch], rate, kbps, ch)[0]
        assert acc[1] == oracle.encode(src[1][:77 * ch], rate, kbps, ch)[0]
        assert acc[2] == oracle.encode(src[2][:2 * full * ch], rate, kbps, ch)[0]
        assert not a.status().any() and not b.status().any()
        # n_rows must be n_streams without a map
        assert a.tick(None, np.zeros((2, a.row), np.int16), [START, START])[0] == -1
    finally:
        a.close()
        b.close()


def three_ticks_then_waits(mp, oracle, S, nf, rate, ch, kbps, pinned):
    """case 4: three ticks without a wait -- the even slots START, then go on while the odd slots run one-call files, then END;
    the third call blocks on the first (two calls in flight), so tick 0 is there when it returns; host_wait(1) delivers tick 1
    and host_wait(0) tick 2"""
    full = nf * 1152
    even, every = list(range(0, S, 2)), list(range(S))
    src = {s: mp.synth(3 * full, ch, rate, 340 + s % 50) for s in range(S)}
    run = HostRun(mp, S, rate, ch, kbps, nf, pinned=pinned)
    try:
        assert run.wait(0) == -1 and run.wait(1) == -1  # no such call yet
        res = []
        for t, rows in enumerate((even, every, even)):
            ctl = [(START, 0, END)[t] if s % 2 == 0 else START | END for s in rows]
            ns = [(full, full, full - 3)[t] if s % 2 == 0 else 1500 for s in rows]
            pcm = np.zeros((len(rows), run.row), np.int16)
            for r, s in enumerate(rows):
                off = t * full if s % 2 == 0 else 0
                pcm[r, :ns[r] * ch] = src[s][off * ch:(off + ns[r]) * ch]
            res.append(run.tick(rows, pcm, ctl, ns))
            assert res[t][0] == 0
            if t == 0:
                assert run.wait(1) == -1  # one call so far
        assert run.wait(2) == -1 and run.wait(-1) == -1
        pick = sorted(set(np.linspace(0, len(even) - 1, 4).astype(int).tolist()))
        data = lambda t, r: res[t][1][r, :res[t][2][r]].tobytes()
        assert all(res[0][2] < run.stride)  # tick 0 is there: the third call waited for it
        first = {r: data(0, r) for r in pick}
        assert run.wait(1) == 0
        assert all(res[1][2] < run.stride)
        for r in pick:
            s = even[r] + 1
            if s < S:
                assert data(1, s) == oracle.encode(src[s][:1500 * ch], rate, run.kbps[s], ch)[0], s
        second = {r: data(1, even[r]) for r in pick}
        assert run.wait(0) == 0
        for r in pick:
            s = even[r]
            assert first[r] + second[r] + data(2, r) == oracle.encode(src[s][:(3 * full - 3) * ch], rate, run.kbps[s], ch)[0], s
        assert run.wait(0) == 0 and run.wait(1) == 0  # waiting again is harmless
        assert run.sync() == 0 and not run.status().any()
        assert run.frames() == [-1] * S
    finally:
        run.close()


def test_three_ticks_then_host_wait_emulated(emu, oracle):
    three_ticks_then_waits(emu, oracle, 4, 2, 44100, 2, 128, pinned=False)


def test_argument_errors_emulated(emu, oracle):
    """case 5: every broken rule returns MP3MI_ERR_ARG and leaves slot_frames and the next call's bytes unchanged"""
    S, nf, rate, ch, kbps = 4, 2, 44100, 2, 128
    full = nf * 1152
    run = HostRun(emu, S, rate, ch, kbps, nf)
    try:
        src = [emu.synth(2 * full, ch, rate, 360 + s) for s in range(S)]
        rc, out0, len0 = run.tick([0, 2], np.stack([src[0][:full * ch], src[2][:full * ch]]), [START, START])
        assert rc == 0 and run.sync() == 0
        before = run.frames()
        assert before == [2, -1, 2, -1]
        z = lambda n: np.zeros((n, run.row), np.int16)
        bad = [
            dict(rows=[0], pcm=z(1), ctl=[0]),                               # open slot 2 without a row
            dict(rows=[0, 1, 2], pcm=z(3), ctl=[0, 0, 0]),                   # a row that is neither open nor starting
            dict(rows=[0, 1, 2], pcm=z(3), ctl=[0, END, 0], ns=[full, 0, full]),
            dict(rows=[2, 0], pcm=z(2), ctl=[0, 0]),                         # out of order
            dict(rows=[0, 0, 2], pcm=z(3), ctl=[0, 0, 0]),                   # a slot twice
            dict(rows=[0, 2, 4], pcm=z(3), ctl=[0, 0, START]),               # out of range
            dict(rows=[-1, 0, 2], pcm=z(3), ctl=[START, 0, 0]),
            dict(rows=[0, 2], pcm=z(2), ctl=[0, 0], n_rows=0),
            dict(rows=[0, 1, 2, 3, 3], pcm=z(5), ctl=[0, START, 0, START, START]),  # more rows than slots
            dict(rows=None, pcm=z(2), ctl=[0, 0]),                           # no map: n_rows must be n_streams
            dict(rows=[0, 2], pcm=z(2), ctl=[4, 0]),                         # the per-slot call's own rules, by row
            dict(rows=[0, 2], pcm=z(2), ctl=[0, 0], ns=[full - 1, full]),
            dict(rows=[0, 2], pcm=z(2), ctl=[END, 0], ns=[full + 1, full]),
            dict(rows=[0, 2], pcm=z(2), ctl=[END, 0], ns=[-1, full]),
            dict(rows=[0, 2, 3], pcm=z(3), ctl=[0, 0, START], ns=[full, full, 7]),
            dict(rows=[0, 2], pcm=z(2), ctl=[0, 0], nf=0),
            dict(rows=[0, 2], pcm=z(2), ctl=[0, 0], nf=nf + 1),
            dict(rows=[0, 2], pcm=z(2), ctl=[0, 0], stride=run.stride - 1),  # below mp3mi_batch_out_stride(b, n_frames)
            dict(rows=[0, 2], pcm=z(2), ctl=[0, 0], null=("pcm",)),
            dict(rows=[0, 2], pcm=z(2), ctl=[0, 0], null=("ctl",)),
            dict(rows=[0, 2], pcm=z(2), ctl=[0, 0], null=("out",)),
            dict(rows=[0, 2], pcm=z(2), ctl=[0, 0], null=("len",)),
        ]
        for kw in bad:
            assert run.tick(**kw)[0] == -1, {k: v for k, v in kw.items() if k != "pcm"}
            assert run.frames() == before, kw
        assert run.L.mp3mi_batch_encode_slots_host_async(None, 1, nf, 1, None, 1, None, 1, run.stride, 1) == -1
        assert run.L.mp3mi_batch_host_wait(None, 0) == -1
        st = run.stats()
        assert st.calls == 1  # the refused calls moved nothing
        # valid: slot 0 ENDs on 100 samples, slot 2 goes on, slot 3 is a one-call file
        pcm = z(3)
        pcm[0, :100 * ch] = src[0][full * ch:(full + 100) * ch]
        pcm[1] = src[2][full * ch:]
        pcm[2, :2000 * ch] = src[3][:2000 * ch]
        rc, out1, len1 = run.tick([0, 2, 3], pcm, [END, 0, START | END], [100, full, 2000])
        assert rc == 0 and run.sync() == 0
        assert out0[0, :len0[0]].tobytes() + out1[0, :len1[0]].tobytes() == oracle.encode(src[0][:(full + 100) * ch], rate, kbps, ch)[0]
        assert out1[2, :len1[2]].tobytes() == oracle.encode(src[3][:2000 * ch], rate, kbps, ch)[0]
        assert run.frames() == [-1, -1, 4, -1]
        rc, out2, len2 = run.tick([2], z(1), [END], [0])
        assert rc == 0 and run.sync() == 0
        assert b"".join(o[r, :n[r]].tobytes() for o, n, r in ((out0, len0, 1), (out1, len1, 1), (out2, len2, 0))) == oracle.encode(src[2], rate, kbps, ch)[0]
        assert not run.status().any()
    finally:
        run.close()


def test_host_io_stats_count_live_rows_only_emulated(emu, monkeypatch):
    """case 6: h2d_bytes grows by exactly n_rows * n_frames * 1152 * channels * 2 per call -- only the live rows crossed --
    with a short call (n_frames < max_frames) and several chunks per call too; calls are counted"""
    S, nf, rate, ch, kbps = 5, 4, 32000, 1, 64
    monkeypatch.setenv("MP3MI_CHUNK_FRAMES", "2")
    run = HostRun(emu, S, rate, ch, kbps, nf)
    try:
        full = nf * 1152
        up = 0
        for t, (rows, ctl, n_frames) in enumerate((([1, 3, 4], [START] * 3, 4), ([1, 3, 4], [0, END, 0], 3), ([0, 1, 4], [START, END, 0], 4),
                                                  ([0, 4], [END, END], 1))):
            run.nf, run.row = n_frames, n_frames * 1152 * ch  # (a call of fewer frames than the batch holds: its own row pitch)
            rc, _, _ = run.tick(rows, np.zeros((len(rows), run.row), np.int16), ctl)
            assert rc == 0
            up += len(rows) * n_frames * 1152 * ch * 2
            st = run.stats()
            assert st.calls == t + 1 and st.h2d_bytes == up, (t, st.calls, st.h2d_bytes, up)
            assert st.d2h_bytes == sum(len(r) for r in ([1, 3, 4], [1, 3, 4], [0, 1, 4], [0, 4])[:t + 1]) * run.stride
        assert run.sync() == 0 and run.frames() == [-1] * S
    finally:
        run.close()


def test_host_and_device_slot_calls_alternate_emulated(emu, oracle):
    """case 7: one batch, the ticks alternately through the host call (rows) and the device call (slots)"""
    S, nf, rate, ch, kbps = 4, 2, 44100, 2, 128
    streams = [(1, 0, 4 * nf * 1152 + 300), (3, 1, 2 * nf * 1152 - 1), (0, 2, 700), (3, 3, nf * 1152 + 5)]
    pcms = stream_pcms(emu, streams, ch, rate, 380)
    plan = plan_ticks(streams, nf)
    dev = SlotRun(emu, S, rate, ch, kbps, nf)
    host = HostRun(emu, S, rate, ch, kbps, nf, b=dev.b)
    try:
        got = [b""] * len(streams)
        for t, p in enumerate(plan):
            if t % 2 == 0:
                rows, pcm, ctl, ns = tick_rows(p, pcms, ch, host.row)
                rc, out, lens = host.tick(rows, pcm, ctl, ns)
                assert rc == 0 and host.sync() == 0
                for r, (_, j, _, _, _) in enumerate(p):
                    got[j] += out[r, :lens[r]].tobytes()
            else:
                pcm, ctl, ns = np.zeros((S, dev.row), np.int16), np.zeros(S, np.uint8), np.zeros(S, np.int32)
                for slot, j, c, n, a in p:
                    pcm[slot, :n * ch] = pcms[j][a * ch:(a + n) * ch]
                    ctl[slot], ns[slot] = c, n
                assert dev.call(pcm, ctl, ns) == 0 and host.sync() == 0
                outs, lens = dev.outputs()
                for slot, j, _, _, _ in p:
                    got[j] += outs[slot]
                assert sum(lens) == sum(len(outs[slot]) for slot, _, _, _, _ in p)
            assert host.frames() == list(dev.frames())
        check_oracle(oracle, streams, pcms, got, rate, host.kbps, ch)
        assert not host.status().any()
    finally:
        host.close()
        dev.close()


def test_python_binding_emulated(emu, oracle, monkeypatch):
    """Batch.encode_slots_host / Batch.host_wait on numpy arrays (the binding loaded over the emulated build)"""
    import importlib
    from mp3common import EMU_SO
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    monkeypatch.setattr(mp3, "LIB_PATH", EMU_SO)
    monkeypatch.setattr(mp3, "_lib", None)
    S, nf, rate, ch, kbps = 3, 2, 44100, 2, 128
    full = nf * 1152
    src = emu.synth(full + 900, ch, rate, 395)
    b = mp3.Batch(S, rate, ch, kbps, nf)
    try:
        stride = b.out_stride(nf)
        pcm = np.zeros((1, full * ch), np.int16)
        pcm[0] = src[:full * ch]
        out0, len0 = np.zeros((1, stride), np.uint8), np.zeros(1, np.uint32)
        b.encode_slots_host(pcm, nf, out0, len0, rows=[2], start=[True])
        b.host_wait()
        assert list(b.slot_frames()) == [-1, -1, 2]
        pcm1 = np.zeros((1, full * ch), np.int16)
        pcm1[0, :900 * ch] = src[full * ch:]
        out1, len1 = np.zeros((1, stride), np.uint8), np.zeros(1, np.uint32)
        b.encode_slots_host(pcm1, nf, out1, len1, rows=[2], end=[True], n_samples=[900])
        b.host_wait(0)
        b.host_wait(1)
        assert out0[0, :len0[0]].tobytes() + out1[0, :len1[0]].tobytes() == oracle.encode(src, rate, kbps, ch)[0]
        with pytest.raises(mp3.Mp3miError):
            b.encode_slots_host(pcm1, nf, out1, len1, rows=[2])  # the slot is closed
        b.sync()
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------------- device

@pytest.mark.gpu
@pytest.mark.parametrize("rate,ch,kbps,chunk", [(44100, 2, 128, None), (48000, 2, 192, 1), (32000, 1, 56, 1), (44100, 1, 320, 1)])
def test_staggered_lifecycles_through_rows_gpu(product, oracle, monkeypatch, rate, ch, kbps, chunk):
    if chunk:
        monkeypatch.setenv("MP3MI_CHUNK_FRAMES", str(chunk))  # a chunk's columns of the rows at a time
    lifecycles(product, oracle, rate, ch, kbps, pinned=True, device_too=True)


def churn_streams(S, n_ticks, nf, seed, p_start=0.4):
    """a seeded server loop at about half occupancy: a closed slot STARTs with probability p_start, a stream lasts one or two
    ticks and ends at a random length (out of a pool of 24 lengths, 1 and a full tick among them, so that the oracle's files
    of all streams are few enough to compute)"""
    rng = np.random.default_rng(seed)
    full = nf * 1152
    pool = np.concatenate([[1, full, 1152, 1153], rng.integers(1, full + 1, 20)])
    free_at = np.zeros(S, np.int64)
    streams = []
    for t in range(n_ticks):
        for s in np.flatnonzero((free_at <= t) & (rng.random(S) < p_start)):
            T = int(rng.integers(1, 3))
            if t + T > n_ticks:
                T = n_ticks - t
            n = (T - 1) * full + int(pool[rng.integers(0, len(pool))])
            streams.append((int(s), t, n))
            free_at[s] = t + T
    return streams


def test_churn_schedule_reuses_every_slot():
    streams = churn_streams(4096, 24, 2, 20261016)
    per_slot = np.bincount([s for s, _, _ in streams], minlength=4096)
    assert per_slot.min() >= 2, per_slot.min()
    rows = [len(p) for p in plan_ticks(streams, 2)]
    assert len(rows) == 24 and all(0.4 * 4096 < r < 0.6 * 4096 for r in rows[1:]), rows


@pytest.mark.gpu
def test_full_chip_churn_through_rows_gpu(product, oracle):
    """4096 slots at about half occupancy over 24 ticks of 2 frames, every slot reused, page-locked buffers, ticks collected
    with host_wait(1) behind the next tick's issue: EVERY stream equals the oracle's file of its samples; only the live rows
    crossed"""
    S, rate, ch, kbps, nf, n_ticks = 4096, 44100, 2, 128, 2, 24
    streams = churn_streams(S, n_ticks, nf, 20261016)
    assert np.bincount([s for s, _, _ in streams], minlength=S).min() >= 2
    # PCM: stream j reads source j % 8 from sample 0 (8 sources x 48 lengths: the oracle encodes every distinct file once)
    full = nf * 1152
    srcs = [product.synth(2 * full, ch, rate, 400 + k) for k in range(8)]
    pcms = [srcs[j % 8] for j in range(len(streams))]
    run = HostRun(product, S, rate, ch, kbps, nf, pinned=True)
    try:
        got, _ = run_host(run, streams, pcms, sync_each=False, wait_prev=True)
        st = run.stats()
        n_rows = sum(len(p) for p in plan_ticks(streams, nf))
        assert st.calls == n_ticks and st.h2d_bytes == n_rows * full * ch * 2, (st.calls, st.h2d_bytes)
    finally:
        run.close()
    refs = {}
    bad = []
    for j, (slot, _, n) in enumerate(streams):
        key = (j % 8, n)
        if key not in refs:
            refs[key] = oracle.encode(pcms[j][:n * ch], rate, kbps, ch)[0]
        if got[j] != refs[key]:
            bad.append(j)
    assert not bad, "%d of %d streams differ from the oracle (first: stream %d, slot %d, %d samples)" % (
        len(bad), len(streams), bad[0], streams[bad[0]][0], streams[bad[0]][2])


@pytest.mark.gpu
def test_back_to_back_ticks_without_sync_gpu(product, monkeypatch):
    """a churn schedule from page-locked buffers issued without any wait between the ticks (call hold on, a different row map
    and control block each tick) gives the bytes of the run that syncs after every tick"""
    monkeypatch.setenv("MP3MI_CALL_HOLD", "1")
    S, rate, ch, kbps, nf, n_ticks = 1024, 44100, 2, 128, 8, 10
    streams = churn_streams(S, n_ticks, nf, 7)
    full = nf * 1152
    srcs = [product.synth(2 * full, ch, rate, 500 + k) for k in range(16)]
    pcms = [srcs[j % 16] for j in range(len(streams))]
    res = []
    for sync_each in (True, False):
        run = HostRun(product, S, rate, ch, kbps, nf, pinned=True)
        try:
            res.append(run_host(run, streams, pcms, sync_each=sync_each))
        finally:
            run.close()
    assert res[0][1] == res[1][1], "per-tick bytes differ"
    assert res[0][0] == res[1][0]
    assert all(len(x) > 0 for x in res[0][0])


@pytest.mark.gpu
def test_three_ticks_then_host_wait_gpu(product, oracle):
    three_ticks_then_waits(product, oracle, 1024, 8, 44100, 2, 128, pinned=True)


@pytest.mark.gpu
def test_aborting_stream_in_a_row_gpu(product, oracle):
    """an input the reference dies on (tests/abort_cases.py's abort_global_gain) travels in one row: its neighbours' bytes are
    the oracle's, its own file is voided, the sync reports the abort once and stream_status finds it in its slot"""
    case = [c for c in aborting_cases() if c["name"] == "abort_global_gain"][0]
    bad = case_pcm(case, product.synth)  # 6 frames: the reference dies in frame 4
    with pytest.raises(ReferenceAborts):
        oracle.encode(bad, 44100, 128, 2)
    S, nf, rate, ch, kbps = 8, 2, 44100, 2, 128
    n_bad = len(bad) // ch
    good = [product.synth(n_bad, ch, rate, 600 + k) for k in range(2)]
    streams = [(1, 0, n_bad), (4, 0, n_bad), (6, 0, n_bad)]
    pcms = [good[0], bad, good[1]]
    plan = plan_ticks(streams, nf)
    run = HostRun(product, S, rate, ch, kbps, nf, pinned=True)
    try:
        got, rcs = [b""] * 3, []
        for p in plan:
            rows, pcm, ctl, ns = tick_rows(p, pcms, ch, run.row)
            rc, out, lens = run.tick(rows, pcm, ctl, ns)
            assert rc == 0
            rcs.append(run.sync())
            for r, (_, j, _, _, _) in enumerate(p):
                got[j] += out[r, :lens[r]].tobytes()
        assert rcs.count(ERR_REFERENCE_ABORT) == 1 and set(rcs) == {0, ERR_REFERENCE_ABORT}, rcs
        assert run.sync() == 0
        st = run.status()
        assert (st[4] & 255) == case["reference_aborts"]["status"] and (st[4] >> 8) == case["reference_aborts"]["frame"], st
        assert not np.delete(st, 4).any(), st
        assert got[0] == oracle.encode(good[0], rate, kbps, ch)[0] and got[2] == oracle.encode(good[1], rate, kbps, ch)[0]
    finally:
        run.close()
