"""A bitrate per stream at START, and park / resume, for Layers I and II on the emulated build (include/mp3mi_l12.h:
mp3mi_l12_batch_encode_slots_kbps, _slot_kbps, _slot_state_bytes, _slots_export, _slots_import).  The judge is byte equality: what a
stream delivers from START through END, over every slot and batch it lived in, is the CPU oracle's file of its samples at its bitrate
and the library's own ragged whole-file call's.  Helpers and the scenarios shared with the GPU tests: tests/l12_park.py."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from l12_park import ParkRun, Ticket, aligned, case_phase, case_rates, case_snapshot, case_travel, check_streams, l12_rates
from l12_slots import START
from mp3common import ROOT, DevMem
from test_kernel_budgets import HIPCC, resources, the


@pytest.mark.parametrize("layer,k", [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2)])
def test_park_and_resume_at_every_phase(emu, oracle, layer, k):
    """Layer I: a frame is 12 filterbank slots against granules of 18 -- three phases; Layer II: the two warm-up passes"""
    case_phase(emu, oracle, layer, k)


@pytest.mark.parametrize("layer", [1, 2])
def test_snapshot_imported_twice(emu, oracle, layer):
    case_snapshot(emu, oracle, layer)


@pytest.mark.parametrize("layer", [1, 2])
def test_import_first_after_flush_and_after_reset(emu, oracle, layer):
    """the same two snapshots resumed on a batch nothing has run on (the history buffers do not exist yet), on their own batch behind
    the flush that ended the originals, and behind a reset that abandoned other streams"""
    pool = DevMem(emu)
    a = ParkRun(emu, layer, 3, 44100, "s", l12_rates(layer, 3), 2, pool=pool)
    b = ParkRun(emu, layer, 4, 44100, "s", [64, 64, 64, 448 if layer == 1 else 384], 1, pool=pool)
    try:
        spf, done = a.spf, []
        done += a.step(2, starts={s: a.stream(100 + s, 9 * spf, slot=s) for s in (0, 1)})
        done += a.step(1)
        snap = a.export([0, 1], close=False)
        first = b.import_([3, 0], snap)  # the first call b sees
        done += b.step(1)
        done += b.step(1, ends={3: 11, 0: 0}, starts={1: b.stream(110, 2 * spf, slot=1)})
        done += b.step(1, ends={1: spf})
        done += a.flush_all()  # the originals end where the snapshots were taken
        assert len(done) == 5
        after_flush = a.import_([1, 2], snap)
        done += a.step(2, starts={0: a.stream(120, 5 * spf, slot=0, noise=True)})
        a.reset()  # abandons all three
        after_reset = a.import_([2, 0], snap)
        done += a.step(1)
        done += a.step(2, ends={2: spf + 1, 0: 2 * spf})
        assert all(st in done for st in first + after_reset) and not any(st in done for st in after_flush)
        check_streams(a, oracle, done, 7)
    finally:
        a.close()
        b.close()
        pool.free()


@pytest.mark.parametrize("layer", [1, 2])
def test_whole_batch_path_on_either_side(emu, oracle, layer):
    """streams that encode_next began are exported while the whole-batch counter is in force -- a snapshot of all of them, then one
    that leaves --, and a fresh batch that imports every slot at one frame count hands over to the whole-batch path: encode_next
    continues them and the flush ends them"""
    pool = DevMem(emu)
    S = 3
    a = ParkRun(emu, layer, S, 44100, "j", l12_rates(layer, S), 2, pool=pool)
    b = ParkRun(emu, layer, S, 44100, "j", 448 if layer == 1 else 384, 2, pool=pool)
    try:
        spf, done = a.spf, []
        done += a.next(2, starts=[a.stream(130 + s, 10 * spf, slot=s) for s in range(S)])
        done += a.next(1)
        moved = b.import_([2, 0, 1], a.export([0, 1, 2], close=False))
        done += b.next(2)
        done += b.next(1)
        done += b.flush_all()
        assert len(done) == S and all(st in done for st in moved)
        # one leaves a for a call and comes back: a call behind its neighbours from here on
        pk = a.export([1])
        done += a.next(2)
        back = a.import_([1], pk)
        done += a.next(1)
        done += a.step(2, ends={0: 5, 1: 2 * spf, 2: 0})
        assert back[0] in done
        check_streams(a, oracle, done, 2 * S)
    finally:
        a.close()
        b.close()
        pool.free()


@pytest.mark.parametrize("layer,nf", [(2, 7), (1, 17)])
def test_several_chunks_per_call(emu, oracle, layer, nf):
    """1 MiB of scratch: a call is two chunks (tests/test_l12_slots.py); a stream leaves between two such calls and comes back"""
    run = ParkRun(emu, layer, 3, 44100, "j", 192 if layer == 1 else 128, nf, scratch_mb=1)
    try:
        spf, done = run.spf, []
        done += run.step(nf, starts={s: run.stream(140 + s, 3 * nf * spf) for s in (0, 1)})
        pk = run.export([1])
        done += run.step(nf, starts={1: run.stream(150, nf * spf, noise=True)}, ends={1: nf * spf - 5})
        back = run.import_([2], pk)
        done += run.step(nf, ends={0: 3 * spf + 17, 2: nf * spf})
        assert run.launches() == [3 * 2] * 4 and back[0] in done
        check_streams(run, oracle, done, 3)
    finally:
        run.close()


@pytest.mark.parametrize("rate,mode,rates", [(44100, "s", [64, 128, 192]), (32000, "m", [48, 64, 96])])
def test_bitrate_at_start_crosses_the_layer_2_tables(emu, oracle, rate, mode, rates):
    """44.1 kHz stereo: 64 kbps selects allocation table 2, 128 table 0, 192 table 1; 32 kHz mono: 48 table 3, 64 table 0, 96 table 1
    (src/common.c:291-318) -- in a batch created at 384 kbps (table 1 / table 0 at 48 kHz only: here table 1)"""
    case_rates(emu, oracle, 2, rate, mode, 384, rates)


def test_bitrate_at_start_layer_1(emu, oracle):
    """two channels, created at 448 kbps: 32 kbps, whose frames outgrow their slots (rows of 38 bytes), and 448"""
    case_rates(emu, oracle, 1, 44100, "s", 448, [32, 448])


def test_bitrate_bookkeeping_and_restore(emu, oracle):
    """kbps 0 is the create-time bitrate; one persistent array serves call after call; the bitrate survives encode_next and ends with
    the flush; a START without a bitrate array in a slot that last ran another bitrate encodes at the create-time one (a stale
    device cfg would show here); the whole-file call and an encode_next that starts every slot, after mixed bitrates, give the
    create-time files"""
    S = 3
    run = ParkRun(emu, 2, S, 44100, "s", [128, 160, 384], 2)
    try:
        spf, done = run.spf, []
        sig = lambda seed, n, **kw: run.stream(seed, n * spf, **kw)
        done += run.step(1, starts={0: sig(160, 6, slot=0)}, kbps="zero")
        done += run.step(2, starts={1: sig(161, 6, kbps=64), 2: sig(162, 6, kbps=96)})
        assert run.slot_kbps() == [128, 64, 96]
        done += run.step(1, kbps="all")
        done += run.next(1)
        done += run.flush_all()
        assert len(done) == 3 and run.slot_kbps() == [128, 160, 384]
        done += run.step(1, starts={1: sig(163, 3, slot=1), 2: sig(164, 3, slot=2)}, kbps=None)
        done += run.step(2, starts={0: sig(165, 2, kbps=48)}, ends={0: spf + 3, 1: 2 * spf, 2: 9}, kbps="all")
        done += run.step(1, starts={0: sig(166, 1, slot=0)}, ends={0: 400}, kbps=None)  # END at 48, then START with no array: 128
        done += run.step(2, starts={s: sig(167 + s, 2, kbps=[56, 80, 112][s]) for s in range(S)}, ends={s: spf for s in range(S)})
        assert len(done) == 10
        done += run.whole_file([sig(170 + s, 2, slot=s) for s in range(S)])
        done += run.step(1, starts={1: sig(175, 1, kbps=32)}, ends={1: 30})
        done += run.next(2, starts=[sig(176 + s, 3, slot=s) for s in range(S)])
        done += run.next(1)
        done += run.flush_all()
        assert [st.kbps for st in done[-3:]] == [128, 160, 384]
        check_streams(run, oracle, done, 17)
    finally:
        run.close()


def test_the_bitrate_travels(emu, oracle):
    case_travel(emu, oracle)


def test_refusals(emu, oracle):
    """every rule of the three calls, one broken per call: MP3MI_ERR_ARG and the batch as it was; afterwards a valid continuation
    gives the oracle's bytes"""
    S = 3
    run = ParkRun(emu, 2, S, 44100, "s", [128, 128, 192], 2)
    one = ParkRun(emu, 1, 2, 44100, "s", 448, 2)
    try:
        spf, done, L = run.spf, [], run.L
        done += run.step(2, starts={0: run.stream(180, 8 * spf, kbps=96), 1: run.stream(181, 8 * spf, kbps=128)})
        done += one.step(2, starts={0: one.stream(182, 8 * one.spf)})
        snap = run.export([0], close=False)[0]
        pk1 = run.export([1])[0]
        pk_one = one.export([0])[0]
        full, B = 2 * spf, run.state_bytes
        books = (run.frames(), run.slot_kbps())  # slot 0 open at 96 kbps, slots 1 and 2 closed
        assert books == ([2, -1, -1], [96, 128, 192])
        pcm = np.zeros((S, full * run.ch), np.int16)
        run.put(pcm)
        ST = START
        for kw in [dict(ctl=[0, 0, ST], ns=[full, 0, full], kb=[0, 0, 224]),   # above the ceiling
                   dict(ctl=[0, 0, ST], ns=[full, 0, full], kb=[0, 0, 100]),   # no bitrate of the layer
                   dict(ctl=[0, 0, ST], ns=[full, 0, full], kb=[0, 0, -64]),
                   dict(ctl=[0, 0, 0], ns=[full, 0, 0], kb=[128, 0, 0]),        # not the open stream's bitrate
                   dict(ctl=[0, 0, 0], ns=[full, 0, 0], kb=[96, 128, 0]),       # a bitrate for a closed slot that does not START
                   dict(ctl=[0, 0, 4], ns=[full, 0, 0], kb=[96, 0, 0]),         # (the rules of mp3mi_l12_batch_encode_slots still hold)
                   dict(ctl=[0, 0, 0], ns=[full - 1, 0, 0], kb=[96, 0, 0])]:
            assert run.raw_step(**kw) == -1, kw
            assert (run.frames(), run.slot_kbps()) == books, kw
        one.put(np.zeros((2, 2 * one.spf * one.ch), np.int16))
        for k in (48, 56, 80, 112):  # Layer II's table, in a Layer I batch
            assert one.raw_step([0, ST], [0, 2 * one.spf], [0, k]) == -1, k
        assert one.frames() == [-1, -1]

        state = aligned(run.mem, 4 * (B + 16))
        tk = (Ticket * 4)()
        sl = lambda *s: np.array(s, np.int32).ctypes.data
        ex = lambda n, slots, p=state, stride=B, t=tk, b=run.b: L.mp3mi_l12_batch_slots_export(b, n, slots, 0, p, stride, t)
        for what, rc in [("n 0", ex(0, sl(0))), ("n above n_streams", ex(4, sl(0, 1, 2, 0))), ("slot -1", ex(1, sl(-1))),
                         ("slot n_streams", ex(1, sl(S))), ("a slot twice", ex(2, sl(0, 0))), ("a closed slot", ex(1, sl(2))),
                         ("a closed slot behind an open one", ex(2, sl(0, 1))), ("stride below state_bytes", ex(1, sl(0), stride=B - 16)),
                         ("stride no multiple of 16", ex(1, sl(0), stride=B + 8)), ("pointer no multiple of 16", ex(1, sl(0), p=state + 8)),
                         ("no state", ex(1, sl(0), p=None)), ("no tickets", ex(1, sl(0), t=None)), ("no slots", ex(1, None)),
                         ("no batch", ex(1, sl(0), b=None))]:
            assert rc == -1, what
            assert (run.frames(), run.slot_kbps()) == books, what

        def im(n, slots, tickets, p=pk1.ptr, stride=B, b=run.b):
            t = None if tickets is None else (Ticket * len(tickets))(*tickets)
            return L.mp3mi_l12_batch_slots_import(b, n, slots, p, stride, t)

        def altered(**kw):
            t = Ticket.from_buffer_copy(pk1.ticket)
            for k, v in kw.items():
                setattr(t, k, v)
            return t

        good = pk1.ticket
        cases = [("an open slot", im(1, sl(0), [good])), ("n 0", im(0, sl(1), [good])), ("a slot twice", im(2, sl(1, 1), [good, good])),
                 ("slot n_streams", im(1, sl(S), [good])), ("slot -1", im(1, sl(-1), [good])), ("stride below state_bytes", im(1, sl(1), [good], stride=B - 16)),
                 ("stride no multiple of 16", im(1, sl(1), [good], stride=B + 8)), ("pointer no multiple of 16", im(1, sl(1), [good], p=pk1.ptr + 8)),
                 ("no state", im(1, sl(1), [good], p=None)), ("no tickets", im(1, sl(1), None)), ("no slots", im(1, None, [good])),
                 ("no batch", im(1, sl(1), [good], b=None)), ("a good ticket behind a bad one", im(2, sl(1, 2), [altered(reserved=1), good])),
                 ("a Layer I ticket", im(1, sl(1), [pk_one.ticket], p=pk_one.ptr))]
        for field, v in [("magic", 0x4B54334D), ("version", 2), ("state_bytes", B + 16), ("state_bytes", B // 2), ("layer", 1), ("rate_hz", 48000),
                         ("channels", 1), ("hdr_mode", 1), ("hdr_flags", 4), ("error_protection", 1), ("reserved", 1), ("kbps", 224), ("kbps", 0),
                         ("kbps", 100), ("kbps", -128), ("frames", -1)]:
            cases.append(("ticket with %s %d" % (field, v), im(1, sl(1), [altered(**{field: v})])))
        for what, rc in cases:
            assert rc == -1, what
        assert (run.frames(), run.slot_kbps()) == books
        t48 = Ticket.from_buffer_copy(pk_one.ticket)
        t48.kbps = 48  # Layer II's table, in a Layer I ticket
        assert L.mp3mi_l12_batch_slots_import(one.b, 1, sl(1), pk_one.ptr, one.state_bytes, (Ticket * 1)(t48)) == -1
        assert L.mp3mi_l12_batch_slot_kbps(run.b, None) == -1 and L.mp3mi_l12_batch_slot_kbps(None, None) == -1
        assert L.mp3mi_l12_batch_slot_state_bytes(None) == 0

        # valid again: the parked stream into slot 2, the snapshot into slot 1, and everything to its END
        moved = run.import_([2, 1], [pk1, snap]) + one.import_([1], [pk_one])
        done += run.step(2)
        done += run.step(1, ends={0: 33, 1: 33, 2: spf})
        done += one.step(1, ends={1: 200})
        assert all(st in done for st in moved) and len(done) == 4
        check_streams(run, oracle, done[:3], 3)
        check_streams(one, oracle, done[3:], 1)
    finally:
        run.close()
        one.close()


@pytest.mark.parametrize("layer,mode", [(2, "s"), (1, "m")])
def test_records_and_the_bytes_between_them(emu, oracle, layer, mode):
    """records exported at a stride above state_bytes into a buffer of 0xA5: the bytes between them are untouched, and a record is the
    slot's history -- the last 1792 samples per channel it was fed, then the last 1056, interleaved as they came (Layer II: after one
    call of two frames; Layer I: after five of one frame, zeros before the stream's first sample)"""
    S = 3
    run = ParkRun(emu, layer, S, 44100, mode, 192 if layer == 1 else 128, 2)
    try:
        spf, ch, B = run.spf, run.ch, run.state_bytes
        src = {s: run.stream(190 + s, 6 * spf) for s in (0, 2)}
        run.step(2, starts=src)
        if layer == 1:
            for _ in range(3):
                run.step(1)
        stride = B + 48
        pk = run.export([2, 0], close=False, stride=stride, fill=0xA5)
        raw = run.pool.download(pk[0].ptr, (2, stride), np.uint8)
        assert (raw[:, B:] == 0xA5).all()
        for i, s in enumerate((2, 0)):
            fed = src[s].fed()
            rec = raw[i, :B].view(np.int16)
            for row, H in ((rec[:1792 * ch], 1792), (rec[1792 * ch:], 1056)):
                want = np.concatenate([np.zeros(max(0, H * ch - len(fed)), np.int16), fed[-H * ch:]])
                assert (row == want).all(), (s, H)
        assert len(src[0].fed()) == (2304 if layer == 2 else 5 * 384) * ch
    finally:
        run.close()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_park_kernels_need_neither_scratch_nor_lds():
    """k_l12.hip compiled for gfx950 with the compiler's resource remarks (no GPU): k12_slot_park and k12_slot_rate"""
    tmp = tempfile.mkdtemp(prefix="mp3mi_budget_l12_park_")
    try:
        kernels = resources("k_l12", tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for name in ("k12_slot_park", "k12_slot_rate"):
        k = the(kernels, r"^_Z\d+%sP" % name)
        assert k["ScratchSize"] == 0 and k["LDS"] == 0, (name, k)


def test_sanitized_park_program():
    """tests/hipemu/l12_park_main.cpp under AddressSanitizer, UndefinedBehaviorSanitizer and LeakSanitizer on the emulator: export,
    import, continue, destroy; the import-first path; one refusal per call.  Passes when the program exits 0 without a report."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "hipemu"), "-f", "l12_park.mk", "l12_park"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
