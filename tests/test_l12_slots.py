"""Continuous batching for Layers I and II (mp3mi_l12_batch_encode_slots, include/mp3mi_l12.h) on the emulated build: the bytes a
slot delivers from a stream's START call through its END call are the CPU oracle's (or a golden vector's) and the library's own
ragged whole-file call's; closed slots deliver nothing; the calls around it behave as documented.  Helpers: tests/l12_slots.py."""
import numpy as np
import pytest

import golden_l12
from l12_slots import (END, FILL, START, SlotRun, check, churn, drive, history_cleared, loud, new_state, plan_from, ragged_whole_file,
                       sources_for)
from mp3common import L12Run, l12_signal, oracle_l12


@pytest.mark.parametrize("layer", [1, 2])
def test_churn_at_the_smallest_calls(emu, oracle, layer):
    """Layer I: 8 slots, 14 calls of one frame; Layer II: 6 slots, 8 calls of one and two frames (l12_slots.L1_SCRIPTS, L2_SCRIPTS)"""
    done = churn(emu, oracle, layer, 8 if layer == 1 else 6)
    lengths = sorted(len(p) for _, p, _ in done)
    assert lengths[0] == 0 and lengths[-1] > 5 * 2 * (384 if layer == 1 else 1152)


@pytest.mark.parametrize("layer", [1, 2])
def test_history_is_cleared_at_start(emu, oracle, layer):
    history_cleared(emu, oracle, layer)


SMALL = [["S", ".", ("E", 301), ("SE", 0)], [".", "S", ".", ("E", 0)], [("SE", 250), ".", "S", ("E", 384)], [".", ("SE", 333), "S", ("E", 1)]]


@pytest.mark.parametrize("layer,rate,mode,kbps", [(2, 48000, "je", 96), (1, 32000, "je", 128), (2, 32000, "m", 48), (1, 48000, "m", 64),
                                                  (1, 44100, "s", 32), (2, 44100, "s", [32, 96, 192, 384])])
def test_formats(emu, oracle, layer, rate, mode, kbps):
    """joint stereo with -e; mono; two-channel Layer I at 32 kbps (frames that outgrow their slots); a bitrate per slot"""
    S = 4 if not np.isscalar(kbps) else 3
    run = SlotRun(emu, layer, S, rate, mode, kbps, 1)
    try:
        done = drive(run, plan_from(SMALL[:S], [1] * 4), sources_for(run, SMALL[:S], 500, 4 * run.spf))
        check(run, oracle, done, S)
    finally:
        run.close()


@pytest.mark.parametrize("name,nfs", [("l2_j44_064", [3, 1, 2, 2]), ("l1_s44_032_fields_exceed_frame", [1, 5, 2, 4])])
def test_golden_through_one_slot(emu, oracle, name, nfs):
    """a golden vector's PCM through slot 1 in unequal pieces while its neighbours churn: the golden's bytes"""
    meta, pcm, mpg, _ = golden_l12.load(name)
    run = SlotRun(emu, meta["layer"], 3, meta["rate"], meta["mode"], meta["kbps"], max(nfs))
    try:
        n = len(pcm) // run.ch
        last = n - sum(nfs[:-1]) * run.spf
        assert 0 < last <= nfs[-1] * run.spf
        scripts = [[("SE", 100), "S", ".", ("E", 0)], ["S", ".", ".", ("E", last)], [".", ("SE", run.spf), ("SE", 0), "S"]]
        src = sources_for(run, scripts, 600, sum(nfs) * run.spf)
        src[1] = [pcm]
        st = new_state(3, src)
        done = drive(run, plan_from(scripts, nfs), src, state=st)
        assert [d[2] for d in done if d[0] == 1] == [mpg]
        assert run.flush() == 0  # slot 2's stream ends here
        outs, lens, _ = run.outputs()
        assert list(lens) == [0, 0, 1]
        done.append((2, st["cur"][2][:st["pos"][2] * run.ch], st["got"][2] + outs[2]))
        check(run, oracle, done, 5)
    finally:
        run.close()


@pytest.mark.parametrize("layer,nf", [(2, 7), (1, 17)])
def test_several_chunks_per_call(emu, oracle, layer, nf):
    """1 MiB of scratch: a call is two chunks; slots start and end inside such calls, in either chunk"""
    run = SlotRun(emu, layer, 3, 44100, "j", 192 if layer == 1 else 128, nf, scratch_mb=1)
    try:
        spf = run.spf
        scripts = [["S", ".", ("E", nf * spf - 5)], ["S", ("E", 3 * spf + 17), ("SE", (nf - 2) * spf)], [".", "S", ("E", 0)]]
        done = drive(run, plan_from(scripts, [nf] * 3), sources_for(run, scripts, 700, 3 * nf * spf))
        assert run.launches() == [3 * 2] * 4  # two chunks per call
        check(run, oracle, done, 4)
    finally:
        run.close()


@pytest.mark.parametrize("layer", [1, 2])
def test_alternation_with_the_whole_batch_calls(emu, oracle, layer):
    """encode_slots, then encode_next (continues the open slots), then flush (ends them; 0 for the closed one); encode_next then
    starts every slot == the whole-file call; reset, and a whole-file call"""
    S, nf = 3, 2
    run = SlotRun(emu, layer, S, 44100, "s", 192 if layer == 1 else 128, nf)
    try:
        full = nf * run.spf
        row = full * run.ch
        src = [l12_signal(4 * full, run.ch, 800 + s) for s in range(S)]
        want = [oracle_l12(oracle, layer, 44100, run.kbps[s], "s", src[s][:2 * row])[0] for s in range(S)]
        got = [b""] * S
        assert run.frames() == [-1] * S
        # slots 0 and 1 START; slot 2 stays closed
        pcm = np.stack([src[0][:row], src[1][:row], loud(row, 1)])
        assert run.call(pcm, [START, START, 0]) == 0
        outs, lens, _ = run.outputs()
        assert lens[2] == 0 and run.frames() == [nf, nf, -1]
        got = [got[s] + outs[s] for s in range(S)]
        # encode_next continues the open ones
        pcm = np.stack([src[0][row:2 * row], src[1][row:2 * row], loud(row, 2)])
        assert run.encode_next(pcm, nf) == 0
        outs, lens, rows = run.outputs()
        assert lens[2] == 0 and (rows[2] == FILL).all() and run.frames() == [2 * nf, 2 * nf, -1]
        got = [got[s] + outs[s] for s in range(S)]
        # flush ends them
        assert run.flush() == 0
        outs, lens, rows = run.outputs()
        assert list(lens) == [1, 1, 0] and (rows[2] == FILL).all() and run.frames() == [-1] * S
        got = [got[s] + outs[s] for s in range(S)]
        assert got[:2] == want[:2] and got[2] == b""
        # every slot is closed: encode_next starts them all, as on a fresh batch
        got = [b""] * S
        for k in range(2):
            assert run.encode_next(np.stack([src[s][k * row:(k + 1) * row] for s in range(S)]), nf) == 0
            outs, _, _ = run.outputs()
            got = [got[s] + outs[s] for s in range(S)]
            assert run.frames() == [(k + 1) * nf] * S
        assert run.flush() == 0
        outs, lens, _ = run.outputs()
        assert list(lens) == [1] * S and run.frames() == [-1] * S
        assert [got[s] + outs[s] for s in range(S)] == want
        # a per-slot call over streams that encode_next began; reset abandons them
        assert run.encode_next(np.stack([src[s][:row] for s in range(S)]), nf) == 0
        assert run.call(np.stack([src[s][row:2 * row] for s in range(S)]), [0, END, 0], [full, 0, full]) == 0
        outs2, lens2, _ = run.outputs()
        assert lens2[1] == 1 and run.frames() == [2 * nf, -1, 2 * nf]
        assert run.L.mp3mi_l12_batch_reset(run.b) == 0 and run.frames() == [-1] * S
        # the whole-file call on the same batch
        run.put(np.stack([src[s][:row] for s in range(S)]))
        ns = np.array([full, 100, 0], np.int32)
        d_ns = run.mem.alloc(4 * S)
        run.mem.upload(d_ns, ns)
        assert run.L.mp3mi_l12_batch_encode(run.b, run.d_pcm, d_ns, nf, run.d_out, run.stride, run.d_len) == 0
        outs, _, _ = run.outputs()
        assert run.frames() == [-1] * S
        assert outs == [oracle_l12(oracle, layer, 44100, run.kbps[s], "s", src[s][:ns[s] * run.ch])[0] for s in range(S)]
    finally:
        run.close()


def test_broken_rules_return_err_arg(emu, oracle):
    """every broken rule: MP3MI_ERR_ARG, the batch as it was -- the next legal call gives the bytes of a batch that never saw them"""
    layer, S, nf, rate = 2, 2, 2, 44100
    runs = [SlotRun(emu, layer, S, rate, "s", 128, nf) for _ in range(2)]
    try:
        run = runs[0]
        full = nf * run.spf
        row = full * run.ch
        src = [l12_signal(2 * full, run.ch, 900 + s) for s in range(S)]
        pcm = np.stack([x[:row] for x in src])
        for r in runs:
            assert r.call(pcm, [START, 0]) == 0  # slot 0 open at 2 frames, slot 1 closed
        first, _, _ = run.outputs()
        L = run.L
        before = run.frames()
        bad = [
            dict(ctl=[4, 0]),                                # unknown bit
            dict(ctl=[0, 128]),
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
            dict(ctl=[0, 0], stride=L.mp3mi_l12_batch_out_stride(run.b, nf) - 1),
        ]
        for kw in bad:
            assert run.call(pcm, **kw) == -1, kw
            assert run.frames() == before, kw
        z = np.zeros(S, np.uint8).ctypes.data
        assert L.mp3mi_l12_batch_encode_slots(run.b, run.d_pcm, nf, z, None, None, run.stride, run.d_len) == -1
        assert L.mp3mi_l12_batch_encode_slots(run.b, run.d_pcm, nf, z, None, run.d_out, run.stride, None) == -1
        assert L.mp3mi_l12_batch_encode_slots(None, run.d_pcm, nf, z, None, run.d_out, run.stride, run.d_len) == -1
        assert L.mp3mi_l12_batch_slot_frames(run.b, None) == -1 and L.mp3mi_l12_batch_slot_frames(None, None) == -1
        assert run.frames() == before
        # legal: slot 0 ENDs on 100 samples, slot 1 is a one-call file of 2000
        pcm2 = loud(S * row, 3).reshape(S, row)
        pcm2[0, :100 * run.ch] = src[0][row:row + 100 * run.ch]
        pcm2[1, :2000 * run.ch] = src[1][:2000 * run.ch]
        second = []
        for r in runs:
            assert r.call(pcm2, [END, START | END], [100, 2000]) == 0
            second.append(r.outputs()[0])
            assert r.frames() == [-1, -1]
        assert second[0] == second[1]
        assert first[0] + second[0][0] == oracle_l12(oracle, layer, rate, 128, "s", src[0][:row + 100 * run.ch])[0]
        assert second[0][1] == oracle_l12(oracle, layer, rate, 128, "s", src[1][:2000 * run.ch])[0]
    finally:
        for r in runs:
            r.close()


@pytest.mark.parametrize("layer,nf,scratch_mb,chunks", [(2, 7, 1, 2), (1, 3, 0, 1)])
def test_no_per_slot_call_no_change(emu, oracle, layer, nf, scratch_mb, chunks):
    """a batch that never made a per-slot call: the flush of a fresh batch gives one byte per stream, and a whole-file call and an
    encode_next launch 4 x chunks kernels (1 MiB of scratch: two chunks per call, as in test_several_chunks_per_call)"""
    S = 3
    run = SlotRun(emu, layer, S, 44100, "s", 192 if layer == 1 else 128, nf, scratch_mb=scratch_mb)
    try:
        assert run.frames() == [-1] * S
        assert run.flush() == 0
        outs, lens, _ = run.outputs()
        assert list(lens) == [1] * S and outs == [b"\0"] * S and run.frames() == [-1] * S
        row = nf * run.spf * run.ch
        src = np.stack([l12_signal(nf * run.spf, run.ch, 950 + s) for s in range(S)])
        run.put(src)
        assert run.L.mp3mi_l12_batch_encode(run.b, run.d_pcm, None, nf, run.d_out, run.stride, run.d_len) == 0
        whole, _, _ = run.outputs()
        assert run.launches() == [chunks] * 4 and run.frames() == [-1] * S
        assert run.encode_next(src, nf) == 0
        nxt, _, _ = run.outputs()
        assert run.launches() == [2 * chunks] * 4 and run.frames() == [nf] * S
        assert run.flush() == 0
        outs, lens, _ = run.outputs()
        assert list(lens) == [1] * S
        want = [oracle_l12(oracle, layer, 44100, run.kbps[s], "s", src[s])[0] for s in range(S)]
        assert whole == want and [nxt[s] + outs[s] for s in range(S)] == want
    finally:
        run.close()
