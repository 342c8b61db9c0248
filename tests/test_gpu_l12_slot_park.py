"""A bitrate per stream at START, and park / resume, for Layers I and II on the MI355X (include/mp3mi_l12.h): the scenarios of
tests/test_l12_slot_park.py over 64 slots (tests/l12_park.py); export, import and per-slot calls issued back to back without a sync
-- three takes of the two-entry control ring per tick: the emulator runs every launch where it is issued and cannot show it --; two
batches on one device; and the torch binding in a seeded server loop."""
import ctypes
import importlib

import numpy as np
import pytest

from l12_park import ParkRun, Stream, Ticket, aligned, bind, case_phase, case_rates, case_snapshot, case_travel, check_streams
from l12_slots import END, START
from mp3common import DevMem, l12_signal, l12_spf, oracle_l12

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layer,k", [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2)])
def test_park_and_resume_at_every_phase_gpu(product, oracle, layer, k):
    case_phase(product, oracle, layer, k, S=64)


@pytest.mark.parametrize("layer", [1, 2])
def test_snapshot_imported_twice_gpu(product, oracle, layer):
    case_snapshot(product, oracle, layer, S=64)


@pytest.mark.parametrize("layer,rate,mode,create,rates", [(2, 44100, "s", 384, [64, 128, 192]), (2, 32000, "m", 384, [48, 64, 96]),
                                                          (1, 44100, "s", 448, [32, 448])])
def test_bitrate_at_start_gpu(product, oracle, layer, rate, mode, create, rates):
    case_rates(product, oracle, layer, rate, mode, create, rates, S=64)


def test_the_bitrate_travels_gpu(product, oracle):
    case_travel(product, oracle, S=64)


@pytest.mark.parametrize("layer,nf,create,rates", [(2, 1, 384, [64, 128, 192, 384]), (1, 2, 448, [32, 192, 448])])
def test_back_to_back_without_sync_gpu(product, oracle, layer, nf, create, rates):
    """Six ticks over 64 slots, nothing synced until the end: per tick an export that closes four slots, the import of the four
    streams the tick before parked -- each into the slot of its neighbour, from the record the export before has not necessarily
    written yet when the call is issued -- and a per-slot call with a bitrate array: three takes of the two-entry control ring, so the
    host meets the fences.  Every call has output buffers and a record buffer of its own.  Every stream is the oracle's."""
    S, T, n, ch, rate = 64, 6, 4, 2, 44100
    L = bind(product)
    spf = l12_spf(layer)
    full = nf * spf
    mem = DevMem(product)
    b = ctypes.c_void_p()
    try:
        assert L.mp3mi_l12_batch_create(ctypes.byref(b), layer, S, rate, ch, None, create, nf, 0) == 0
        stride, B = L.mp3mi_l12_batch_out_stride(b, nf), L.mp3mi_l12_batch_slot_state_bytes(b)
        streams = [Stream(l12_signal((T + 1) * full, ch, 400 + s, rate), rates[s % len(rates)], ch) for s in range(S)]
        # the plan, from the test's own books: per tick the slots that leave, the slots that come back, and the per-slot call
        cur, plan, away = list(streams), [], []
        for t in range(T):
            last = t == T - 1
            p = dict(back=[], leave=[])
            if t > 0:  # the parked streams come back, each into its neighbour's slot; then, but in the last tick, four others leave
                p["back"] = [(away[(i + 1) % n][0], away[i][1]) for i in range(n)]
                for s, st in p["back"]:
                    cur[s] = st
                p["leave"] = [] if last else [(7 * t + 16 * i) % S for i in range(n)]
            away = [(s, cur[s]) for s in p["leave"]]
            for s in p["leave"]:
                cur[s] = None
            pcm, ctl, ns, kb = np.zeros((S, full * ch), np.int16), np.zeros(S, np.uint8), np.zeros(S, np.int32), np.zeros(S, np.int32)
            for s, st in enumerate(cur):
                if st is None:
                    continue
                ctl[s] = (START if t == 0 else 0) | (END if last else 0)
                ns[s] = (s * 37) % (full + 1) if last else full
                kb[s] = st.kbps  # (a persistent array: at START the stream's choice, afterwards what it has)
                pcm[s, :ns[s] * ch] = st.take(int(ns[s]))
            p.update(pcm=pcm, ctl=ctl, ns=ns, kb=kb, slots=[(s, st) for s, st in enumerate(cur) if st is not None])
            if t == 0:  # the first tick STARTs every slot; four leave behind the call
                p["leave"] = [16 * i for i in range(n)]
                away = [(s, cur[s]) for s in p["leave"]]
                for s in p["leave"]:
                    cur[s] = None
            plan.append(p)
        assert not away and all(st is not None for st in cur)  # the last tick ENDs all 64
        for p in plan:
            p["d_pcm"], p["d_out"], p["d_len"], p["d_rec"] = mem.alloc(p["pcm"].nbytes), mem.alloc(S * stride), mem.alloc(4 * S), aligned(mem, n * B)
            mem.upload(p["d_pcm"], p["pcm"])
            mem.upload(p["d_out"], np.full(S * stride, 0xA5, np.uint8))
            p["tk"] = (Ticket * n)()
        # issued in a row
        prev = None
        for t, p in enumerate(plan):
            sl = lambda slots: np.ascontiguousarray(slots, dtype=np.int32).ctypes.data
            call = lambda: L.mp3mi_l12_batch_encode_slots_kbps(b, p["d_pcm"], nf, p["ctl"].ctypes.data, p["ns"].ctypes.data, p["kb"].ctypes.data,
                                                               p["d_out"], stride, p["d_len"])
            export = lambda: L.mp3mi_l12_batch_slots_export(b, len(p["leave"]), sl(p["leave"]), 1, p["d_rec"], B, p["tk"])
            if t == 0:
                assert call() == 0 and export() == 0
            else:
                assert L.mp3mi_l12_batch_slots_import(b, len(p["back"]), sl([s for s, _ in p["back"]]), prev["d_rec"], B, prev["tk"]) == 0
                if p["leave"]:
                    assert export() == 0
                assert call() == 0
            prev = p
        assert L.mp3mi_l12_batch_sync(b) == 0
        fr = np.zeros(S, np.int64)
        assert L.mp3mi_l12_batch_slot_frames(b, fr.ctypes.data) == 0
        for p in plan:
            out, lens = mem.download(p["d_out"], (S, stride), np.uint8), mem.download(p["d_len"], (S,), np.uint32)
            open_ = {s for s, _ in p["slots"]}
            for s in range(S):
                if s not in open_:
                    assert lens[s] == 0 and (out[s] == 0xA5).all(), s
            for s, st in p["slots"]:
                st.got += out[s, :lens[s]].tobytes()
        assert len({st.pos // full for st in streams}) >= 2  # some sat out a tick, some did not
        for i, st in enumerate(streams):
            assert st.got == oracle_l12(oracle, layer, rate, st.kbps, "s", st.fed())[0], "stream %d, %d kbps, %d samples" % (i, st.kbps, st.pos)
    finally:
        if b:
            L.mp3mi_l12_batch_destroy(b)
        mem.free()


def test_two_batches_on_one_device_gpu(product, oracle):
    """Layer I, mono: 32 streams leave a batch of 64 slots in one export and, after its sync, fill every slot of a second batch in one
    import -- which hands that batch over to its whole-batch path: encode_next continues them, the flush ends them -- while the first
    batch goes on and takes new streams into the vacated slots"""
    pool = DevMem(product)
    a = ParkRun(product, 1, 64, 48000, "m", [64, 96, 128, 160] * 16, 3, pool=pool)
    b = ParkRun(product, 1, 32, 48000, "m", 448, 3, pool=pool)
    try:
        spf, done = a.spf, []
        done += a.step(3, starts={s: a.stream(500 + s, 12 * spf, slot=s) for s in range(64)})
        done += a.step(2)
        odd = list(range(1, 64, 2))
        moved = b.import_(list(range(32)), a.export(odd))
        done += a.step(1, starts={s: a.stream(600 + s, 4 * spf, kbps=32) for s in odd[:8]})
        done += b.next(3)
        done += b.next(1)
        done += b.flush_all()
        done += a.step(3, ends={s: (41 * s) % (3 * spf + 1) for s in range(64) if a.cur[s] is not None})
        assert all(st in done for st in moved) and a.frames() == [-1] * 64 and len(done) == 32 + 32 + 8
        check_streams(a, oracle, done, 72)
    finally:
        a.close()
        b.close()
        pool.free()


def test_binding_server_loop_gpu(product, oracle):
    """BatchL12.export_slots, import_slots, encode_slots(kbps=...) and slot_kbps on torch tensors: 64 slots of Layer II created at 384
    kbps, 12 calls of two frames; per call two streams are parked and two parked ones resumed, three END and up to two START at one
    of four bitrates.  slot_frames and slot_kbps follow the test's books; 8 finished streams, parked ones among them, are the oracle's."""
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    dev = torch.device("cuda:0")
    layer, S, nf, rate, ch, n_calls, rates = 2, 64, 2, 44100, 2, 12, [64, 128, 192, 384]
    full = nf * 1152
    rng = np.random.default_rng(20261021)
    b = mp3.BatchL12(layer, S, rate, ch, 384, nf)
    stride, B = b.out_stride(nf), b.slot_state_bytes()
    assert B == 11392 and ctypes.sizeof(mp3.SlotTicketL12) == 56
    n_made = [0]

    def new_stream():
        n_made[0] += 1
        st = Stream(l12_signal((n_calls + 1) * full, ch, 700 + n_made[0], rate), rates[n_made[0] % 4], ch)
        st.parks = 0
        return st

    cur, parked, done = [None] * S, [], []
    for k in range(n_calls):
        closed = [s for s in range(S) if cur[s] is None]
        if len(parked) >= 2 and k > 0:  # two come back, into closed slots, from records of two different exports
            (s0, t0, r0), (s1, t1, r1) = parked.pop(0), parked.pop(0)
            slots = [closed.pop(), closed.pop(0)]
            b.import_slots(slots, torch.stack([r0, r1]).contiguous(), [t0, t1])
            cur[slots[0]], cur[slots[1]] = s0, s1
        if k > 0:  # two leave
            slots = [int(s) for s in rng.choice([s for s in range(S) if cur[s] is not None], 2, replace=False)]
            state = torch.full((2, B + 16), 0xA5, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            tk = b.export_slots(slots, state, close=True)
            b.sync()  # (torch reads the records on its own stream)
            assert (state[:, B:] == 0xA5).all().item()
            for i, s in enumerate(slots):
                assert (tk[i].kbps, tk[i].frames, tk[i].layer, tk[i].reserved) == (cur[s].kbps, cur[s].frames, layer, 0)
                cur[s].parks += 1
                parked.append((cur[s], mp3.SlotTicketL12.from_buffer_copy(tk[i]), state[i, :B].clone()))
                cur[s] = None
        start, end, ns, kb = np.zeros(S, bool), np.zeros(S, bool), np.zeros(S, np.int32), np.zeros(S, np.int32)
        closed = [s for s in range(S) if cur[s] is None]
        for s in (closed if k == 0 else closed[2:4])[:S - 8]:  # (at least two slots stay closed for the streams that come back)
            cur[s], start[s] = new_stream(), True
            cur[s].frames = 0
        ending = [] if k == 0 else [int(s) for s in rng.choice([s for s in range(S) if cur[s] is not None], 3, replace=False)]
        if k == n_calls - 1:
            ending = [s for s in range(S) if cur[s] is not None]
        pcm = np.full((S, full * ch), 32767, np.int16)
        for s, st in enumerate(cur):
            if st is None:
                continue
            end[s] = s in ending
            ns[s] = full if not end[s] else (0 if s == ending[0] else int(rng.integers(0, full + 1)))
            kb[s] = st.kbps  # a persistent array: the open streams' own bitrates, and the starting ones'
            pcm[s, :ns[s] * ch] = st.take(int(ns[s]))
        out = torch.full((S, stride), 0xA5, dtype=torch.uint8, device=dev)
        ln = torch.full((S,), -1, dtype=torch.int32, device=dev)
        b.encode_slots(torch.from_numpy(pcm).to(dev), nf, out, ln, start=start, end=end, n_samples=ns, kbps=kb)
        b.sync()
        o, n = out.cpu().numpy(), ln.cpu().numpy()
        for s, st in enumerate(cur):
            if st is None:
                assert n[s] == 0 and (o[s] == 0xA5).all(), (k, s)
                continue
            st.got += o[s, :n[s]].tobytes()
            if end[s]:
                done.append(st)
                cur[s] = None
            else:
                st.frames += nf
        kbps_now, ceiling = b.slot_kbps()
        assert ceiling == 384 and list(kbps_now) == [384 if st is None else st.kbps for st in cur], k
        assert list(b.slot_frames()) == [-1 if st is None else st.frames for st in cur], k
    b.close()
    was_parked = [st for st in done if st.parks]
    assert len(done) >= 56 and len(was_parked) >= 6
    pick = was_parked[:5] + [st for st in done if not st.parks][:2] + [min(done, key=lambda st: st.pos)]
    assert len({st.kbps for st in pick}) >= 3
    for st in pick:
        assert st.got == oracle_l12(oracle, layer, rate, st.kbps, "s", st.fed())[0], "%d kbps, %d samples, parked %d times" % (st.kbps, st.pos, st.parks)
