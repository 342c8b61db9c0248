#!/usr/bin/env python3
"""Times per-slot streaming (mp3mi_batch_encode_slots) against whole-batch streaming (mp3mi_batch_encode_next) on the device.

4096 stereo slots, 44.1 kHz, 128 kbps, calls of 32 frames on resident PCM, issued back to back (one sync at the end of a run):
  (a) encode_next                                  every stream goes on
  (b) encode_slots, every slot continuing          the per-slot path with nothing to start or end
  (c) encode_slots with churn                      in every call 1/32 of the slots END (at random partial lengths) and as
                                                   many closed slots START
Prints one JSON line: ms per call of each case and the library's source hash.

--mixed-kbps: the batch is created at 320 kbps and every START of (b) and (c) draws its stream's bitrate from 64 / 128 / 192 / 320
(mp3mi_batch_encode_slots_kbps; seeded); (a) runs at the create-time 320.  The line also carries the mean bitrate of (b)'s streams.

--host [--occupancy F]: the per-slot cases on PAGE-LOCKED HOST buffers (mp3mi_batch_encode_slots_host_async; ticks issued back
to back, tick t collected with mp3mi_batch_host_wait(1) after tick t + 1 has been issued), with a fraction F of the slots live
(the others stay closed; with F < 1, or with --map, the rows go through a row map, so only the live rows cross PCIe):
  (d) resident_slots      encode_slots on resident PCM with the same live slots                    the floor
  (e) sync_copy           what a caller had before the host call: hipMemcpy of full [n_streams] rows up, encode_slots,
                          sync, hipMemcpy down, tick by tick                                       the baseline to beat
  (f) host_continue       the host call, every live slot continuing
  (g) host_churn          the host call; in every tick 1/32 of the live slots END and as many closed ones START, so the row
                          set changes from tick to tick

--park N: one more resident case.  In every tick after the first, N streams are PARKED (mp3mi_batch_slots_export, closing their
slots) and the N streams parked one tick before RESUME in the slots they left (mp3mi_batch_slots_import): 2 N <= streams, and
streams - N of them are live in every tick:
  (p) slots_park          import N, export N, encode_slots per tick, issued back to back like the others
The line then carries park_vs_continue and the bytes of a state record.

--layer 1|2: cases (a), (b), (c) on the Layer I / II batch (mp3mi_l12_batch_encode_next, mp3mi_l12_batch_encode_slots): Layer I at
192 kbps in ticks of 12 frames, Layer II at 128 kbps in ticks of 4 (--frames sets another length); in (b) one slot STARTs a tick
after the others, or the batch would hand every tick back to the whole-batch path (profiles/l12_slots_bench.jsonl).  --mixed-kbps:
the batch is created at the layer's largest bitrate (448 / 384) and every START of (b) and (c) draws 64 / 128 / 192 / 448 (Layer I) or
64 / 128 / 192 / 384 (Layer II: allocation tables 2, 0, 1, 1 -- mp3mi_l12_batch_encode_slots_kbps).  --park N: case (p) as above, on
mp3mi_l12_batch_slots_export / _import (profiles/l12_park_bench.jsonl).

usage: slots_bench.py [--calls 20] [--frames 32] [--streams 4096] [--reps 3] [--mixed-kbps] [--park N] [--host [--occupancy 1.0] [--map]]
       slots_bench.py --layer 1|2 [--calls 20] [--frames N] [--streams 4096] [--reps 3] [--mixed-kbps] [--park N]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3, help="runs of every case; the fastest counts")
    ap.add_argument("--mixed-kbps", action="store_true", help="a batch created at 320 kbps; every START draws 64 / 128 / 192 / 320")
    ap.add_argument("--park", type=int, default=0, help="per tick, park this many streams and resume as many parked ones")
    ap.add_argument("--host", action="store_true", help="the per-slot cases on page-locked host buffers")
    ap.add_argument("--occupancy", type=float, default=1.0, help="--host: fraction of the slots that are live")
    ap.add_argument("--map", action="store_true", help="--host: a row map at occupancy 1.0 too (k_rows_in / k_rows_out run)")
    ap.add_argument("--layer", type=int, default=3, choices=(1, 2, 3), help="1 | 2: the Layer I / II batch (mp3mi_l12_batch_encode_slots)")
    a = ap.parse_args()
    if a.layer != 3:
        if a.host:
            ap.error("--layer 1|2 times the resident cases only")
        return l12_main(a)
    if a.host:
        if a.mixed_kbps or a.park:
            ap.error("--mixed-kbps and --park time the resident cases (without --host)")
        return host_main(a)
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    S, nf, rate, ch, kbps = a.streams, a.frames, 44100, 2, 320 if a.mixed_kbps else 128
    full = nf * 1152
    dev = torch.device("cuda:0")
    pcm = torch.empty((S, full * ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    mp3.synth_pcm_device(pcm, full, ch, rate)
    b = mp3.Batch(S, rate, ch, kbps, nf)
    out = torch.zeros((S, b.out_stride(nf)), dtype=torch.uint8, device=dev)
    out_len = torch.zeros(S, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rng = np.random.default_rng(1)
    every = np.ones(S, bool)
    rates = np.array([64, 128, 192, 320], np.int32)
    drawn = []  # the bitrates of run_continue's streams

    def draw(start):
        """kbps of a call: a drawn bitrate for every START (None without --mixed-kbps: the call without the array)"""
        return np.where(start, rates[rng.integers(0, 4, S)], 0).astype(np.int32) if a.mixed_kbps else None

    def run_next():
        for _ in range(a.calls):
            b.encode_next(pcm, nf, out, out_len)

    def run_continue():
        kb = draw(every)
        drawn[:] = [] if kb is None else [kb]
        b.encode_slots(pcm, nf, out, out_len, start=every, kbps=kb)
        for _ in range(a.calls - 1):
            b.encode_slots(pcm, nf, out, out_len)

    def run_churn():
        b.encode_slots(pcm, nf, out, out_len, start=every, kbps=draw(every))
        closed = np.zeros(S, bool)
        for _ in range(a.calls - 1):
            start = closed.copy()
            cand = np.flatnonzero(~closed)
            end = np.zeros(S, bool)
            end[rng.choice(cand, S // 32, replace=False)] = True
            ns = np.full(S, full, np.int32)
            ns[end] = rng.integers(0, full + 1, int(end.sum()))
            b.encode_slots(pcm, nf, out, out_len, start=start, end=end, n_samples=ns, kbps=draw(start))
            closed = end

    N = a.park
    if N and not 0 < 2 * N <= S:
        ap.error("--park N needs 2 N <= streams")
    state = [torch.zeros((N, b.slot_state_bytes()), dtype=torch.uint8, device=dev) for _ in range(2)] if N else None

    def run_park():
        """every slot STARTs; tick k >= 1 resumes the N streams tick k - 1 parked, in the slots they left, parks the streams of the
        next N slots of a random walk (record sets by the tick's parity), and encodes: S - N streams are live in every tick"""
        order = rng.permutation(S).astype(np.int32)
        b.encode_slots(pcm, nf, out, out_len, start=every)
        away = None  # (slots, tickets) of the tick before
        for k in range(1, a.calls):
            if away is not None:
                b.import_slots(away[0], state[(k - 1) & 1], away[1])
            sl = order[((k - 1) * N + np.arange(N)) % S]
            away = (sl, b.export_slots(sl, state[k & 1]))
            b.encode_slots(pcm, nf, out, out_len)

    cases = (("encode_next", run_next), ("slots_continue", run_continue), ("slots_churn", run_churn)) + ((("slots_park", run_park),) if N else ())
    res = {}
    for name, fn in cases:
        best = None
        for r in range(a.reps + 1):  # the first run warms up
            b.reset()
            b.sync()
            t0 = time.perf_counter()
            fn()
            b.flush(out, out_len)
            b.sync()
            ms = (time.perf_counter() - t0) * 1e3 / a.calls
            if r > 0:
                best = ms if best is None else min(best, ms)
        res[name] = round(best, 3)
    b_state_bytes = b.slot_state_bytes() if N else 0
    b.close()
    print(json.dumps({"tool": "slots_bench", "streams": S, "frames_per_call": nf, "calls": a.calls, "rate": rate, "channels": ch,
                      "kbps": kbps, "mixed_kbps": bool(a.mixed_kbps), "mean_kbps_continue": round(float(drawn[0].mean()), 1) if drawn else kbps,
                      "ms_per_call": res,
                      "continue_vs_next": round(res["slots_continue"] / res["encode_next"], 4),
                      "churn_vs_continue": round(res["slots_churn"] / res["slots_continue"], 4),
                      **({"park": N, "park_vs_continue": round(res["slots_park"] / res["slots_continue"], 4),
                          "state_bytes": b_state_bytes} if N else {}),
                      "source_hash": mp3.lib().mp3mi_source_hash().decode()}))


def l12_main(a):
    """--layer 1|2: cases (a), (b), (c) and, with --park, (p) on the Layer I / II batch; calls of --frames frames (default: 12 Layer I,
    4 Layer II -- about 0.1 s of audio a tick), Layer I at 192 kbps, Layer II at 128; --mixed-kbps: created at 448 / 384, a drawn
    bitrate per START"""
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    S, rate, ch = a.streams, 44100, 2
    kbps = ((448 if a.layer == 1 else 384) if a.mixed_kbps else (192 if a.layer == 1 else 128))
    rates = np.array([64, 128, 192, kbps], np.int32)
    N = a.park
    if N and not 0 < 2 * N <= S:
        raise SystemExit("--park N needs 2 N <= streams")
    nf = a.frames if a.frames != 32 else (12 if a.layer == 1 else 4)
    full = nf * mp3.L12_FRAME_SAMPLES[a.layer]
    dev = torch.device("cuda:0")
    pcm = torch.empty((S, full * ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    mp3.synth_pcm_device(pcm, full, ch, rate)
    b = mp3.BatchL12(a.layer, S, rate, ch, kbps, nf)
    out = torch.zeros((S, b.out_stride(nf)), dtype=torch.uint8, device=dev)
    out_len = torch.zeros(S, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rng = np.random.default_rng(1)
    every = np.ones(S, bool)
    drawn = []  # the bitrates of run_continue's streams

    def draw(start):
        """kbps of a call: a drawn bitrate for every START (None without --mixed-kbps: the call without the array)"""
        return np.where(start, rates[rng.integers(0, 4, S)], 0).astype(np.int32) if a.mixed_kbps else None

    def slots(**kw):
        if kw.get("kbps") is None:
            kw.pop("kbps", None)  # (the call as it was before there was an array)
        b.encode_slots(pcm, nf, out, out_len, **kw)

    def run_next():
        for _ in range(a.calls):
            b.encode_next(pcm, nf, out, out_len)

    def run_continue():
        # (one slot STARTs a call later than the others: with every slot at the same frame the batch would hand the calls
        # back to the whole-batch path, which is case (a))
        first = every.copy()
        first[S - 1] = False
        kb = draw(every)
        drawn[:] = [] if kb is None else [kb]
        slots(start=first, kbps=None if kb is None else np.where(first, kb, 0))
        slots(start=~first, kbps=None if kb is None else np.where(first, 0, kb))
        for _ in range(a.calls - 2):
            slots()

    def run_churn():
        slots(start=every, kbps=draw(every))
        closed = np.zeros(S, bool)
        for _ in range(a.calls - 1):
            start = closed.copy()
            end = np.zeros(S, bool)
            end[rng.choice(np.flatnonzero(~closed), S // 32, replace=False)] = True
            ns = np.full(S, full, np.int32)
            ns[end] = rng.integers(0, full + 1, int(end.sum()))
            slots(start=start, end=end, n_samples=ns, kbps=draw(start))
            closed = end

    state = [torch.zeros((N, b.slot_state_bytes()), dtype=torch.uint8, device=dev) for _ in range(2)] if N else None

    def run_park():
        """every slot STARTs; tick k >= 1 resumes the N streams tick k - 1 parked, in the slots they left, parks the streams of the
        next N slots of a random walk (record sets by the tick's parity), and encodes: S - N streams are live in every tick"""
        order = rng.permutation(S).astype(np.int32)
        slots(start=every, kbps=draw(every))
        away = None  # (slots, tickets) of the tick before
        for k in range(1, a.calls):
            if away is not None:
                b.import_slots(away[0], state[(k - 1) & 1], away[1])
            sl = order[((k - 1) * N + np.arange(N)) % S]
            away = (sl, b.export_slots(sl, state[k & 1]))
            slots()

    res = {}
    for name, fn in (("encode_next", run_next), ("slots_continue", run_continue), ("slots_churn", run_churn)) + ((("slots_park", run_park),) if N else ()):
        best = None
        for r in range(a.reps + 1):  # the first run warms up
            b.reset()
            b.sync()
            t0 = time.perf_counter()
            fn()
            b.flush(out, out_len)
            b.sync()
            ms = (time.perf_counter() - t0) * 1e3 / a.calls
            if r > 0:
                best = ms if best is None else min(best, ms)
        res[name] = round(best, 3)
    state_bytes = b.slot_state_bytes() if N else 0
    b.close()
    print(json.dumps({"tool": "slots_bench --layer", "layer": a.layer, "streams": S, "frames_per_call": nf, "calls": a.calls, "rate": rate,
                      "channels": ch, "kbps": kbps, "ms_per_call": res,
                      "continue_vs_next": round(res["slots_continue"] / res["encode_next"], 4),
                      "churn_vs_continue": round(res["slots_churn"] / res["slots_continue"], 4),
                      **({"mixed_kbps": True, "mean_kbps_continue": round(float(drawn[0].mean()), 1)} if a.mixed_kbps else {}),
                      **({"park": N, "park_vs_continue": round(res["slots_park"] / res["slots_continue"], 4), "state_bytes": state_bytes} if N else {}),
                      "source_hash": mp3.lib().mp3mi_source_hash().decode()}))


def host_main(a):
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    S, nf, rate, ch, kbps = a.streams, a.frames, 44100, 2, 128
    full = nf * 1152
    dev = torch.device("cuda:0")
    pcm = torch.empty((S, full * ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    mp3.synth_pcm_device(pcm, full, ch, rate)
    b = mp3.Batch(S, rate, ch, kbps, nf)
    stride = b.out_stride(nf)
    out = torch.zeros((S, stride), dtype=torch.uint8, device=dev)
    out_len = torch.zeros(S, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(1)
    R = max(1, min(S, int(round(a.occupancy * S))))
    live = np.sort(rng.choice(S, R, replace=False))
    mapped = a.map or R < S
    is_live = np.zeros(S, bool)
    is_live[live] = True
    # page-locked: the PCM of all slots (the baseline moves all of it; the host call reads the first rows of it as its dense
    # rows -- every row holds a stream's worth of synthetic PCM, which row is immaterial to the time), two sets of outputs
    pcm_h = torch.empty((S, full * ch), dtype=torch.int16).pin_memory()
    pcm_h.copy_(pcm)
    out_h = [torch.zeros((S, stride), dtype=torch.uint8).pin_memory() for _ in range(2)]
    len_h = [torch.zeros(S, dtype=torch.int32).pin_memory() for _ in range(2)]
    torch.cuda.synchronize()

    def resident():
        b.encode_slots(pcm, nf, out, out_len, start=is_live)
        for _ in range(a.calls - 1):
            b.encode_slots(pcm, nf, out, out_len)

    def sync_copy():
        for k in range(a.calls):
            pcm.copy_(pcm_h)  # full rows, blocking
            torch.cuda.synchronize()
            b.encode_slots(pcm, nf, out, out_len, start=is_live if k == 0 else None)
            b.sync()
            out_h[0].copy_(out)
            len_h[0].copy_(out_len)
            torch.cuda.synchronize()

    def host_tick(k, rows, **kw):
        n = len(rows)
        b.encode_slots_host(pcm_h[:n], nf, out_h[k & 1][:n], len_h[k & 1][:n], rows=rows if mapped else None, **kw)
        if k >= 1:
            b.host_wait(1)  # collect tick k - 1 behind tick k's issue

    def host_continue():
        host_tick(0, live, start=np.ones(R, bool))
        for k in range(1, a.calls):
            host_tick(k, live)
        b.host_wait(0)

    def host_churn():
        open_ = is_live.copy()
        host_tick(0, live, start=np.ones(R, bool))
        closed_last = np.zeros(S, bool)
        for k in range(1, a.calls):
            start = closed_last
            end = np.zeros(S, bool)
            end[rng.choice(np.flatnonzero(open_), max(1, R // 32), replace=False)] = True
            rows = np.flatnonzero(open_ | start)
            ns = np.full(S, full, np.int32)
            ns[end] = rng.integers(0, full + 1, int(end.sum()))
            host_tick(k, rows, start=start[rows], end=end[rows], n_samples=ns[rows])
            open_ = (open_ | start) & ~end
            closed_last = end
        b.host_wait(0)

    if not mapped:
        # without a row map a closed slot still has a row, and a row must carry a stream: churn cannot leave slots closed
        cases = (("resident_slots", resident), ("sync_copy", sync_copy), ("host_continue", host_continue))
    else:
        cases = (("resident_slots", resident), ("sync_copy", sync_copy), ("host_continue", host_continue), ("host_churn", host_churn))
    res = {}
    for name, fn in cases:
        best = None
        for r in range(a.reps + 1):  # the first run warms up
            b.reset()
            b.sync()
            t0 = time.perf_counter()
            fn()
            b.flush(out, out_len)
            b.sync()
            ms = (time.perf_counter() - t0) * 1e3 / a.calls
            if r > 0:
                best = ms if best is None else min(best, ms)
        res[name] = round(best, 3)
    st = b.host_io_stats()
    b.close()
    print(json.dumps({"tool": "slots_bench --host", "streams": S, "live_slots": R, "row_map": bool(mapped), "frames_per_call": nf, "calls": a.calls,
                      "rate": rate, "channels": ch, "kbps": kbps, "ms_per_call": res,
                      "host_vs_resident": round(res["host_continue"] / res["resident_slots"], 4),
                      "host_vs_sync_copy": round(res["host_continue"] / res["sync_copy"], 4),
                      "h2d_GBps": round(st["h2d_bytes"] / max(st["h2d_ms"], 1e-9) / 1e6, 2), "d2h_GBps": round(st["d2h_bytes"] / max(st["d2h_ms"], 1e-9) / 1e6, 2),
                      "source_hash": mp3.lib().mp3mi_source_hash().decode()}))


if __name__ == "__main__":
    main()
