#!/usr/bin/env python3
"""Times the feeder (mp3mi_feed_tick, include/mp3mi.h) in front of a slot batch on the device.

4096 stereo slots, 44.1 kHz, 128 kbps, ticks of 32 frames on resident push rows, 20 ticks issued back to back (one sync at the end
of a run), three scenarios (--scenario):
  a   every lane pushes exactly a tick: all ready, nobody is parked -- beside it the plain mp3mi_batch_encode_slots tick of the same
      library on the same samples, every slot continuing (slots_continue_ms): the difference is what the feeder costs
  b   48 kHz packets of 960 samples, 38 or 39 packets a tick at random (a tick is 38.4): lanes run short and sit out.  (38.5 on
      average: a lane's backlog creeps up by a tenth of a packet per tick, so the lanes are sized for two ticks' packets)
  c   half of the lanes (the odd ones) push nothing every other tick: they are short then, parked, and resume the tick after
  d   (--lanes N) more lanes than slots, mp3mi_feed_tick_lanes: N lanes in front of the slots, 48 kHz, every lane pushes one packet a
      tick (--packet samples; default a tick's samples / (N / streams), so that streams lanes become ready in every tick and every
      slot changes hands in every tick: with N = 8 x streams each lane is ready every 8th tick).  The lanes START staggered over
      the first N / streams ticks, which are not timed.  Beside it the plain mp3mi_batch_encode_slots tick (the floor).  Reports
      the lanes that waited for a slot per tick as well.
  --host-time ROWS   (with --lanes N) the host time of mp3mi_feed_tick_lanes per call, wall clock around the call with nothing
      waited for and the device idle before it: ROWS lanes of N bring a one-call file of a tick each, 50 ticks; reported for N and
      for 4096 lanes, and their ratio.  Use a small batch (--streams 128 --frames 1): the rings are N times a tick.
  --host   scenarios a, b and d (--lanes N) as defined above, on HOST buffers (mp3mi_feed_tick_lanes_host_async; for a and b a feeder
      with as many lanes as slots).  Three variants of the same ticks on the same library, alternating, --reps runs each: `device`,
      mp3mi_feed_tick_lanes on resident packets (the floor); `device_copies`, the same call between synchronous copies -- the packet
      rectangle [n_rows][max_push][C] up, [streams][out_stride] and the lengths down -- which is what a caller with host buffers had
      before; `host`, ticks issued back to back from page-locked buffers, tick t collected with host_wait(1) behind tick t + 1's
      issue.  Prints per variant the ms per tick of every run, for `host` the wall-clock ms from collection to collection of one run
      and h2d_bytes / d2h_bytes per tick (mp3mi_feed_host_io_stats), and the workgroups k_feed_lanes and k_feed_packed launch per
      tick (from the descriptors' arithmetic).  The packed buffer is the first sum(n_push) samples of the rectangle: the same
      samples where every row pushes max_push (a, d), the same amount elsewhere (b).
Prints one JSON line per run: ms per tick, the parks and resumes per tick (from mp3mi_feed_lanes, host bookkeeping), the bytes
k_feed moves per tick (read + written, from the descriptors' arithmetic) and the library's source hash.

usage: feed_bench.py [--scenario a|b|c] [--host] [--lanes N [--packet P] [--host-time ROWS]] [--ticks 20] [--frames 32] [--streams 4096] [--reps 3]"""
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
    ap.add_argument("--scenario", default="a", choices=("a", "b", "c"))
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3, help="runs; the fastest counts (one more warms up)")
    ap.add_argument("--lanes", type=int, default=0, help="scenario d: that many lanes in front of the slots")
    ap.add_argument("--packet", type=int, default=0, help="scenario d: samples a lane pushes per tick")
    ap.add_argument("--host-time", type=int, default=0, help="with --lanes: rows per tick of the host-time measurement")
    ap.add_argument("--host", action="store_true", help="scenarios a, b, d on host buffers, beside the device tick with and without copies")
    a = ap.parse_args()
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    if a.host:
        if a.scenario == "c" or a.host_time:
            ap.error("--host takes scenarios a, b and d (--lanes)")
        return host(a, torch, mp3)
    if a.lanes:
        return host_time(a, torch, mp3) if a.host_time else lanes(a, torch, mp3)
    S, nf, ch, kbps, T = a.streams, a.frames, 2, 128, a.ticks
    rate = 48000 if a.scenario == "b" else 44100
    full = nf * 1152
    max_push = {"a": full, "b": 2 * 39 * 960, "c": full}[a.scenario]
    dev = torch.device("cuda:0")
    pcm = torch.empty((S, max_push * ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    mp3.synth_pcm_device(pcm, max_push, ch, rate)
    b = mp3.Batch(S, rate, ch, kbps, nf)
    out = torch.zeros((S, b.out_stride(nf)), dtype=torch.uint8, device=dev)
    out_len = torch.zeros(S, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rng = np.random.default_rng(1)
    every = np.ones(S, bool)
    odd = (np.arange(S) & 1).astype(bool)

    def pushes(t):
        if a.scenario == "a":
            return np.full(S, full, np.int32)
        if a.scenario == "b":
            return (960 * rng.integers(38, 40, S)).astype(np.int32)
        n = np.full(S, full, np.int32)
        n[odd] = 0 if t % 2 == 0 else full
        return n

    def run_feed(stats):
        feed = b.feeder(nf, max_push)
        pending, parked = np.zeros(S, np.int64), np.zeros(S, bool)
        parks = resumes = moved = 0
        for t in range(T):
            n = pushes(t)
            feed.tick(pcm, out, out_len, start=every if t == 0 else None, n_push=n)
            p, _, g, _ = feed.lanes()
            now = (g & 1).astype(bool)
            parks += int((now & ~parked).sum())
            resumes += int((parked & ~now).sum())
            parked = now
            moved += 2 * ch * 2 * int(n.sum() + (pending + n - p).clip(0, None).clip(None, pending).sum())  # pushed + ring -> row, read and written
            pending = p.astype(np.int64)
        stats.update(parks_per_tick=round(parks / T, 1), resumes_per_tick=round(resumes / T, 1), k_feed_bytes_per_tick=moved // T)
        return feed

    def run_slots():
        b.encode_slots(pcm[:, :full * ch].contiguous(), nf, out, out_len, start=every)
        for _ in range(T - 1):
            b.encode_slots(row, nf, out, out_len)

    row = pcm[:, :full * ch].contiguous()
    res = {}
    for name in ("feed",) + (("slots_continue",) if a.scenario == "a" else ()):
        best, stats = None, {}
        for r in range(a.reps + 1):
            b.sync()
            t0 = time.perf_counter()
            if name == "feed":
                feed = run_feed(stats)
                b.sync()
                ms = (time.perf_counter() - t0) * 1e3 / T
                feed.close()
            else:
                run_slots()
                b.sync()
                ms = (time.perf_counter() - t0) * 1e3 / T
                b.reset()
            if r > 0:
                best = ms if best is None else min(best, ms)
        res[name + "_ms"] = round(best, 3)
        res.update(stats)
    L = mp3.lib()
    print(json.dumps(dict(tool="feed_bench", scenario=a.scenario, streams=S, frames_per_tick=nf, ticks=T, rate=rate, channels=ch, kbps=kbps,
                          max_push=max_push, **res, source_hash=L.mp3mi_source_hash().decode(), version=L.mp3mi_version().decode())))
    b.close()


def lanes(a, torch, mp3):
    """scenario d"""
    S, N, nf, ch, kbps, T, rate = a.streams, a.lanes, a.frames, 2, 128, a.ticks, 48000
    full = nf * 1152
    ratio = max(N // S, 1)
    packet = a.packet or full // ratio
    dev = torch.device("cuda:0")
    pcm = torch.empty((N, packet * ch), dtype=torch.int16, device=dev)
    row = torch.empty((S, full * ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    mp3.synth_pcm_device(pcm, packet, ch, rate)
    mp3.synth_pcm_device(row, full, ch, rate)
    b = mp3.Batch(S, rate, ch, kbps, nf)
    out = torch.zeros((S, b.out_stride(nf)), dtype=torch.uint8, device=dev)
    out_len = torch.zeros(S, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    every = np.ones(S, bool)
    all_lanes = np.arange(N, dtype=np.int32)
    phase = all_lanes % ratio
    res, stats = {}, {}

    def run_feed():
        feed = b.feeder(nf, packet, lanes=N, ring_samples=full + 2 * packet)
        parked = np.zeros(N, bool)
        parks = resumes = waited = encoded = 0
        t0 = None
        for t in range(ratio + T):
            if t == ratio:  # every lane has STARTed and the first are ready: the timed ticks begin
                b.sync()
                t0 = time.perf_counter()
            if t < ratio:
                rows = all_lanes[phase <= t]
                sl = feed.tick_lanes(pcm[:len(rows)], out, out_len, rows, start=phase[rows] == t, n_push=np.full(len(rows), packet, np.int32))
            else:
                sl = feed.tick_lanes(pcm, out, out_len, all_lanes, n_push=np.full(N, packet, np.int32))
                g = feed.lanes()[2]
                now = (g & 1).astype(bool)
                parks += int((now & ~parked).sum())
                resumes += int((parked & ~now).sum())
                parked = now
                waited += int(((g & 8) != 0).sum())
                encoded += int((sl >= 0).sum())
        b.sync()
        ms = (time.perf_counter() - t0) * 1e3 / T
        feed.close()
        stats.update(parks_per_tick=round(parks / T, 1), resumes_per_tick=round(resumes / T, 1), waited_per_tick=round(waited / T, 1),
                     encoded_per_tick=round(encoded / T, 1))
        return ms

    def run_slots():
        b.encode_slots(row, nf, out, out_len, start=every)
        b.sync()
        t0 = time.perf_counter()
        for _ in range(T):
            b.encode_slots(row, nf, out, out_len)
        b.sync()
        ms = (time.perf_counter() - t0) * 1e3 / T
        b.reset()
        return ms

    for name, fn in (("feed_lanes", run_feed), ("slots_continue", run_slots)):
        res[name + "_ms"] = round(min([fn() for _ in range(a.reps + 1)][1:]), 3)
    L = mp3.lib()
    print(json.dumps(dict(tool="feed_bench", scenario="d", streams=S, lanes=N, packet=packet, frames_per_tick=nf, ticks=T, rate=rate, channels=ch,
                          kbps=kbps, **res, **stats, source_hash=L.mp3mi_source_hash().decode(), version=L.mp3mi_version().decode())))
    b.close()


def host(a, torch, mp3):
    """ticks on host buffers against the device tick, with and without synchronous copies around it"""
    S, nf, ch, kbps, T = a.streams, a.frames, 2, 128, a.ticks
    full, esz = nf * 1152, 4
    rng = np.random.default_rng(1)
    if a.lanes:
        name, N, rate = "d", a.lanes, 48000
        ratio = max(N // S, 1)
        max_push = a.packet or full // ratio
        ring, skip = full + 2 * max_push, ratio
        lane = np.arange(N, dtype=np.int32)
        plan = [(lane[lane % ratio <= t], lane[lane % ratio <= t] % ratio == t, None) for t in range(ratio)]
        plan += [(lane, None, None)] * T
    else:
        name, N, rate = a.scenario, S, 48000 if a.scenario == "b" else 44100
        max_push, ring, skip = (full, 0, 0) if name == "a" else (2 * 39 * 960, 0, 0)
        lane = np.arange(N, dtype=np.int32)
        plan = [(lane, np.ones(N, bool) if t == 0 else None, None if name == "a" else (960 * rng.integers(38, 40, N)).astype(np.int32)) for t in range(T)]
    plan = [(r, st, np.full(len(r), max_push, np.int32) if n is None else n) for r, st, n in plan]
    dev = torch.device("cuda:0")
    rect_d = torch.empty((N, max_push * ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    mp3.synth_pcm_device(rect_d, max_push, ch, rate)
    rect_h = torch.empty((N, max_push * ch), dtype=torch.int16).pin_memory()
    rect_h.copy_(rect_d)
    b = mp3.Batch(S, rate, ch, kbps, nf)
    stride = b.out_stride(nf)
    out_d = torch.zeros((S, stride), dtype=torch.uint8, device=dev)
    len_d = torch.zeros(S, dtype=torch.int32, device=dev)
    outs_h = [torch.zeros((S, stride), dtype=torch.uint8).pin_memory() for _ in range(3)]
    lens_h = [torch.zeros(S, dtype=torch.int32).pin_memory() for _ in range(3)]
    torch.cuda.synchronize()
    work = {}

    def run(variant):
        feed = b.feeder(nf, max_push, lanes=N, ring_samples=ring)
        marks, wg_lanes, wg_packed = [], 0, 0
        for t, (rows, st, n) in enumerate(plan):
            if t == skip:
                feed.host_wait(0) if variant == "host" and t else None
                b.sync()
                t0 = time.perf_counter()
                marks = [t0]
            R = len(rows)
            if variant == "host":
                lanes_t, _ = feed.tick_lanes_host(rect_h, outs_h[t % 3], lens_h[t % 3], rows, start=st, n_push=n)
                if t > skip:
                    feed.host_wait(1)
                    marks.append(time.perf_counter())
            else:
                if variant == "device_copies":
                    rect_d[:R].copy_(rect_h[:R])
                    torch.cuda.synchronize()
                sl = feed.tick_lanes(rect_d[:R], out_d, len_d, rows, start=st, n_push=n)
                if variant == "device_copies":
                    outs_h[0].copy_(out_d)
                    lens_h[0].copy_(len_d)
                    torch.cuda.synchronize()
                if t >= skip and "wg" not in work:  # what the two kernels launch for this tick: a descriptor per lane that pushes or takes
                    take = np.zeros(N, np.int64)
                    take[sl[sl >= 0]] = full
                    longest = np.maximum(take[rows], n) * esz
                    per = 256 * 16 * 4
                    wg_lanes += R * int(min(max(-(-int(longest.max()) // per), 1), 8))
                    wg_packed += int(np.clip(-(-longest // per), 1, 8).sum())
        if variant == "host":
            feed.host_wait(0)
            marks.append(time.perf_counter())
        b.sync()
        ms = (time.perf_counter() - t0) * 1e3 / T
        extra = {}
        if variant == "host":
            st = feed.host_io_stats()
            extra = dict(h2d_bytes_per_tick=st["h2d_bytes"] / st["calls"], d2h_bytes_per_tick=st["d2h_bytes"] / st["calls"],
                         h2d_ms_per_tick=round(st["h2d_ms"] / st["calls"], 3), d2h_ms_per_tick=round(st["d2h_ms"] / st["calls"], 3),
                         per_tick_ms=[round((y - x) * 1e3, 3) for x, y in zip(marks, marks[1:])])
        elif "wg" not in work:
            work["wg"] = dict(k_feed_lanes_workgroups_per_tick=wg_lanes // T, k_feed_packed_workgroups_per_tick=wg_packed // T)
        feed.close()
        return ms, extra

    variants = ("device", "device_copies", "host")
    ms = {v: [] for v in variants}
    extra = {}
    for r in range(a.reps + 1):  # the variants alternate; the first round warms up
        for v in variants:
            m, e = run(v)
            if r > 0:
                ms[v].append(round(m, 3))
                extra.update(e)
    L = mp3.lib()
    print(json.dumps(dict(tool="feed_bench", mode="host", scenario=name, streams=S, lanes=N, max_push=max_push, frames_per_tick=nf, ticks=T, rate=rate,
                          channels=ch, kbps=kbps, call_hold=os.environ.get("MP3MI_CALL_HOLD", "default"),
                          **{v + "_ms": ms[v] for v in variants}, **{v + "_ms_median": float(np.median(ms[v])) for v in variants},
                          copies_h2d_bytes_per_tick=len(plan[-1][0]) * max_push * esz, copies_d2h_bytes_per_tick=S * (stride + 4), **extra, **work.get("wg", {}),
                          source_hash=L.mp3mi_source_hash().decode(), version=L.mp3mi_version().decode())))
    b.close()


def host_time(a, torch, mp3):
    """wall clock around mp3mi_feed_tick_lanes, the device idle before each call"""
    S, nf, ch, kbps, rate, R, T = a.streams, a.frames, 2, 128, 48000, a.host_time, 50
    full = nf * 1152
    dev = torch.device("cuda:0")
    pcm = torch.empty((R, full * ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    mp3.synth_pcm_device(pcm, full, ch, rate)
    res = {}
    for N in (a.lanes, 4096):
        b = mp3.Batch(S, rate, ch, kbps, nf)
        out = torch.zeros((S, b.out_stride(nf)), dtype=torch.uint8, device=dev)
        out_len = torch.zeros(S, dtype=torch.int32, device=dev)
        feed = b.feeder(nf, full, lanes=N, max_rows=R)
        one = np.ones(R, bool)
        n = np.full(R, full, np.int32)
        us = []
        for t in range(T + 5):
            rows = np.sort((np.arange(R, dtype=np.int64) * (N // R) + t * 37) % N).astype(np.int32)  # spread over the lane table
            b.sync()
            t0 = time.perf_counter()
            feed.tick_lanes(pcm, out, out_len, rows, start=one, end=one, n_push=n)
            us.append((time.perf_counter() - t0) * 1e6)
        b.sync()
        feed.close()
        b.close()
        res["us_per_call_%d" % N] = round(float(np.median(us[5:])), 1)
    L = mp3.lib()
    print(json.dumps(dict(tool="feed_bench", scenario="host_time", streams=S, rows=R, frames_per_tick=nf, **res,
                          ratio=round(res["us_per_call_%d" % a.lanes] / res["us_per_call_4096"], 3),
                          source_hash=L.mp3mi_source_hash().decode(), version=L.mp3mi_version().decode())))


if __name__ == "__main__":
    main()
