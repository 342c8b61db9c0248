#!/usr/bin/env python3
"""Times the feeder (mp3mi_feed_tick, include/mp3mi.h) in front of a slot batch on the device.

4096 stereo slots, 44.1 kHz, 128 kbps, ticks of 32 frames on resident push rows, 20 ticks issued back to back (one sync at the end
of a run), three scenarios (--scenario):
  a   every lane pushes exactly a tick: all ready, nobody is parked -- beside it the plain mp3mi_batch_encode_slots tick of the same
      library on the same samples, every slot continuing (slots_continue_ms): the difference is what the feeder costs
  b   48 kHz packets of 960 samples, 38 or 39 packets a tick at random (a tick is 38.4): lanes run short and sit out.  (38.5 on
      average: a lane's backlog creeps up by a tenth of a packet per tick, so the lanes are sized for two ticks' packets)
  c   half of the lanes (the odd ones) push nothing every other tick: they are short then, parked, and resume the tick after
Prints one JSON line per run: ms per tick, the parks and resumes per tick (from mp3mi_feed_lanes, host bookkeeping), the bytes
k_feed moves per tick (read + written, from the descriptors' arithmetic) and the library's source hash.

usage: feed_bench.py [--scenario a|b|c] [--ticks 20] [--frames 32] [--streams 4096] [--reps 3]"""
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
    a = ap.parse_args()
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
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


if __name__ == "__main__":
    main()
