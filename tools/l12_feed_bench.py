#!/usr/bin/env python3
"""Times the feeder of Layers I and II (mp3mi_l12_feed_tick, include/mp3mi_l12.h) in front of a slot batch on the device.

4096 stereo slots, 44.1 kHz, Layer I at 192 or Layer II at 128 kbps, ticks of 32 frames on resident push rows, 20 ticks issued back to
back (one sync at the end of a run).  Without --lanes: one lane per slot, every lane pushes exactly a tick in every tick -- all ready,
nobody leaves a slot.  With --lanes N: N lanes in front of the slots, every lane pushes one packet (--packet samples, default 960) in
every tick, so a lane is ready every (tick / packet)-th tick and every tick lends the slots to other lanes: each encoding lane is
resumed out of its ring.  The lanes START staggered over the first tick / packet ticks; those and as many more, in which every
lane encodes for the first time, are not timed.  Beside either the plain
mp3mi_l12_batch_encode_slots tick of the same library on resident full rows, every slot continuing (slots_continue_ms): the floor.
Prints one JSON line: ms per tick of every run and their medians, the ratio over the floor, the lanes that encoded, left a slot and
were resumed per tick (from mp3mi_l12_feed_lanes and the returned slot map: host bookkeeping) and the library's source hash.

usage: l12_feed_bench.py --layer 1|2 [--lanes N [--packet 960]] [--ticks 20] [--frames 32] [--streams 4096] [--reps 3]"""
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
    ap.add_argument("--layer", type=int, required=True, choices=(1, 2))
    ap.add_argument("--lanes", type=int, default=0, help="that many lanes in front of the slots (default: one per slot, a tick per push)")
    ap.add_argument("--packet", type=int, default=960, help="with --lanes: samples a lane pushes per tick")
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3, help="runs of each kind, alternating (one more warms up)")
    a = ap.parse_args()
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    S, nf, ch, T, rate = a.streams, a.frames, 2, a.ticks, 44100
    kbps = 192 if a.layer == 1 else 128
    full = nf * mp3.L12_FRAME_SAMPLES[a.layer]
    N = a.lanes or S
    packet = a.packet if a.lanes else full
    period = -(-full // packet)  # ticks from one encode of a lane to the next
    dev = torch.device("cuda:0")
    pcm = torch.empty((N, packet * ch), dtype=torch.int16, device=dev)
    row = torch.empty((S, full * ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    mp3.synth_pcm_device(pcm, packet, ch, rate)
    mp3.synth_pcm_device(row, full, ch, rate)
    b = mp3.BatchL12(a.layer, S, rate, ch, kbps, nf)
    out = torch.zeros((S, b.out_stride(nf)), dtype=torch.uint8, device=dev)
    out_len = torch.zeros(S, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    all_lanes = np.arange(N, dtype=np.int32)
    phase = all_lanes % period if a.lanes else np.zeros(N, np.int32)
    warm = 2 * period if a.lanes else 1  # (every lane has encoded once: the timed ticks resume parked streams, they START none)
    stats = {}

    def run_feed():
        feed = b.feeder(nf, packet, lanes=N, ring_samples=full + 2 * packet)
        parked = np.zeros(N, bool)
        parks = resumes = waited = encoded = 0
        t0 = None
        for t in range(warm + T):
            if t == warm:  # the timed ticks begin
                b.sync()
                t0 = time.perf_counter()
            if t < period:
                rows = all_lanes[phase <= t]
                feed.tick(pcm[:len(rows)], out, out_len, rows, start=phase[rows] == t, n_push=np.full(len(rows), packet, np.int32))
                continue
            sl = feed.tick(pcm, out, out_len, all_lanes, n_push=np.full(N, packet, np.int32))
            if t < warm:
                parked = (feed.lanes()[2] & 1).astype(bool)
                continue
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
        stats.update(encoded_per_tick=round(encoded / T, 1), parks_per_tick=round(parks / T, 1), resumes_per_tick=round(resumes / T, 1),
                     waited_per_tick=round(waited / T, 1))
        return ms

    def run_slots():
        b.encode_slots(row, nf, out, out_len, start=np.ones(S, bool))
        b.sync()
        t0 = time.perf_counter()
        for _ in range(T):
            b.encode_slots(row, nf, out, out_len)
        b.sync()
        ms = (time.perf_counter() - t0) * 1e3 / T
        b.reset()
        return ms

    ms = {"feed": [], "slots_continue": []}
    for r in range(a.reps + 1):  # the two kinds alternate; the first round warms up
        for name, fn in (("feed", run_feed), ("slots_continue", run_slots)):
            m = fn()
            if r > 0:
                ms[name].append(round(m, 3))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    L = mp3.lib()
    print(json.dumps(dict(tool="l12_feed_bench", layer=a.layer, streams=S, lanes=N, packet=packet, frames_per_tick=nf, ticks=T, rate=rate, channels=ch,
                          kbps=kbps, feed_ms=ms["feed"], slots_continue_ms=ms["slots_continue"], feed_ms_median=med["feed"],
                          slots_continue_ms_median=med["slots_continue"], ratio_over_floor=round(med["feed"] / med["slots_continue"], 4), **stats,
                          source_hash=L.mp3mi_source_hash().decode(), version=L.mp3mi_version().decode())))
    b.close()


if __name__ == "__main__":
    main()
