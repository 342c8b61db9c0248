#!/usr/bin/env python3
"""Times per-slot streaming (mp3mi_batch_encode_slots) against whole-batch streaming (mp3mi_batch_encode_next) on the device.

4096 stereo slots, 44.1 kHz, 128 kbps, calls of 32 frames on resident PCM, issued back to back (one sync at the end of a run):
  (a) encode_next                                  every stream goes on
  (b) encode_slots, every slot continuing          the per-slot path with nothing to start or end
  (c) encode_slots with churn                      in every call 1/32 of the slots END (at random partial lengths) and as
                                                   many closed slots START
Prints one JSON line: ms per call of each case and the library's source hash.

usage: slots_bench.py [--calls 20] [--frames 32] [--streams 4096] [--reps 3]"""
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
    a = ap.parse_args()
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    S, nf, rate, ch, kbps = a.streams, a.frames, 44100, 2, 128
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

    def run_next():
        for _ in range(a.calls):
            b.encode_next(pcm, nf, out, out_len)

    def run_continue():
        b.encode_slots(pcm, nf, out, out_len, start=every)
        for _ in range(a.calls - 1):
            b.encode_slots(pcm, nf, out, out_len)

    def run_churn():
        b.encode_slots(pcm, nf, out, out_len, start=every)
        closed = np.zeros(S, bool)
        for _ in range(a.calls - 1):
            start = closed.copy()
            cand = np.flatnonzero(~closed)
            end = np.zeros(S, bool)
            end[rng.choice(cand, S // 32, replace=False)] = True
            ns = np.full(S, full, np.int32)
            ns[end] = rng.integers(0, full + 1, int(end.sum()))
            b.encode_slots(pcm, nf, out, out_len, start=start, end=end, n_samples=ns)
            closed = end

    cases = (("encode_next", run_next), ("slots_continue", run_continue), ("slots_churn", run_churn))
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
    b.close()
    print(json.dumps({"tool": "slots_bench", "streams": S, "frames_per_call": nf, "calls": a.calls, "rate": rate, "channels": ch,
                      "kbps": kbps, "ms_per_call": res,
                      "continue_vs_next": round(res["slots_continue"] / res["encode_next"], 4),
                      "churn_vs_continue": round(res["slots_churn"] / res["slots_continue"], 4),
                      "source_hash": mp3.lib().mp3mi_source_hash().decode()}))


if __name__ == "__main__":
    main()
