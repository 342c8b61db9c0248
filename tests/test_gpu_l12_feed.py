"""The feeder of Layers I and II on the device (mp3mi_l12_feed_*, include/mp3mi_l12.h): k12_feed alone against the numpy model, and
the scenarios of tests/l12_feed.py -- judged by the CPU oracle and the library's own ragged whole-file call, with a Python model of
the scheduler beside every tick -- at sizes the emulated build does not run: 64 slots under 160 lanes, ticks issued back to back
without a sync, two feeders on one device, and the torch binding in a seeded server loop."""
import importlib

import numpy as np
import pytest

from l12_feed import END, START, FeedRun, Model, back_to_back_case, check, cuts, kernel_case, more_lanes_case
from mp3common import oracle_l12

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", [384, 1152])
@pytest.mark.parametrize("ch", [1, 2])
def test_l12_feed_kernel_gpu(product, ch, row):
    kernel_case(product, ch, row)


@pytest.mark.parametrize("layer", [1, 2])
def test_more_lanes_than_slots_wide_gpu(product, oracle, layer):
    more_lanes_case(product, oracle, layer, 1, S=64, n_lanes=160)


@pytest.mark.parametrize("layer", [1, 2])
def test_eight_ticks_back_to_back_gpu(product, oracle, layer):
    back_to_back_case(product, oracle, layer)


def test_two_feeders_on_one_device_gpu(product, oracle):
    """a Layer I and a Layer II batch, each with a feeder, their ticks interleaved"""
    one = FeedRun(product, 1, 3, 5, 44100, "s", 192, 2, 768, ring=3 * 768)
    two = FeedRun(product, 2, 2, 4, 48000, "je", 128, 1, 1152, ring=3 * 1152)
    try:
        todo = []
        for run in (one, two):
            full = run.full
            sts = [run.stream(720 + i, 3 * full - 7 - i, kbps=run.kbps[0]) for i in range(run.n_lanes)]
            todo.append((run, sts, [[full] + cuts(len(st.pcm) // run.ch - full, (960, 160, full), full) for st in sts]))
        first = True
        while any(any(p for p in pieces) or any(l.open for l in run.m.lane) for run, _, pieces in todo):
            for run, sts, pieces in todo:
                feeds = {}
                for i, p in enumerate(pieces):
                    if p and (first or run.m.lane[i].pending + p[0] <= run.capacity):
                        n = p.pop(0)
                        feeds[i] = (sts[i], (START if first else 0) | (0 if p else END), n)
                run.tick(feeds)
            first = False
            assert one.ticks < 200
        for run, sts, _ in todo:
            assert run.m.over > 0 and run.m.resumes > 0
            check(run, oracle, sts)
    finally:
        one.close()
        two.close()


@pytest.mark.parametrize("layer", [1, 2])
def test_torch_binding_server_loop_gpu(product, oracle, layer):
    """BatchL12.feeder / FeedL12.tick: ten lanes over four slots receive packets of 960 samples at seeded times; every lane's bytes,
    gathered through the returned slot -> lane array, are the oracle's file"""
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    S, n_lanes, rate, ch, tick = 4, 10, 44100, 2, 2
    kbps, spf = (192, 384) if layer == 1 else (128, 1152)
    full = tick * spf
    dev = torch.device("cuda:0")
    b = mp3.BatchL12(layer, S, rate, ch, kbps, tick, mode=1)
    feed = b.feeder(tick, 960, lanes=n_lanes, ring_samples=full + 4 * 960)
    assert feed.n_lanes == n_lanes and feed.capacity == full + 4 * 960
    m = Model(S, n_lanes, tick, spf, feed.capacity, [kbps] * S)
    rng = np.random.default_rng(31 + layer)
    from mp3common import l12_signal
    length = [int(rng.integers(2, 4)) * full + int(rng.integers(1, 960)) for _ in range(n_lanes)]
    src = [l12_signal(n, ch, 740 + i, rate) for i, n in enumerate(length)]
    pos, started, got = [0] * n_lanes, [False] * n_lanes, [b""] * n_lanes
    stride = b.out_stride(tick)
    out = torch.zeros((S, stride), dtype=torch.uint8, device=dev)
    out_len = torch.zeros(S, dtype=torch.int32, device=dev)
    for t in range(400):
        rows, packets = [], []
        for i in range(n_lanes):
            n = min(960, length[i] - pos[i])
            if pos[i] < length[i] and rng.random() < 0.7 and (not started[i] or m.lane[i].pending + n <= feed.capacity):
                rows.append(i)
                packets.append((n, not started[i], pos[i] + n == length[i]))
        pcm = torch.zeros((max(len(rows), 1), 960 * ch), dtype=torch.int16)
        for r, (i, (n, _, _)) in enumerate(zip(rows, packets)):
            pcm[r, :n * ch] = torch.from_numpy(src[i][pos[i] * ch:(pos[i] + n) * ch])
            pos[i] += n
            started[i] = True
        sl = feed.tick(pcm.to(dev) if rows else None, out, out_len, rows, start=[p[1] for p in packets], end=[p[2] for p in packets],
                       n_push=[p[0] for p in packets], kbps=[kbps if p[1] else 0 for p in packets])
        enc = m.tick({i: ((START if p[1] else 0) | (END if p[2] else 0), p[0], kbps if p[1] else 0) for i, p in zip(rows, packets)})
        want = [-1] * S
        for i, s, _, _, _ in enc:
            want[s] = i
        assert list(sl) == want, (t, list(sl), want)
        assert list(feed.lanes()[2]) == m.flags(), t
        b.sync()
        o, n = out.cpu().numpy(), out_len.cpu().numpy()
        for s, i in enumerate(want):
            if i >= 0:
                got[i] += o[s, :int(n[s])].tobytes()
            else:
                assert n[s] == 0
        if all(p == n_ for p, n_ in zip(pos, length)) and not any(l.open for l in m.lane):
            break
    assert feed.lanes()[3] == 0 and m.over > 0 and m.resumes > 0
    feed.close()
    b.close()
    for i in range(n_lanes):
        assert got[i] == oracle_l12(oracle, layer, rate, kbps, "j", src[i])[0], i
