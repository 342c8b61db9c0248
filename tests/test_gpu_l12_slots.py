"""Continuous batching for Layers I and II on the MI355X (mp3mi_l12_batch_encode_slots, include/mp3mi_l12.h): the churn plans of
tests/test_l12_slots.py over 64 slots, a full-width server loop, per-slot calls issued back to back without a sync -- the control
ring's test: the emulator runs every launch where it is issued and cannot show it -- and the torch binding."""
import importlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from l12_slots import END, START, churn, history_cleared
from mp3common import l12_signal, l12_spf, oracle_l12

pytestmark = pytest.mark.gpu
SEED = 0x6D70336D


@pytest.mark.parametrize("layer", [1, 2])
def test_churn_at_the_smallest_calls_gpu(product, oracle, layer):
    done = churn(product, oracle, layer, 64, seed=layer)
    assert len(done) >= 2 * 64


@pytest.mark.parametrize("layer", [1, 2])
def test_history_is_cleared_at_start_gpu(product, oracle, layer):
    history_cleared(product, oracle, layer, S=64)


def churn_schedule(S, n_calls, full, seed):
    """a seeded server loop: every slot STARTs in the first call; in every later call 1/32 of the slots END -- on a random length,
    the first of them with 0 samples and the second on a full call -- and the slots that ENDed two calls before START: a slot
    stays closed for one call in between.  Returns per call (ctl, n_samples)."""
    rng = np.random.default_rng(seed)
    open_ = np.ones(S, bool)
    ended = []  # the slots every call ended
    out = [(np.full(S, START, np.uint8), np.full(S, full, np.int32))]
    for _ in range(1, n_calls):
        start = np.zeros(S, bool)
        if len(ended) >= 2:
            start[ended[-2]] = True
        ending = rng.choice(np.flatnonzero(open_ | start), S // 32, replace=False)  # (a slot that STARTs now may END now: a one-call file)
        if start.any():  # the one with 0 samples is a slot that STARTs, where there is one: an empty file
            s0 = np.flatnonzero(start)[0]
            ending = np.concatenate(([s0], ending[ending != s0]))[:S // 32]
        ns = np.where(open_ | start, full, 0).astype(np.int32)
        ns[ending] = rng.integers(0, full + 1, len(ending))
        ns[ending[0]], ns[ending[1]] = 0, full
        ctl = np.where(start, START, 0).astype(np.uint8)
        ctl[ending] |= END
        out.append((ctl, ns))
        open_ |= start
        open_[ending] = False
        ended.append(ending)
    return out


def tick_run(product, layer, S, nf, sched, sync_each, kbps):
    """Runs the schedule through BatchL12.encode_slots, every call with output buffers of its own: the stream a slot STARTs in call
    k reads source row s from sample k * nf * frame on.  Returns the finished streams [(slot, first sample, samples, bytes)], the
    per-call (rows, lengths) and the source."""
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    dev = torch.device("cuda:0")
    ch, rate, n_calls, full = 2, 44100, len(sched), nf * l12_spf(layer)
    src = torch.empty((S, n_calls * full * ch), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    assert product.lib.mp3mi_synth_pcm_device(src.data_ptr(), S, n_calls * full, ch, rate, 700, SEED) == 0
    b = mp3.BatchL12(layer, S, rate, ch, kbps, nf)
    stride = b.out_stride(nf)
    pcms = [src[:, k * full * ch:(k + 1) * full * ch].contiguous() for k in range(n_calls)]
    outs = [torch.full((S, stride), 0xA5, dtype=torch.uint8, device=dev) for _ in range(n_calls)]
    lens = [torch.full((S,), -1, dtype=torch.int32, device=dev) for _ in range(n_calls)]
    torch.cuda.synchronize()
    frames = np.full(S, -1, np.int64)
    for k, (ctl, ns) in enumerate(sched):
        b.encode_slots(pcms[k], nf, outs[k], lens[k], start=ctl & START > 0, end=ctl & END > 0, n_samples=ns)
        if sync_each:
            b.sync()
        frames = np.where(ctl & START > 0, 0, frames)
        frames = np.where(ctl & END > 0, -1, np.where(frames >= 0, frames + nf, frames))
        assert (b.slot_frames() == frames).all(), k
    b.sync()
    b.close()
    got_o = [o.cpu().numpy() for o in outs]
    got_l = [x.cpu().numpy() for x in lens]
    first, acc, done = [None] * S, [b""] * S, []
    for k, (ctl, ns) in enumerate(sched):
        for s in range(S):
            if ctl[s] & START:
                first[s], acc[s] = k, b""
            if first[s] is None:
                assert got_l[k][s] == 0 and (got_o[k][s] == 0xA5).all(), (k, s)
                continue
            acc[s] += got_o[k][s, :got_l[k][s]].tobytes()
            if ctl[s] & END:
                done.append((s, first[s] * full, (k - first[s]) * full + int(ns[s]), acc[s]))
                first[s] = None
    return done, (got_o, got_l), src


@pytest.mark.parametrize("layer,nf", [(2, 4), (1, 12)])
def test_full_width_ticks_gpu(product, oracle, layer, nf):
    """4096 slots, 6 ticks, 1/32 of the slots ENDing and as many STARTing per tick: every ended stream equals the library's own
    ragged whole-file call (one batch), 32 of them spread over the batch -- the empty and the longest among them -- the oracle"""
    import torch
    S, kbps, ch = 4096, 192 if layer == 1 else 128, 2
    spf = l12_spf(layer)
    sched = churn_schedule(S, 6, nf * spf, 20261019 + layer)
    done, _, src = tick_run(product, layer, S, nf, sched, True, kbps)
    N = len(done)
    assert N == 5 * (S // 32)
    max_nf = 6 * nf
    pcm = torch.zeros((N, max_nf * spf * ch), dtype=torch.int16, device=src.device)
    for j, (s, a, n, _) in enumerate(done):
        pcm[j, :n * ch] = src[s, a * ch:(a + n) * ch]
    ns = torch.tensor([n for _, _, n, _ in done], dtype=torch.int32, device=src.device)
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    b = mp3.BatchL12(layer, N, 44100, ch, kbps, max_nf)
    out = torch.zeros((N, b.out_stride(max_nf)), dtype=torch.uint8, device=src.device)
    ln = torch.zeros(N, dtype=torch.int32, device=src.device)
    b.encode(pcm, max_nf, out, ln, n_samples=ns)
    b.sync()
    b.close()
    out_h, ln_h = out.cpu().numpy(), ln.cpu().numpy()
    bad = [j for j in range(N) if out_h[j, :ln_h[j]].tobytes() != done[j][3]]
    assert not bad, "%d of %d streams differ from the ragged call (first: slot %d, %d samples)" % (len(bad), N, done[bad[0]][0], done[bad[0]][2])
    order = sorted(range(N), key=lambda j: done[j][2])
    by_slot = sorted(range(N), key=lambda j: done[j][0])
    pick = sorted(set(order[:3] + order[-3:] + [by_slot[len(by_slot) * q // 26] for q in range(26)]))
    assert len(pick) >= 26 and done[order[0]][2] == 0
    src_h = {j: src[done[j][0], done[j][1] * ch:(done[j][1] + done[j][2]) * ch].cpu().numpy() for j in pick}
    with ThreadPoolExecutor(max_workers=8) as ex:
        refs = list(ex.map(lambda j: oracle_l12(oracle, layer, 44100, kbps, "s", src_h[j])[0], pick))
    for j, ref in zip(pick, refs):
        assert done[j][3] == ref, "slot %d, %d samples" % (done[j][0], done[j][2])


@pytest.mark.parametrize("layer,nf", [(2, 2), (1, 6)])
def test_back_to_back_without_sync_gpu(product, layer, nf):
    """five per-slot calls, each with its own output buffers and its own ctl / n_samples, issued without a sync between them:
    the bytes of the same five calls synced one by one.  The control block exists twice and an entry's fence makes the host wait
    before it writes it again; without that a call's kernels would read the arrays of a later call."""
    S = 2048
    sched = churn_schedule(S, 5, nf * l12_spf(layer), 7 + layer)
    a_done, (a_o, a_l), _ = tick_run(product, layer, S, nf, sched, True, 192 if layer == 1 else 128)
    b_done, (b_o, b_l), _ = tick_run(product, layer, S, nf, sched, False, 192 if layer == 1 else 128)
    for k in range(5):
        assert (a_l[k] == b_l[k]).all(), "call %d: lengths differ" % k
        assert (a_o[k] == b_o[k]).all(), "call %d: bytes differ" % k
    assert len(a_done) == 4 * (S // 32) and [d[3] for d in a_done] == [d[3] for d in b_done]


def test_binding_gpu(product, oracle):
    """BatchL12.encode_slots / encode_next / flush / reset / slot_frames on torch tensors: three slots of Layer II"""
    import torch
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
    dev = torch.device("cuda:0")
    layer, S, nf, rate, ch, kbps = 2, 3, 2, 44100, 2, 128
    full = nf * 1152
    row = full * ch
    src = [l12_signal(3 * full, ch, 40 + s) for s in range(S)]
    b = mp3.BatchL12(layer, S, rate, ch, kbps, nf, mode=1)
    stride = b.out_stride(nf)
    got = [b""] * S

    def step(fn, rows, **kw):
        pcm = torch.from_numpy(np.stack(rows)).to(dev)
        out = torch.zeros((S, stride), dtype=torch.uint8, device=dev)
        ln = torch.zeros(S, dtype=torch.int32, device=dev)
        fn(pcm, nf, out, ln, **kw)
        b.sync()
        o, n = out.cpu().numpy(), ln.cpu().numpy()
        return [o[s, :n[s]].tobytes() for s in range(S)]

    assert list(b.slot_frames()) == [-1] * S
    noise = np.full(row, 32767, np.int16)
    o = step(b.encode_slots, [src[0][:row], noise, src[2][:row]], start=[True, False, True])
    assert o[1] == b"" and list(b.slot_frames()) == [nf, -1, nf]
    got = [got[s] + o[s] for s in range(S)]
    r1 = np.zeros(row, np.int16)
    r1[:777 * ch] = src[1][:777 * ch]
    o = step(b.encode_slots, [src[0][row:2 * row], r1, src[2][row:2 * row]], start=[False, True, False], end=[False, True, False],
             n_samples=[full, 777, full])
    assert list(b.slot_frames()) == [2 * nf, -1, 2 * nf]
    got = [got[s] + o[s] for s in range(S)]
    o = step(b.encode_next, [src[0][2 * row:3 * row], noise, src[2][2 * row:3 * row]])
    assert o[1] == b"" and list(b.slot_frames()) == [3 * nf, -1, 3 * nf]
    got = [got[s] + o[s] for s in range(S)]
    out = torch.zeros((S, stride), dtype=torch.uint8, device=dev)
    ln = torch.zeros(S, dtype=torch.int32, device=dev)
    b.flush(out, ln)
    b.sync()
    assert ln.cpu().tolist() == [1, 0, 1] and list(b.slot_frames()) == [-1] * S
    got = [got[0] + b"\0", got[1], got[2] + b"\0"]
    want = [oracle_l12(oracle, layer, rate, kbps, "j", p)[0] for p in (src[0], src[1][:777 * ch], src[2])]
    assert got == want
    b.encode_slots(torch.from_numpy(np.stack([src[s][:row] for s in range(S)])).to(dev), nf, out, ln, start=[True] * S)
    b.reset()
    assert list(b.slot_frames()) == [-1] * S
    b.close()
