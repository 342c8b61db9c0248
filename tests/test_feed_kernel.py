"""k_feed alone (mp3mi_debug_feed, include/mp3mi.h): the kernel that cuts a feeder's rows out of the lanes' device FIFOs, against a
numpy model of what mp3mi.h says it moves, on the heads, fills, pushes and takes at which its alignment paths and the ring's wrap
change.  Rows, rings and push rows lie between canaries; whatever the model does not write must still hold the canary, or what it
held before."""
import ctypes
import itertools

import numpy as np
import pytest

CANARY = 0x5A5A
FULL, MAX_PUSH = 1152, 1500
CAP = FULL + MAX_PUSH
RING_PITCH, ROW_PITCH, PUSH_PITCH = CAP + 20, FULL + 16, MAX_PUSH + 7  # (16-byte multiples for both channel counts; the push rows' odd)


def lanes():
    """every (head, pending, push, take) of the listed values that the feeder's rules allow, between two idle lanes"""
    out = [(0, 0, 0, 0)]
    for head, pending, push in itertools.product((0, 1, 7, 8, CAP - 3, CAP - 1), (0, 1, 7, 8, 9, 1151, 1152), (0, 1, 8, 9, 1500)):
        have = pending + push
        assert have <= CAP
        for take in sorted({0, FULL, have}):
            if take <= have and take <= FULL:
                out.append((head, pending, push, take))
    return out + [(0, 0, 0, 0)]


def model(desc, ring, push, rows):
    """ring [S, RING_PITCH, C], push [S, PUSH_PITCH, C], rows [S, ROW_PITCH, C]: what they hold afterwards"""
    ring, rows = ring.copy(), rows.copy()
    for s, (head, pending, n, take) in enumerate(desc):
        stream = np.concatenate([ring[s, (head + np.arange(pending)) % CAP], push[s, :n]])
        rows[s, :take] = stream[:take]
        u = max(take - pending, 0)  # pushed samples the row took
        ring[s, (head + pending + u + np.arange(n - u)) % CAP] = push[s, u:n]
    return ring, rows


def feed_case(mp, ch):
    L = mp.lib
    L.mp3mi_debug_feed.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                                        ctypes.c_void_p, ctypes.c_size_t]
    desc = lanes()
    S = len(desc)
    assert S == 416  # 210 (head, pending, push) with one to three takes each, and the two idle lanes
    ring = np.full((S, RING_PITCH, ch), CANARY, np.int16)
    push = np.full((S, PUSH_PITCH, ch), CANARY, np.int16)
    rows = np.full((S, ROW_PITCH, ch), CANARY, np.int16)
    chan = np.arange(ch) * 5000
    for s, (head, pending, n, take) in enumerate(desc):
        i = np.arange(pending)
        ring[s, (head + i) % CAP] = (1 + (s * 7 + i) % 5000)[:, None] + chan      # 1 .. 10000: never the canary
        push[s, :n] = -(1 + (s * 13 + np.arange(n)) % 5000)[:, None] - chan       # negative: never a ring sample
    want_ring, want_rows = model(desc, ring, push, rows)
    d = np.ascontiguousarray(desc, dtype=np.uint32)
    got_ring, got_push, got_rows = ring.copy(), push.copy(), rows.copy()
    rc = L.mp3mi_debug_feed(ch, S, CAP, FULL, d.ctypes.data, got_ring.ctypes.data, RING_PITCH, got_push.ctypes.data, PUSH_PITCH,
                            got_rows.ctypes.data, ROW_PITCH)
    assert rc == 0, rc
    assert np.array_equal(got_push, push)
    for s in range(S):
        assert np.array_equal(got_rows[s], want_rows[s]), ("row", desc[s])
        assert np.array_equal(got_ring[s], want_ring[s]), ("ring", desc[s])
    assert (want_rows[:, FULL:] == CANARY).all() and (want_ring[:, CAP:] == CANARY).all()  # (the model keeps inside its records)
    # a descriptor outside the rules launches nothing
    for bad in [(CAP, 0, 0, 0), (0, CAP, 1, 0), (0, 5, 5, 11), (0, 1152, 100, 1153), (0, 0, PUSH_PITCH + 1, 0)]:
        d1 = np.ascontiguousarray([bad], dtype=np.uint32)
        assert L.mp3mi_debug_feed(ch, 1, CAP, FULL, d1.ctypes.data, got_ring.ctypes.data, RING_PITCH, got_push.ctypes.data, PUSH_PITCH,
                                  got_rows.ctypes.data, ROW_PITCH) == -1, bad
    assert L.mp3mi_debug_feed(ch, 1, CAP, FULL, d.ctypes.data, got_ring.ctypes.data, CAP + 1, got_push.ctypes.data, PUSH_PITCH,
                              got_rows.ctypes.data, ROW_PITCH) == -1  # a ring pitch that is no multiple of 16 bytes


@pytest.mark.parametrize("ch", [1, 2])
def test_feed_kernel_emulated(emu, ch):
    feed_case(emu, ch)


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [1, 2])
def test_feed_kernel_gpu(product, ch):
    feed_case(product, ch)
