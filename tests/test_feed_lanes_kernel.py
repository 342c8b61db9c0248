"""k_feed_lanes alone (mp3mi_debug_feed_lanes, include/mp3mi.h): the kernel that cuts the rows of a tick of a feeder with more lanes
than slots -- k_feed over a LIST of lanes, each with a ring of its own, a push row and a slot's row named in its descriptor.  The 416
descriptors of test_feed_kernel.py (the heads, fills, pushes and takes at which the alignment paths and the ring's wrap change) in a
shuffled order, on shuffled lanes, push rows and slots, with lanes, push rows and slots that no descriptor names in between; a numpy
model says what the three arrays hold afterwards, and whatever it does not write must hold what it held."""
import ctypes

import numpy as np
import pytest

from test_feed_kernel import CANARY, CAP, FULL, MAX_PUSH, lanes

ROW_PITCH, PUSH_PITCH = FULL + 16, MAX_PUSH + 7  # (the rows' a 16-byte multiple for both channel counts; the push rows' odd)


def bind(mp):
    L = mp.lib
    L.mp3mi_debug_feed_lanes.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                                              ctypes.c_void_p, ctypes.c_size_t]
    return L


def call(L, ch, desc, cap, ring, ring_pitch, push, rows, row_samples=FULL, push_pitch=PUSH_PITCH):
    d = np.ascontiguousarray(desc, dtype=np.uint32).reshape(-1, 8)
    return L.mp3mi_debug_feed_lanes(ch, len(d), ring.shape[0], push.shape[0], rows.shape[0], cap, row_samples, d.ctypes.data, ring.ctypes.data,
                                    ring_pitch, push.ctypes.data, push_pitch, rows.ctypes.data, ROW_PITCH)


def model(desc, cap, ring, push, rows):
    """ring [n_lanes, pitch, C], push [n_push_rows, PUSH_PITCH, C], rows [n_slots, ROW_PITCH, C]: what they hold afterwards"""
    ring, rows = ring.copy(), rows.copy()
    for head, pending, n, take, ln, pr, sl, _ in desc:
        stream = np.concatenate([ring[ln, (head + np.arange(pending)) % cap], push[pr, :n]])
        if take:
            rows[sl, :take] = stream[:take]
        u = max(take - pending, 0)  # pushed samples the row took
        ring[ln, (head + pending + u + np.arange(n - u)) % cap] = push[pr, u:n]
    return ring, rows


def feed_lanes_case(mp, ch, cap):
    """cap: the ring's samples -- the least (FULL + MAX_PUSH) or more; the heads near the ring's end move with it"""
    L = bind(mp)
    base = [(cap - (CAP - h) if h >= CAP - 3 else h, p, n, t) for h, p, n, t in lanes()]
    A = len(base)
    assert A == 416
    ring_pitch = cap + 20 + (-(cap + 20)) % 8
    rng = np.random.default_rng(2024 + ch + cap)
    n_lanes, n_prow, n_slots = 2 * A + 3, A + 37, A + 11
    order = rng.permutation(A)
    lane_of = rng.permutation(n_lanes)[:A]      # shuffled, with unnamed lanes in between
    prow_of = rng.permutation(n_prow)[:A]
    slot_of = rng.permutation(n_slots)[:A]
    assert (np.diff(lane_of) < 0).any() and (np.diff(prow_of) < 0).any() and (np.diff(slot_of) < 0).any()
    desc = [base[i] + (int(lane_of[k]), int(prow_of[k]) if base[i][2] else 0, int(slot_of[k]) if base[i][3] else 0, 0) for k, i in enumerate(order)]
    # unnamed lanes, push rows and slots hold data of their own, not the canary alone: a copy that lands there shows, and so does one from there
    ring = np.full((n_lanes, ring_pitch, ch), CANARY, np.int16)
    push = np.full((n_prow, PUSH_PITCH, ch), CANARY, np.int16)
    rows = np.full((n_slots, ROW_PITCH, ch), CANARY, np.int16)
    ring[:, :cap] = (20000 + np.arange(n_lanes) % 1000)[:, None, None]
    push[:, :MAX_PUSH] = (-20000 - np.arange(n_prow) % 1000)[:, None, None]
    rows[:, :FULL] = (30000 + np.arange(n_slots) % 1000)[:, None, None]
    chan = np.arange(ch) * 5000
    for k, (head, pending, n, take, ln, pr, sl, _) in enumerate(desc):
        i = np.arange(pending)
        ring[ln, (head + i) % cap] = (1 + (k * 7 + i) % 5000)[:, None] + chan      # 1 .. 10000
        if n:
            push[pr, :n] = -(1 + (k * 13 + np.arange(n)) % 5000)[:, None] - chan   # negative: never a ring sample
    want_ring, want_rows = model(desc, cap, ring, push, rows)
    got_ring, got_push, got_rows = ring.copy(), push.copy(), rows.copy()
    assert call(L, ch, desc, cap, got_ring, ring_pitch, got_push, got_rows) == 0
    assert np.array_equal(got_push, push)
    for k, d in enumerate(desc):
        assert np.array_equal(got_rows[d[6]], want_rows[d[6]]), ("row", d)
        assert np.array_equal(got_ring[d[4]], want_ring[d[4]]), ("ring", d)
    assert np.array_equal(got_rows, want_rows) and np.array_equal(got_ring, want_ring)  # the unnamed ones too
    assert (want_rows[:, FULL:] == CANARY).all() and (want_ring[:, cap:] == CANARY).all()  # (the model keeps inside its records)
    named = np.zeros(n_lanes, bool)
    named[lane_of] = True
    assert np.array_equal(got_ring[~named], ring[~named]) and (~named).sum() == A + 3
    # descriptor sets outside the rules launch nothing
    ok = (0, 8, 8, 16)
    bad_sets = [
        [ok + (1, 0, 0, 0), ok + (1, 1, 1, 0)],             # a lane twice
        [ok + (1, 0, 5, 0), ok + (2, 1, 5, 0)],             # a slot twice
        [ok + (1, 3, 0, 0), ok + (2, 3, 1, 0)],             # a push row twice
        [ok + (n_lanes, 0, 0, 0)], [ok + (0, n_prow, 0, 0)], [ok + (0, 0, n_slots, 0)],  # an index out of range
        [ok + (0, 0, 0, 1)],                                # the last word
        [(0, cap, 1, 0, 0, 0, 0, 0)],                       # pending + push > cap
        [(cap, 0, 0, 0, 0, 0, 0, 0)],                       # head outside the ring
        [(0, 5, 5, 11, 0, 0, 0, 0)],                        # take above what there is
        [(0, 1152, 100, 1153, 0, 0, 0, 0)],                 # take above the row
        [(0, 0, PUSH_PITCH + 1, 0, 0, 0, 0, 0)],            # a push beyond its row
    ]
    for bad in bad_sets:
        assert call(L, ch, bad, cap, got_ring, ring_pitch, got_push, got_rows) == -1, bad
    assert call(L, ch, desc[:1], cap, got_ring, cap + 1, got_push, got_rows) == -1  # a ring pitch that is no multiple of 16 bytes
    assert np.array_equal(got_rows, want_rows) and np.array_equal(got_ring, want_ring) and np.array_equal(got_push, push)
    # the same slot and push row may be named by descriptors that do not use them: a lane that only pushes, one that only takes
    quiet = [(0, 8, 0, 8, 1, 0, 1, 0), (0, 0, 8, 0, 2, 0, 1, 0), (0, 8, 0, 0, 3, 0, 1, 0)]
    r2, p2, w2 = ring.copy(), push.copy(), rows.copy()
    m_ring, m_rows = model(quiet, cap, ring, push, rows)
    assert call(L, ch, quiet, cap, r2, ring_pitch, p2, w2) == 0
    assert np.array_equal(r2, m_ring) and np.array_equal(w2, m_rows) and np.array_equal(p2, push)


@pytest.mark.parametrize("cap", [CAP, CAP + 41])
@pytest.mark.parametrize("ch", [1, 2])
def test_feed_lanes_kernel_emulated(emu, ch, cap):
    feed_lanes_case(emu, ch, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [CAP, CAP + 41])
@pytest.mark.parametrize("ch", [1, 2])
def test_feed_lanes_kernel_gpu(product, ch, cap):
    feed_lanes_case(product, ch, cap)
