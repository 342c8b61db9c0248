"""k_feed_packed alone (mp3mi_debug_feed_packed, include/mp3mi.h): the kernel that cuts the rows of a feeder's tick on host buffers.
It is k_feed_lanes with two differences, and both are what this file is about.  The pushes lie PACKED in one buffer, back to back,
so a push begins at any even byte and its neighbours' samples lie right beside it: the 416 descriptors of test_feed_kernel.py (the
heads, fills, pushes and takes at which the alignment paths and the ring's wrap change), shuffled over lanes and slots as in
test_feed_lanes_kernel.py, with their pushes packed in descriptor order -- once from sample 0 and once from sample 1 of the buffer.
And the grid goes over a work list that deals a descriptor to 1 .. 8 workgroups by its own longest copy: at 256 * 16 bytes per
workgroup every descriptor of these small shapes that moves more than a few KB is dealt to several, at the product's value to one
or two.  A numpy model says what rings and rows hold afterwards; whatever it does not write must hold what it held, and the packed
buffer is unchanged."""
import ctypes
import os
import shutil
import tempfile

import numpy as np
import pytest

from test_feed_kernel import CANARY, CAP, FULL, MAX_PUSH, lanes
from test_kernel_budgets import HIPCC, resources, the

ROW_PITCH = FULL + 16
WG_SMALL, WG_PRODUCT = 256 * 16, 256 * 16 * 4  # bytes a workgroup moves: forcing up to 8 parts; csrc/mp3mi_host.h MP3MI_FEED_WG_BYTES


def bind(mp):
    L = mp.lib
    L.mp3mi_debug_feed_packed.argtypes = [ctypes.c_int] * 7 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                               ctypes.c_void_p, ctypes.c_size_t]
    return L


def call(L, ch, desc, cap, ring, ring_pitch, packed, rows, wg, row_samples=FULL, n_packed=None):
    d = np.ascontiguousarray(desc, dtype=np.uint32).reshape(-1, 8)
    return L.mp3mi_debug_feed_packed(ch, len(d), ring.shape[0], packed.shape[0] if n_packed is None else n_packed, rows.shape[0], cap, row_samples,
                                     wg, d.ctypes.data, ring.ctypes.data, ring_pitch, packed.ctypes.data, rows.ctypes.data, ROW_PITCH)


def model(desc, cap, ring, packed, rows):
    """ring [n_lanes, pitch, C], packed [n_packed, C], rows [n_slots, ROW_PITCH, C]: what rings and rows hold afterwards"""
    ring, rows = ring.copy(), rows.copy()
    for head, pending, n, take, ln, first, sl, _ in desc:
        stream = np.concatenate([ring[ln, (head + np.arange(pending)) % cap], packed[first:first + n]])
        if take:
            rows[sl, :take] = stream[:take]
        u = max(take - pending, 0)  # pushed samples the row took
        ring[ln, (head + pending + u + np.arange(n - u)) % cap] = packed[first + u:first + n]
    return ring, rows


def feed_packed_case(mp, ch, cap, wg, first0):
    """cap: the ring's samples; wg: bytes per workgroup; first0: the sample of the packed buffer at which the first push begins"""
    L = bind(mp)
    esz = 2 * ch
    base = [(cap - (CAP - h) if h >= CAP - 3 else h, p, n, t) for h, p, n, t in lanes()]
    A = len(base)
    assert A == 416 and {n for _, _, n, _ in base} == {0, 1, 8, 9, 1500}
    ring_pitch = cap + 20 + (-(cap + 20)) % 8
    rng = np.random.default_rng(4048 + ch + cap)
    n_lanes, n_slots = 2 * A + 3, A + 11
    order = rng.permutation(A)
    lane_of = rng.permutation(n_lanes)[:A]  # shuffled, with unnamed lanes and slots in between
    slot_of = rng.permutation(n_slots)[:A]
    assert (np.diff(lane_of) < 0).any() and (np.diff(slot_of) < 0).any()
    desc, at = [], first0
    for k, i in enumerate(order):  # the pushes back to back, in descriptor order
        n = base[i][2]
        desc.append(base[i] + (int(lane_of[k]), at if n else 0, int(slot_of[k]) if base[i][3] else 0, 0))
        at += n
    n_packed = at + 5  # (a canary behind the last push)
    # every source alignment the packing can give: with mono every even residue mod 16, with stereo every multiple of 4
    residues = {d[5] * esz % 16 for d in desc if d[2]}
    assert residues == (set(range(0, 16, 2)) if ch == 1 else set(range(0, 16, 4))), residues
    assert first0 * esz % 16 != 0 or first0 == 0
    ring = np.full((n_lanes, ring_pitch, ch), CANARY, np.int16)
    packed = np.full((n_packed, ch), CANARY, np.int16)
    rows = np.full((n_slots, ROW_PITCH, ch), CANARY, np.int16)
    ring[:, :cap] = (20000 + np.arange(n_lanes) % 1000)[:, None, None]
    rows[:, :FULL] = (30000 + np.arange(n_slots) % 1000)[:, None, None]
    chan = np.arange(ch) * 5000
    for k, (head, pending, n, take, ln, first, sl, _) in enumerate(desc):
        i = np.arange(pending)
        ring[ln, (head + i) % cap] = (1 + (k * 7 + i) % 5000)[:, None] + chan      # 1 .. 10000
        if n:
            packed[first:first + n] = -(1 + (k * 13 + np.arange(n)) % 5000)[:, None] - chan   # negative: never a ring sample; differs packet by packet
    want_ring, want_rows = model(desc, cap, ring, packed, rows)
    got_ring, got_packed, got_rows = ring.copy(), packed.copy(), rows.copy()
    assert call(L, ch, desc, cap, got_ring, ring_pitch, got_packed, got_rows, wg) == 0
    assert np.array_equal(got_packed, packed)
    for d in desc:
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
        [ok + (1, 0, 0, 0), ok + (1, 8, 1, 0)],             # a lane twice
        [ok + (1, 0, 5, 0), ok + (2, 8, 5, 0)],             # a slot twice
        [ok + (1, 3, 0, 0), ok + (2, 3, 1, 0)],             # two pushes that share samples
        [ok + (1, 0, 0, 0), ok + (2, 7, 1, 0)],
        [ok + (n_lanes, 0, 0, 0)], [ok + (0, 0, n_slots, 0)],  # an index out of range
        [ok + (0, n_packed - 7, 0, 0)],                     # a source span past the end of the packed buffer
        [(0, 0, 0, 0, 0, n_packed + 1, 0, 0)],
        [ok + (0, 0, 0, 1)],                                # the last word
        [(0, cap, 1, 0, 0, 0, 0, 0)],                       # pending + push > cap
        [(cap, 0, 0, 0, 0, 0, 0, 0)],                       # head outside the ring
        [(0, 5, 5, 11, 0, 0, 0, 0)],                        # take above what there is
        [(0, 1152, 100, 1153, 0, 0, 0, 0)],                 # take above the row
    ]
    for bad in bad_sets:
        assert call(L, ch, bad, cap, got_ring, ring_pitch, got_packed, got_rows, wg) == -1, bad
    assert call(L, ch, desc[:1], cap, got_ring, cap + 1, got_packed, got_rows, wg) == -1  # a ring pitch that is no multiple of 16 bytes
    assert call(L, ch, desc[:1], cap, got_ring, ring_pitch, got_packed, got_rows, 0) == -1  # no bytes per workgroup
    assert call(L, ch, desc, cap, got_ring, ring_pitch, got_packed, got_rows, wg, n_packed=at - 1) == -1  # the good set in a buffer one sample short
    assert np.array_equal(got_rows, want_rows) and np.array_equal(got_ring, want_ring) and np.array_equal(got_packed, packed)
    # a span that ends exactly at the buffer's end is inside it; a slot may be named by descriptors that do not take
    quiet = [(0, 8, 0, 8, 1, 0, 1, 0), (0, 0, 8, 0, 2, n_packed - 8, 1, 0), (0, 8, 0, 0, 3, n_packed, 1, 0)]
    r2, p2, w2 = ring.copy(), packed.copy(), rows.copy()
    m_ring, m_rows = model(quiet, cap, ring, packed, rows)
    assert call(L, ch, quiet, cap, r2, ring_pitch, p2, w2, wg) == 0
    assert np.array_equal(r2, m_ring) and np.array_equal(w2, m_rows) and np.array_equal(p2, packed)


PARAMS = [(ch, cap, wg, first0) for ch in (1, 2) for cap in (CAP, CAP + 41) for wg, first0 in ((WG_SMALL, 0), (WG_PRODUCT, 0), (WG_SMALL, 1))]


@pytest.mark.parametrize("ch,cap,wg,first0", PARAMS)
def test_feed_packed_kernel_emulated(emu, ch, cap, wg, first0):
    feed_packed_case(emu, ch, cap, wg, first0)


@pytest.mark.gpu
@pytest.mark.parametrize("ch,cap,wg,first0", PARAMS)
def test_feed_packed_kernel_gpu(product, ch, cap, wg, first0):
    feed_packed_case(product, ch, cap, wg, first0)


def test_work_list_follows_each_descriptors_own_work(emu):
    """a packet of a few KB beside a row of 147 KB: at the product's bytes per workgroup the small one is one workgroup's work -- seen
    from outside as: the launch is right whatever the split, for a long take beside short pushes"""
    L = bind(emu)
    cap, full = 40000, 32 * 1152
    ring = np.full((3, cap + 8, 2), CANARY, np.int16)
    rows = np.full((2, ROW_PITCH + full, 2), CANARY, np.int16)
    packed = (np.arange(3000 * 2, dtype=np.int16) - 3000).reshape(3000, 2)
    ring[:, :cap] = (np.arange(cap) % 30000)[None, :, None]
    desc = [(5, full - 100, 960, full, 0, 1, 1, 0), (0, 0, 960, 0, 2, 961, 0, 0), (7, 3, 1, 0, 1, 0, 0, 0)]
    want_ring, want_rows = model(desc, cap, ring, packed, rows)
    for wg in (WG_PRODUCT, WG_SMALL):
        r, p, w = ring.copy(), packed.copy(), rows.copy()
        d = np.ascontiguousarray(desc, dtype=np.uint32)
        assert L.mp3mi_debug_feed_packed(2, 3, 3, 3000, 2, cap, full, wg, d.ctypes.data, r.ctypes.data, cap + 8, p.ctypes.data, w.ctypes.data,
                                         ROW_PITCH + full) == 0
        assert np.array_equal(r, want_ring) and np.array_equal(w, want_rows) and np.array_equal(p, packed)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_feed_packed_fits_beside_k_loop():
    """one wavefront per SIMD beside k_loop's four: no LDS, no scratch, and the 160 vector registers test_kernel_budgets.py calls `beside`"""
    tmp = tempfile.mkdtemp(prefix="mp3mi_budget_feed_")
    try:
        k = the(resources("k_format", tmp), r"^_Z13k_feed_packedPK")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("k_feed_packed:", k)
    assert k["ScratchSize"] == 0 and k["LDS"] == 0 and k["VGPRs"] <= 512 - 4 * 88, k
