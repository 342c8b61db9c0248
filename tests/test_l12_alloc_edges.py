"""k12_alloc on crafted subband samples and mask ratios, on the CPU (tests/l12_alloc_edges.py has the sets A1..A6 and what each is
for): the oracle's frame encoder against the unmodified reference's own functions (oracle/_ref/ref_harness_l12_alloc, a process per
format), the emulated build of the hook mp3mi_debug_l12_alloc -- k12_alloc as the batch launches it -- against the oracle, the
hook's refusals, and, from the oracle's outputs and trace, that every set reaches what it was built for.  Everything bit for bit:
the frames' bytes and every seam (ratios, scale factors after the transmission pattern, joint scale factors, scfsi, allocation,
mode, mode_ext, bound, sblimit, bits left, CRC).  The device runs every case (test_gpu_l12_alloc_edges.py).

Cases: 452 in 80 formats (A1 19, A2 6, A3 85, A4 87, A5 119, A6 136; l12_alloc_edges.COUNTS, asserted).  Generation, which searches
with the oracle, 2.7 s; the oracle on all of them 0.05 s; the reference on ALL of them 0.4 s.  One emulated frame costs 43 ms
(every case as three frames at one phase: 58 s), so the emulated build takes the 127 cases the generator marks (A1 8, A2 2, A3 10,
A4 48, A5 35, A6 24), as frames 0, 1 and 2 at each of the three phases of l12_alloc_edges.SLOT0: 1143 frames, 49 s.  The file: 55 s
serial.

What the sets catch (each line a one-statement change of k_l12.hip, on a copy; the sets whose cases then differ from the oracle on
the emulated build, all 452 cases at phase 0, with the number of cases, and in brackets those among the marked ones):
  the round's `k > T` as `>=`                       A4 1 (1): the band that waits exactly on another's ratio after its step
  T without the rounding up (`| 0xffffffff` gone)   A4 2 (2): that case and the one a float above it
  the tie taken from the highest lane               A1 19 (8), A4 24 (12), A5 38 (5)
  the round's `ad >= spent + cost` as `>`           nothing, and nothing can: a round that fits exactly then goes down the
                                                    one-band-at-a-time path, which is the reference's own order
  the end game's `ad >= spent + wneed` as `>`       A1 9 (3), A2 1 (1), A4 15 (10), A5 18 (7), A6 30 (5)
  the early stop's `ad - spent < mn` as `<=`        A2 1 (1), A4 3 (1), A5 2 (1), A6 6 (1)
  `lim > mnr` as `>=`                               A4 4 (4): band (0, 0) full and closed, the other band on the limit
  `999999.0 > m` as `>=`                            A4 2 (2)
  `mult[mid - 1] >= m` as `>`                       A1 17 (6), A3 85 (10)
  one cell of L12_PATTERN ([2][4]: 3 -> 0)          A1 1 (1), A2 6 (2), A4 22 (12), A5 40 (8), A6 41 (4)
  `rq > frame_bits` as `>=`, in front of the loop   A5 3 (3)
  `rq > frame_bits` as `>=`, in the loop            A5 2 (2)
  the sign undo dropped                             every set at every phase: 1322 of the 1356 streams of the three phases (353 of 381)"""
import os

import numpy as np
import pytest

import l12_alloc_edges as ae

ERR_ARG = -1


@pytest.fixture(scope="module")
def oracle_out(oracle):
    pairs = []
    for group in ae.by_key(ae.cases(oracle.lib)):
        pairs += list(zip(group, ae.run_oracle(oracle.lib, group)))
    return pairs


def test_sets_reach_what_they_are_for(oracle_out, oracle):
    """the oracle's outputs and trace: every case reaches what it was built for, and the sets between them every outcome they are
    to cover"""
    assert {c.set for c, _ in oracle_out} == set(ae.SET_NAMES)
    for c, r in oracle_out:
        msg = ae.check_expectations(c, r)
        assert msg is None, msg
    n_set = {k: sum(c.set == k for c, _ in oracle_out) for k in ae.SET_NAMES}
    assert n_set == ae.COUNTS, n_set
    T = ae.tables(oracle.lib)
    ae.assert_reached(ae.reached(oracle_out, T), T)


@pytest.mark.skipif(not os.path.exists(ae.REF_HARNESS), reason="oracle/_ref/ref_harness_l12_alloc is built only where the reference sources are")
def test_oracle_is_the_unmodified_reference(oracle_out, tmp_path):
    """EVERY case: the frame's bytes (the frame that outgrows its slot included) and every member of the stage dump"""
    want = {id(c): r for c, r in oracle_out}
    compared = 0
    for group in ae.by_key([c for c, _ in oracle_out]):
        for c, ref in zip(group, ae.run_reference(group, str(tmp_path))):
            msg = ae.mismatch_dump(c, ref, want[id(c)])
            assert msg is None, msg
            compared += 1
    assert compared == sum(ae.COUNTS.values())


@pytest.mark.parametrize("slot0", ae.SLOT0)
def test_emulated_hook_is_the_oracle(oracle_out, emu, slot0):
    """the hook of the emulated build on the cases marked for it, every set among them, as frames 0, 1 and 2 of streams at their
    own bitrates: bytes, the file's last byte, and every seam of every frame"""
    sub = [(c, r) for c, r in oracle_out if c.emu]
    assert {c.set for c, _ in sub} == set(ae.SET_NAMES)
    want = {id(c): r for c, r in sub}
    for group in ae.by_key([c for c, _ in sub]):
        rc, got = ae.run_hook(emu.lib, group, slot0)
        assert rc == 0, (rc, group[0].name)
        for c, r in zip(group, got):
            msg = ae.mismatch_hook(c, r, want[id(c)])
            assert msg is None, msg


def _legal(layer, C=2):
    """a small legal launch: two streams of two frames"""
    rng = np.random.default_rng(11)
    parts = 1 if layer == 1 else 3
    a = dict(layer=layer, rate=44100, C=C, mode=0 if C == 2 else 3, crc=0, flags=0, slot0=0, kbps=[128, 192],
             sb=rng.uniform(-1.0, 1.0, (2, 2, C, parts, 12, 32)), ratio=rng.uniform(-10, 30, (2, 2, layer, C, 32)).astype(np.float32), nf=2)
    return a


def _set(a, key, v, at=None):
    if at is None:
        a[key] = v
    else:
        a[key][at] = v


BREAKS = {
    "a NaN sample": lambda a: _set(a, "sb", np.nan, (1, 0, 1, 0, 3, 7)),
    "an infinite sample": lambda a: _set(a, "sb", -np.inf, (0, 1, 0, 0, 11, 31)),
    "a sample above 2.0": lambda a: _set(a, "sb", np.nextafter(2.0, 3.0), (0, 0, 0, 0, 0, 0)),
    "a sample below -2.0": lambda a: _set(a, "sb", -np.nextafter(2.0, 3.0), (1, 1, 1, 0, 5, 30)),
    "a NaN ratio": lambda a: _set(a, "ratio", np.nan, (0, 0, 0, 1, 4)),
    "an infinite ratio": lambda a: _set(a, "ratio", np.inf, (1, 1, 0, 0, 0)),
    "a ratio of minus infinity": lambda a: _set(a, "ratio", -np.inf, (1, 0, 0, 1, 31)),
    "a bitrate that is none": lambda a: _set(a, "kbps", [128, 100]),
    "a bitrate of the other layer": lambda a: _set(a, "kbps", [128, 288 if a["layer"] == 2 else 48]),
    "layer 3": lambda a: _set(a, "layer", 3),
    "an MPEG-2 rate": lambda a: _set(a, "rate", 22050),
    "two channels in mono": lambda a: _set(a, "mode", 3),
    "mode 4": lambda a: _set(a, "mode", 4),
    "crc 2": lambda a: _set(a, "crc", 2),
    "header flags 16": lambda a: _set(a, "flags", 16),
    "slot0 18": lambda a: _set(a, "slot0", 18),
    "slot0 -1": lambda a: _set(a, "slot0", -1),
    "65 frames": lambda a: (_set(a, "nf", 65), _set(a, "sb", np.zeros((2, 65) + a["sb"].shape[2:])), _set(a, "ratio", np.zeros((2, 65) + a["ratio"].shape[2:], np.float32))),
    "a row too short for the frames and the last byte": lambda a: _set(a, "stride", 2 * ae.frame_bits_of(a["layer"], 44100, 192) // 8),
}
_LEGAL_RAN = {}


@pytest.mark.parametrize("layer", (1, 2))
@pytest.mark.parametrize("what", sorted(BREAKS))
def test_hook_refuses_what_lies_outside_its_domain(emu, what, layer):
    """a legal launch with one thing changed: refused before anything is launched; the launch itself passes"""
    if layer not in _LEGAL_RAN:
        _LEGAL_RAN[layer] = ae.hook_call(emu.lib, **_legal(layer))[0]
    assert _LEGAL_RAN[layer] == 0
    a = _legal(layer)
    BREAKS[what](a)
    assert ae.hook_call(emu.lib, **a)[0] == ERR_ARG, what


def test_mono_refuses_a_stereo_mode(emu):
    a = _legal(2, C=1)
    assert ae.hook_call(emu.lib, **a)[0] == 0
    a["mode"] = 0
    assert ae.hook_call(emu.lib, **a)[0] == ERR_ARG


@pytest.mark.parametrize("layer", (1, 2))
def test_hook_takes_the_ends_of_its_domain(emu, oracle, layer):
    """... and on the bounds themselves it runs, and is the oracle: samples of +-2.0, ratios of +-FLT_MAX, the last phase, 64 frames,
    a row of exactly the frames and the last byte"""
    rng = np.random.default_rng(12)
    T = ae.tables(oracle.lib)
    big = np.float32(3.4028234663852886e38)
    sb = ae.random_sb(rng, layer, 2, T)
    sb[0, :, 3, 0], sb[1, :, 7, 0], sb[0, :, 0, 5] = 2.0, -2.0, 2.0
    ratio = rng.uniform(-10, 30, (2, 32)).astype(np.float32)
    ratio[0, 0], ratio[1, 1], ratio[0, 2] = big, -big, -0.0
    c = ae.Case("X", "ends", layer, 44100, "je", 192, sb, ratio)
    want = ae.run_oracle(oracle.lib, [c])[0]
    rc, got = ae.run_hook(emu.lib, [c], 17, 64)
    assert rc == 0
    msg = ae.mismatch_hook(c, got[0], want, 64)
    assert msg is None, msg
    stride = 2 * len(want.bytes) + 1
    rc, out, lens, _ = ae.hook_call(emu.lib, layer, 44100, 2, 1, 1, 0, 0, [192], np.stack([c.sb] * 2)[None], np.stack([c.ratio] * 2)[None], 2, stride)
    assert rc == 0 and lens[0] == stride and out[0].tobytes() == want.bytes * 2 + b"\0"
