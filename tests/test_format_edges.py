"""The Layer III formatter on crafted frame chains, on the CPU (tests/format_edges.py has the sets F1..F7, the model and the decoder):
the model's back pointers against the unmodified reference's, the oracle's bytes against the reference's, the emulated build of
k_format (mp3mi_debug_format_frames) and of the drop-in III_format_bitstream (fmt_probe_emu) against the oracle, and the decoder's
reading of the oracle's bytes against the inputs.  Everything bit for bit.  The device runs every chain (test_gpu_format_edges.py)."""
import os

import numpy as np
import pytest

import format_edges as fe
from mp3common import Mp3mi, Oracle

EMU_STRIDE = 5     # fe.subset(): of F1 every table once and every position six times, every 5th chain of F7, all of F2..F6
PROBE_STRIDE = 24  # ... through the emulated drop-in six chains of F1 (every position), every 24th of F7, all of F2..F6: a process each
ERR_ARG = -1


@pytest.fixture(scope="module")
def oracle_out():
    lib = Oracle().lib
    return {r: [fe.run_oracle(lib, c) for c in fe.chains(r)] for r in fe.RATES}


def test_tables_fixture_is_a_complete_prefix_code():
    """every table of tests/golden/huff_tables.npz: no code word is a prefix of another and the Kraft sum is exactly 1; the tables that
    share their cells (16..23, 24..31) differ in linbits only; and the model's frame length is the driver's for every format"""
    H = fe.HT
    for t in list(fe.TABLES) + [32, 33]:
        words = [H.cell(t, x, y) for x in range(H.xlen[t]) for y in range(H.ylen[t])]
        assert sum(2 ** (32 - n) for _, n in words) == 2 ** 32, t
        bits = sorted(format(c, "0%db" % n) for c, n in words)
        assert all(not b.startswith(a) for a, b in zip(bits, bits[1:])), t
        assert all(0 < n <= 19 and c < (1 << n) for c, n in words), t
    assert [H.linbits[t] for t in range(16, 32)] == [1, 2, 3, 4, 6, 8, 10, 13, 4, 5, 6, 7, 8, 9, 11, 13]
    assert all(H.linmax[t] == (1 << H.linbits[t]) - 1 for t in range(16, 32)) and H.xlen[4] == H.xlen[14] == 0
    for rate, f in zip(fe.RATES, (44.1, 48, 32)):
        for kbps in fe.BITRATES:
            assert fe.frame_bytes_of(rate, kbps) == int((1152 / f) * (kbps / 8.0)), (rate, kbps)


@pytest.mark.skipif(not os.path.exists(fe.PROBE_REF), reason="oracle/_ref/fmt_probe_ref is built only where the reference sources are")
def test_tables_fixture_is_the_reference(tmp_path):
    import subprocess
    p = str(tmp_path / "tables.bin")
    assert subprocess.run([fe.PROBE_REF, "--dump-tables", p]).returncode == 0
    raw, H, k = np.fromfile(p, "<i4"), fe.HT, 0
    for t in range(34):
        assert raw[k:k + 5].tolist() == [H.xlen[t], H.ylen[t], H.linbits[t], H.linmax[t], H.off[t + 1] - H.off[t]], t
        cells = raw[k + 5:k + 5 + 2 * raw[k + 4]].reshape(-1, 2)
        assert cells[:, 0].astype(np.uint32).tolist() == H.code[H.off[t]:H.off[t + 1]] and cells[:, 1].tolist() == H.length[H.off[t]:H.off[t + 1]], t
        k += 5 + 2 * raw[k + 4]
    assert k == len(raw)


@pytest.mark.skipif(not os.path.exists(fe.PROBE_REF), reason="oracle/_ref/fmt_probe_ref is built only where the reference sources are")
@pytest.mark.parametrize("rate", fe.RATES)
def test_model_and_oracle_are_the_unmodified_reference(oracle_out, rate, tmp_path):
    """every chain of every set: the back pointer every call of the reference's III_format_bitstream leaves behind is the model's, its
    file is the oracle's; where the model says the flush dies, the reference does (and the oracle says so), and nowhere else"""
    died = 0
    for c, (data, after, ab) in zip(fe.chains(rate), oracle_out[rate]):
        assert after.tolist() == c.mdb[1:], c.name
        if not c.n_frames:
            assert data == b"" and ab == 0
            continue
        rc, ref, ref_after, err = fe.run_probe(fe.PROBE_REF, c, str(tmp_path))
        assert ref_after.tolist() == c.mdb[1:], (c.name, rc, err)
        if c.flush_dies():
            died += 1
            assert rc == -6 and b"Assertion" in err and ab == (fe.FLUSH_SLOT | c.n_frames << 8) and data == b"", (c.name, rc, err, ab)
        else:
            assert rc == 0 and ab == 0, (c.name, rc, err, ab)
            assert ref == data, "%s: the oracle's %d bytes differ from the reference's %d" % (c.name, len(data), len(ref))
    assert died >= 2


@pytest.mark.parametrize("rate", fe.RATES)
def test_decoder_reads_back_the_inputs(oracle_out, rate):
    dec = fe.Decoder()
    for c, (data, after, ab) in zip(fe.chains(rate), oracle_out[rate]):
        if not ab:
            msg = fe.roundtrip_mismatch(dec, c, data)
            assert msg is None, msg


@pytest.mark.parametrize("rate", fe.RATES)
def test_emulated_formatter_is_the_oracle(oracle_out, rate):
    """mp3mi_debug_format_frames of the emulated build (k_format's own code) on every chain of F2..F6 and the fe.subset() of F1
    and F7: bytes, length and status; MP3MI_STREAM_ABORT_FLUSH_SLOT with no file exactly where the reference dies in its flush"""
    lib = Mp3mi(emu=True).lib
    want = {id(c): o for c, o in zip(fe.chains(rate), oracle_out[rate])}
    sub = fe.subset(fe.chains(rate), EMU_STRIDE)
    assert {c.set for c in sub} == set(fe.SET_NAMES)
    assert {c.tag[1] for c in sub if c.set == "F1"} == set(range(30)) and {c.tag[0] for c in sub if c.set == "F1"} == set(range(5))
    outcomes = set()
    for group in fe.by_format(sub):
        rc, got, status = fe.run_hook(lib, group)
        assert rc == 0, (rc, group[0].name)
        for c, data, st in zip(group, got, status):
            ref, _, ab = want[id(c)]
            outcomes.add(c.flush_dies())
            if c.flush_dies():
                assert st == (fe.FLUSH_SLOT | c.n_frames << 8) == ab and data == b"", (c.name, st, len(data))
            else:
                assert st == 0 and data == ref, "%s: status %d, %d bytes against the oracle's %d" % (c.name, st, len(data), len(ref))
    assert outcomes == {False, True}


@pytest.mark.skipif(not os.path.exists(fe.PROBE_EMU), reason="oracle/_ref/fmt_probe_emu is built only where the reference sources are")
@pytest.mark.parametrize("rate", fe.RATES)
def test_emulated_dropin_formatter_is_the_oracle(oracle_out, rate, tmp_path):
    """the drop-in III_format_bitstream (k_format_marked) of the emulated build, given the caller's own frames, a process per chain"""
    want = {id(c): o for c, o in zip(fe.chains(rate), oracle_out[rate])}
    sub = [c for c in fe.subset(fe.chains(rate), PROBE_STRIDE) if c.n_frames]
    assert {c.set for c in sub} == set(fe.SET_NAMES)
    for c in sub:
        ref, _, ab = want[id(c)]
        rc, data, after, err = fe.run_probe(fe.PROBE_EMU, c, str(tmp_path))
        assert after.tolist() == c.mdb[1:], (c.name, rc, err)
        if c.flush_dies():
            assert rc != 0 and b"Assertion" in err, (c.name, rc, err)
        else:
            assert rc == 0 and data == ref, (c.name, rc, err, len(data), len(ref))


def _broken(make):
    """a legal two-frame chain with one thing changed behind the generator's back"""
    c = fe.Chain("X", "broken", 44100, 1, 128)
    body = np.zeros(576, np.int16)
    body[:12] = (3, -2, 0, 1, 1, 1, 0, -1, 1, 0, 0, 1)
    for _ in range(2):
        c.frame([fe.granule(body, 0, (5, 0, 0), 2, 2, 7, 7, sfc=5, sf=[1] * 21 + [0] * 18), fe.granule(body, 2, (7, 7), 288)])
    c.check()
    make(c)
    return c


def _set(c, n, gr, field, v, k=None):
    if k is None:
        c.sides[n]["gr"][gr][0][field] = v
    else:
        c.sides[n]["gr"][gr][0][field][k] = v


BREAKS = {
    "back pointer not the model's": lambda c: c.sides[1].__setitem__("main_data_begin", c.mdb[1] + 1),
    "bits not a multiple of 8": lambda c: c.sides[0].__setitem__("resvDrain", c.sides[0]["resvDrain"] + 4),
    "part2_3_length above 4095": lambda c: _set(c, 0, 0, "part2_3_length", 4096),
    "part2_3_length below its contents": lambda c: (_set(c, 0, 0, "part2_3_length", 8), _set(c, 0, 1, "part2_3_length", c.sides[0]["gr"][1][0]["part2_3_length"] + c.sides[0]["gr"][0][0]["part2_3_length"] - 8)),
    "part2_length not the scalefactors'": lambda c: _set(c, 0, 0, "part2_length", 20),
    "table too small for its region": lambda c: _set(c, 0, 0, "table_select", 2, 0),
    "table 4": lambda c: _set(c, 0, 0, "table_select", 4, 0),
    "table 14": lambda c: _set(c, 0, 1, "table_select", 14, 1),
    "short block with count1": lambda c: _set(c, 0, 1, "count1", 1),
    "short block with 100 big values": lambda c: _set(c, 0, 1, "big_values", 100),
    "block type 3 with region counts of its own": lambda c: (_set(c, 0, 0, "window_switching_flag", 1), _set(c, 0, 0, "block_type", 3)),
    "block type without the flag": lambda c: _set(c, 0, 0, "block_type", 1),
    "more than 576 lines": lambda c: _set(c, 0, 0, "count1", 144),
    "a 2 in the count1 region": lambda c: c.ixs[0].__setitem__((0, 0, 5), 2),
    "a line behind the count1 region": lambda c: c.ixs[0].__setitem__((0, 0, 100), 1),
    "a scalefactor beyond its slen": lambda c: _set(c, 0, 0, "scalefac", 2, 3),
    "scalefac_compress 16": lambda c: _set(c, 0, 0, "scalefac_compress", 16),
    "region counts beyond the band table": lambda c: (_set(c, 0, 0, "region0_count", 15), _set(c, 0, 0, "region1_count", 7)),
    "negative resvDrain": lambda c: c.sides[0].__setitem__("resvDrain", -8),
}


@pytest.mark.parametrize("what", sorted(BREAKS))
def test_hook_refuses_an_illegal_chain(what):
    lib = Mp3mi(emu=True).lib
    assert fe.run_hook(lib, [_broken(lambda c: None)])[0] == 0
    assert fe.run_hook(lib, [_broken(BREAKS[what])])[0] == ERR_ARG, what


@pytest.mark.parametrize("table", (23, 31))
def test_hook_refuses_a_magnitude_beyond_13_linbits(table):
    """15 + 8191 is the largest value a table codes; the same frame with 8207 in its place (the same cell, the same bit count)"""
    lib = Mp3mi(emu=True).lib
    ix = np.zeros(576, np.int16)
    ix[:4] = (8206, -8206, 3, -8206)
    c = fe.Chain("X", "largest value", 44100, 1, 128)
    c.frame([fe.granule(ix, 0, (table, 0, 0), 2, 0, 7, 7), fe.granule(ix, 2, (table, 1), 288)])
    c.check()
    assert fe.run_hook(lib, [c])[0] == 0
    for gr, line, v in ((0, 1, -8207), (1, 3, -8207), (0, 0, 8207)):
        c.ixs[0][gr, 0, line] = v
        assert fe.run_hook(lib, [c])[0] == ERR_ARG, (gr, line)
        c.ixs[0][gr, 0, line] = ix[line]


def test_hook_refuses_a_frame_beyond_its_image_or_its_row():
    """more bits than the kernel's frame image holds (resvDrain makes them), a back pointer above 511, an output row too short"""
    lib = Mp3mi(emu=True).lib
    c = fe.Chain("X", "long drain", 32000, 1, 320)
    for _ in range(3):
        c.frame([fe.granule(stuff=4095), fe.granule(stuff=4095)])
    assert fe.run_hook(lib, [c])[0] == 0
    c.sides[2]["resvDrain"] += 8 * 1200  # 8190 + 3162 + 9600 > 640 * 32
    assert fe.run_hook(lib, [c])[0] == ERR_ARG
    c = fe.Chain("X", "reservoir above 511", 32000, 1, 320)
    c.frame([fe.granule(), fe.granule()], take=c.slot - 512)
    c.frame([fe.granule(), fe.granule()], take=c.slot)
    assert fe.run_hook(lib, [c])[0] == ERR_ARG
