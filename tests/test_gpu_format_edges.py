"""k_format on the DEVICE (mp3mi_debug_format_frames) against the oracle on every chain of the sets F1..F7 (tests/format_edges.py) at
every rate, the drop-in III_format_bitstream (k_format_marked, oracle/_ref/fmt_probe) on a subset that contains every set, the decoder
on the device's bytes -- and the sets reach what they are for: all 30 tables (the 29 with cells and table 0 on a region of zeros) in every region position, every cell, both ends of every
linbits width, a put at every bit offset and a two-word put that is not stuffing at each of 5..31 (the longest is 28 bits) and a two-word stuffing put at each of 1..31, both outcomes of the flush, the largest reach-back."""
import os

import pytest

import format_edges as fe
from mp3common import Oracle

pytestmark = pytest.mark.gpu
PROBE_STRIDE = 24  # fe.subset(): six chains of F1 (every position), every 24th of F7 and all of F2..F6: a child process each


@pytest.mark.parametrize("rate", fe.RATES)
def test_device_formatter_is_the_oracle_at_the_edges(product, rate):
    lib = Oracle().lib
    dec = fe.Decoder()
    cov = fe.Coverage()
    outcomes = set()
    for group in fe.by_format(fe.chains(rate)):
        rc, got, status = fe.run_hook(product.lib, group)
        assert rc == 0, (rc, group[0].name)
        for c, data, st in zip(group, got, status):
            ref, after, ab = fe.run_oracle(lib, c)
            assert after.tolist() == c.mdb[1:], c.name
            cov.add(c)
            outcomes.add(c.flush_dies())
            if c.flush_dies():
                assert st == (fe.FLUSH_SLOT | c.n_frames << 8) == ab and data == b"", (c.name, st, len(data))
                continue
            assert st == 0 and data == ref, "%s: status %d, %d bytes against the oracle's %d" % (c.name, st, len(data), len(ref))
            msg = fe.roundtrip_mismatch(dec, c, data)
            assert msg is None, msg
    assert cov.missing() == []
    assert outcomes == {False, True}
    assert cov.reach == -(-511 // (fe.frame_bytes_of(rate, 32) - 36)) and (rate != 48000 or cov.reach == 9)


@pytest.mark.skipif(not os.path.exists(fe.PROBE_DEV), reason="oracle/_ref/fmt_probe is built only where the reference sources are")
@pytest.mark.parametrize("rate", fe.RATES)
def test_device_dropin_formatter_is_the_oracle(product, rate, tmp_path):
    lib = Oracle().lib
    sub = [c for c in fe.subset(fe.chains(rate), PROBE_STRIDE) if c.n_frames]
    assert {c.set for c in sub} == set(fe.SET_NAMES)
    for c in sub:
        ref, _, ab = fe.run_oracle(lib, c)
        rc, data, after, err = fe.run_probe(fe.PROBE_DEV, c, str(tmp_path), timeout=60)
        assert after.tolist() == c.mdb[1:], (c.name, rc, err)
        if c.flush_dies():
            assert rc != 0 and b"Assertion" in err, (c.name, rc, err)
        else:
            assert rc == 0 and data == ref, (c.name, rc, err, len(data), len(ref))
