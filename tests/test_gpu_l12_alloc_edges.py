"""k12_alloc on the DEVICE (mp3mi_debug_l12_alloc: the kernel as the Layer I / II batch launches it) against the oracle on every case
of the sets A1..A6 (tests/l12_alloc_edges.py): each case as frames 0, 1 and 2 of a stream, the streams of a launch at their own
bitrates, at each of the three phases of l12_alloc_edges.SLOT0 -- the frames' bytes, the file's last byte and every seam of every
frame, bit for bit -- and, from the oracle's outputs and trace, that the sets reach what they are for (tests/test_l12_alloc_edges.py
says what that is).  Nothing of the reference is read.  452 cases in 80 launches a phase, each of a few dozen single-wavefront
workgroups; on an MI355X the three phases take 2 s together, 1.5 s of them the generator's searches with the oracle."""
import pytest

import l12_alloc_edges as ae
from mp3common import Oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("slot0", ae.SLOT0)
def test_device_frames_are_the_oracle_at_the_edges(product, slot0):
    lib = Oracle().lib
    cases = ae.cases(lib)
    assert {c.set for c in cases} == set(ae.SET_NAMES)
    n_set = {k: sum(c.set == k for c in cases) for k in ae.SET_NAMES}
    assert n_set == ae.COUNTS, n_set
    pairs, compared = [], 0
    for group in ae.by_key(cases):
        want = ae.run_oracle(lib, group)
        rc, got = ae.run_hook(product.lib, group, slot0)
        assert rc == 0, (rc, group[0].name)
        for c, r, w in zip(group, got, want):
            msg = ae.check_expectations(c, w)
            assert msg is None, msg
            msg = ae.mismatch_hook(c, r, w)
            assert msg is None, msg
            compared += 1
        pairs += list(zip(group, want))
    assert compared == len(cases)
    T = ae.tables(lib)
    ae.assert_reached(ae.reached(pairs, T), T)
