"""k_loop's search on the DEVICE (mp3mi_debug_iteration_loop: k_prep_tail, k_prep and k_loop as the drop-in iteration_loop launches
them) against the oracle on every chain of the sets L1..L8 (tests/loop_edges.py) at every rate: every field of the side
information, the scalefactors, the declared quantised values, the final reservoir and addresses, the status word -- and, from the
oracle's trace and k_prep's list, that the sets reach what they are for (tests/test_loop_edges.py says what that is).
2375 chains, 791 or 793 a rate, in some forty launches; about two seconds a rate, most of it the generator's searches."""
import pytest

import loop_edges as le
from mp3common import Oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rate", le.RATES)
def test_device_search_is_the_oracle_at_the_edges(product, rate):
    lib = Oracle().lib
    chains = le.chains(rate, lib)
    want = {id(c): le.run_oracle(lib, c) for c in chains}
    assert {c.set for c in chains} == set(le.SET_NAMES)
    compared = 0
    for group in le.by_format(chains):
        rc, got, listed = le.run_hook(product.lib, group)
        assert rc == 0, (rc, group[0].name)
        assert not group[0].expect.get("listed") or listed > 0, group[0].name
        for c, r in zip(group, got):
            msg = le.check_expectations(c, want[id(c)])
            assert msg is None, msg
            msg = le.mismatch(c, r, want[id(c)])
            assert msg is None, msg
            compared += 1
    assert compared == len(chains)
    got = le.reached([(c, want[id(c)]) for c in chains])
    assert le.MISSING == []  # (every search of the generator found its chain: none of the named cases is silently absent)
    n_set = {k: sum(c.set == k for c in chains) for k in le.SET_NAMES}
    assert n_set == dict(le.COUNTS, L6=le.COUNTS["L6"] + 2 * (rate == 48000)), n_set
    # both outcomes of xfsf > xmin among the inside cases, in the iteration each chain was built for: the first comparison in
    # iteration 1 and in iteration 2, and the one behind pre-emphasis' multiplication
    assert got["inside_violates"] == {False, True} and got["inside_violates_it2"] == {False, True} and got["inside_violates_pre"] == {False, True}
    assert got["clamp_4095"] and got["one_step_apart"]
    assert got["exits"] == {le.EXIT_NO_OVER, le.EXIT_LOOP_BREAK, le.EXIT_SCALE_BITCOUNT} and got["compress"] == set(range(16))
    assert got["fired"] == {False, True}
    assert got["mask_bits"] == {(b, v) for b in range(4) for v in (0, 1)} and got["more_iterations"]
    assert got["add_branch"] >= {0, 1, 2} and got["bisect_equal"] and le.GLOBAL_GAIN in got["aborts"]
    assert got["drain"] == (rate == 32000) and (le.HUFF_BITS in got["aborts"]) == (rate == 48000)  # (test_loop_edges.py says why)
