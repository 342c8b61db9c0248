"""k_loop's search on crafted chains, on the CPU (tests/loop_edges.py has the sets L1..L8 and what each is for): the oracle's
iteration loop against the unmodified reference's (oracle/_ref/ref_harness_loop, a process per chain), the emulated build of the
hook mp3mi_debug_iteration_loop -- k_prep_tail, k_prep and k_loop as the drop-in iteration_loop launches them -- against the
oracle, the hook's refusals, and, from the oracle's trace, that every set reaches what it was built for.  Everything bit for bit.
The device runs every chain (test_gpu_loop_edges.py).

Chains at the three rates together: 2375 (L1 1557, L2 153, L3 30, L4 135, L5 285, L6 14, L7 33, L8 168; loop_edges.COUNTS, asserted).
The oracle takes all of them (generation, which searches with the oracle, and its run: 17 s); the reference 764 (every fresh-start
chain of L2..L7, every 9th of L1, every 4th of L8: 2.5 s); the emulated build, at ~0.1 s a granule, the 314 the generator marks
(L1 108, L2 79, L3 24, L4 30, L5 30, L6 13, L7 27, L8 3: 49 s).  The file: 70 s serial.

What the sets catch (each line a one-statement change of k_loop.hip, on a copy; the sets whose chains then differ from the oracle
on the emulated build): `xfsf_r > xmin_r` as `>=` in the amplification: L1, L5..L8; loop_noise_close's 1e-12 as 0 -- no exact
tier --: L1 alone (nine chains: the partial sums' order decides a comparison there, which no PCM-driven test sees); one nibble of
scale_bitcount's table: L2's cell and L1, L4, L5, L7, L8; `more_bits > 100` as `>=`: L5; sc_xrmax[ch][gr2] as [gr2][ch]: L4, L5,
L8; sfb 17..20 `any` for `all` in pre-emphasis: L1, L3..L6, L8; the bisection's `> 1` as `> 0`: every set.  ResvFrameEnd's
`< 4095` as `<= 4095` changes nothing anywhere: on 4095 exactly the other branch fills granule 0 to 4095 and drains 0, the same
numbers (L5 has the 4094 / 4095 pair all the same)."""
import os

import numpy as np
import pytest

import loop_edges as le

ERR_ARG = -1
REF_STRIDE = {"L1": 9, "L8": 4}  # of L1 and L8 every 9th / 4th chain goes to the reference, of L2..L7 every fresh-start chain


@pytest.fixture(scope="module")
def oracle_out(oracle):
    return {r: [(c, le.run_oracle(oracle.lib, c)) for c in le.chains(r, oracle.lib)] for r in le.RATES}


@pytest.mark.parametrize("rate", le.RATES)
def test_sets_reach_what_they_are_for(oracle_out, rate):
    """the oracle's trace: every chain reaches what it was built for, and the sets between them every outcome they are to cover"""
    pairs = oracle_out[rate]
    assert {c.set for c, _ in pairs} == set(le.SET_NAMES)
    for c, r in pairs:
        msg = le.check_expectations(c, r)
        assert msg is None, msg
    got = le.reached(pairs)
    assert le.MISSING == []  # (every search of the generator found its chain: none of the named cases is silently absent)
    n_set = {k: sum(c.set == k for c in [c for c, _ in pairs]) for k in le.SET_NAMES}
    assert n_set == dict(le.COUNTS, L6=le.COUNTS["L6"] + 2 * (rate == 48000)), n_set
    # both outcomes of xfsf > xmin among the inside cases, in the iteration each chain was built for: the first comparison in
    # iteration 1 and in iteration 2, and the one behind pre-emphasis' multiplication
    assert got["inside_violates"] == {False, True} and got["inside_violates_it2"] == {False, True} and got["inside_violates_pre"] == {False, True}
    assert got["clamp_4095"] and got["one_step_apart"]
    assert got["exits"] == {le.EXIT_NO_OVER, le.EXIT_LOOP_BREAK, le.EXIT_SCALE_BITCOUNT} and got["compress"] == set(range(16))
    assert got["fired"] == {False, True}
    assert got["mask_bits"] == {(b, v) for b in range(4) for v in (0, 1)} and got["more_iterations"]
    assert got["add_branch"] >= {0, 1, 2} and got["bisect_equal"]
    assert le.GLOBAL_GAIN in got["aborts"]
    # (what only one rate can reach: 2 * 4095 bits of stuffing fit every mono frame but 32 kHz's at 320 kbit/s; a short block's
    # scalefactors pass a granule's budget only at 48 kHz, 32 kbit/s, stereo: 120 bits against 18 * 7)
    assert got["drain"] == (rate == 32000) and (le.HUFF_BITS in got["aborts"]) == (rate == 48000)


@pytest.mark.skipif(not os.path.exists(le.REF_HARNESS_LOOP), reason="oracle/_ref/ref_harness_loop is built only where the reference sources are")
@pytest.mark.parametrize("rate", le.RATES)
def test_oracle_is_the_unmodified_reference(oracle_out, rate, tmp_path):
    """fresh-start chains: every field, scalefactor and declared value of every frame, the reservoir and the addresses at the end;
    where the oracle says the reference dies it dies, in that frame and with that assertion's words, and nowhere else"""
    n, died, sets = {}, set(), set()
    for c, want in oracle_out[rate]:
        k = n[c.set] = n.get(c.set, -1) + 1
        if c.state is not None or k % REF_STRIDE.get(c.set, 1):
            continue
        sets.add(c.set)
        rc, ref, err = le.run_reference(c, str(tmp_path))
        if want.status:
            words = {le.GLOBAL_GAIN: b"global_gain < 256", le.HUFF_BITS: b"max_bits >= 0"}[want.status & 255]
            assert rc == -6 and words in err and len(ref.side) == want.status >> 8, (c.name, rc, err, len(ref.side))
            died.add(want.status & 255)
            continue
        assert rc == 0, (c.name, rc, err)
        msg = le.mismatch(c, want, ref)
        assert msg is None, msg
    assert sets == set(le.SET_NAMES) and le.GLOBAL_GAIN in died and (le.HUFF_BITS in died) == (rate == 48000)


@pytest.mark.parametrize("rate", le.RATES)
def test_emulated_search_is_the_oracle(oracle_out, emu, rate):
    """the hook of the emulated build on the chains marked for it, every set among them: side information, scalefactors, declared
    values, final state and status word; and k_prep's list is not empty where 8 ln sfm sits on a rounding boundary"""
    sub = [(c, r) for c, r in oracle_out[rate] if c.expect.get("emu")]
    assert {c.set for c, _ in sub} == set(le.SET_NAMES)
    want = {id(c): r for c, r in sub}
    for group in le.by_format([c for c, _ in sub]):
        rc, got, listed = le.run_hook(emu.lib, group)
        assert rc == 0, (rc, group[0].name)
        assert not group[0].expect.get("listed") or listed > 0, group[0].name
        for c, r in zip(group, got):
            msg = le.mismatch(c, r, want[id(c)])
            assert msg is None, msg


def _legal(state=False):
    """a small legal chain: stereo, granule 1 the lighter one"""
    rng = np.random.default_rng(7)
    st = np.zeros((), le.STATE_DT) if state else None
    c = le.Chain("X", "legal", 44100, 2, 128, state=st)
    return c.frame([[le.random_granule(rng, loud=0.05)[:2] + (le.BIG, le.BIG, bt) for bt in (0, 2)], [le.random_granule(rng, loud=1e-3)[:2] + (le.BIG, le.BIG, 0)] * 2])


def _psy(c, field, v, k=None):
    if k is None:
        c.psy[0][1, 0][field] = v
    else:
        c.psy[0][1, 0][field][k] = v


def _state(c, field, v, k=None):
    if k is None:
        c.state[field] = v
    else:
        c.state[field][k] = v


BREAKS = {
    "a NaN in xr": (False, lambda c: c.xr[0].__setitem__((1, 1, 5), np.nan)),
    "an infinity in xr": (False, lambda c: c.xr[0].__setitem__((0, 0, 575), -np.inf)),
    "xr above 2^64": (False, lambda c: c.xr[0].__setitem__((0, 1, 0), 2.0 ** 64 * (1 + 2.0 ** -52))),
    "a non-zero xr below 2^-500": (False, lambda c: c.xr[0].__setitem__((0, 1, 7), -2.0 ** -501)),
    "a NaN pe": (False, lambda c: _psy(c, "pe", np.nan)),
    "a negative pe": (False, lambda c: _psy(c, "pe", -1e-300)),
    "pe above 1e8": (False, lambda c: _psy(c, "pe", 1.0000001e8)),
    "an infinite long ratio": (False, lambda c: _psy(c, "ratio_l", np.inf, 20)),
    "a negative long ratio": (False, lambda c: _psy(c, "ratio_l", -1e-9, 0)),
    "a NaN short ratio": (False, lambda c: _psy(c, "ratio_s", np.nan, (11, 2))),
    "a negative short ratio": (False, lambda c: _psy(c, "ratio_s", -1.0, (0, 0))),
    "a ratio above 1e30": (False, lambda c: _psy(c, "ratio_l", 1.1e30, 3)),
    "block type 4": (False, lambda c: _psy(c, "block_type", 4)),
    "block type -1": (False, lambda c: _psy(c, "block_type", -1)),
    "a bitrate that is none": (False, lambda c: setattr(c, "kbps", 100)),
    "ResvSize not a multiple of 8": (True, lambda c: _state(c, "ResvSize", 100)),
    "ResvSize above ResvMax": (True, lambda c: _state(c, "ResvSize", le.resv_max_of(44100, 128) + 8)),
    "a negative ResvSize": (True, lambda c: _state(c, "ResvSize", -8)),
    "a status word already set": (True, lambda c: _state(c, "status", 1)),
    "an address above 576": (True, lambda c: _state(c, "addr", 578, (1, 1, 2))),
    "a stored logarithm beyond 2^20": (True, lambda c: _state(c, "sc_xm", -(1 << 20) - 1, (0, 1, 20))),
    "a start step above the table": (False, lambda c: c.xr[0].__setitem__((1, 0), le._lines([9], 2.0 ** -39))),
}


_LEGAL_RAN = {}


@pytest.mark.parametrize("what", sorted(BREAKS))
def test_hook_refuses_what_lies_outside_its_domain(emu, what):
    """a legal chain with one thing changed: refused before anything is launched; the chain itself passes"""
    state, make = BREAKS[what]
    if state not in _LEGAL_RAN:
        _LEGAL_RAN[state] = le.run_hook(emu.lib, [_legal(state)])[0]
    assert _LEGAL_RAN[state] == 0
    c = _legal(state)
    make(c)
    assert le.run_hook(emu.lib, [c])[0] == ERR_ARG, what


def test_hook_takes_the_ends_of_its_domain(emu, oracle):
    """... and on the bounds themselves it runs, and is the oracle: 2^64 and 2^-500 side by side, pe 1e8, ratios 0 and 1e30, a
    reservoir at ResvMax, a start step of exactly 400 (the reference dies there: global_gain 609)"""
    c = _legal(True)
    c.xr[0][0, 0, 3], c.xr[0][0, 0, 4], c.xr[0][1, 1, 100] = 2.0 ** 64, -2.0 ** -500, -2.0 ** -500
    _psy(c, "pe", 1e8)
    _psy(c, "ratio_l", 1e30, 4)
    _psy(c, "ratio_l", 0.0, 5)
    c.state["ResvSize"] = le.resv_max_of(44100, 128)
    rc, got, _ = le.run_hook(emu.lib, [c])
    assert rc == 0
    msg = le.mismatch(c, got[0], le.run_oracle(oracle.lib, c))
    assert msg is None, msg
    # every state_out is a legal state_in: sc_xrmax is (int) max |xr|, whatever that cast gives above 2^31
    c = _legal(True)
    c.state["sc_xrmax"] = [[-2 ** 31, 2 ** 31 - 1], [7, 0]]
    rc, got, _ = le.run_hook(emu.lib, [c])
    assert rc == 0
    msg = le.mismatch(c, got[0], le.run_oracle(oracle.lib, c))
    assert msg is None, msg
    edge = [c for c in le.chains(44100, oracle.lib) if c.expect.get("q0") == le.STEP_MAX]
    assert len(edge) == 1 and le.host_start_step(edge[0].xr[0][0, 0])[1] == le.STEP_MAX
    rc, got, _ = le.run_hook(emu.lib, edge)
    assert rc == 0 and got[0].status == le.GLOBAL_GAIN == le.run_oracle(oracle.lib, edge[0]).status
