"""The per-slot bookkeeping of both batches (csrc/host_util.h: slot_book) against tests/golden/slot_book_trace.json: what the library
answered to the calls of tests/slot_book_trace.py -- return code and *_batch_slot_frames after every call -- when each batch still
kept its own copy of the rules.  On the emulated build, in this process."""
import json

import pytest

import slot_book_trace as sbt


@pytest.fixture(scope="module")
def trace():
    with open(sbt.TRACE) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def replayed(emu, trace):
    """every sequence of the trace run again, on both layers: {layer: [[[rc, n, frames] per call] per sequence]}"""
    return {layer: [sbt.run(emu.lib, layer, q["calls"]) for q in trace["sequences"]] for layer in (3, 2)}


def test_the_trace_is_the_generators(trace):
    assert (trace["seed"], trace["slots"]) == (sbt.SEED, sbt.S)
    assert [q["calls"] for q in trace["sequences"]] == sbt.as_json(sbt.sequences())


@pytest.mark.parametrize("layer", [3, 2])
def test_trace_is_reproduced(trace, replayed, layer):
    for i, q in enumerate(trace["sequences"]):
        for k, (want, got) in enumerate(zip(q["layer%d" % layer], replayed[layer][i])):
            assert got == want, "sequence %d, call %d %r: %r, recorded %r" % (i, k, q["calls"][k], got, want)
        assert len(replayed[layer][i]) == len(q["calls"]) == len(q["layer%d" % layer])


def test_layers_agree_where_both_accept(trace, replayed):
    both = 0
    for i, q in enumerate(trace["sequences"]):
        for k, (a, b) in enumerate(zip(replayed[3][i], replayed[2][i])):
            if a[0] == 0 and b[0] == 0:
                both += 1
                assert a[1:] == b[1:], "sequence %d, call %d %r: Layer III %r, Layer II %r" % (i, k, q["calls"][k], a, b)
    assert both > 40  # (most calls of the trace are legal ones)
