"""The per-slot bookkeeping both batches keep (csrc/host_util.h: slot_book) as a recorded trace: seeded sequences of calls on a Layer III
and a Layer II batch of S slots -- mp3mi_batch_encode_slots / mp3mi_l12_batch_encode_slots with legal, broken and random ctl and
n_samples_host, encode_next, flush, reset and a whole-file call in between -- and after EVERY call its return code and what
*_batch_slot_frames answers.  tests/golden/slot_book_trace.json holds what the library answered BEFORE the book existed (each batch
with its own copy of the rules); tests/test_slot_book.py replays the calls on the emulated build and wants the same answers.

    python tests/slot_book_trace.py [--lib libmp3mi_emu.so] [--write]

records the trace on a build of the emulated library, counts the situations it must contain (COVER) and fails where one is missing.
The calls are a function of SEED alone: a model of the documented rules (include/mp3mi.h) steers them and names the rule a broken
call breaks; nothing of the model is recorded, only the library's answers."""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TRACE = os.path.join(HERE, "golden", "slot_book_trace.json")
SEED, S, RATE, CH, KBPS, MAX_NF, SPF = 11, 3, 44100, 1, 64, 2, 1152  # (Layer II and Layer III: 1152 samples per frame both)
N_RANDOM, N_CALLS = 5, 12
START, END, ILLEGAL = 1, 2, 4
ERR_ARG = -1
# what the recorded trace holds at least once (counted by record())
COVER = ["refused: illegal bit", "refused: END of nothing", "refused: samples for a closed slot", "refused: part of a frame without END",
         "refused: more than the call's frames", "settle hands back", "encode_next, book on, none open", "encode_next, book on, some open",
         "flush, book on, none open"]


def n_of(kind, full):
    """the five n_samples_host values of the issue: 0, 1, full - 1, full, full + 1"""
    return [0, 1, full - 1, full, full + 1][kind]


class Model:
    """the documented rules, to steer the calls and to name what a refused call breaks (never recorded)"""

    def __init__(self):
        self.f, self.on = [-1] * S, False

    def refusal(self, nf, ctl, ns):
        full = nf * SPF
        for s in range(S):
            c = ctl[s]
            if c & ~(START | END):
                return "refused: illegal bit"
            part = self.f[s] >= 0 or bool(c & START)
            if c & END and not part:
                return "refused: END of nothing"
            n = (full if part else 0) if ns is None else ns[s]
            if not part:
                if n != 0:
                    return "refused: samples for a closed slot"
            elif not c & END:
                if n != full:
                    return "refused: part of a frame without END"
            elif n < 0 or n > full:
                return "refused: more than the call's frames"
        return None

    def slots(self, nf, ctl):
        for s in range(S):
            if ctl[s] & START:
                self.f[s] = 0
            if ctl[s] & END:
                self.f[s] = -1
            elif self.f[s] >= 0:
                self.f[s] += nf
        self.on = not (self.f[0] > 0 and all(x == self.f[0] for x in self.f))
        return not self.on  # handed back to the whole-batch counter

    def encode_next(self, nf):
        if any(x >= 0 for x in self.f):
            self.f = [x + nf if x >= 0 else x for x in self.f]
            if self.on:
                self.slots(0, [0] * S)
        else:
            self.f, self.on = [nf] * S, False

    def close(self):
        self.f, self.on = [-1] * S, False


def legal_call(rng, m, nf):
    """a call that keeps every rule in the model's state"""
    full = nf * SPF
    no_ns = rng.random() < 0.3
    ctl, ns = [], []
    for s in range(S):
        if m.f[s] >= 0:
            c = END if rng.random() < 0.3 else (START if rng.random() < 0.1 else 0)
        else:
            c = [0, START, START | END][rng.choice(3, p=[0.4, 0.45, 0.15])]
        part = m.f[s] >= 0 or bool(c & START)
        ctl.append(int(c))
        ns.append(0 if not part else (n_of(int(rng.integers(0, 4)), full) if c & END and not no_ns else full))
    return ctl, (None if no_ns else ns)


def broken_call(rng, m, nf):
    """a legal call with ONE rule broken in one slot"""
    full = nf * SPF
    ctl, ns = legal_call(rng, m, nf)
    ns = [(full if m.f[s] >= 0 or ctl[s] & START else 0) for s in range(S)] if ns is None else ns
    s, how = int(rng.integers(0, S)), int(rng.integers(0, 5))
    part = m.f[s] >= 0 or bool(ctl[s] & START)
    if how == 0:
        ctl[s] |= ILLEGAL
    elif how == 1 and not part:
        ctl[s] = END
    elif how == 2 and not part:
        ns[s] = n_of(int(rng.choice([1, 2, 3, 4])), full)
    elif how == 3 and part and not ctl[s] & END:
        ns[s] = n_of(int(rng.choice([0, 1, 2, 4])), full)
    elif part:
        ctl[s] |= END
        ns[s] = full + 1
    return ctl, ns


def random_call(rng, nf):
    full = nf * SPF
    ctl = [int(c) for c in rng.choice([0, START, END, START | END, ILLEGAL], S)]
    ns = None if rng.random() < 0.3 else [n_of(int(k), full) for k in rng.integers(0, 5, S)]
    return ctl, ns


# the situations of COVER, whatever the random sequences reach
SCRIPTED = [
    [("slots", 1, [START, START, START], None), ("next", 2), ("slots", 1, [0, END, 0], [SPF, 1, SPF]), ("next", 1), ("flush",),
     ("slots", 2, [START | END, 0, START | END], [2 * SPF, 0, 0]), ("next", 1), ("slots", 1, [START, END, 0], None), ("flush",), ("flush",)],
    [("slots", 1, [START, 0, 0], None), ("slots", 1, [END, START | END, 0], [0, SPF - 1, 0]), ("flush",), ("slots", 1, [0, START, 0], None),
     ("encode", 2), ("next", 1), ("slots", 2, [END, 0, 0], [2 * SPF + 1, 2 * SPF, 2 * SPF]), ("slots", 2, [END, 0, 0], [2 * SPF, 2 * SPF, 2 * SPF]),
     ("reset",), ("slots", 1, [0, 0, END], None), ("slots", 1, [ILLEGAL, 0, 0], None), ("slots", 1, [0, 0, 0], [0, 1, 0]),
     ("slots", 1, [START, 0, 0], [SPF - 1, 0, 0])],
]


def sequences():
    """the calls of the trace: [[(op, ...)]], a function of SEED"""
    rng = np.random.default_rng(SEED)
    seqs = [list(q) for q in SCRIPTED]
    for _ in range(N_RANDOM):
        m, seq = Model(), []
        for _ in range(N_CALLS):
            nf = int(rng.integers(1, MAX_NF + 1))
            kind = rng.choice(["legal", "broken", "random", "next", "flush", "reset", "encode"], p=[0.4, 0.15, 0.1, 0.15, 0.1, 0.04, 0.06])
            if kind in ("legal", "broken", "random"):
                ctl, ns = legal_call(rng, m, nf) if kind == "legal" else broken_call(rng, m, nf) if kind == "broken" else random_call(rng, nf)
                seq.append(("slots", nf, ctl, ns))
                if m.refusal(nf, ctl, ns) is None:
                    m.slots(nf, ctl)
            elif kind == "next":
                seq.append(("next", nf))
                m.encode_next(nf)
            elif kind == "encode":
                seq.append(("encode", nf))
                m.close()
            else:
                seq.append((str(kind),))
                m.close()
        seqs.append(seq)
    return seqs


class Batch:
    """a batch of S slots of `layer` (3 or 2) on the emulated library: its memory is host memory, the PCM silence"""

    def __init__(self, lib, layer):
        vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        self.lib, self.b = lib, vp()
        p = "mp3mi_batch_" if layer == 3 else "mp3mi_l12_batch_"
        self.fn = {k: getattr(lib, p + k) for k in ("destroy", "out_stride", "encode", "encode_next", "encode_slots", "flush", "reset",
                                                    "slot_frames", "sync")}
        self.fn["out_stride"].restype = sz
        self.fn["out_stride"].argtypes = [vp, ci]
        self.fn["destroy"].argtypes = self.fn["reset"].argtypes = self.fn["sync"].argtypes = [vp]
        self.fn["encode_next"].argtypes = [vp, vp, ci, vp, sz, vp]
        self.fn["encode_slots"].argtypes = [vp, vp, ci, vp, vp, vp, sz, vp]
        self.fn["flush"].argtypes = [vp, vp, sz, vp]
        self.fn["slot_frames"].argtypes = [vp, vp]
        if layer == 3:
            lib.mp3mi_batch_create.argtypes = [ctypes.POINTER(vp), ci, ci, ci, vp, ci, ci]
            self.fn["encode"].argtypes = [vp, vp, ci, vp, sz, vp]
            assert lib.mp3mi_batch_create(ctypes.byref(self.b), S, RATE, CH, None, KBPS, MAX_NF) == 0
            self.whole = lambda nf: self.fn["encode"](self.b, self.pcm.ctypes.data, nf, self.out.ctypes.data, self.stride, self.len.ctypes.data)
        else:
            lib.mp3mi_l12_batch_create.argtypes = [ctypes.POINTER(vp)] + [ci] * 4 + [vp, ci, ci, ctypes.c_uint]
            self.fn["encode"].argtypes = [vp] * 3 + [ci, vp, sz, vp]
            assert lib.mp3mi_l12_batch_create(ctypes.byref(self.b), layer, S, RATE, CH, None, KBPS, MAX_NF, 0) == 0
            self.whole = lambda nf: self.fn["encode"](self.b, self.pcm.ctypes.data, None, nf, self.out.ctypes.data, self.stride, self.len.ctypes.data)
        self.stride = self.fn["out_stride"](self.b, MAX_NF)
        self.pcm = np.zeros(S * MAX_NF * SPF * CH, np.int16)
        self.out = np.zeros(S * self.stride, np.uint8)
        self.len = np.zeros(S, np.uint32)

    def call(self, op):
        """one call of a sequence: [its return code, *_batch_slot_frames' return value, its vector]"""
        io = (self.out.ctypes.data, self.stride, self.len.ctypes.data)
        if op[0] == "slots":
            ctl = np.array(op[2], np.uint8)
            ns = None if op[3] is None else np.array(op[3], np.int32)
            rc = self.fn["encode_slots"](self.b, self.pcm.ctypes.data, op[1], ctl.ctypes.data, None if ns is None else ns.ctypes.data, *io)
        elif op[0] == "next":
            rc = self.fn["encode_next"](self.b, self.pcm.ctypes.data, op[1], *io)
        elif op[0] == "encode":
            rc = self.whole(op[1])
        else:
            rc = self.fn[op[0]](self.b, *io) if op[0] == "flush" else self.fn["reset"](self.b)
        f = np.full(S, -7, np.int64)
        n = self.fn["slot_frames"](self.b, f.ctypes.data)
        return [int(rc), int(n), [int(x) for x in f]]

    def close(self):
        assert self.fn["sync"](self.b) == 0
        self.fn["destroy"](self.b)


def run(lib, layer, seq):
    b = Batch(lib, layer)
    try:
        return [b.call(op) for op in seq]
    finally:
        b.close()


def as_json(seqs):
    return [[list(op) for op in seq] for seq in seqs]


def record(lib):
    """the trace of `lib`, and how often it holds each situation of COVER (the model says where to look, the library what happened)"""
    count = dict.fromkeys(COVER, 0)
    out = []
    for seq in sequences():
        got = {layer: run(lib, layer, seq) for layer in (3, 2)}
        m = Model()
        for k, op in enumerate(seq):
            open_before = sum(x >= 0 for x in m.f)
            if op[0] == "slots":
                why = m.refusal(op[1], op[2], op[3])
                for layer in (3, 2):
                    assert (got[layer][k][0] == ERR_ARG) == (why is not None) and got[layer][k][0] in (0, ERR_ARG), (layer, op, got[layer][k])
                if why:
                    count[why] += 1
                elif m.slots(op[1], op[2]):
                    count["settle hands back"] += 1
            elif op[0] == "next":
                if m.on:
                    count["encode_next, book on, some open" if open_before else "encode_next, book on, none open"] += 1
                m.encode_next(op[1])
            else:
                if op[0] == "flush" and m.on and not open_before:
                    count["flush, book on, none open"] += 1
                m.close()
            for layer in (3, 2):  # the model follows the library, or the counts above are of something else
                assert got[layer][k][2] == m.f, (layer, k, op, got[layer][k], m.f)
        out.append({"calls": as_json([seq])[0], "layer3": got[3], "layer2": got[2]})
    return {"seed": SEED, "slots": S, "sequences": out}, count


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(HERE, "hipemu", "_build", "libmp3mi_emu.so"))
    ap.add_argument("--write", action="store_true", help="write tests/golden/slot_book_trace.json")
    a = ap.parse_args()
    trace, count = record(ctypes.CDLL(a.lib))
    for k in COVER:
        print("%4d  %s" % (count[k], k))
    print("%d sequences, %d calls" % (len(trace["sequences"]), sum(len(q["calls"]) for q in trace["sequences"])))
    missing = [k for k in COVER if not count[k]]
    if missing:
        sys.exit("the trace lacks: " + "; ".join(missing))
    if a.write:
        with open(TRACE, "w") as fh:
            json.dump(trace, fh, separators=(",", ":"))
            fh.write("\n")
        print("wrote", TRACE)
