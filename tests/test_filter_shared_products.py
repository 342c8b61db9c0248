"""k_filter computes one matrixing product for the four subbands g, 15-g, 16+g and 31-g (csrc/k_fbmdct.hip).  That rests
on the 32 x 32 coefficient table mirroring itself bit for bit; every table build checks it (mp3mi_filt_mirror_check,
csrc/tables_host.cpp).  Here: the shipped table has the property, the check refuses a table with one coefficient
altered, and the emulated kernels still return the oracle's subband samples as 64-bit patterns, for seeded PCM and
for rows in which every product is large and the signs of the shared products decide the result."""
import ctypes
import os
import struct

import numpy as np
import pytest

from mp3common import ROOT
from stage_check import compare_stages, run_batch_with_stages

TB_FILT = 5  # csrc/tables_host.cpp: enum { TB_WINDOW = 1, TB_WINDOW_S, TB_S3_L, TB_EXP_SNR_S, TB_FILT, ...
SIGN = np.uint64(1 << 63)


def shipped_filt():
    """The matrixing coefficients as csrc/tables_blob.bin holds them: "MP3MITB1", the entry count, entries of
    (id, rate, offset, size), then the data the offsets count from."""
    blob = open(os.path.join(ROOT, "mp3-enc-bsd_amd", "csrc", "tables_blob.bin"), "rb").read()
    assert blob[:8] == b"MP3MITB1"
    n = struct.unpack_from("<I", blob, 8)[0]
    for i in range(n):
        tid, rate, off, size = struct.unpack_from("<IiII", blob, 16 + 16 * i)
        if tid == TB_FILT:
            assert rate == -1 and size == 32 * 32 * 8
            return np.frombuffer(blob, "<f8", 32 * 32, 16 + 16 * n + off).reshape(32, 32).copy()
    raise AssertionError("the blob has no matrixing table")


def n_of(j):
    return 16 - j if j < 16 else j + 1


def mirror_violations(filt):
    """the three identities on a [32, 32] float64 array, compared as integers"""
    b = np.ascontiguousarray(filt, np.float64).view(np.uint64)
    bad = []
    for g in range(8):
        for j in range(31):
            n = n_of(j)
            flip = SIGN if n & 1 else np.uint64(0)
            if b[31 - g, j] != b[g, j] ^ flip:
                bad.append((31 - g, j))
            if b[16 + g, j] != b[15 - g, j] ^ flip:
                bad.append((16 + g, j))
            if not n & 1 and b[15 - g, j] != b[g, j] ^ (SIGN if (n >> 1) & 1 else np.uint64(0)):
                bad.append((15 - g, j))
    return bad


def lib_check(emu, filt):
    f = emu.lib.mp3mi_filt_mirror_check
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p]
    a = np.ascontiguousarray(filt, np.float64)
    return f(a.ctypes.data)


def test_the_shipped_table_mirrors_itself(emu):
    filt = shipped_filt()
    assert mirror_violations(filt) == []
    assert lib_check(emu, filt) == 0
    # ... and it is the table the formula gives: cos((2i+1) n pi/64) to nine decimals
    for i in range(32):
        for j in range(31):
            assert abs(filt[i, j] - np.cos((2 * i + 1) * n_of(j) * np.pi / 64)) < 0.6e-9, (i, j)


@pytest.mark.parametrize("i,j,how", [(0, 0, "ulp"), (7, 30, "ulp"), (8, 15, "ulp"), (15, 1, "sign"), (16, 16, "ulp"), (23, 2, "ulp"),
                                     (24, 0, "sign"), (31, 30, "ulp"), (12, 8, "zero")])
def test_one_altered_coefficient_is_refused(emu, i, j, how):
    """every row takes part in some identity at every column: a last-bit change, a flipped sign or a zero in any of
    them fails the check (its own code, -14), and the Python restatement agrees on where"""
    filt = shipped_filt()
    b = filt.view(np.uint64)
    if how == "ulp":
        b[i, j] ^= np.uint64(1)
    elif how == "sign":
        b[i, j] ^= SIGN
    else:
        filt[i, j] = 0.0
    assert mirror_violations(filt)
    assert lib_check(emu, filt) == -14


def crafted_rows(n, channels):
    """rows in which every product of the matrixing is large: alternating full scale, constant -32768, one impulse"""
    alt = np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)
    low = np.full(n, -32768, np.int16)
    imp = np.zeros(n, np.int16)
    imp[700] = 32767
    return [np.repeat(r, channels) for r in (alt, low, imp)]


@pytest.mark.parametrize("channels,S,nf", [(1, 1, 1), (2, 4, 2)])
def test_emulated_filter_returns_the_oracles_subband_samples(emu, oracle, channels, S, nf):
    rate, kbps = 44100, 128 if channels == 2 else 64
    rows = [emu.synth(nf * 1152, channels, rate, 40 + channels)] + crafted_rows(nf * 1152, channels)
    pcm = np.stack(rows[:S])
    got, st = run_batch_with_stages(emu, pcm, rate, channels, kbps, nf)
    for s in range(S):
        ref, dumps = oracle.encode(pcm[s], rate, kbps, channels, dumps=nf)
        for f in range(nf):
            for gr in range(2):
                for c in range(channels):
                    a = np.ascontiguousarray(st["sb"][s, 2 * f + gr, c]).view(np.uint64)
                    b = np.ascontiguousarray(dumps[f]["sb"][c, gr]).view(np.uint64)
                    assert np.array_equal(a, b), "stream %d frame %d gr %d ch %d: subband samples differ in %d of 576" % (s, f, gr, c, int(np.sum(a != b)))
        bad = compare_stages(st, s, dumps, channels)  # the psychoacoustic records and everything after them
        assert not bad, bad[:8]
        assert got[s] == ref
