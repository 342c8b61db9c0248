"""k_filter (shared matrixing products, csrc/k_fbmdct.hip) and k_cw (items laid across wavefronts, csrc/k_fft.hip) at the
smallest shapes at which they can go wrong: partial blocks, grids that are no multiple of 16, a continued batch, a ragged
stream, record boundaries inside a wavefront, a partial last wavefront.  Every case against the oracle: the subband samples
as 64-bit patterns, the psychoacoustic records, the bytes.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import ctypes

from mp3common import PSY_DT, SIDE_DT, BatchRun
from stage_check import compare_stages, run_batch_with_stages

pytestmark = pytest.mark.gpu

RATE = 44100


def crafted_rows(n, channels):
    """every product of the matrixing large, the signs of the shared products decide: alternating full scale,
    constant -32768, one full-scale impulse"""
    alt = np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)
    low = np.full(n, -32768, np.int16)
    imp = np.zeros(n, np.int16)
    imp[700] = 32767
    return [np.repeat(r, channels) for r in (alt, low, imp)]


def assert_stages(st, s, dumps, channels):
    """the subband samples (what = 4) as 64-bit patterns, then the psychoacoustic records (what = 0) and every later
    seam; st holds the frames of ONE call, dumps the oracle's records of the same frames"""
    for f in range(len(dumps)):
        for gr in range(2):
            for c in range(channels):
                a = np.ascontiguousarray(st["sb"][s, 2 * f + gr, c]).view(np.uint64)
                b = np.ascontiguousarray(dumps[f]["sb"][c, gr]).view(np.uint64)
                assert np.array_equal(a, b), "stream %d frame %d gr %d ch %d: %d of 576 subband samples differ" % (s, f, gr, c, int(np.sum(a != b)))
    bad = compare_stages(st, s, dumps, channels)
    assert not bad, bad[:8]


def check_against_oracle(product, oracle, pcm, channels, kbps, nf, flags=0):
    got, st = run_batch_with_stages(product, pcm, RATE, channels, kbps, nf, flags=flags)
    for s in range(pcm.shape[0]):
        ref, dumps = oracle.encode(pcm[s], RATE, kbps, channels, dumps=nf)
        assert_stages(st, s, dumps, channels)
        assert got[s] == ref, "stream %d: bytes differ" % s
    return got


def fetch_stages(run, nfp):
    """the stage seams of the last call of a BatchRun (nfp frames in one chunk), as run_batch_with_stages returns them"""
    S, G, C = run.S, 2 * nfp, run.ch
    st = {"psy": np.zeros((S, G, C), PSY_DT), "xr": np.zeros((S, G, C, 576)), "ix": np.zeros((S, G, C, 576), np.int16),
          "side": np.zeros((S, nfp), SIDE_DT), "sb": np.zeros((S, G, C, 18, 32))}
    for what, key in ((0, "psy"), (1, "xr"), (2, "ix"), (3, "side"), (4, "sb")):
        n = run.mp.lib.mp3mi_batch_debug_fetch(run.b, what, st[key].ctypes.data, st[key].nbytes)
        assert n == st[key].nbytes, (key, n, st[key].nbytes)
    return st


def test_mono_one_frame_one_partial_block(product, oracle):
    """k_filter: 54 slots in one block of 64.  k_cw: 2 records = 100 + 12 items, a record boundary inside the first
    wavefront, the long lines behind the values in the second, which is partial"""
    pcm = product.synth(1152, 1, RATE, 11)[None, :]
    check_against_oracle(product, oracle, pcm, 1, 64, 1)


@pytest.mark.parametrize("flags", [2, 32], ids=["phase_exact", "cw_exact"])
def test_mono_one_frame_with_the_exact_tiers(product, oracle, flags):
    """the same with the correctly rounded atan2 only (MP3MI_TEST_PHASE_EXACT = 2) and with the second tier's sines and
    cosines for every value (MP3MI_TEST_CW_EXACT = 32): the bytes of the plain run"""
    pcm = product.synth(1152, 1, RATE, 11)[None, :]
    plain = check_against_oracle(product, oracle, pcm, 1, 64, 1)
    assert check_against_oracle(product, oracle, pcm, 1, 64, 1, flags=flags) == plain


def test_stereo_crafted_rows_four_frames(product, oracle):
    """k_filter: 3 streams stereo x 4 frames -- 162 slots a track, the last block 34 slots, a grid of 18 (no multiple of 16:
    the fallback block order too); the seeded generator would do, the crafted rows ask more of the signs"""
    nf = 4
    pcm = np.stack(crafted_rows(nf * 1152, 2))
    check_against_oracle(product, oracle, pcm, 2, 128, nf)


def test_stereo_three_streams_two_frames(product, oracle):
    """k_cw: 24 records, 1200 + 144 items = 18.75 wavefronts of values; k_filter: the seeded generator"""
    nf = 2
    pcm = np.stack([product.synth(nf * 1152, 2, RATE, 20 + s) for s in range(3)])
    check_against_oracle(product, oracle, pcm, 2, 128, nf)


def test_a_batch_continued_by_a_second_call(product, oracle):
    """the second call's first block starts in the history granule; the first call's lies before the stream (gi_first).
    The seams of each call against the oracle's records of the same frames, the bytes of both calls and the flush"""
    nf, S, C, piece = 4, 3, 2, 2
    run = BatchRun(product, S, RATE, C, 128, nf, stream0=30)
    L = product.lib
    try:
        L.mp3mi_batch_debug_enable(run.b, 1)
        refs = [oracle.encode(run.pcm_of(s), RATE, 128, C, dumps=nf) for s in range(S)]
        whole = run.mem.download(run.d_pcm, (S, nf * 1152 * C), np.int16)
        got = [b""] * S

        def collect():
            assert L.mp3mi_batch_sync(run.b) == 0
            out = run.mem.download(run.d_out, (S, run.stride), np.uint8)
            lens = run.mem.download(run.d_len, (S,), np.uint32)
            for s in range(S):
                got[s] += out[s, :lens[s]].tobytes()

        for f0 in range(0, nf, piece):
            part = np.ascontiguousarray(whole[:, f0 * 1152 * C:(f0 + piece) * 1152 * C])
            d_part = run.mem.alloc(part.nbytes)
            run.mem.upload(d_part, part)
            assert L.mp3mi_batch_encode_next(run.b, d_part, piece, run.d_out, run.stride, run.d_len) == 0
            collect()
            st = fetch_stages(run, piece)
            for s in range(S):
                assert_stages(st, s, refs[s][1][f0:f0 + piece], C)
        assert L.mp3mi_batch_flush(run.b, run.d_out, run.stride, run.d_len) == 0
        collect()
        for s in range(S):
            assert got[s] == refs[s][0], "stream %d: bytes differ" % s
    finally:
        run.close()


def test_a_ragged_stream_ends_inside_a_block(product, oracle):
    """n_samples ends inside a block of 64 slots: the slow load path, and the tail reads as zero (what lies beyond
    n_samples in the buffer is the generator's, and must be ignored)"""
    nf, C, n = 3, 2, 2 * 1152 + 333
    pcm = np.stack([product.synth(nf * 1152, C, RATE, 50), product.synth(nf * 1152, C, RATE, 51)])
    n_samples = np.array([n, nf * 1152], np.int32)
    run = BatchRun(product, 2, RATE, C, 128, nf, pcm=pcm)
    L = product.lib
    L.mp3mi_batch_encode_ragged.restype = ctypes.c_int
    L.mp3mi_batch_encode_ragged.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    try:
        L.mp3mi_batch_debug_enable(run.b, 1)
        d_ns = run.mem.alloc(n_samples.nbytes)
        run.mem.upload(d_ns, n_samples)
        assert L.mp3mi_batch_encode_ragged(run.b, run.d_pcm, d_ns, nf, run.d_out, run.stride, run.d_len) == 0
        assert L.mp3mi_batch_sync(run.b) == 0
        out = run.mem.download(run.d_out, (2, run.stride), np.uint8)
        lens = run.mem.download(run.d_len, (2,), np.uint32)
        st = fetch_stages(run, nf)
        for s in range(2):
            ref, dumps = oracle.encode(pcm[s, :int(n_samples[s]) * C], RATE, 128, C, dumps=nf)
            assert_stages(st, s, dumps, C)
            assert out[s, :lens[s]].tobytes() == ref, "stream %d: bytes differ" % s
    finally:
        run.close()


def test_silence_beside_a_live_stream(product, oracle):
    """every c_w of the silent stream is an exact zero, marked -0.0 by k_cw: its records stay off the second tier's list"""
    nf = 2
    live = product.synth(nf * 1152, 2, RATE, 60)
    pcm = np.stack([np.zeros_like(live), live])
    check_against_oracle(product, oracle, pcm, 2, 128, nf)
    run = BatchRun(product, 1, RATE, 2, 128, nf, pcm=pcm[:1])
    try:
        run.encode()
        listed, records = run.cw_fixups()
        assert listed == 0, "%d of %d records of the silent stream listed for the second tier" % (listed, records)
    finally:
        run.close()
