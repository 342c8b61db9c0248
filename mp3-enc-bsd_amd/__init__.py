"""mp3-enc-bsd_amd: MI355X-native MPEG-1 Layer III encoding hot path.

The product is the C-ABI shared library next to this file (libmp3mi.so, built from csrc/ by
`make -C csrc` or `__graft_entry__.build()`); this module is only a thin ctypes binding used by
bench.py, smoke() and the tests.  There is no Python or CPU implementation of the path here:
if the library or a GPU is missing, everything fails loudly.

Import with importlib (the directory name carries a hyphen):
    mp3 = importlib.import_module("mp3-enc-bsd_amd")
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MP3MI_LIB: another build of the same library (tools/gpu_ab.sh: A/B of two builds on one device; tools/gpu_loop_profile.sh:
# a diagnostic build) -- so that measurements never overwrite the product library
LIB_PATH = os.environ.get("MP3MI_LIB") or os.path.join(_HERE, "libmp3mi.so")
FRAME_SAMPLES = 1152


class Mp3miError(RuntimeError):
    pass


class ReferenceAborts(Mp3miError):
    """mp3mi_batch_sync returned MP3MI_ERR_REFERENCE_ABORT: the work is done, but the reference would have died on
    at least one stream's input (include/mp3mi.h); that stream's out_len is 0, Batch.stream_status() says why."""


ERR_REFERENCE_ABORT = -6


class BatchOptions(ctypes.Structure):
    """include/mp3mi.h: mp3mi_batch_options"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("scratch_mb", ctypes.c_uint32), ("chunk_frames", ctypes.c_int32),
                ("test_flags", ctypes.c_uint32), ("dropin_lookahead", ctypes.c_int32), ("call_hold", ctypes.c_int32),
                ("dropin_stats", ctypes.c_int32), ("abi", ctypes.c_uint32)]


class SlotTicket(ctypes.Structure):
    """include/mp3mi.h: mp3mi_slot_ticket -- what the host knows of a parked stream (Batch.export_slots / import_slots)"""
    _fields_ = [("magic", ctypes.c_uint32), ("version", ctypes.c_uint32), ("state_bytes", ctypes.c_uint64),
                ("rate_hz", ctypes.c_int32), ("channels", ctypes.c_int32), ("hdr_mode", ctypes.c_int32), ("hdr_flags", ctypes.c_int32),
                ("error_protection", ctypes.c_int32), ("kbps", ctypes.c_int32), ("frames", ctypes.c_int64)]


class SlotTicketL12(ctypes.Structure):
    """include/mp3mi_l12.h: mp3mi_l12_slot_ticket -- what the host knows of a parked Layer I / II stream (BatchL12.export_slots /
    import_slots)"""
    _fields_ = [("magic", ctypes.c_uint32), ("version", ctypes.c_uint32), ("state_bytes", ctypes.c_uint64), ("layer", ctypes.c_int32),
                ("rate_hz", ctypes.c_int32), ("channels", ctypes.c_int32), ("hdr_mode", ctypes.c_int32), ("hdr_flags", ctypes.c_int32),
                ("error_protection", ctypes.c_int32), ("kbps", ctypes.c_int32), ("reserved", ctypes.c_int32), ("frames", ctypes.c_int64)]


def default_options(**kw):
    o = BatchOptions()
    lib().mp3mi_batch_options_default(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


_lib = None


def lib():
    """Load libmp3mi.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Mp3miError("libmp3mi.so not found at %s -- run __graft_entry__.build()" % LIB_PATH)
        # PyTorch bundles its own HIP runtime.  Load torch first (when it is installed) so that this
        # process has ONE runtime whatever the caller's import order: libmp3mi.so then binds to the
        # already loaded libamdhip64 instead of bringing in a second one that sees no device.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        L.mp3mi_batch_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.mp3mi_batch_create_ex.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.mp3mi_batch_options_default.argtypes = [ctypes.c_void_p]
        L.mp3mi_batch_options_from_env.argtypes = [ctypes.c_void_p]
        L.mp3mi_batch_stream_status.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.mp3mi_batch_destroy.argtypes = [ctypes.c_void_p]
        L.mp3mi_batch_out_stride.restype = ctypes.c_size_t
        L.mp3mi_batch_out_stride.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.mp3mi_batch_encode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_batch_sync.argtypes = [ctypes.c_void_p]
        L.mp3mi_batch_encode_host_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_batch_host_io_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.mp3mi_host_alloc.argtypes = [ctypes.c_size_t]
        L.mp3mi_host_alloc.restype = ctypes.c_void_p
        L.mp3mi_host_free.argtypes = [ctypes.c_void_p]
        L.mp3mi_batch_last_timing.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float),
                                              ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
        L.mp3mi_batch_total_timing.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                               ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long)]
        L.mp3mi_synth_pcm.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
        L.mp3mi_synth_pcm_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
        L.mp3mi_batch_set_test_flags.argtypes = [ctypes.c_void_p, ctypes.c_uint]
        L.mp3mi_batch_encode_next.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_batch_flush.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_batch_reset.argtypes = [ctypes.c_void_p]
        L.mp3mi_batch_encode_slots.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_batch_slot_frames.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.mp3mi_batch_encode_slots_kbps.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_batch_slot_kbps.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.mp3mi_batch_slot_state_bytes.restype = ctypes.c_size_t
        L.mp3mi_batch_slot_state_bytes.argtypes = [ctypes.c_void_p]
        L.mp3mi_batch_slots_export.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                               ctypes.c_void_p]
        L.mp3mi_batch_slots_import.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_feed_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.mp3mi_feed_destroy.argtypes = [ctypes.c_void_p]
        L.mp3mi_feed_destroy.restype = None
        L.mp3mi_feed_capacity.restype = ctypes.c_size_t
        L.mp3mi_feed_capacity.argtypes = [ctypes.c_void_p]
        L.mp3mi_feed_tick.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_feed_lanes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.mp3mi_feed_create_lanes.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p] + [ctypes.c_int] * 5
        L.mp3mi_feed_n_lanes.argtypes = [ctypes.c_void_p]
        L.mp3mi_feed_tick_lanes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        L.mp3mi_feed_tick_lanes_host_async.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_size_t] + [ctypes.c_void_p] * 4
        L.mp3mi_feed_host_wait.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.mp3mi_feed_host_io_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.mp3mi_batch_encode_slots_host_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_batch_encode_slots_kbps_host_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                               ctypes.c_void_p]
        L.mp3mi_batch_host_wait.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.mp3mi_batch_set_mode.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.mp3mi_batch_set_error_protection.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.mp3mi_batch_set_header.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        # Layers I and II (include/mp3mi_l12.h)
        L.mp3mi_l12_batch_create.argtypes = [ctypes.POINTER(ctypes.c_void_p)] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint]
        L.mp3mi_l12_batch_destroy.argtypes = [ctypes.c_void_p]
        L.mp3mi_l12_batch_set_mode.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.mp3mi_l12_batch_set_error_protection.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.mp3mi_l12_batch_set_header.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.mp3mi_l12_batch_set_test_flags.argtypes = [ctypes.c_void_p, ctypes.c_uint]
        L.mp3mi_l12_batch_out_stride.restype = ctypes.c_size_t
        L.mp3mi_l12_batch_out_stride.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.mp3mi_l12_batch_encode.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_l12_batch_sync.argtypes = [ctypes.c_void_p]
        L.mp3mi_l12_batch_encode_next.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_l12_batch_flush.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_l12_batch_reset.argtypes = [ctypes.c_void_p]
        L.mp3mi_l12_batch_encode_slots.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_l12_batch_slot_frames.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.mp3mi_l12_batch_encode_slots_kbps.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_l12_batch_slot_kbps.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.mp3mi_l12_batch_slot_state_bytes.restype = ctypes.c_size_t
        L.mp3mi_l12_batch_slot_state_bytes.argtypes = [ctypes.c_void_p]
        L.mp3mi_l12_batch_slots_export.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                                   ctypes.c_void_p]
        L.mp3mi_l12_batch_slots_import.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.mp3mi_l12_batch_total_timing.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]
        L.mp3mi_l12_feed_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p] + [ctypes.c_int] * 5
        L.mp3mi_l12_feed_destroy.argtypes = [ctypes.c_void_p]
        L.mp3mi_l12_feed_destroy.restype = None
        L.mp3mi_l12_feed_capacity.restype = ctypes.c_size_t
        L.mp3mi_l12_feed_capacity.argtypes = [ctypes.c_void_p]
        L.mp3mi_l12_feed_n_lanes.argtypes = [ctypes.c_void_p]
        L.mp3mi_l12_feed_tick.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        L.mp3mi_l12_feed_lanes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.mp3mi_l12_batch_kernel_timing.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.mp3mi_version.restype = ctypes.c_char_p
        L.mp3mi_source_hash.restype = ctypes.c_char_p
        _lib = L
    return _lib


def frame_bytes(rate_hz, kbps):
    """slots per frame, never padded (reference: src/musicin.c:562-581)"""
    return int((1152.0 / (rate_hz / 1000.0)) * (kbps / 8.0))


def synth_pcm_device(pcm, n_per_ch, channels, rate_hz, stream0=0, seed=0x6D70336D):
    """Fill the int16 cuda tensor pcm [S, n_per_ch*channels] with the deterministic synthetic PCM of streams
    stream0 .. stream0+S-1 (csrc/pcm_synth_core.h: the same bytes as the host's mp3mi_synth_pcm)."""
    assert pcm.is_cuda and pcm.is_contiguous() and pcm.shape[1] == n_per_ch * channels
    rc = lib().mp3mi_synth_pcm_device(pcm.data_ptr(), pcm.shape[0], n_per_ch, channels, rate_hz, stream0, seed)
    if rc != 0:
        raise Mp3miError("mp3mi_synth_pcm_device failed with %d" % rc)


class Batch:
    """Batched encoder over device memory handed in as torch tensors (device pointers)."""

    def __init__(self, n_streams, rate_hz, channels, kbps, max_frames, options=None):
        """options: a BatchOptions (mp3mi_batch_create_ex: no environment variable is read), or None
        (mp3mi_batch_create: the defaults, overridden by the MP3MI_* variables of tools/ and tests/)"""
        import numpy as np
        self.L = lib()
        self.n_streams, self.rate_hz, self.channels, self.max_frames = n_streams, rate_hz, channels, max_frames
        self.h = ctypes.c_void_p()
        arr = None if isinstance(kbps, int) else np.ascontiguousarray(kbps, dtype=np.int32)
        karg, kall = (None, kbps) if arr is None else (arr.ctypes.data, 0)
        if options is None:
            rc = self.L.mp3mi_batch_create(ctypes.byref(self.h), n_streams, rate_hz, channels, karg, kall, max_frames)
        else:
            rc = self.L.mp3mi_batch_create_ex(ctypes.byref(self.h), n_streams, rate_hz, channels, karg, kall, max_frames, ctypes.byref(options))
        if rc != 0:
            raise Mp3miError("mp3mi_batch_create failed with %d" % rc)

    def set_test_flags(self, flags):
        """force the exact tier of the two-tier decisions (include/mp3mi.h, MP3MI_TEST_*)"""
        rc = self.L.mp3mi_batch_set_test_flags(self.h, flags)
        if rc != 0:
            raise Mp3miError("mp3mi_batch_set_test_flags failed with %d" % rc)

    def out_stride(self, n_frames):
        return self.L.mp3mi_batch_out_stride(self.h, n_frames)

    def encode(self, pcm, n_frames, out, out_len):
        """pcm: int16 cuda tensor [S, n_frames*1152*C]; out: uint8 cuda [S, stride]; out_len: int32 cuda [S]."""
        assert pcm.is_cuda and out.is_cuda and out_len.is_cuda and pcm.is_contiguous() and out.is_contiguous()
        rc = self.L.mp3mi_batch_encode(self.h, pcm.data_ptr(), n_frames, out.data_ptr(), out.shape[1], out_len.data_ptr())
        if rc != 0:
            raise Mp3miError("mp3mi_batch_encode failed with %d" % rc)

    def _check(self, rc, what):
        if rc != 0:
            raise Mp3miError("%s failed with %d" % (what, rc))

    def encode_host_async(self, pcm, n_frames, out, out_len):
        """Host tensors in and out (pinned: torch's pin_memory), PCM up and file bytes down chunk by chunk beside the
        kernels (mp3mi_batch_encode_host_async); the results are there after sync()."""
        assert not pcm.is_cuda and not out.is_cuda and not out_len.is_cuda and pcm.is_contiguous() and out.is_contiguous()
        self._check(self.L.mp3mi_batch_encode_host_async(self.h, pcm.data_ptr(), n_frames, out.data_ptr(), out.shape[1], out_len.data_ptr()),
                    "mp3mi_batch_encode_host_async")

    def host_io_stats(self):
        """{h2d_bytes, d2h_bytes, h2d_ms, d2h_ms, calls} over the host-buffer calls so far (waits for them)"""
        class S(ctypes.Structure):
            _fields_ = [("h2d_bytes", ctypes.c_double), ("d2h_bytes", ctypes.c_double), ("h2d_ms", ctypes.c_double), ("d2h_ms", ctypes.c_double), ("calls", ctypes.c_long)]
        st = S()
        self._check(self.L.mp3mi_batch_host_io_stats(self.h, ctypes.byref(st)), "mp3mi_batch_host_io_stats")
        return {k: getattr(st, k) for k, _ in S._fields_}

    def encode_next(self, pcm, n_frames, out, out_len):
        """Streaming: the NEXT n_frames frames of every stream (pcm holds only these); out / out_len receive the file
        bytes that became final with this call.  Concatenate them call after call, then flush()."""
        assert pcm.is_cuda and out.is_cuda and out_len.is_cuda and pcm.is_contiguous() and out.is_contiguous()
        self._check(self.L.mp3mi_batch_encode_next(self.h, pcm.data_ptr(), n_frames, out.data_ptr(), out.shape[1], out_len.data_ptr()),
                    "mp3mi_batch_encode_next")

    def flush(self, out, out_len):
        """III_FlushBitstream + close_bit_stream_w: the remaining bytes of every stream; ends the streams."""
        self._check(self.L.mp3mi_batch_flush(self.h, out.data_ptr(), out.shape[1], out_len.data_ptr()), "mp3mi_batch_flush")

    def reset(self):
        self._check(self.L.mp3mi_batch_reset(self.h), "mp3mi_batch_reset")

    def encode_slots(self, pcm, n_frames, out, out_len, start=None, end=None, n_samples=None, kbps=None):
        """Continuous batching (mp3mi_batch_encode_slots): every stream index is a slot in which one stream after another
        begins (start[s] true: with this call's first sample, from fresh state) and ends (end[s] true: this call holds its last
        n_samples[s] samples per channel).  start / end: boolean sequences of n_streams (None: all false); n_samples: an int
        sequence (None: a full call for every open or starting slot, 0 for the others).  Tensors as for encode_next; out /
        out_len receive per slot the bytes of its file that became final with this call (0 for a closed slot).  kbps: an int
        sequence, per slot the bitrate of the stream that STARTs there (0: the slot's create-time bitrate; at most the largest
        bitrate the batch was created with) and 0 or the open stream's own bitrate elsewhere (mp3mi_batch_encode_slots_kbps);
        None: the call without it."""
        import numpy as np
        assert pcm.is_cuda and out.is_cuda and out_len.is_cuda and pcm.is_contiguous() and out.is_contiguous()
        S = self.n_streams
        ctl = np.zeros(S, np.uint8)
        if start is not None:
            ctl |= np.asarray(start, dtype=bool).reshape(S).astype(np.uint8) * 1  # MP3MI_SLOT_START
        if end is not None:
            ctl |= np.asarray(end, dtype=bool).reshape(S).astype(np.uint8) * 2  # MP3MI_SLOT_END
        ns = None if n_samples is None else np.ascontiguousarray(n_samples, dtype=np.int32).reshape(S)
        if kbps is not None:
            kb = np.ascontiguousarray(kbps, dtype=np.int32).reshape(S)
            self._check(self.L.mp3mi_batch_encode_slots_kbps(self.h, pcm.data_ptr(), n_frames, ctl.ctypes.data, None if ns is None else ns.ctypes.data,
                                                             kb.ctypes.data, out.data_ptr(), out.shape[1], out_len.data_ptr()),
                        "mp3mi_batch_encode_slots_kbps")
            return
        self._check(self.L.mp3mi_batch_encode_slots(self.h, pcm.data_ptr(), n_frames, ctl.ctypes.data, None if ns is None else ns.ctypes.data,
                                                    out.data_ptr(), out.shape[1], out_len.data_ptr()), "mp3mi_batch_encode_slots")

    def encode_slots_host(self, pcm, n_frames, out, out_len, rows=None, start=None, end=None, n_samples=None, kbps=None):
        """Continuous batching on host buffers that hold a row per LIVE slot (mp3mi_batch_encode_slots_host_async): rows is the
        strictly increasing sequence of the rows' slots (None: a row per slot), and start / end / n_samples / kbps are as for
        encode_slots but indexed by ROW.  pcm int16 [n_rows, n_frames*1152*C], out uint8 [n_rows, stride], out_len int32 or
        uint32 [n_rows]: CPU tensors (pinned ones overlap with the kernels) or numpy arrays, which must stay alive until the
        call's results have been waited for (host_wait, sync).  Only the rows cross PCIe."""
        import numpy as np

        def ptr(a):
            if isinstance(a, np.ndarray):
                assert a.flags.c_contiguous
                return a.ctypes.data
            assert not a.is_cuda and a.is_contiguous()
            return a.data_ptr()
        R = self.n_streams if rows is None else len(rows)
        assert pcm.shape[0] == R and out.shape[0] == R and out_len.shape[0] == R and pcm.dtype.itemsize == 2 and out_len.dtype.itemsize == 4
        rows_a = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32).reshape(R)
        ctl = np.zeros(R, np.uint8)
        if start is not None:
            ctl |= np.asarray(start, dtype=bool).reshape(R).astype(np.uint8) * 1  # MP3MI_SLOT_START
        if end is not None:
            ctl |= np.asarray(end, dtype=bool).reshape(R).astype(np.uint8) * 2  # MP3MI_SLOT_END
        ns = None if n_samples is None else np.ascontiguousarray(n_samples, dtype=np.int32).reshape(R)
        if kbps is not None:
            kb = np.ascontiguousarray(kbps, dtype=np.int32).reshape(R)
            self._check(self.L.mp3mi_batch_encode_slots_kbps_host_async(self.h, ptr(pcm), n_frames, R, None if rows_a is None else rows_a.ctypes.data,
                                                                        ctl.ctypes.data, None if ns is None else ns.ctypes.data, kb.ctypes.data,
                                                                        ptr(out), out.shape[1], ptr(out_len)), "mp3mi_batch_encode_slots_kbps_host_async")
            return
        self._check(self.L.mp3mi_batch_encode_slots_host_async(self.h, ptr(pcm), n_frames, R, None if rows_a is None else rows_a.ctypes.data,
                                                               ctl.ctypes.data, None if ns is None else ns.ctypes.data, ptr(out), out.shape[1],
                                                               ptr(out_len)), "mp3mi_batch_encode_slots_host_async")

    def host_wait(self, calls_back=0):
        """waits until the host-buffer call issued calls_back calls ago (0: the latest, 1: the one before) has delivered its
        out / out_len, and for nothing later (mp3mi_batch_host_wait)"""
        self._check(self.L.mp3mi_batch_host_wait(self.h, calls_back), "mp3mi_batch_host_wait")

    def slot_frames(self):
        """numpy int64 [n_streams]: frames encoded so far by the stream open in each slot, -1 where none is (no device wait)"""
        import numpy as np
        f = np.zeros(self.n_streams, np.int64)
        rc = self.L.mp3mi_batch_slot_frames(self.h, f.ctypes.data)
        if rc < 0:
            raise Mp3miError("mp3mi_batch_slot_frames failed with %d" % rc)
        return f

    def slot_kbps(self):
        """(numpy int32 [n_streams]: the bitrate of the stream open in each slot, the slot's create-time bitrate where none is;
        the batch's ceiling in kbps -- the largest bitrate a START may choose) (no device wait)"""
        import numpy as np
        k = np.zeros(self.n_streams, np.int32)
        rc = self.L.mp3mi_batch_slot_kbps(self.h, k.ctypes.data)
        if rc < 0:
            raise Mp3miError("mp3mi_batch_slot_kbps failed with %d" % rc)
        return k, rc

    def slot_state_bytes(self):
        """bytes of one parked stream's device record (a multiple of 16): the least row size of export_slots' state tensor"""
        return self.L.mp3mi_batch_slot_state_bytes(self.h)

    def export_slots(self, slots, state, close=True):
        """Parks the streams open in `slots` (distinct slot indices): row i of state -- a contiguous uint8 cuda tensor
        [len(slots), stride], stride >= slot_state_bytes() and a multiple of 16 -- receives the device record of slots[i]'s
        stream; returns the tickets, a ctypes array of SlotTicket, one per slot (host bookkeeping; no device wait).  close: the
        slots are closed afterwards without a flush -- the pending bytes travel in the record; False: the streams go on and the
        records are a snapshot.  sync() before the records are read by anything but this batch's own import_slots
        (mp3mi_batch_slots_export)."""
        import numpy as np
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        assert state.is_cuda and state.is_contiguous() and state.dtype.itemsize == 1 and state.dim() == 2 and state.shape[0] >= len(sl)
        tickets = (SlotTicket * max(len(sl), 1))()
        self._check(self.L.mp3mi_batch_slots_export(self.h, len(sl), sl.ctypes.data, 1 if close else 0, state.data_ptr(), state.shape[1],
                                                    ctypes.addressof(tickets)), "mp3mi_batch_slots_export")
        return tickets

    def import_slots(self, slots, state, tickets):
        """Resumes parked streams in the closed slots `slots`: row i of state (as export_slots wrote it, of this batch or of
        another batch of the same format) and tickets[i] go into slots[i], which is open afterwards at the ticket's frame count
        and bitrate; the next encode_slots continues it (start and end false).  No device wait (mp3mi_batch_slots_import)."""
        import numpy as np
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        assert state.is_cuda and state.is_contiguous() and state.dtype.itemsize == 1 and state.dim() == 2 and state.shape[0] >= len(sl)
        assert len(tickets) >= len(sl)
        arr = (SlotTicket * max(len(sl), 1))(*list(tickets)[:len(sl)])
        self._check(self.L.mp3mi_batch_slots_import(self.h, len(sl), sl.ctypes.data, state.data_ptr(), state.shape[1], ctypes.addressof(arr)),
                    "mp3mi_batch_slots_import")

    def feeder(self, tick_frames, max_push, lanes=None, max_rows=None, ring_samples=0):
        """A Feed in front of this batch (mp3mi_feed_create): streams bring any number of samples per tick, up to max_push, and a
        tick encodes tick_frames frames of every lane that has them.  No stream may be open, and while the Feed is attached the
        batch's encode, flush, reset, park and header calls are refused: the Feed makes them.
        lanes: that many lanes in front of the batch's slots, more than slots as a rule (mp3mi_feed_create_lanes): ticks go through
        Feed.tick_lanes then.  max_rows: the most lanes that push in one tick (None: lanes); ring_samples: a lane's FIFO (0: the
        least, tick_frames * 1152 + max_push)."""
        return Feed(self, tick_frames, max_push, lanes, max_rows, ring_samples)

    def set_mode(self, mode):
        """0 stereo, 2 dual channel, 3 mono (the reference's -m s|d|m); joint stereo is refused as in the reference"""
        self._check(self.L.mp3mi_batch_set_mode(self.h, mode), "mp3mi_batch_set_mode")

    def set_error_protection(self, on):
        """the reference's -e: protection bit cleared, zero CRC word after the header"""
        self._check(self.L.mp3mi_batch_set_error_protection(self.h, 1 if on else 0), "mp3mi_batch_set_error_protection")

    def set_header(self, copyright=0, original=0, emphasis=0):
        self._check(self.L.mp3mi_batch_set_header(self.h, copyright, original, emphasis), "mp3mi_batch_set_header")

    def sync(self):
        rc = self.L.mp3mi_batch_sync(self.h)
        if rc == ERR_REFERENCE_ABORT:
            raise ReferenceAborts("the reference would have died on at least one stream's input: out_len 0 there (stream_status())")
        if rc != 0:
            raise Mp3miError("mp3mi_batch_sync failed with %d" % rc)

    def stream_status(self):
        """per stream 0, or code | frame << 8 (include/mp3mi.h, MP3MI_STREAM_ABORT_*); waits for the work issued"""
        import numpy as np
        st = np.zeros(self.n_streams, np.int32)
        rc = self.L.mp3mi_batch_stream_status(self.h, st.ctypes.data)
        if rc < 0:
            raise Mp3miError("mp3mi_batch_stream_status failed with %d" % rc)
        return st

    def last_timing(self):
        a, b, n = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
        rc = self.L.mp3mi_batch_last_timing(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n))
        if rc != 0:
            raise Mp3miError("mp3mi_batch_last_timing failed with %d (no encode call yet?)" % rc)
        return a.value, b.value, n.value

    def total_timing(self):
        """(ms inside the loop kernel, ms inside all kernels, loop kernel launches, calls) summed over every encode
        call of this batch so far; waits for them"""
        a, b, n, k = ctypes.c_double(), ctypes.c_double(), ctypes.c_long(), ctypes.c_long()
        rc = self.L.mp3mi_batch_total_timing(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n), ctypes.byref(k))
        if rc != 0:
            raise Mp3miError("mp3mi_batch_total_timing failed with %d" % rc)
        return a.value, b.value, n.value, k.value

    def close(self):
        if self.h:
            if getattr(self, "_feed", None) is not None:
                self._feed.h = ctypes.c_void_p()  # (mp3mi_batch_destroy frees an attached feeder with the batch)
                self._feed = None
            self.L.mp3mi_batch_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Feed:
    """The feeder of a Batch (include/mp3mi.h, mp3mi_feed_*): a device FIFO per lane, so that every stream may bring any number
    of samples per call.  Lane s is slot s, unless the feeder was made with lanes=: then a slot is lent to a lane for the ticks in
    which it encodes (tick_lanes).  Made by Batch.feeder()."""

    def __init__(self, batch, tick_frames, max_push, lanes=None, max_rows=None, ring_samples=0):
        self.batch, self.L = batch, batch.L
        self.tick_frames, self.max_push = tick_frames, max_push
        self.h = ctypes.c_void_p()
        if lanes is None:
            rc = self.L.mp3mi_feed_create(ctypes.byref(self.h), batch.h, tick_frames, max_push)
        else:
            rc = self.L.mp3mi_feed_create_lanes(ctypes.byref(self.h), batch.h, lanes, lanes if max_rows is None else max_rows, tick_frames,
                                                max_push, ring_samples)
        if rc != 0:
            raise Mp3miError("mp3mi_feed_create%s failed with %d" % ("" if lanes is None else "_lanes", rc))
        batch._feed = self

    @property
    def n_lanes(self):
        """the feeder's lanes (mp3mi_feed_n_lanes): the batch's slots unless it was made with lanes="""
        return self.L.mp3mi_feed_n_lanes(self.h)

    def tick_lanes(self, pcm, out, out_len, rows, start=None, end=None, n_push=None, kbps=None):
        """One tick of a feeder made with lanes= (mp3mi_feed_tick_lanes).  rows: the lanes that push, strictly increasing; pcm: int16
        cuda tensor [len(rows), pitch * C] or [len(rows), pitch, C], pitch >= max_push (None without rows); start, end, n_push, kbps:
        per ROW, as in tick().  out [S, stride] and out_len [S] are by SLOT.  Returns the int32 array [S] of the lane that encodes
        in each slot in this tick, -1 where none does (host bookkeeping).  Nothing is waited for."""
        import numpy as np
        S, C = self.batch.n_streams, self.batch.channels
        rl = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        R = len(rl)
        assert out.is_cuda and out_len.is_cuda and out.is_contiguous() and out.shape[0] == S
        ctl = np.zeros(R, np.uint8)
        if start is not None:
            ctl |= np.asarray(start, dtype=bool).reshape(R).astype(np.uint8) * 1  # MP3MI_SLOT_START
        if end is not None:
            ctl |= np.asarray(end, dtype=bool).reshape(R).astype(np.uint8) * 2  # MP3MI_SLOT_END
        ns = np.zeros(R, np.int32) if n_push is None else np.ascontiguousarray(n_push, dtype=np.int32).reshape(R)
        kb = np.zeros(R, np.int32) if kbps is None else np.ascontiguousarray(kbps, dtype=np.int32).reshape(R)
        pitch = 0
        if R:
            assert pcm.is_cuda and pcm.is_contiguous() and pcm.shape[0] == R
            pitch = pcm.numel() // (R * C)
        slot_lane = np.full(S, -1, np.int32)
        rc = self.L.mp3mi_feed_tick_lanes(self.h, R, rl.ctypes.data if R else None, pcm.data_ptr() if R else None, pitch,
                                          ctl.ctypes.data if R else None, ns.ctypes.data if R else None, kb.ctypes.data if R else None,
                                          out.data_ptr(), out.shape[1], out_len.data_ptr(), slot_lane.ctypes.data)
        if rc != 0:
            raise Mp3miError("mp3mi_feed_tick_lanes failed with %d" % rc)
        return slot_lane

    def tick_lanes_host(self, pcm, out, out_len, rows, start=None, end=None, n_push=None, kbps=None):
        """tick_lanes on host buffers (mp3mi_feed_tick_lanes_host_async).  pcm: a 1-D or 2-D int16 CPU tensor or numpy array that holds
        the rows' samples PACKED, row r's n_push[r] samples per channel behind row r - 1's (None when nothing is pushed); out uint8
        [S, stride] and out_len int32 or uint32 [S]: CPU tensors (page-locked ones overlap with the kernels) or numpy arrays, which
        must stay alive and untouched until host_wait for this tick, or the batch's sync, has returned.  Returns (lanes, slots): int32
        arrays of the lanes that encode in this tick, ascending, and the slot of each; row i of out and out_len[i] are lane
        lanes[i]'s, and rows from len(lanes) on are not written.  Nothing is waited for."""
        import numpy as np

        def ptr(a):
            if a is None:
                return None
            if isinstance(a, np.ndarray):
                assert a.flags.c_contiguous
                return a.ctypes.data
            assert not a.is_cuda and a.is_contiguous()
            return a.data_ptr()
        S, C = self.batch.n_streams, self.batch.channels
        rl = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        R = len(rl)
        assert out.shape[0] == S and out_len.shape[0] == S and out.dtype.itemsize == 1 and out_len.dtype.itemsize == 4
        ctl = np.zeros(R, np.uint8)
        if start is not None:
            ctl |= np.asarray(start, dtype=bool).reshape(R).astype(np.uint8) * 1  # MP3MI_SLOT_START
        if end is not None:
            ctl |= np.asarray(end, dtype=bool).reshape(R).astype(np.uint8) * 2  # MP3MI_SLOT_END
        ns = np.zeros(R, np.int32) if n_push is None else np.ascontiguousarray(n_push, dtype=np.int32).reshape(R)
        kb = np.zeros(R, np.int32) if kbps is None else np.ascontiguousarray(kbps, dtype=np.int32).reshape(R)
        if pcm is not None:
            assert pcm.dtype.itemsize == 2 and len(pcm.shape) in (1, 2)
            n_have = 1
            for d in pcm.shape:
                n_have *= int(d)
            assert n_have >= int(ns.sum()) * C, "pcm holds fewer samples than the rows push"
        lanes, slots, n_out = np.full(S, -1, np.int32), np.full(S, -1, np.int32), ctypes.c_int32(0)
        rc = self.L.mp3mi_feed_tick_lanes_host_async(self.h, R, rl.ctypes.data if R else None, ptr(pcm), ctl.ctypes.data if R else None,
                                                     ns.ctypes.data if R else None, kb.ctypes.data if R else None, ptr(out), out.shape[1],
                                                     ptr(out_len), lanes.ctypes.data, slots.ctypes.data, ctypes.addressof(n_out))
        if rc != 0:
            raise Mp3miError("mp3mi_feed_tick_lanes_host_async failed with %d" % rc)
        return lanes[:n_out.value].copy(), slots[:n_out.value].copy()

    def host_wait(self, ticks_back=0):
        """waits until the host tick issued ticks_back host ticks ago (0: the latest, 1: the one before) has taken its samples and
        delivered its rows, and for nothing later (mp3mi_feed_host_wait)"""
        rc = self.L.mp3mi_feed_host_wait(self.h, ticks_back)
        if rc != 0:
            raise Mp3miError("mp3mi_feed_host_wait failed with %d" % rc)

    def host_io_stats(self):
        """{h2d_bytes, d2h_bytes, h2d_ms, d2h_ms, calls} over the host ticks so far (waits for them; mp3mi_feed_host_io_stats)"""
        class S(ctypes.Structure):
            _fields_ = [("h2d_bytes", ctypes.c_double), ("d2h_bytes", ctypes.c_double), ("h2d_ms", ctypes.c_double), ("d2h_ms", ctypes.c_double), ("calls", ctypes.c_long)]
        st = S()
        rc = self.L.mp3mi_feed_host_io_stats(self.h, ctypes.byref(st))
        if rc != 0:
            raise Mp3miError("mp3mi_feed_host_io_stats failed with %d" % rc)
        return {k: getattr(st, k) for k, _ in S._fields_}

    @property
    def capacity(self):
        """samples per channel a lane holds: tick_frames * 1152 + max_push"""
        return self.L.mp3mi_feed_capacity(self.h)

    def tick(self, pcm, out, out_len, start=None, end=None, n_push=None, kbps=None):
        """One tick (mp3mi_feed_tick).  pcm: int16 cuda tensor [S, pitch * C] or [S, pitch, C], pitch >= max_push: lane s brings
        its first n_push[s] samples per channel (None: none).  start[s]: a new stream begins in lane s with them, at kbps[s] (0 /
        None: the slot's create-time bitrate); end[s]: they are the stream's last.  Every lane that has tick_frames * 1152 samples,
        or is ending, encodes; out uint8 cuda [S, stride >= batch.out_stride(tick_frames)] and out_len int32 cuda [S] receive per
        lane the bytes of its file that became final (0 for a lane that sits out).  Nothing is waited for."""
        import numpy as np
        S, C = self.batch.n_streams, self.batch.channels
        assert pcm.is_cuda and out.is_cuda and out_len.is_cuda and pcm.is_contiguous() and out.is_contiguous() and pcm.shape[0] == S
        pitch = pcm.numel() // (S * C)
        ctl = np.zeros(S, np.uint8)
        if start is not None:
            ctl |= np.asarray(start, dtype=bool).reshape(S).astype(np.uint8) * 1  # MP3MI_SLOT_START
        if end is not None:
            ctl |= np.asarray(end, dtype=bool).reshape(S).astype(np.uint8) * 2  # MP3MI_SLOT_END
        ns = None if n_push is None else np.ascontiguousarray(n_push, dtype=np.int32).reshape(S)
        kb = None if kbps is None else np.ascontiguousarray(kbps, dtype=np.int32).reshape(S)
        rc = self.L.mp3mi_feed_tick(self.h, pcm.data_ptr(), pitch, ctl.ctypes.data, None if ns is None else ns.ctypes.data,
                                    None if kb is None else kb.ctypes.data, out.data_ptr(), out.shape[1], out_len.data_ptr())
        if rc != 0:
            raise Mp3miError("mp3mi_feed_tick failed with %d" % rc)

    def lanes(self):
        """(pending int32 [n_lanes], frames int64 [n_lanes] (-1: closed), flags uint8 [n_lanes]: 1 parked, 2 draining, 4 started but not
        yet in the batch, 8 ready and waiting for a slot; lanes that are not closed) -- host bookkeeping, no device wait"""
        import numpy as np
        S = self.n_lanes
        p, f, g = np.zeros(S, np.int32), np.zeros(S, np.int64), np.zeros(S, np.uint8)
        rc = self.L.mp3mi_feed_lanes(self.h, p.ctypes.data, f.ctypes.data, g.ctypes.data)
        if rc < 0:
            raise Mp3miError("mp3mi_feed_lanes failed with %d" % rc)
        return p, f, g, rc

    def close(self):
        """resets the batch and detaches (mp3mi_feed_destroy)"""
        if self.h:
            self.L.mp3mi_feed_destroy(self.h)
            self.h = ctypes.c_void_p()
            self.batch._feed = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


L12_KERNELS = ("k_fft12", "k12_psy", "k_filter", "k12_alloc")
L12_FRAME_SAMPLES = {1: 384, 2: 1152}


def frame_bytes_l12(layer, rate_hz, kbps):
    """slots per frame times the slot size, never padded (reference: src/musicin.c:562-581)"""
    if layer == 1:
        return 4 * int((384.0 / (rate_hz / 1000.0)) * (kbps / 32.0))
    return int((1152.0 / (rate_hz / 1000.0)) * (kbps / 8.0))


class BatchL12:
    """Layer I / II batched encoder (include/mp3mi_l12.h) over device memory handed in as torch tensors."""

    def __init__(self, layer, n_streams, rate_hz, channels, kbps, max_frames, mode=None, error_protection=False, scratch_mb=0):
        import numpy as np
        self.L = lib()
        self.layer, self.n_streams, self.rate_hz, self.channels, self.max_frames = layer, n_streams, rate_hz, channels, max_frames
        self.h = ctypes.c_void_p()
        arr = None if isinstance(kbps, int) else np.ascontiguousarray(kbps, dtype=np.int32)
        karg, kall = (None, kbps) if arr is None else (arr.ctypes.data, 0)
        rc = self.L.mp3mi_l12_batch_create(ctypes.byref(self.h), layer, n_streams, rate_hz, channels, karg, kall, max_frames, scratch_mb)
        if rc != 0:
            raise Mp3miError("mp3mi_l12_batch_create failed with %d" % rc)
        if mode is not None:
            self._check(self.L.mp3mi_l12_batch_set_mode(self.h, mode), "mp3mi_l12_batch_set_mode")
        if error_protection:
            self._check(self.L.mp3mi_l12_batch_set_error_protection(self.h, 1), "mp3mi_l12_batch_set_error_protection")

    def _check(self, rc, what):
        if rc != 0:
            raise Mp3miError("%s failed with %d" % (what, rc))

    def out_stride(self, n_frames):
        return self.L.mp3mi_l12_batch_out_stride(self.h, n_frames)

    def encode(self, pcm, n_frames, out, out_len, n_samples=None):
        assert pcm.is_cuda and out.is_cuda and out_len.is_cuda and pcm.is_contiguous() and out.is_contiguous()
        self._check(self.L.mp3mi_l12_batch_encode(self.h, pcm.data_ptr(), n_samples.data_ptr() if n_samples is not None else None,
                                                  n_frames, out.data_ptr(), out.stride(0), out_len.data_ptr()), "mp3mi_l12_batch_encode")

    def encode_next(self, pcm, n_frames, out, out_len):
        """Streaming: the NEXT n_frames frames of every stream (pcm holds only these); out / out_len receive their bytes.
        Concatenate them call after call, then flush()."""
        assert pcm.is_cuda and out.is_cuda and out_len.is_cuda and pcm.is_contiguous() and out.is_contiguous()
        self._check(self.L.mp3mi_l12_batch_encode_next(self.h, pcm.data_ptr(), n_frames, out.data_ptr(), out.stride(0), out_len.data_ptr()),
                    "mp3mi_l12_batch_encode_next")

    def flush(self, out, out_len):
        """close_bit_stream_w: the file's one byte past the last frame of every open stream; ends the streams."""
        self._check(self.L.mp3mi_l12_batch_flush(self.h, out.data_ptr(), out.stride(0), out_len.data_ptr()), "mp3mi_l12_batch_flush")

    def reset(self):
        self._check(self.L.mp3mi_l12_batch_reset(self.h), "mp3mi_l12_batch_reset")

    def encode_slots(self, pcm, n_frames, out, out_len, start=None, end=None, n_samples=None, kbps=None):
        """Continuous batching (mp3mi_l12_batch_encode_slots): every stream index is a slot in which one stream after another
        begins (start[s] true: with this call's first sample, from silence) and ends (end[s] true: this call holds its last
        n_samples[s] samples per channel).  start / end: boolean sequences of n_streams (None: all false); n_samples: an int
        sequence (None: a full call for every open or starting slot, 0 for the others).  Tensors as for encode_next; out /
        out_len receive per slot the bytes of its file this call produced (0 for a closed slot).  kbps: an int sequence, per slot
        the bitrate of the stream that STARTs there (0: the slot's create-time bitrate; a bitrate of the layer, at most the largest
        the batch was created with) and 0 or the open stream's own bitrate elsewhere (mp3mi_l12_batch_encode_slots_kbps); None: the
        call without it."""
        import numpy as np
        assert pcm.is_cuda and out.is_cuda and out_len.is_cuda and pcm.is_contiguous() and out.is_contiguous()
        S = self.n_streams
        ctl = np.zeros(S, np.uint8)
        if start is not None:
            ctl |= np.asarray(start, dtype=bool).reshape(S).astype(np.uint8) * 1  # MP3MI_SLOT_START
        if end is not None:
            ctl |= np.asarray(end, dtype=bool).reshape(S).astype(np.uint8) * 2  # MP3MI_SLOT_END
        ns = None if n_samples is None else np.ascontiguousarray(n_samples, dtype=np.int32).reshape(S)
        if kbps is not None:
            kb = np.ascontiguousarray(kbps, dtype=np.int32).reshape(S)
            self._check(self.L.mp3mi_l12_batch_encode_slots_kbps(self.h, pcm.data_ptr(), n_frames, ctl.ctypes.data, None if ns is None else ns.ctypes.data,
                                                                 kb.ctypes.data, out.data_ptr(), out.stride(0), out_len.data_ptr()),
                        "mp3mi_l12_batch_encode_slots_kbps")
            return
        self._check(self.L.mp3mi_l12_batch_encode_slots(self.h, pcm.data_ptr(), n_frames, ctl.ctypes.data, None if ns is None else ns.ctypes.data,
                                                        out.data_ptr(), out.stride(0), out_len.data_ptr()), "mp3mi_l12_batch_encode_slots")

    def slot_frames(self):
        """numpy int64 [n_streams]: frames encoded so far by the stream open in each slot, -1 where none is (no device wait)"""
        import numpy as np
        f = np.zeros(self.n_streams, np.int64)
        rc = self.L.mp3mi_l12_batch_slot_frames(self.h, f.ctypes.data)
        if rc < 0:
            raise Mp3miError("mp3mi_l12_batch_slot_frames failed with %d" % rc)
        return f

    def slot_kbps(self):
        """(numpy int32 [n_streams]: the bitrate of the stream open in each slot, the slot's create-time bitrate where none is;
        the batch's ceiling in kbps -- the largest bitrate a START may choose) (no device wait)"""
        import numpy as np
        k = np.zeros(self.n_streams, np.int32)
        rc = self.L.mp3mi_l12_batch_slot_kbps(self.h, k.ctypes.data)
        if rc < 0:
            raise Mp3miError("mp3mi_l12_batch_slot_kbps failed with %d" % rc)
        return k, rc

    def slot_state_bytes(self):
        """bytes of one parked stream's device record (a multiple of 16): the least row size of export_slots' state tensor"""
        return self.L.mp3mi_l12_batch_slot_state_bytes(self.h)

    def export_slots(self, slots, state, close=True):
        """Parks the streams open in `slots` (distinct slot indices): row i of state -- a uint8 cuda tensor [len(slots), stride] with
        contiguous rows, stride >= slot_state_bytes() and a multiple of 16 -- receives the device record of slots[i]'s stream, its PCM
        history; returns the tickets, a ctypes array of SlotTicketL12, one per slot (host bookkeeping; no device wait).  close: the
        slots are closed afterwards without a flush -- nothing is delivered; False: the streams go on and the records are a
        snapshot.  sync() before the records are read by anything but this batch's own import_slots
        (mp3mi_l12_batch_slots_export)."""
        import numpy as np
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        assert state.is_cuda and state.is_contiguous() and state.dtype.itemsize == 1 and state.dim() == 2 and state.shape[0] >= len(sl)
        tickets = (SlotTicketL12 * max(len(sl), 1))()
        self._check(self.L.mp3mi_l12_batch_slots_export(self.h, len(sl), sl.ctypes.data, 1 if close else 0, state.data_ptr(), state.stride(0),
                                                        ctypes.addressof(tickets)), "mp3mi_l12_batch_slots_export")
        return tickets

    def import_slots(self, slots, state, tickets):
        """Resumes parked streams in the closed slots `slots`: row i of state (as export_slots wrote it, of this batch or of
        another batch of the same format) and tickets[i] go into slots[i], which is open afterwards at the ticket's frame count
        and bitrate; the next encode_slots continues it (start and end false).  No device wait (mp3mi_l12_batch_slots_import)."""
        import numpy as np
        sl = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        assert state.is_cuda and state.is_contiguous() and state.dtype.itemsize == 1 and state.dim() == 2 and state.shape[0] >= len(sl)
        assert len(tickets) >= len(sl)
        arr = (SlotTicketL12 * max(len(sl), 1))(*list(tickets)[:len(sl)])
        self._check(self.L.mp3mi_l12_batch_slots_import(self.h, len(sl), sl.ctypes.data, state.data_ptr(), state.stride(0), ctypes.addressof(arr)),
                    "mp3mi_l12_batch_slots_import")

    def feeder(self, tick_frames, max_push, lanes=None, max_rows=None, ring_samples=0):
        """A feeder in front of this batch (mp3mi_l12_feed_create): lanes that take any number of samples per call (up to max_push)
        and encode tick_frames frames per tick in the slots the feeder lends them.  lanes None: one lane per slot; max_rows: the most
        lanes that push in one tick (None: all); ring_samples: the pending samples a lane's FIFO holds (0: tick_frames * frame +
        max_push).  While it is attached the batch's streams are the feeder's.  Returns the FeedL12."""
        return FeedL12(self, tick_frames, max_push, lanes, max_rows, ring_samples)

    def sync(self):
        self._check(self.L.mp3mi_l12_batch_sync(self.h), "mp3mi_l12_batch_sync")

    def total_timing(self):
        """(ms inside all kernels, calls) since create; waits for the work issued so far"""
        a, k = ctypes.c_double(), ctypes.c_long()
        self._check(self.L.mp3mi_l12_batch_total_timing(self.h, ctypes.byref(a), ctypes.byref(k)), "mp3mi_l12_batch_total_timing")
        return a.value, k.value

    def kernel_timing(self):
        """{kernel: (ms, launches)} since create (HIP events around every launch)"""
        ms, n = (ctypes.c_double * 4)(), (ctypes.c_long * 4)()
        self._check(self.L.mp3mi_l12_batch_kernel_timing(self.h, ms, n), "mp3mi_l12_batch_kernel_timing")
        return {L12_KERNELS[i]: (ms[i], n[i]) for i in range(4)}

    def close(self):
        if self.h:
            feed = getattr(self, "_feed", None)
            if feed is not None:
                feed.close()
            self.L.mp3mi_l12_batch_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FeedL12:
    """The feeder of a BatchL12 (include/mp3mi_l12.h, mp3mi_l12_feed_*): a device FIFO per lane, so that every stream may bring any
    number of samples per call; a slot is lent to a lane for the ticks in which it encodes.  Made by BatchL12.feeder()."""

    def __init__(self, batch, tick_frames, max_push, lanes=None, max_rows=None, ring_samples=0):
        self.batch, self.L = batch, batch.L
        self.tick_frames, self.max_push = tick_frames, max_push
        self.h = ctypes.c_void_p()
        lanes = batch.n_streams if lanes is None else lanes
        rc = self.L.mp3mi_l12_feed_create(ctypes.byref(self.h), batch.h, lanes, lanes if max_rows is None else max_rows, tick_frames,
                                          max_push, ring_samples)
        if rc != 0:
            raise Mp3miError("mp3mi_l12_feed_create failed with %d" % rc)
        batch._feed = self

    @property
    def n_lanes(self):
        return self.L.mp3mi_l12_feed_n_lanes(self.h)

    @property
    def capacity(self):
        """pending samples per channel a lane's FIFO holds (the 1792 samples of history in the ring come on top)"""
        return self.L.mp3mi_l12_feed_capacity(self.h)

    def tick(self, pcm, out, out_len, rows, start=None, end=None, n_push=None, kbps=None):
        """One tick (mp3mi_l12_feed_tick).  rows: the lanes that push, strictly increasing; pcm: int16 cuda tensor [len(rows), pitch * C]
        or [len(rows), pitch, C], pitch >= max_push (None without rows); start, end, n_push, kbps: per ROW -- start[r]: a new stream
        begins in the lane with the row's samples, at kbps[r] (0 / None: the create-time bitrate of the slot it first encodes in);
        end[r]: they are the stream's last.  out uint8 cuda [S, stride >= batch.out_stride(tick_frames)] and out_len int32 cuda [S] are
        by SLOT.  Returns the int32 array [S] of the lane that encodes in each slot in this tick, -1 where none does (host
        bookkeeping).  Nothing is waited for."""
        import numpy as np
        S, C = self.batch.n_streams, self.batch.channels
        rl = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        R = len(rl)
        assert out.is_cuda and out_len.is_cuda and out.is_contiguous() and out.shape[0] == S
        ctl = np.zeros(R, np.uint8)
        if start is not None:
            ctl |= np.asarray(start, dtype=bool).reshape(R).astype(np.uint8) * 1  # MP3MI_SLOT_START
        if end is not None:
            ctl |= np.asarray(end, dtype=bool).reshape(R).astype(np.uint8) * 2  # MP3MI_SLOT_END
        ns = np.zeros(R, np.int32) if n_push is None else np.ascontiguousarray(n_push, dtype=np.int32).reshape(R)
        kb = np.zeros(R, np.int32) if kbps is None else np.ascontiguousarray(kbps, dtype=np.int32).reshape(R)
        pitch = 0
        if R:
            assert pcm.is_cuda and pcm.is_contiguous() and pcm.shape[0] == R
            pitch = pcm.numel() // (R * C)
        slot_lane = np.full(S, -1, np.int32)
        rc = self.L.mp3mi_l12_feed_tick(self.h, R, rl.ctypes.data if R else None, pcm.data_ptr() if R else None, pitch,
                                        ctl.ctypes.data if R else None, ns.ctypes.data if R else None, kb.ctypes.data if R else None,
                                        out.data_ptr(), out.shape[1], out_len.data_ptr(), slot_lane.ctypes.data)
        if rc != 0:
            raise Mp3miError("mp3mi_l12_feed_tick failed with %d" % rc)
        return slot_lane

    def lanes(self):
        """(pending int32 [n_lanes], frames int64 [n_lanes] (-1: closed), flags uint8 [n_lanes]: 1 parked, 2 draining, 4 started but not
        yet in the batch, 8 ready and waiting for a slot; lanes that are not closed) -- host bookkeeping, no device wait"""
        import numpy as np
        n = self.n_lanes
        p, f, g = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.uint8)
        rc = self.L.mp3mi_l12_feed_lanes(self.h, p.ctypes.data, f.ctypes.data, g.ctypes.data)
        if rc < 0:
            raise Mp3miError("mp3mi_l12_feed_lanes failed with %d" % rc)
        return p, f, g, rc

    def close(self):
        """resets the batch and detaches (mp3mi_l12_feed_destroy)"""
        if self.h:
            self.L.mp3mi_l12_feed_destroy(self.h)
            self.h = ctypes.c_void_p()
            self.batch._feed = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
