/* libmp3mi -- MI355X-native MPEG-1 Layer III encoding hot path, C ABI.
 *
 * Two surfaces:
 *
 * 1. The batched API (mp3mi_batch_*): thousands of independent streams per call, device
 *    pointers in, device pointers out.  This is where the throughput is.
 *
 * 2. The reference's own per-frame call surface (section "drop-in symbols" below): the seven
 *    external-linkage functions that the reference's driver calls for Layer III
 *    (/root/reference/src/musicin.c:751-786, 803), with identical names, argument meaning and
 *    in-place side effects, backed by one hidden default stream that runs the same kernels with
 *    n_streams = 1.  A maintainer links musicin.o + common.o against libmp3mi.so instead of
 *    l3psy.o encode.o(filterbank part) mdct.o loop.o l3bitstream.o -- see INTEGRATION.md.
 *
 * Every function fails loudly (non-zero return / abort with a message for the void drop-in
 * symbols, like the reference's exit()/abort()) when no gfx950 device is usable: there is no
 * CPU fallback in this library.
 *
 * Threads ("one thread or process per device"):
 *   - A batch object (mp3mi_batch, mp3mi_l12_batch) belongs to ONE thread at a time: calls on the same object must not
 *     overlap; the caller serialises them (any thread may make the next call once the previous one has returned --
 *     every entry point selects the batch's own device for its duration and restores the caller's).
 *   - DIFFERENT batch objects are independent: they may be created, used and destroyed concurrently from different
 *     threads, on the same device or on different ones.  A batch owns its HIP streams, events and device buffers;
 *     the only library-wide state is the construction of the constant tables, which the library serialises itself
 *     (csrc/tables_host.cpp).  Two batches on one device share its compute units: correct, each at a part of
 *     the rate (tests/test_threads.py: two threads, two batches, one device, interleaved calls, both bit-exact).
 *   - mp3mi_encode_host / mp3mi_encode_host_ex / mp3mi_encode_host_async create a batch of their own per call: reentrant.
 *   - The drop-in symbols (section 2 above) keep the reference's contract: ONE stream per process, one caller at a
 *     time -- the reference's own functions hold their state in function statics (src/l3psy.c:130-160, src/loop.c:240).
 *   - The mp3mi_debug_* accessors of diagnostic builds read device-global counters: single-threaded use only.
 */
#ifndef MP3MI_H
#define MP3MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ batched API */

typedef struct mp3mi_batch mp3mi_batch;

enum {
    MP3MI_OK = 0,
    MP3MI_ERR_ARG = -1,       /* unsupported rate / bitrate / channel count (what the reference refuses) */
    MP3MI_ERR_NO_DEVICE = -2, /* no usable GPU */
    MP3MI_ERR_HIP = -3,       /* a HIP call failed; message on stderr */
    MP3MI_ERR_NOMEM = -4,
    MP3MI_ERR_TABLES = -5,    /* the init tables do not hash to their pinned values (csrc/tables_pins.h): a damaged build;
                                 the bitstream would not be bit-exact, so nothing is encoded */
    MP3MI_ERR_REFERENCE_ABORT = -6 /* mp3mi_batch_sync / mp3mi_encode_host: the work completed, but for at least one stream the
                                 REFERENCE would have died on the input (an assertion of its code fails); that stream's
                                 out_len is 0, every other stream's output is valid -- see mp3mi_batch_stream_status */
};

/* Scratch, scheduling and drop-in options of a batch.  The defaults are right for production use.  Fill the struct with
 * mp3mi_batch_options_default (or mp3mi_batch_options_from_env), then change fields: it sets struct_size and abi, and a
 * struct without them -- a zero-initialised one among them -- is refused. */
typedef struct mp3mi_batch_options {
    uint32_t struct_size;     /* sizeof(mp3mi_batch_options) of the caller's build */
    uint32_t scratch_mb;      /* budget of the per-chunk scratch buffers in MiB (~78 KB per frame and stream); 0 = 32768 */
    int32_t chunk_frames;     /* upper limit of a chunk's length in frames; 0 = whatever the budget allows */
    uint32_t test_flags;      /* MP3MI_TEST_*: force the exact tier of the two-tier decisions (as mp3mi_batch_set_test_flags) */
    int32_t dropin_lookahead; /* the drop-in symbols' look-ahead (mp3mi_dropin.h): -1 default = 2 the filterbank's (and mdct_sub behind it: memory of the current frame only), 0 none, 1 all (buffer lifetime requirement: mp3mi_dropin.h),
                                 3 L3psycho_anal's only, 4 all but iteration_loop's / III_format_bitstream's.  Not a property of a batch: the hidden default stream of the drop-in symbols
                                 reads it through mp3mi_batch_options_from_env (MP3MI_DROPIN_LOOKAHEAD) */
    int32_t call_hold;        /* the LAST loop kernel of a call waits (on the device, at most 20 ms -- 0.4 ms per frame of a chunk where that is more, at most 200 ms --) until the call after it has run its first
                                 transforms, or until a call that waits for results lets it go (sync, stream_status, timing, flush, reset,
                                 destroy): calls issued back to back then lose no pipeline fill: -1 default (on), 0, 1 */
    int32_t dropin_stats;     /* the drop-in symbols print, at III_FlushBitstream, the frames they served, the time from the first frame's
                                 first call to the flush and the waits for the device: 0 default, 1 (MP3MI_DROPIN_STATS) */
    uint32_t abi;             /* MP3MI_OPTIONS_ABI of the header the caller was built against.  The struct's size alone does not tell two
                                 layouts apart (round 5 replaced a field in the middle and kept the size): a caller built against another layout is
                                 refused (MP3MI_ERR_ARG) instead of having its fields read as their neighbours */
} mp3mi_batch_options;
#define MP3MI_OPTIONS_ABI 7u  /* raised whenever the struct's layout or a field's meaning changes; new fields go at the END */
/* mp3mi_batch_create_ex returns MP3MI_ERR_ARG for a value outside the ranges named above (chunk_frames >= 0; call_hold
 * -1, 0, 1; dropin_lookahead -1 .. 4; dropin_stats 0, 1; unknown test flags). */
void mp3mi_batch_options_default(mp3mi_batch_options *opt);
/* The same, then overridden by the MP3MI_* environment variables that tools/ and tests/ use (MP3MI_SCRATCH_MB,
 * MP3MI_CHUNK_FRAMES, MP3MI_{NOISE,PHASE,PSY,QUANT,PREP,CW}_EXACT, MP3MI_CALL_HOLD, MP3MI_DROPIN_LOOKAHEAD, MP3MI_DROPIN_STATS).
 * This is the ONLY place the library reads its environment: mp3mi_batch_create calls it once; mp3mi_batch_create_ex never does. */
void mp3mi_batch_options_from_env(mp3mi_batch_options *opt);

/* Creates an encoder for n_streams independent streams that share sample rate and channel
 * count.  rate_hz in {44100, 48000, 32000}; channels 1 or 2; kbps points to n_streams MPEG-1
 * Layer III bitrates (32..320) or is NULL, in which case every stream uses kbps_all.
 * max_frames bounds n_frames of later encode calls.  Replaces the set-up part of
 * /root/reference/src/musicin.c:456-581 (parse_args defaults, hdr_to_frps, slots per frame). */
int mp3mi_batch_create(mp3mi_batch **out, int n_streams, int rate_hz, int channels,
                       const int *kbps, int kbps_all, int max_frames);
/* The same with explicit options (NULL = the defaults); reads no environment variable. */
int mp3mi_batch_create_ex(mp3mi_batch **out, int n_streams, int rate_hz, int channels,
                          const int *kbps, int kbps_all, int max_frames, const mp3mi_batch_options *opt);
void mp3mi_batch_destroy(mp3mi_batch *b);

/* Bytes to reserve per stream in the output buffer for n_frames frames. */
size_t mp3mi_batch_out_stride(const mp3mi_batch *b, int n_frames);

/* Encodes n_frames whole frames of every stream, from a fresh encoder state, including the
 * final flush (III_FlushBitstream + close_bit_stream_w, musicin.c:802-805).
 *   pcm_dev     device pointer, int16, [n_streams][n_frames*1152][channels] (WAV sample order)
 *   out_dev     device pointer, [n_streams][out_stride] bytes
 *   out_len_dev device pointer, [n_streams] uint32: bytes produced per stream
 * Work is enqueued on the batch's stream; call mp3mi_batch_sync before reading results. */
int mp3mi_batch_encode(mp3mi_batch *b, const int16_t *pcm_dev, int n_frames, uint8_t *out_dev,
                       size_t out_stride, uint32_t *out_len_dev);
int mp3mi_batch_sync(mp3mi_batch *b);

/* Inputs the reference DIES on.  A few assertions of the reference's Layer III code fail on real inputs
 * (tests/golden/coverage_notes.json, "reference_aborts", with the fixtures that reach them):
 *   MP3MI_STREAM_ABORT_GLOBAL_GAIN  assert( cod_info->global_gain < 256 ), /root/reference/src/loop.c:358 -- a granule with
 *                                   exact-zero lines beside a few tiny ones (a click behind digital silence)
 *   MP3MI_STREAM_ABORT_HUFF_BITS    assert( max_bits >= 0 ) in inner_loop, src/loop.c:579 -- scalefactor bits above the
 *                                   granule's budget (48 kHz, 32 kbps, stereo, short blocks)
 *   MP3MI_STREAM_ABORT_FLUSH_SLOT   assert( l ) in get_side_info, src/formatBitstream.c:390, reached from BF_FlushBitstream
 *                                   when the last main data ends exactly on a slot boundary with headers still queued
 * The reference's process ends there and leaves no usable file.  A batch cannot end for one stream: the stream's status
 * records the first such event, its out_len becomes 0 for that call and every later one, the other streams are not
 * affected, and mp3mi_batch_sync returns MP3MI_ERR_REFERENCE_ABORT once -- the first sync after the call in which the
 * event happened (whole-file and streaming calls alike; the final flush reports what it finds itself), while the
 * status is there to be read.  (The drop-in symbols abort() with the reference's message, as the reference does.)
 * mp3mi_batch_stream_status waits for the work issued so far and copies the status of every stream of the most recent
 * streams (since the last reset / whole-file call; after mp3mi_batch_flush: of the streams it ended, until the next
 * encode starts new ones) to status_host[n_streams]: 0, or code | frame << 8 where frame is the
 * index of the frame it happened in (the number of frames for the final flush; the field is 22 bits wide and saturates
 * at 4194303, ~30 h of audio fed call by call).  Returns the number of streams with a
 * non-zero status, or a negative MP3MI_ERR_*. */
enum { MP3MI_STREAM_OK = 0, MP3MI_STREAM_ABORT_GLOBAL_GAIN = 1, MP3MI_STREAM_ABORT_HUFF_BITS = 2, MP3MI_STREAM_ABORT_FLUSH_SLOT = 3 };
int mp3mi_batch_stream_status(mp3mi_batch *b, int32_t *status_host);

/* Streaming: the reference is a frame-streaming encoder (/root/reference/src/musicin.c:585-805); these calls encode
 * a stream piece by piece with everything it carries from frame to frame kept in the batch (psychoacoustic
 * history and thresholds, the filterbank's and the FFT window's past samples, the bit reservoir, the main data
 * that is formatted but whose slot is still open).
 *   mp3mi_batch_encode_next  encodes the NEXT n_frames frames of every stream: pcm_dev holds only these frames,
 *                            [n_streams][n_frames*1152][channels].  out_dev / out_len_dev receive, per stream, the
 *                            file bytes that became final with this call -- in file order, so concatenating the
 *                            outputs of successive calls and of the final flush gives the stream's file.  (Up to
 *                            511 bytes of main data, plus the headers in between, stay behind in the reservoir's
 *                            open slots until later frames fill them: src/formatBitstream.c:52-120.)  The first call
 *                            after create, reset, flush or a whole-file encode starts new streams.
 *   mp3mi_batch_flush        III_FlushBitstream + close_bit_stream_w (musicin.c:802-805): delivers what is left and
 *                            ends the streams.  out_stride >= 2049 here.
 *   mp3mi_batch_reset        abandons the current streams: fresh encoder state.
 * mp3mi_batch_encode (above) is the same encoder run over a whole stream in one call.  With these three calls all
 * streams of the batch begin and end together; mp3mi_batch_encode_slots (below) lets them begin and end in different
 * calls, and end on a partial frame.  out_stride >= mp3mi_batch_out_stride(b, n_frames). */
int mp3mi_batch_encode_next(mp3mi_batch *b, const int16_t *pcm_dev, int n_frames, uint8_t *out_dev,
                            size_t out_stride, uint32_t *out_len_dev);
int mp3mi_batch_flush(mp3mi_batch *b, uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev);
int mp3mi_batch_reset(mp3mi_batch *b);

/* Continuous batching: every stream index of a batch is a SLOT through which one stream after another passes, each
 * beginning and ending in a call of its own while the other slots go on encoding.
 *   mp3mi_batch_encode_slots  one streaming call (pcm_dev [n_streams][n_frames*1152][channels], as for encode_next) with
 *                             per-slot control in two HOST arrays, which the library copies before it returns:
 *     ctl_host[s]             MP3MI_SLOT_START: slot s begins a new stream with this call's first sample, from fresh state (a
 *                             stream still open there is abandoned, as by mp3mi_batch_reset: its pending bytes are not
 *                             delivered).  MP3MI_SLOT_END: this call holds the stream's last samples; the call also flushes
 *                             and closes it (src/formatBitstream.c:87-120, src/common.c:843-868) and the slot is closed
 *                             afterwards.  START | END: a one-call file.  0: an open stream goes on, a closed slot stays closed.
 *     n_samples_host[s]       valid samples per channel of slot s in the call: n_frames*1152 for an open or starting stream
 *                             that does not end, 0 .. n_frames*1152 for one that ends (the last partial frame is zero-filled,
 *                             src/encode.c:162-166), 0 for a closed slot.  NULL: n_frames*1152 for every open or starting
 *                             slot, 0 for the others.
 *                             out_len_dev[s] receives the bytes of slot s's file that became final with the call, in file
 *                             order (0 for a closed slot): the outputs of the START call through the END call, concatenated,
 *                             are the stream's file -- the bytes mp3mi_batch_encode_ragged gives for its samples.  Any broken
 *                             rule (unknown ctl bits, END on a closed slot, a wrong sample count, a NULL pointer other than
 *                             n_samples_host, n_frames outside 1..max_frames, out_stride < mp3mi_batch_out_stride(b, n_frames))
 *                             returns MP3MI_ERR_ARG before anything is enqueued, and the batch is unchanged.
 *                             mp3mi_batch_stream_status reports per slot the status of the open stream, or of the stream
 *                             that last ended there, until the slot's next START; an abort is reported by the next sync as for
 *                             encode_next, and the final flush's one (MP3MI_STREAM_ABORT_FLUSH_SLOT) is found at an END.
 *   mp3mi_batch_slot_frames   host-side only, no wait: frames_host[s] = frames encoded so far by the stream open in slot s,
 *                             -1 if none is.  Returns the number of open slots.
 * Alongside: encode_next starts every slot when none is open and otherwise continues the open ones (closed slots stay
 * closed, out_len 0); flush ends every open slot (out_len 0 for the closed ones); after reset and after a whole-file,
 * ragged or host-buffer call every slot is closed. */
enum { MP3MI_SLOT_START = 1, MP3MI_SLOT_END = 2 };
int mp3mi_batch_encode_slots(mp3mi_batch *b, const int16_t *pcm_dev, int n_frames, const uint8_t *ctl_host,
                             const int32_t *n_samples_host, uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev);
int mp3mi_batch_slot_frames(const mp3mi_batch *b, int64_t *frames_host);

/* A bitrate per STREAM of a slot batch, chosen at its START: mp3mi_batch_encode_slots / mp3mi_batch_encode_slots_host_async with
 * one more HOST array, copied before the call returns and indexed like ctl_host (by slot in the device call, by row in the host
 * call).  kbps_host == NULL: exactly the calls without it, which are wrappers that pass NULL.
 *   kbps_host[s], slot s STARTs   0: the slot's create-time bitrate (mp3mi_batch_create's kbps[s] / kbps_all).  Otherwise an MPEG-1
 *                                 Layer III bitrate (32 .. 320, what mp3mi_batch_create accepts for the batch's rate and channel
 *                                 count) that does not exceed the batch's CEILING: the largest bitrate the batch was created with.
 *                                 That bitrate sizes the largest frame and with it mp3mi_batch_out_stride, so a server that takes
 *                                 requests of every bitrate creates its batch with kbps_all = 320 and chooses per START.  The cost:
 *                                 output rows -- and the host call's download, which moves whole rows -- are sized for the ceiling
 *                                 whatever the streams' bitrates are.
 *   kbps_host[s], no START        0, or, where a stream is open in the slot, the bitrate that stream has: a caller may pass one
 *                                 persistent array call after call.
 * Anything else returns MP3MI_ERR_ARG before anything is enqueued, and the batch is unchanged, like every other broken rule of a
 * per-slot call.
 * The bitrate belongs to the STREAM, not to the slot: it holds from the stream's START until the stream ends -- by END, by
 * mp3mi_batch_flush, by mp3mi_batch_reset, abandoned by a new START in its slot, or by a whole-file, ragged or host whole-file
 * call -- and afterwards the slot is back at its create-time bitrate.  Open streams keep their bitrates through every call that
 * continues them: per-slot calls with ctl 0, mp3mi_batch_encode_next going on with the open slots (also once every slot is open
 * at the same frame and the whole-batch bookkeeping has taken over), and the flush that ends them.  The calls that start EVERY
 * stream afresh -- mp3mi_batch_encode, mp3mi_batch_encode_ragged, mp3mi_batch_encode_host_async and an mp3mi_batch_encode_next
 * that starts every slot -- encode at the create-time bitrates, exactly as on a batch that never saw another one.
 *   mp3mi_batch_slot_kbps   host-side only, no wait: kbps_host[s] = the bitrate of the stream open in slot s, the slot's
 *                           create-time bitrate where none is.  Returns the batch's ceiling in kbps, or a negative MP3MI_ERR_*. */
int mp3mi_batch_encode_slots_kbps(mp3mi_batch *b, const int16_t *pcm_dev, int n_frames, const uint8_t *ctl_host,
                                  const int32_t *n_samples_host, const int32_t *kbps_host,
                                  uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev);
int mp3mi_batch_slot_kbps(const mp3mi_batch *b, int32_t *kbps_host);

/* Parking and resuming the streams of slots.  Every open slot must supply a full call of samples in every per-slot call; a
 * stream whose next samples are late is PARKED instead: exported out of its slot into a record the caller owns, and imported
 * later into any closed slot -- of this batch or of another batch of the same format, on another device too -- where the next
 * call continues it with ctl 0.  The same two calls move a stream to a lower slot (so that the live slots stay dense) and
 * take a checkpoint of a long stream.  The bytes the stream delivers from its START through its END, concatenated over every
 * slot and batch it lived in, are its file, as if it had never moved.
 *   A parked stream is a TICKET, host memory, and a STATE RECORD, device memory:
 *   mp3mi_slot_ticket             what the host must know of the stream; plain data, may be stored and sent anywhere.
 *     magic, version              MP3MI_SLOT_TICKET_MAGIC, MP3MI_SLOT_TICKET_VERSION (the layout of ticket and record)
 *     state_bytes                 mp3mi_batch_slot_state_bytes of the batch that exported it
 *     rate_hz, channels           the format of that batch, and what mp3mi_batch_set_mode, mp3mi_batch_set_header
 *     hdr_mode, hdr_flags,        (copyright << 3 | original << 2 | emphasis) and mp3mi_batch_set_error_protection had been
 *     error_protection            given when it was exported: a stream goes on under the header it began with
 *     kbps                        the stream's bitrate (mp3mi_batch_slot_kbps)
 *     frames                      frames encoded so far (mp3mi_batch_slot_frames)
 *   mp3mi_batch_slot_state_bytes  the size of one stream's state record, a multiple of 16: opaque device data -- the
 *                                 psychoacoustic state, the PCM history, the loop state with the bit reservoir and the stream's
 *                                 status, the file position, the carried bytes and their count, the two live bitrate words.
 *                                 It depends on the channel count only (and on the library's version: state_bytes is checked).
 *   mp3mi_batch_slots_export      parks the streams of the n slots slots_host[0 .. n-1] (HOST array, copied before the call
 *                                 returns): record i, of slot slots_host[i], is written at (char *) state_dev + i * state_stride,
 *                                 tickets_host[i] is filled before the call returns.  The slots must be distinct, in range and
 *                                 OPEN; n in 1 .. n_streams; state_stride >= mp3mi_batch_slot_state_bytes(b) and, like state_dev,
 *                                 a multiple of 16.  close != 0: the slots are closed afterwards WITHOUT a flush -- nothing is
 *                                 delivered, the pending bytes travel in the record -- so mp3mi_batch_slot_frames reports -1 for
 *                                 them, mp3mi_batch_slot_kbps their create-time bitrate again, and every later call treats them
 *                                 like any closed slot (out_len 0; a host call with a row map gives them no row).  close == 0:
 *                                 the streams go on; the records are a snapshot, which may be imported elsewhere any number of
 *                                 times (each import continues from the snapshot's frame).
 *   mp3mi_batch_slots_import      resumes n parked streams: record i goes into slot slots_host[i], which must be CLOSED
 *                                 (distinct, in range, n in 1 .. n_streams; stride and alignment as above).  Every ticket must
 *                                 carry the library's magic and version, this batch's state_bytes, rate, channels, header mode,
 *                                 header flags and error-protection setting, and a Layer III bitrate that does not exceed the
 *                                 batch's ceiling (mp3mi_batch_slot_kbps); frames >= 0.  Afterwards the slot is open at the
 *                                 ticket's frame count and bitrate -- whatever bitrate the slot was created with, exactly as
 *                                 after a START at that bitrate -- and the next per-slot call continues the stream with ctl 0
 *                                 (mp3mi_batch_encode_next too; a host call with a row map gives it a row).  Works as the first
 *                                 call on a fresh batch, and after a flush or reset.
 * Any broken rule returns MP3MI_ERR_ARG before anything is enqueued, and the batch is unchanged.
 * Order: neither call waits for the device.  Both run behind everything the batch has been given before and ahead of everything
 * it is given later, so a record may be imported into the batch that exported it at once.  Whoever else reads or writes a record
 * -- another batch's import, a copy to another device or to the host -- waits for the exporting batch first
 * (mp3mi_batch_sync), and an importing batch must be synced before its record is overwritten or freed.
 * Status: the stream's status word travels in the record.  A stream the reference would have died on stays void after it
 * resumes (out_len 0 in every call) and mp3mi_batch_stream_status reports the same code | frame << 8 from its new slot; the
 * abort is not reported a second time by mp3mi_batch_sync.
 * Until a batch's first export or import nothing of this exists: it launches and copies exactly what it did without. */
#define MP3MI_SLOT_TICKET_MAGIC 0x4B54334Du /* "M3TK" */
#define MP3MI_SLOT_TICKET_VERSION 1u
typedef struct mp3mi_slot_ticket {
    uint32_t magic, version;
    uint64_t state_bytes;
    int32_t rate_hz, channels;
    int32_t hdr_mode, hdr_flags;
    int32_t error_protection, kbps;
    int64_t frames;
} mp3mi_slot_ticket; /* 48 bytes, no padding */
size_t mp3mi_batch_slot_state_bytes(const mp3mi_batch *b);
int mp3mi_batch_slots_export(mp3mi_batch *b, int n, const int32_t *slots_host, int close, void *state_dev, size_t state_stride,
                             mp3mi_slot_ticket *tickets_host);
int mp3mi_batch_slots_import(mp3mi_batch *b, int n, const int32_t *slots_host, const void *state_dev, size_t state_stride,
                             const mp3mi_slot_ticket *tickets_host);

/* The feeder: any number of samples per call.  A per-slot call wants a full call of samples from every open slot; real streams
 * arrive in packets of 960 samples, in bursts, in whatever a decoder upstream hands over.  A feeder sits in front of a slot batch,
 * keeps a FIFO of samples per slot ON THE DEVICE, cuts the rows of every tick there (k_feed, csrc/k_format.hip) and parks and
 * resumes, with the two calls above, the streams that are short of a tick.  It touches no encoding kernel: a tick ends in one
 * mp3mi_batch_encode_slots_kbps call on rows the feeder owns.
 *   mp3mi_feed_create    a feeder for batch b -- on which no stream is open, and which has no feeder yet -- that encodes
 *                        tick_frames frames (1 .. the batch's max_frames) per ready lane and tick and takes up to max_push (>= 1)
 *                        samples per lane and call.  LANE s is slot s of the batch, one to one.
 *   mp3mi_feed_capacity  what a lane's FIFO holds: tick_frames * 1152 + max_push samples per channel.
 *   mp3mi_feed_tick      pcm_dev: device, int16 [n_streams][pcm_pitch][channels] in WAV order, pcm_pitch >= max_push; lane s brings
 *                        its first n_push_host[s] samples per channel (0 .. max_push; NULL: 0 for every lane).  ctl_host,
 *                        n_push_host and kbps_host are HOST arrays, copied before the call returns.
 *     A lane is READY when its pending samples and the pushed ones make a tick (tick_frames * 1152), or when it is ending (below).
 *     A ready lane encodes tick_frames frames; out_len_dev[s] receives the bytes of its file that became final, as for
 *     mp3mi_batch_encode_slots.  A lane that is not ready delivers out_len 0; its samples stay pending, nothing of it is lost, and
 *     a stream it holds in the batch is parked until the lane is ready again.  A tick in which no lane is ready launches no
 *     encoding kernel; out_len_dev is zeroed all the same, in stream order.
 *     ctl_host[s]   MP3MI_SLOT_START: a new stream begins in the lane with this call's first pushed sample, at kbps_host[s] (the
 *                   rules of mp3mi_batch_encode_slots_kbps, checked here; NULL or 0: the slot's create-time bitrate).  A stream
 *                   open in the lane is abandoned with its pending samples and its parked record, as mp3mi_batch_encode_slots
 *                   abandons one.  The batch sees the START in the first tick in which the lane is ready.
 *                   MP3MI_SLOT_END: this call's samples are the stream's last.  From here the lane DRAINS: tick_frames frames per
 *                   tick while more than tick_frames * 1152 samples are pending; in the first tick with that many or fewer (0
 *                   too) the batch gets its END with exactly that count, and the lane closes.  START | END with few samples is a
 *                   one-call file.
 *     MP3MI_ERR_ARG, with nothing enqueued and feeder and batch unchanged -- the check runs over all lanes first --: unknown ctl
 *     bits; a push or an END on a closed lane without START; START, END or a push on a draining lane; n_push outside
 *     0 .. max_push; pending + push above mp3mi_feed_capacity; a NULL pointer other than n_push_host / kbps_host; pcm_pitch <
 *     max_push; out_stride < mp3mi_batch_out_stride(b, tick_frames); a kbps the per-slot call would refuse.
 *     The bytes a lane delivers from a stream's START through the tick that closes it, concatenated, are byte for byte what
 *     mp3mi_batch_encode_ragged gives for the stream's samples at its bitrate -- however the samples were cut into pushes and
 *     however often the stream sat out a tick.  The call waits for nothing: ticks may be issued back to back.
 *   mp3mi_feed_lanes     host bookkeeping only, no wait: per lane the pending samples, the frames encoded so far (-1: closed) and
 *                        flags -- bit 0 parked, bit 1 draining, bit 2 started but not yet in the batch.  Returns the number of
 *                        lanes that are not closed.
 *   mp3mi_feed_destroy   resets the batch (streams in lanes are abandoned) and detaches; mp3mi_batch_destroy on a batch with a
 *                        feeder attached frees the feeder with it (do not destroy it afterwards).
 * While a feeder is attached the batch's streams are the feeder's: mp3mi_batch_encode, _encode_ragged, _encode_next,
 * _encode_slots(_kbps), _flush, _reset, _slots_export, _slots_import, the host-buffer calls (_encode_host_async,
 * _encode_slots(_kbps)_host_async) and _set_header / _set_mode / _set_error_protection return MP3MI_ERR_ARG; mp3mi_batch_sync,
 * _stream_status, _slot_frames, _slot_kbps and the timing accessors work as ever (a parked lane's slot reads as closed).  A batch
 * that never gets a feeder allocates and launches exactly what it did without.
 *
 * MORE LANES THAN SLOTS.  Streams that arrive in packets are slow: a tick of 32 frames holds 0.84 s of audio and takes milliseconds, so
 * a lane that is tied to a slot leaves the slot idle nearly all the time.  A feeder made by mp3mi_feed_create_lanes has n_lanes lanes in
 * front of the batch's n_streams slots, in any relation (fewer, as many, more): a lane's FIFO and its parked record are the lane's, a
 * slot is lent to a lane for the ticks in which it encodes.  Each kind of feeder has its own tick: mp3mi_feed_tick returns MP3MI_ERR_ARG
 * on a feeder made by mp3mi_feed_create_lanes, mp3mi_feed_tick_lanes on one made by mp3mi_feed_create.
 *   mp3mi_feed_create_lanes  n_lanes >= 1; max_rows in 1 .. n_lanes: the most lanes that may push in one tick (it sizes the upload
 *                        blocks); ring_samples: a lane's FIFO in samples per channel, at least tick_frames * 1152 + max_push, 0: exactly
 *                        that (mp3mi_feed_capacity reports it).  A lane that is ready but waits for a slot keeps taking pushes until
 *                        its FIFO is full, so a server sizes it for the wait it accepts.  Otherwise the rules of mp3mi_feed_create.
 *   mp3mi_feed_n_lanes   the lanes of a feeder (n_streams for one made by mp3mi_feed_create); mp3mi_feed_lanes takes arrays of that
 *                        many entries.
 *   mp3mi_feed_tick_lanes  the pushes come as ROWS: row r is lane row_lane_host[r] (strictly increasing, each in 0 .. n_lanes-1; n_rows
 *                        in 0 .. max_rows), its samples row r of pcm_dev [n_rows][pcm_pitch][channels], and ctl_host, n_push_host and
 *                        kbps_host are indexed by row, with the meaning they have in mp3mi_feed_tick word for word.  A lane that no
 *                        row names pushes nothing and has ctl 0; it may encode all the same (it drains, or gets a slot at last).  With
 *                        n_rows == 0 the four row arrays and pcm_dev may be NULL; with n_rows > 0 none of them may.  All host arrays
 *                        are copied before the call returns.
 *     Who encodes.  A lane is READY as above.  If no more than n_streams lanes are ready, all encode.  Otherwise the n_streams lanes
 *     encode whose current unbroken spell of being ready began in the earliest tick, ties going to the lower lane; a lane that encodes
 *     and is still ready begins a new spell in the next tick.  So no ready lane encodes twice while another that was ready before it
 *     has not encoded once.  A ready lane that gets no slot keeps its samples, delivers nothing, is parked if its stream is in a slot,
 *     and shows bit 3 (value 8: ready, waiting for a slot) in mp3mi_feed_lanes' flags until the tick in which it encodes.
 *     Where.  A chosen lane whose stream is in a slot keeps the slot.  Every other stream in a slot leaves it (parked).  The other
 *     chosen lanes take the free slots -- those vacated in this very tick among them --, the lowest free slot going to the lowest lane:
 *     a parked stream is resumed there, a stream the batch has not seen STARTs there.  A START at kbps 0 means the create-time bitrate
 *     of the slot in which the stream first encodes; until then only kbps 0 may be passed with the lane's pushes.
 *     Output is by SLOT, as mp3mi_batch_encode_slots writes it: out_dev [n_streams][out_stride], out_len_dev [n_streams].
 *     slot_lane_host [n_streams] is filled before the call returns (host bookkeeping, no device wait): entry i is the lane that encodes
 *     in slot i in this tick, or -1, and out_len_dev[i] is 0 where it is -1.  A tick in which nothing encodes launches no encoding
 *     kernel and zeroes out_len_dev in stream order.  The bytes a LANE delivers from a stream's START through the tick that closes it,
 *     gathered slot by slot through slot_lane_host and concatenated, are the stream's file, as above.
 *     MP3MI_ERR_ARG, nothing enqueued, feeder and batch unchanged: everything mp3mi_feed_tick refuses, per row's lane; n_rows outside
 *     0 .. max_rows; a row map out of order or out of range; a NULL row array or pcm_dev with n_rows > 0; a NULL out_dev, out_len_dev
 *     or slot_lane_host; pending + push above mp3mi_feed_capacity (a waiting lane whose FIFO is full).
 *     Status: mp3mi_batch_stream_status stays by SLOT; with the slot_lane_host of the tick it names the lane.  The status word travels
 *     in the record and an abort is reported by one sync only (above).  There is no status query per lane.
 *
 * TICKS ON HOST BUFFERS.  A server receives packets into host memory and writes MP3 bytes from host memory.  For a feeder made by
 * mp3mi_feed_create_lanes (for one lane per slot: n_lanes == n_streams), mp3mi_feed_tick_lanes_host_async is mp3mi_feed_tick_lanes --
 * its rules, its scheduler, its lane bookkeeping and its refusals, word for word -- on host buffers; on a feeder made by
 * mp3mi_feed_create it returns MP3MI_ERR_ARG.  Ticks on device buffers and on host buffers may alternate on one feeder.
 *     Input is PACKED: pcm_host holds the tick's packets back to back, no pitch; row r's n_push_host[r] samples per channel begin at
 *     sample sum(n_push_host[0 .. r)).  A row may push 0 samples.  Exactly sum(n_push) * channels * 2 bytes cross PCIe, in one copy;
 *     with n_rows == 0, or every push 0, pcm_host may be NULL and nothing is uploaded.
 *     Output is by ENCODING LANE, dense.  Filled before the call returns, without a device wait: *n_out_host (0 .. n_streams),
 *     out_lane_host[0 .. n_out) (the lanes that encode in this tick, ascending) and out_slot_host[0 .. n_out) (the slot each encodes
 *     in: mp3mi_batch_stream_status stays by slot, so this names the lane of a reference abort).  Row i of out_host (out_stride >=
 *     mp3mi_batch_out_stride(b, tick_frames)) and out_len_host[i] receive what slot out_slot_host[i] would have delivered in
 *     mp3mi_feed_tick_lanes; a row is zero behind its length.  Only n_out rows and lengths come down: the caller provides room for
 *     n_streams of each, and rows and lengths from n_out on are not touched.  A tick in which nothing encodes downloads nothing.
 *     Asynchronous, two ticks in flight; the third waits for the first.  The three lists are filled and the control arrays copied
 *     before the call returns; pcm_host, out_host and out_len_host must stay valid until mp3mi_feed_host_wait for that tick, or
 *     mp3mi_batch_sync, has returned.  Page-locked buffers (mp3mi_host_alloc) overlap with the kernels; pageable ones work and block.
 *     MP3MI_ERR_ARG, nothing enqueued, feeder and batch unchanged: everything mp3mi_feed_tick_lanes refuses (there is no pcm_pitch);
 *     a NULL out_host, out_len_host, out_lane_host, out_slot_host or n_out_host; a NULL pcm_host with a non-zero push.
 *   mp3mi_feed_host_wait  waits for the upload and the download of the host tick issued ticks_back (0 or 1) HOST ticks ago and for
 *                        nothing later.  It lets no call hold go: a host tick leaves none in force (its samples are still crossing
 *                        PCIe when it is issued, so its kernels neither join the tick before nor are held for the next), and a
 *                        later tick's stays.  MP3MI_ERR_ARG when there is no such tick.
 *   mp3mi_feed_host_io_stats  over the host ticks so far, waiting for them: h2d_bytes, exactly sum(n_push) * channels * 2; d2h_bytes,
 *                        exactly n_out * (out_stride + 4) per tick; the copies' event times; calls, the ticks.
 * A feeder that never makes a host tick creates no stream, no event and no buffer for them.
 * Not yet: a status query per lane, and, for Layer III, a direct path for a parked record between a lane and a slot (the records of a
 * tick pass through a dense block).  Layers I and II have a feeder of their own, with that path: mp3mi_l12_feed_* (mp3mi_l12.h). */
typedef struct mp3mi_feed mp3mi_feed;
int mp3mi_feed_create(mp3mi_feed **out, mp3mi_batch *b, int tick_frames, int max_push);
void mp3mi_feed_destroy(mp3mi_feed *f);
size_t mp3mi_feed_capacity(const mp3mi_feed *f);
int mp3mi_feed_tick(mp3mi_feed *f, const int16_t *pcm_dev, size_t pcm_pitch, const uint8_t *ctl_host, const int32_t *n_push_host,
                    const int32_t *kbps_host, uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev);
int mp3mi_feed_lanes(const mp3mi_feed *f, int32_t *pending_host, int64_t *frames_host, uint8_t *flags_host);
int mp3mi_feed_create_lanes(mp3mi_feed **out, mp3mi_batch *b, int n_lanes, int max_rows, int tick_frames, int max_push, int ring_samples);
int mp3mi_feed_n_lanes(const mp3mi_feed *f);
int mp3mi_feed_tick_lanes(mp3mi_feed *f, int n_rows, const int32_t *row_lane_host, const int16_t *pcm_dev, size_t pcm_pitch,
                          const uint8_t *ctl_host, const int32_t *n_push_host, const int32_t *kbps_host, uint8_t *out_dev, size_t out_stride,
                          uint32_t *out_len_dev, int32_t *slot_lane_host);

/* Ragged batch: stream s has n_samples_dev[s] valid samples per channel (0 <= n <= n_frames*1152) in
 * its row of pcm_dev (row pitch n_frames*1152*channels as above).  As the reference's get_audio /
 * read_samples do (/root/reference/src/encode.c:123-269, zero fill :162-166), the last partial frame
 * is zero-filled and the stream ends after ceil(n/1152) frames; out_len_dev[s] is its own file
 * length (0 for a stream without samples). */
int mp3mi_batch_encode_ragged(mp3mi_batch *b, const int16_t *pcm_dev, const int32_t *n_samples_dev, int n_frames,
                              uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev);

/* Header bits the reference's driver sets from -c, -o and -d (/root/reference/src/musicin.c:263-275,
 * written at src/l3bitstream.c:330-334): copyright 0/1, original 0/1, emphasis 0..3.  Applies to later
 * encode calls of this batch. */
int mp3mi_batch_set_header(mp3mi_batch *b, int copyright, int original, int emphasis);

/* Header mode field, -m of the reference's driver (/root/reference/src/musicin.c:226-234, src/common.h:233-236):
 * stereo or dual channel for two-channel batches, mono for one-channel ones (the default follows the channel
 * count).  Dual channel changes nothing but the header field -- the reference's Layer III encoder treats the two
 * channels independently in every mode.  Joint stereo is refused (MP3MI_ERR_ARG) as the reference refuses it for
 * Layer III (src/musicin.c:548-552). */
enum { MP3MI_MODE_STEREO = 0, MP3MI_MODE_JOINT_STEREO = 1, MP3MI_MODE_DUAL_CHANNEL = 2, MP3MI_MODE_MONO = 3 };
int mp3mi_batch_set_mode(mp3mi_batch *b, int mode);

/* Error protection, -e of the reference's driver: the protection bit of the header is cleared and a 16-bit CRC
 * word follows the header, which the reference never computes for Layer III and writes as zero
 * (/root/reference/src/l3bitstream.c:312, 325, 338-342); the side information grows by 16 bits, so the mean bits
 * per granule shrink (src/musicin.c:744-746).  Reproduced bit for bit -- including the zero CRC. */
int mp3mi_batch_set_error_protection(mp3mi_batch *b, int on);

/* Milliseconds spent inside the dominant (iteration loop) kernel and inside all kernels during
 * the last encode call, measured with HIP events on the batch's stream. */
int mp3mi_batch_last_timing(mp3mi_batch *b, float *loop_kernel_ms, float *all_kernels_ms,
                            int *loop_kernel_launches);

/* The same summed over all encode calls since the batch was created (waits for the calls issued so far): calls
 * may be issued back to back without a sync in between -- a call's feed-forward kernels then run beside the loop
 * kernels of the call before -- and their timing read once at the end. */
int mp3mi_batch_total_timing(mp3mi_batch *b, double *loop_kernel_ms, double *all_kernels_ms,
                             long *loop_kernel_launches, long *calls);

/* Host buffers in, host buffers out, OVERLAPPED with the encode -- what the reference's driver does frame by frame with
 * get_audio / read_samples and fwrite (/root/reference/src/encode.c:123-269, src/common.c:843-868), for a whole batch:
 * the call's PCM crosses PCIe chunk by chunk on a copy stream while the chunks before it are encoded, and the call's
 * file bytes come back in one copy behind its last formatter; with calls issued back to back the next call's PCM goes up
 * and this call's bytes come down beside the next call's kernels (two calls may be in flight; the batch keeps two
 * device copies of PCM and output).  out_stride = mp3mi_batch_out_stride(b, max_frames) makes the download one plain copy.
 *   pcm_host: [n_streams][n_frames*1152][channels]; out_host: [n_streams][out_stride], out_stride >= n_frames * the largest
 *   frame size + 1; out_len_host: [n_streams].  A whole-file call like mp3mi_batch_encode: every stream starts afresh.
 * Asynchronous: returns once everything is enqueued; the buffers must stay valid -- and the results are there -- when
 * mp3mi_batch_sync returns (which reports MP3MI_ERR_REFERENCE_ABORT as for device calls).  Page-locked buffers
 * (mp3mi_host_alloc, hipHostMalloc, hipHostRegister) move at the full PCIe rate beside the kernels; pageable memory
 * works, but the runtime stages it and the call blocks while it does.  bench.py --host-io measures this path. */
int mp3mi_batch_encode_host_async(mp3mi_batch *b, const int16_t *pcm_host, int n_frames, uint8_t *out_host, size_t out_stride,
                                  uint32_t *out_len_host);
/* Continuous batching on HOST buffers that hold a row per LIVE slot: mp3mi_batch_encode_slots with every array indexed by
 * ROW instead of by slot, the PCM taken from and the bytes delivered to host memory, overlapped with the kernels like
 * mp3mi_batch_encode_host_async (two calls in flight, the third blocks on the first; page-locked buffers overlap, pageable
 * ones work and block).  Only the n_rows rows cross PCIe: a slot batch is sized for the peak, and closed slots cost no transfer.
 *   row_slot_host[n_rows]   the slot of each row: strictly increasing, each in 0 .. n_streams-1.  NULL: n_rows == n_streams
 *                           and row r is slot r.
 *   ctl_host[r], n_samples_host[r] (may be NULL)   as for mp3mi_batch_encode_slots, for the slot of row r.
 *   pcm_host [n_rows][n_frames*1152][channels]; out_host [n_rows][out_stride], out_stride >= mp3mi_batch_out_stride(b,
 *   n_frames); out_len_host [n_rows]: per row the bytes of its stream's file that became final with the call (the rest of the
 *   row is zero when a row map is given).
 * A slot that no row names must be closed and stays closed.  An open slot without a row, a row whose slot is neither open nor
 * starting, a slot index out of range or out of order, n_rows outside 1 .. n_streams, and every error
 * mp3mi_batch_encode_slots refuses return MP3MI_ERR_ARG before anything is enqueued, and the batch is unchanged.  The three
 * control arrays are copied before the call returns; pcm_host, out_host and out_len_host must stay valid until the call's
 * results have been waited for (mp3mi_batch_host_wait, mp3mi_batch_sync).  Slots opened or closed here are the slots of
 * mp3mi_batch_encode_slots, slot_frames, stream_status, encode_next, flush and reset: device and host calls may alternate.
 * mp3mi_batch_host_io_stats counts these calls: h2d_bytes grows by n_rows * n_frames*1152 * channels * 2 per call.
 *
 * mp3mi_batch_host_wait(b, k) waits until the host-buffer call (this one or mp3mi_batch_encode_host_async) issued k calls
 * ago -- 0: the latest, 1: the one before -- has delivered out_host / out_len_host, and for nothing later: a server issues
 * tick t+1 and then collects tick t.  Returns MP3MI_OK, MP3MI_ERR_ARG (k not 0 or 1, or no such call) or MP3MI_ERR_HIP;
 * reference aborts are reported by mp3mi_batch_sync and mp3mi_batch_stream_status as ever. */
int mp3mi_batch_encode_slots_host_async(mp3mi_batch *b, const int16_t *pcm_host, int n_frames, int n_rows,
                                        const int32_t *row_slot_host, const uint8_t *ctl_host, const int32_t *n_samples_host,
                                        uint8_t *out_host, size_t out_stride, uint32_t *out_len_host);
/* The same with a bitrate per row's stream, kbps_host[n_rows] (mp3mi_batch_encode_slots_kbps above: NULL is the call without it) */
int mp3mi_batch_encode_slots_kbps_host_async(mp3mi_batch *b, const int16_t *pcm_host, int n_frames, int n_rows,
                                  const int32_t *row_slot_host, const uint8_t *ctl_host, const int32_t *n_samples_host,
                                  const int32_t *kbps_host, uint8_t *out_host, size_t out_stride, uint32_t *out_len_host);
int mp3mi_batch_host_wait(mp3mi_batch *b, int calls_back);
/* Bytes moved and time spent inside the copies (HIP events on the two copy streams) over all host-buffer calls since the
 * batch was created; waits for the calls issued so far. */
typedef struct mp3mi_host_io_stats {
    double h2d_bytes, d2h_bytes; /* PCM up, file bytes down */
    double h2d_ms, d2h_ms;       /* summed durations of the copies */
    long calls;
} mp3mi_host_io_stats;
int mp3mi_batch_host_io_stats(mp3mi_batch *b, mp3mi_host_io_stats *st);
/* The feeder's ticks on host buffers (TICKS ON HOST BUFFERS, above) */
int mp3mi_feed_tick_lanes_host_async(mp3mi_feed *f, int n_rows, const int32_t *row_lane_host, const int16_t *pcm_host,
                                     const uint8_t *ctl_host, const int32_t *n_push_host, const int32_t *kbps_host, uint8_t *out_host,
                                     size_t out_stride, uint32_t *out_len_host, int32_t *out_lane_host, int32_t *out_slot_host,
                                     int32_t *n_out_host);
int mp3mi_feed_host_wait(mp3mi_feed *f, int ticks_back);
int mp3mi_feed_host_io_stats(mp3mi_feed *f, mp3mi_host_io_stats *st);
/* page-locked host memory for the call above, for callers that do not link HIP themselves; NULL on failure */
void *mp3mi_host_alloc(size_t bytes);
void mp3mi_host_free(void *p);

/* Host-buffer convenience wrapper (tests, smoke): a batch of its own per call, mp3mi_batch_encode_host_async, sync.
 * pcm: [n_streams][n_frames*1152*channels]; out: [n_streams][out_stride]; out_len: [n_streams]. */
int mp3mi_encode_host(int n_streams, int rate_hz, int channels, const int *kbps, int kbps_all,
                      const int16_t *pcm, int n_frames, uint8_t *out, size_t out_stride,
                      uint32_t *out_len);

/* The same with per-stream sample counts (n_samples, host, may be NULL) and header bits
 * (mp3mi_batch_encode_ragged, mp3mi_batch_set_header). */
int mp3mi_encode_host_ex(int n_streams, int rate_hz, int channels, const int *kbps, int kbps_all,
                         const int16_t *pcm, const int32_t *n_samples, int n_frames, int copyright,
                         int original, int emphasis, uint8_t *out, size_t out_stride, uint32_t *out_len);

/* Stage seams of the LAST chunk of the last encode call, copied to host memory (parity tests
 * compare them with oracle/stage_dump.h).  what: 0 = psychoacoustic records (mp3mi_psy_out),
 * 1 = xr (f64[576] per granule-channel), 2 = quantised values (int16[576]), 3 = side info
 * (mp3mi_frame_side per frame), 4 = raw subband samples (f64[576], enabled by
 * mp3mi_batch_debug_enable), 5 = the loop's stateless head (csrc/mp3mi_dev.h: the first 472 bytes of mp3mi_loop_prep
 * per granule-channel); the psychoacoustic transforms' outputs (src/subs.c:38-123): 6 = long energies (f32, rows of 544
 * per granule-channel: lines 0..512, the rest padding), 7 = short energies (f32[3][129]), 8 = raw lines (f32[312]:
 * (re, im) of short lines 2..51 of the three windows, then re[6], im[6] of long lines 0..5).  Returns the number of
 * bytes written, or a negative error. */
long mp3mi_batch_debug_fetch(mp3mi_batch *b, int what, void *host_dst, size_t cap);
void mp3mi_batch_debug_enable(mp3mi_batch *b, int on);

/* Two-tier decisions: six places decide from a cheap value with a proven error bound and
 * repeat the computation the reference's way only when the decision could depend on the last bits.  Each bit
 * forces the second (exact) tier everywhere; the emitted bytes must not change (tests/test_gpu_tiers.py).  The
 * environment variables MP3MI_{NOISE,PHASE,PSY,QUANT,PREP}_EXACT=1 set the same bits at mp3mi_batch_create. */
enum {
    MP3MI_TEST_NOISE_EXACT = 1,  /* calc_noise: the reference's sequential band sums (k_loop) */
    MP3MI_TEST_PHASE_EXACT = 2,  /* phases: correctly rounded atan2 (k_cw) */
    MP3MI_TEST_PSY_EXACT = 4,    /* masking threshold: dm_log / dm_exp (k_psy) */
    MP3MI_TEST_QUANT_EXACT = 8,  /* quantiser: every line against the (i - 0.4054)^(4/3) table (k_loop) */
    MP3MI_TEST_PREP_EXACT = 16,  /* the loop's stateless head by k_prep for every record, the reference's walk with correctly
                                    rounded logs, instead of k_mdct's tail */
    MP3MI_TEST_CW_EXACT = 32,    /* unpredictability: correctly rounded sines and cosines for every record (k_cw) */
    MP3MI_TEST_ALL_EXACT = 63,
    MP3MI_TEST_PREP_LIST = 64    /* not a tier: k_mdct's tail lists every third record as undecided and spoils what it wrote for
                                    it, so that the loop reads what k_prep computed through the list (the path of the ~1e-7
                                    records the tail really cannot decide) */
};
int mp3mi_batch_set_test_flags(mp3mi_batch *b, unsigned flags);

/* Deterministic synthetic PCM (benchmarks / tests): interleaved int16, n_per_ch samples per channel. */
void mp3mi_synth_pcm(int16_t *out, long n_per_ch, int channels, int rate_hz, uint32_t stream,
                     uint32_t seed);

/* Self-test hook: evaluates function fn of the device math layer (see csrc/k_debug.hip) on the
 * GPU for n host-side arguments.  Used by tests to prove device == host bit for bit. */
int mp3mi_debug_dmath(int fn, const double *x, const double *y, double *out, size_t n);

/* Self-test hook: maximum relative error, on this device, of the three approximate expressions the quantiser's
 * first tier is built from (csrc/k_debug.hip): out[0] raw sqrt(a * raw sqrt(a)) vs a^(3/4) over all 2^24 floats
 * of [1, 4); out[1] raw exp2 at the 801 step sizes the search can ask for; out[2] raw exp2 over 2^24 arguments
 * of [-80, 80].  tests/test_gpu_tiers.py asserts that their sum stays inside the guard band's 7e-7 budget. */
int mp3mi_debug_fastmath_bounds(double out[3]);
/* What v_cvt_pknorm_u16_f32 -- the rounding step of the quantiser's first tier -- returns on this device, over every float of the
 * range the quantiser feeds it (csrc/k_debug.hip): out[0] = max |n - a * 65535| (the proof in csrc/loop_pass.h needs <= 0.5),
 * out[1] = non-monotone neighbours, out[2] = clamp / half mismatches (both 0). */
int mp3mi_debug_pknorm_bound(double out[3]);
/* Self-test hook: one quantise+count pass of k_loop (csrc/loop_pass.h; the hook: csrc/k_loop_qc.hip), on n_gran granules of 576 xr each (rate_hz one of
 * 44100 / 48000 / 32000).  gran[4 i ..]: the step q (MP3MI_STEP_MIN .. +800, the reference's quantizerStepSize), the block type
 * (0..3), a rescale plan -- n_amp (0..16) amplifications of every scalefactor band by sqrt(2) and, before them, pre (0 / 1) one
 * pre-emphasis (not with block type 2) -- applied by the kernel's own statements to xr in double and to its cached |xr|^(3/4) in
 * float.  Out per granule: ix[576] (magnitudes), the rescaled xr[576] and MP3MI_QC_FIELDS words indexed by MP3MI_QC_*.  The
 * last four are diagnostics: the all-zero shortcut was taken, the rare (exact-table) tier ran, the number of lines whose upper
 * and lower estimates differ, the clamp at the table's end (`over`) was armed.  MP3MI_ERR_NO_DEVICE without a GPU. */
enum {
    MP3MI_QC_N_NZ, MP3MI_QC_N_BIG, MP3MI_QC_M1, MP3MI_QC_M2, MP3MI_QC_BITS, MP3MI_QC_BIG_VALUES, MP3MI_QC_COUNT1,
    MP3MI_QC_COUNT1TABLE_SELECT, MP3MI_QC_TABLE_SELECT0, MP3MI_QC_TABLE_SELECT1, MP3MI_QC_TABLE_SELECT2,
    MP3MI_QC_REGION0_COUNT, MP3MI_QC_REGION1_COUNT, MP3MI_QC_ADDRESS1, MP3MI_QC_ADDRESS2, MP3MI_QC_ADDRESS3,
    MP3MI_QC_ALL_ZERO, MP3MI_QC_RARE_TIER, MP3MI_QC_N_DIFFER, MP3MI_QC_OVER, MP3MI_QC_FIELDS
};
int mp3mi_debug_quantize_count(int rate_hz, int n_gran, const double *xr, const int32_t *gran, int16_t *ix, double *xr_out,
                               int32_t *fields);
/* Self-test hook: the peak lines of n_gran granules of 576 xr each, as k_mdct's tail records them for k_loop's region maxima
 * (csrc/mp3mi_dev.h, peak cells): peak[32 i + c] = a line of cell c of granule i with the largest |xr|; cell_first[33]: the cells'
 * first lines and, last, 576.  MP3MI_ERR_NO_DEVICE without a GPU. */
int mp3mi_debug_peak_lines(int rate_hz, int n_gran, const double *xr, uint16_t *peak, int32_t *cell_first);
/* Self-test hook: k_format (csrc/k_format.hip), as a whole-file batch call launches it, on n_streams chains of GIVEN frames of one
 * format: rate_hz, channels, kbps, the header's mode field (0 stereo, 1 joint, 2 dual, 3 mono) and hdr_flags (mode_ext << 4 |
 * copyright << 3 | original << 2 | emphasis), crc (error protection).  Chain s has n_frames_s[s] <= n_frames frames; ix holds
 * the signed quantised values [n_streams][2 * n_frames][channels][576], side the mp3mi_frame_side records (csrc/mp3mi_dev.h)
 * [n_streams][n_frames].  Out: the files' bytes in rows of out_stride >= n_frames * frame bytes + 1, their lengths and per
 * stream 0 or MP3MI_STREAM_* | frames << 8 (a chain the reference dies on in its flush: length 0).
 * MP3MI_ERR_ARG, and nothing is launched, for a chain outside the formatter's domain ("III_format_bitstream"):
 * main_data_begin is the reservoir's (0 for frame 0, then + slot bytes - the frame's bytes, 0..511, never negative), a frame's
 * part2_3_length sum + resvDrain is a multiple of 8, part2_3_length <= 4095 covers part2_length (the scalefactor bits as
 * scalefac_compress, scfsi and the granule give them) + the code bits, each region's table exists and takes the region's
 * maximum (0 only for zeros), block type 2 has (big_values, count1) = (288, 0) or (0, 0), types 1 and 3 region counts 7 / 13,
 * 2 big_values + 4 count1 <= 576, count1 lines are 0 / +-1 and the lines behind them 0, scalefactors fit their slen. */
int mp3mi_debug_format_frames(int rate_hz, int channels, int kbps, int hdr_mode, int hdr_flags, int crc, int n_streams, int n_frames,
                              const int32_t *n_frames_s, const int16_t *ix, const void *side, uint8_t *out, size_t out_stride,
                              uint32_t *out_len, int32_t *status);
/* Self-test hook: k_feed (csrc/k_format.hip), as mp3mi_feed_tick launches it, on GIVEN rings, descriptors and push rows.  Lane s of
 * n_lanes: desc[4 s ..] = {head, pending, n_push, take} in samples per channel; its ring of cap samples at ring + s * ring_pitch *
 * channels, its push row at push + s * push_pitch * channels, its dense row of row_samples at rows + s * row_pitch * channels (the
 * pitches in samples per channel; ring_pitch >= cap and row_pitch >= row_samples, both multiples of 16 bytes; what lies between the
 * records is the caller's to fill and to check).  The first `take` samples of ring[head .. head + pending) (wrapping at cap)
 * followed by push[0 .. n_push) go to the row; the pushed samples behind them are appended to the ring at
 * (head + pending + the pushed samples the row took) % cap.  All three arrays come back as the device holds them afterwards.
 * MP3MI_ERR_ARG, and nothing is launched, unless for every lane head < cap, pending + n_push <= cap, take <= pending + n_push,
 * take <= row_samples and n_push <= push_pitch.  MP3MI_ERR_NO_DEVICE without a GPU. */
int mp3mi_debug_feed(int channels, int n_lanes, int cap, int row_samples, const uint32_t *desc, int16_t *ring, size_t ring_pitch,
                     int16_t *push, size_t push_pitch, int16_t *rows, size_t row_pitch);
/* Self-test hook: k_feed_lanes (csrc/k_format.hip), as mp3mi_feed_tick_lanes launches it, over n_active descriptors of eight uint32
 * {head, pending, n_push, take, lane, push_row, slot, 0}: the ring is lane `lane` of n_lanes, the push row `push_row` of n_push_rows, the
 * row that is cut `slot` of n_slots (pitches and copies as for mp3mi_debug_feed; the three arrays go up and come back whole).
 * MP3MI_ERR_ARG (-1), and nothing is launched, unless every descriptor keeps the rules of mp3mi_debug_feed, its three indices are in
 * range, its last word is 0, no lane is named twice, no slot by two descriptors that take and no push row by two that push.
 * MP3MI_ERR_NO_DEVICE without a GPU. */
int mp3mi_debug_feed_lanes(int channels, int n_active, int n_lanes, int n_push_rows, int n_slots, int cap, int row_samples,
                           const uint32_t *desc, int16_t *ring, size_t ring_pitch, int16_t *push, size_t push_pitch, int16_t *rows,
                           size_t row_pitch);
/* Self-test hook: k_feed_packed (csrc/k_format.hip), as mp3mi_feed_tick_lanes_host_async launches it.  As mp3mi_debug_feed_lanes, but
 * the pushes lie in ONE buffer `packed` of n_packed samples (of all channels) and word 5 of a descriptor is its push's first sample
 * there; the work list is built as the tick builds it, with wg_bytes as the bytes a workgroup moves (the product's: 256 * 16 * 4).
 * MP3MI_ERR_ARG (-1), and nothing is launched, unless every descriptor keeps the rules of mp3mi_debug_feed (but for the push pitch),
 * lane and slot are in range, the last word is 0, no lane is named twice, no slot by two descriptors that take, every push lies
 * inside the packed buffer and no two pushes share a sample.  MP3MI_ERR_NO_DEVICE without a GPU. */
int mp3mi_debug_feed_packed(int channels, int n_active, int n_lanes, int n_packed, int n_slots, int cap, int row_samples, size_t wg_bytes,
                            const uint32_t *desc, int16_t *ring, size_t ring_pitch, int16_t *packed, int16_t *rows, size_t row_pitch);
/* Self-test hook: the iteration loop on n_streams chains of n_frames frames of GIVEN records, through the three launches of the
 * drop-in iteration_loop (csrc/dropin.cpp): k_prep_tail, k_prep on the list it leaves, k_loop with no placement and no gate
 * (csrc/loop_debug.cpp; k_loop.hip is the product's).  One format per call -- rate_hz, channels, crc (error protection) -- and a
 * bitrate per stream, kbps[n_streams].  xr[n_streams][2 * n_frames][channels][576] is the spectrum, psy the mp3mi_psy_out records
 * (csrc/mp3mi_dev.h: pe, ratio_l[21], ratio_s[12][3], block_type) in the same order; state_in is NULL (fresh streams) or one loop
 * state per stream, as state_out returns them: int32 words, [0] ResvSize, then sc_en_tot[2][2], sc_en[2][2][21], sc_xm[2][2][21],
 * sc_xrmax[2][2], addr[2][2][3] (address1..3 of the last frame) and, last, the status word (0 or MP3MI_STREAM_* | frame << 8).
 * Out: the signed quantised values ix[n_streams][2 * n_frames][channels][576], the mp3mi_frame_side records
 * side[n_streams][n_frames], state_out, and *n_listed = the records k_mdct's tail could not decide and k_prep redid.
 * MP3MI_ERR_ARG, and nothing is launched, for anything outside the loop's domain ("iteration_loop"; the bounds are
 * derived in csrc/loop_debug.cpp): every xr is 0 (either sign) or 2^-500 <= |xr| <= 2^64; pe in [0, 1e8]; every ratio in [0, 1e30]
 * (no NaN, no infinity anywhere); block_type 0..3; a known bitrate; at most 4096 streams of at most 64 frames; an initial state
 * whose ResvSize is a multiple of 8 in [0, ResvMax] (ResvMax = min(7680 - bits per frame, 4088), 0 if negative), whose status word
 * is 0, whose addresses lie in 0..576 and whose stored logarithms (sc_en_tot, sc_en, sc_xm) are within +-2^20 -- sc_xrmax, which is
 * only compared with 0, may hold anything: every state_out of a legal chain is a legal state_in --; and no granule whose start step
 * (quantanf_init, recomputed on the host in double, plus a margin of 1e-6 on 8 ln sfm) or whose all-zero step lies above 400,
 * the end of the table of step sizes the search reads.  MP3MI_ERR_NO_DEVICE without a GPU. */
int mp3mi_debug_iteration_loop(int rate_hz, int channels, int crc, int n_streams, int n_frames, const int32_t *kbps, const double *xr,
                               const void *psy, const void *state_in, int16_t *ix, void *side, void *state_out, int32_t *n_listed);
/* diagnostics: of the (granule, channel) records of the last call's LAST chunk, how many needed the second tier of
 * the unpredictability (k_part's check); *n_records receives their number.  Call after
 * mp3mi_batch_sync. */
int mp3mi_batch_debug_cw_fixups(mp3mi_batch *b, int *n_listed, int *n_records);
/* likewise: the records of the last item whose loop-prep values k_mdct's tail could not decide (k_prep recomputed them) */
int mp3mi_batch_debug_prep_fixups(mp3mi_batch *b, int *n_listed);

/* Library / device identification string for logs. */
const char *mp3mi_version(void);
/* sha256 (first 16 hex digits) over the sources the library was built from (csrc/Makefile): measurements carry it, and
 * bench.py only quotes counter figures of a committed profile that was taken on the same sources. */
const char *mp3mi_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif
