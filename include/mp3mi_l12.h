/* libmp3mi -- MPEG-1 Layer I and Layer II encoding on the MI355X, C ABI.
 *
 * The batched counterpart of the Layer I / II cases of the reference's frame loop
 * (/root/reference/src/musicin.c:620-704) with psychoacoustic model 2 (-p 2, the default; src/psy.c):
 *
 *   reference call (per frame, per stream)                              here (per batch)
 *   get_audio                         src/encode.c:187-269              the caller's PCM rows, read on the device
 *   window_subband / filter_subband   src/encode.c:287-409              k_filter (shared with Layer III)
 *   I_/II_scale_factor_calc, I_/II_combine_LR, II_transmission_pattern  src/encode.c:469-691          k12_alloc
 *   psycho_anal                       src/psy.c:36-421                  k_fft12, k12_psy
 *   I_/II_main_bit_allocation         src/encode.c:782-1172             k12_alloc
 *   I_/II_CRC_calc, encode_info, encode_CRC, *_encode_bit_alloc, *_encode_scale,
 *   *_subband_quantization, *_sample_encoding, put1bit                  src/common.c:1251-1327, src/encode.c:418-437, 695-748, 1174-1430   k12_alloc
 *   close_bit_stream_w                src/common.c:968                  the file's one byte past the last frame
 *
 * The emitted bytes are bit-exact to the reference's `encode -l 1|2` on the same PCM (tests/test_gpu_l12.py,
 * tests/golden/l12_*).  Psychoacoustic model 1 (-p 1) cannot be offered: the reference as shipped cannot run it
 * (src/tonal.c:86-150 reads table files -- "2cb0", "2th0", ... -- that the repository does not contain, and exits).
 * MPEG-2 LSF rates are refused as the reference's psycho_anal refuses them (src/psy.c:131-136).  Frames are never
 * padded (src/musicin.c:566-581 drops the fraction before looking at it).
 *
 * No CPU fallback: every entry point returns MP3MI_ERR_NO_DEVICE when HIP has no device.  Error codes: mp3mi.h.
 * Threads: as for mp3mi_batch (mp3mi.h, "Threads"): one thread at a time per mp3mi_l12_batch, different batches independent.
 */
#ifndef MP3MI_L12_H
#define MP3MI_L12_H

#include "mp3mi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mp3mi_l12_batch mp3mi_l12_batch;

/* layer 1 or 2; rate_hz in {44100, 48000, 32000}; channels 1 or 2; kbps: n_streams bitrates of the layer's table
 * (src/common.c:122-123: Layer I 32..448 in steps of 32, Layer II 32 48 56 64 80 96 112 128 160 192 224 256 320 384) or
 * NULL = kbps_all for every stream.  max_frames bounds n_frames of later calls; a frame is 384 (Layer I) or 1152
 * (Layer II) samples per channel.  scratch_mb: budget of the inter-kernel buffers in MiB, 0 = 32768. */
int mp3mi_l12_batch_create(mp3mi_l12_batch **out, int layer, int n_streams, int rate_hz, int channels,
                           const int *kbps, int kbps_all, int max_frames, unsigned scratch_mb);
void mp3mi_l12_batch_destroy(mp3mi_l12_batch *b);

/* the driver's -m (MP3MI_MODE_*; joint stereo IS available for these layers: src/encode.c:882-948), -e (a computed
 * CRC-16 here, src/common.c:1251-1327), -c -o -d */
int mp3mi_l12_batch_set_mode(mp3mi_l12_batch *b, int mode);
int mp3mi_l12_batch_set_error_protection(mp3mi_l12_batch *b, int on);
int mp3mi_l12_batch_set_header(mp3mi_l12_batch *b, int copyright, int original, int emphasis);

/* bytes to reserve per stream for n_frames frames */
size_t mp3mi_l12_batch_out_stride(const mp3mi_l12_batch *b, int n_frames);

/* Encodes n_frames frames of every stream from a fresh encoder state, the file's last byte included.
 *   pcm_dev     device, int16 [n_streams][n_frames * (384 | 1152)][channels] (WAV sample order)
 *   n_samples_dev  device, [n_streams] valid samples per channel of each stream, or NULL: all.  The last partial frame
 *               is zero-filled and the stream ends after ceil(n / frame) frames (src/encode.c:123-185)
 *   out_dev     device, [n_streams][out_stride] bytes;  out_len_dev  device, [n_streams] uint32
 * Work is enqueued on the batch's stream; mp3mi_l12_batch_sync waits for it. */
int mp3mi_l12_batch_encode(mp3mi_l12_batch *b, const int16_t *pcm_dev, const int32_t *n_samples_dev, int n_frames,
                           uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev);
int mp3mi_l12_batch_sync(mp3mi_l12_batch *b);

/* Streaming, as mp3mi_batch_encode_next / _flush / _reset of mp3mi.h: the reference is a frame-streaming encoder
 * (src/musicin.c:585-705), and for these layers a stream carries nothing from frame to frame but PCM history (the
 * filterbank's taps, the FFT windows of the passes that predict the next one) -- kept in the batch.
 *   mp3mi_l12_batch_encode_next  the NEXT n_frames frames of every stream: pcm_dev holds only these frames; out_dev /
 *                                out_len_dev receive their bytes (whole frames: nothing stays behind).  The first call after
 *                                create, reset, flush or a whole-file encode starts new streams.
 *   mp3mi_l12_batch_flush        close_bit_stream_w: the file's one byte past the last frame (src/common.c:843-868); ends the streams
 *   mp3mi_l12_batch_reset        abandons the streams in progress
 * Concatenating the outputs of the calls and of the flush gives the bytes of mp3mi_l12_batch_encode over the whole stream. */
int mp3mi_l12_batch_encode_next(mp3mi_l12_batch *b, const int16_t *pcm_dev, int n_frames, uint8_t *out_dev, size_t out_stride,
                                uint32_t *out_len_dev);
int mp3mi_l12_batch_flush(mp3mi_l12_batch *b, uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev);
int mp3mi_l12_batch_reset(mp3mi_l12_batch *b);

/* Continuous batching, as mp3mi_batch_encode_slots / mp3mi_batch_slot_frames of mp3mi.h: every stream index is a SLOT through
 * which one stream after another passes, each beginning and ending in a call of its own while the other slots go on.  A frame
 * is 384 (Layer I) or 1152 (Layer II) samples per channel; full = n_frames of them.
 *   ctl_host       host, [n_streams] uint8: MP3MI_SLOT_START | MP3MI_SLOT_END (mp3mi.h)
 *     START  the slot begins a new stream at this call's first sample, from silence before it; a stream still open in the slot
 *            is abandoned
 *     END    the call holds the stream's last n_samples_host[s] samples per channel, 0 .. full: the last partial frame is
 *            zero-filled (src/encode.c:162-166), the slot delivers ceil(n / frame) frames and then the file's one byte past
 *            the last frame (close_bit_stream_w), and is closed afterwards.  START | END is a one-call file; END with 0
 *            samples (with START or on an open stream) delivers exactly that one byte
 *     0      an open stream goes on, with a full call of samples; a closed slot stays closed
 *   n_samples_host host, [n_streams] int32, or NULL: full for every open or starting slot, 0 for the others
 *   pcm_dev        device, int16 [n_streams][full][channels]; the rows of closed slots are not looked at
 *   out_dev, out_len_dev  device, [n_streams][out_stride] and [n_streams]: out_len_dev[s] is the bytes of slot s's file the call
 *                  produced -- 0 for a closed slot, whose row is left alone whatever its PCM row holds
 * The bytes a slot delivers from a stream's START call through its END call, concatenated, are byte for byte what
 * mp3mi_l12_batch_encode gives for the same samples as one stream of a ragged whole-file call (bitrate: the slot's, from create,
 * unless the stream's START chose another: mp3mi_l12_batch_encode_slots_kbps below).
 * MP3MI_ERR_ARG, with nothing enqueued and the batch unchanged: ctl bits other than the two; END on a closed slot without
 * START; a sample count that is not full for a continuing or starting slot, outside 0 .. full for an ending one, not 0 for a
 * closed one; a NULL pointer other than n_samples_host; n_frames outside 1 .. max_frames; out_stride below
 * mp3mi_l12_batch_out_stride(b, n_frames).  The two host arrays are copied before the call returns; calls may follow each
 * other without a sync in between (the work is enqueued on the batch's stream, as ever).
 *
 * Alongside the other calls: mp3mi_l12_batch_encode_next starts every slot when none is open, and otherwise continues the open
 * ones (closed slots stay closed, out_len 0); mp3mi_l12_batch_flush ends every open slot (out_len 0 for the closed ones);
 * mp3mi_l12_batch_reset and mp3mi_l12_batch_encode close every slot.  A batch that is never given a per-slot call behaves in
 * every respect as if these two functions did not exist -- mp3mi_l12_batch_flush then delivers the one byte for every stream,
 * a fresh batch's included. */
int mp3mi_l12_batch_encode_slots(mp3mi_l12_batch *b, const int16_t *pcm_dev, int n_frames, const uint8_t *ctl_host,
                                 const int32_t *n_samples_host, uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev);
/* frames_host[s] = frames encoded so far by the stream open in slot s, -1 if none is; returns the number of open slots.
 * Host-side bookkeeping only: waits for nothing. */
int mp3mi_l12_batch_slot_frames(const mp3mi_l12_batch *b, int64_t *frames_host);

/* A bitrate per stream, chosen at START -- as mp3mi_batch_encode_slots_kbps / mp3mi_batch_slot_kbps of mp3mi.h.  The call is
 * mp3mi_l12_batch_encode_slots with one more host array; kbps_host == NULL is exactly that call.
 *   kbps_host   host, [n_streams] int32, copied before the call returns
 *     a slot that STARTs      0: the bitrate the slot was created with; otherwise a bitrate of the batch's layer (the table at
 *                             mp3mi_l12_batch_create) that is not above the batch's CEILING, the largest bitrate it was created
 *                             with.  In Layer II the bitrate also selects the stream's allocation table and subband limit
 *                             (src/common.c:291-318), exactly as at create
 *     any other slot          0, or the bitrate of the stream open there: one persistent array serves call after call
 * The ceiling sizes the output rows: a frame's bytes do not decrease as the bitrate grows, so mp3mi_l12_batch_out_stride holds for
 * every bitrate a START may name.  The bitrate belongs to the STREAM: it holds until the stream is over -- by END, by
 * mp3mi_l12_batch_flush or _reset, abandoned by a new START in its slot, or by a whole-file mp3mi_l12_batch_encode -- through every
 * call that continues it (mp3mi_l12_batch_encode_next among them), and afterwards the slot is back at its create-time bitrate.  Calls
 * that start every stream afresh (mp3mi_l12_batch_encode; an encode_next with no slot open) encode at the create-time bitrates, as
 * on a batch that never saw another.  The bytes of a stream are those of mp3mi_l12_batch_encode of its samples at ITS bitrate.
 * MP3MI_ERR_ARG, nothing enqueued, the batch unchanged: the rules of mp3mi_l12_batch_encode_slots, and a kbps_host entry that breaks
 * the two above.
 *   mp3mi_l12_batch_slot_kbps   kbps_host[s] = the bitrate of the stream open in slot s, the slot's create-time bitrate where none is;
 *                               returns the ceiling.  Host-side bookkeeping only: waits for nothing. */
int mp3mi_l12_batch_encode_slots_kbps(mp3mi_l12_batch *b, const int16_t *pcm_dev, int n_frames, const uint8_t *ctl_host,
                                      const int32_t *n_samples_host, const int32_t *kbps_host, uint8_t *out_dev, size_t out_stride,
                                      uint32_t *out_len_dev);
int mp3mi_l12_batch_slot_kbps(const mp3mi_l12_batch *b, int32_t *kbps_host);

/* Parking and resuming streams -- as mp3mi_batch_slots_export / _import of mp3mi.h: an open stream leaves its slot, sits out any
 * number of calls, and goes on later in any closed slot of this batch or of another batch of the same format, on this GPU or
 * another; or a snapshot of it is taken while it goes on.  The bytes the stream delivers from START through END, concatenated
 * over every slot and batch it lived in, are its file, as if it had never moved.
 *   A parked stream is a TICKET, host memory, and a STATE RECORD, device memory.
 *   mp3mi_l12_slot_ticket       plain data, may be stored and sent anywhere
 *     magic, version            MP3MI_L12_SLOT_TICKET_MAGIC, MP3MI_L12_SLOT_TICKET_VERSION (the layout of ticket and record)
 *     state_bytes               mp3mi_l12_batch_slot_state_bytes of the batch that exported it
 *     layer, rate_hz, channels  the format of that batch, and what mp3mi_l12_batch_set_mode, _set_header (copyright << 3 |
 *     hdr_mode, hdr_flags,      original << 2 | emphasis) and _set_error_protection had been given when it was exported
 *     error_protection
 *     kbps                      the stream's bitrate
 *     reserved                  0
 *     frames                    frames the stream has encoded
 *   the state record            all a stream of these layers carries from call to call: its PCM history, the row of the FFT
 *                               windows' ([1792][channels] int16) and behind it the row of the filterbank's ([1056][channels]
 *                               int16) -- channels * 5696 bytes, a multiple of 16 that depends on the channel count alone
 *                               (mp3mi_l12_batch_slot_state_bytes).  No reservoir, no carried bytes, no status word.  The
 *                               bitrate travels in the ticket alone: nothing in a record is ever used as an index, so a damaged
 *                               record gives wrong audio and nothing worse
 *   mp3mi_l12_batch_slots_export  slots_host: n DISTINCT slots, 1 .. n_streams of them, each with a stream open.  Record i goes to
 *                               (char *) state_dev + i * state_stride, ticket i to tickets_host[i].  state_stride >=
 *                               state_bytes; it and state_dev multiples of 16.  close != 0: the slots are closed WITHOUT a
 *                               flush -- nothing is delivered, the file's last byte included; slot_frames gives -1 and slot_kbps
 *                               the create-time bitrate there.  close == 0: a snapshot; the streams go on, and the record may be
 *                               imported any number of times
 *   mp3mi_l12_batch_slots_import  slots_host: n distinct CLOSED slots.  Every ticket must match the library and the batch in every
 *                               field: magic, version, state_bytes; layer, rate, channels; mode, header flags, error protection
 *                               as the batch has them NOW; reserved 0; kbps a bitrate of the layer not above the batch's ceiling;
 *                               frames >= 0.  Afterwards slot i is open at the ticket's frame count and bitrate, whatever the
 *                               slot was created with: the next per-slot call continues the stream with ctl 0, and so does
 *                               mp3mi_l12_batch_encode_next.  Works as the first call on a fresh batch, after a flush or a reset
 * Both return MP3MI_ERR_ARG, with nothing enqueued and the batch unchanged, where a rule is broken.  Neither waits for the device:
 * the copies run on the batch's stream, behind every call before and ahead of every call after, so a record may be imported into
 * the batch that exported it at once; any other reader or writer of the record (another batch, a copy to the host) calls
 * mp3mi_l12_batch_sync on the exporting batch first.  Until a batch's first bitrate array, export or import nothing of this exists:
 * it allocates, copies and launches exactly what it did without. */
#define MP3MI_L12_SLOT_TICKET_MAGIC 0x4B54324Du /* "M2TK" */
#define MP3MI_L12_SLOT_TICKET_VERSION 1u
typedef struct mp3mi_l12_slot_ticket {
    uint32_t magic, version;
    uint64_t state_bytes;
    int32_t layer, rate_hz, channels, hdr_mode;
    int32_t hdr_flags, error_protection, kbps, reserved;
    int64_t frames;
} mp3mi_l12_slot_ticket; /* 56 bytes, no padding */
size_t mp3mi_l12_batch_slot_state_bytes(const mp3mi_l12_batch *b);
int mp3mi_l12_batch_slots_export(mp3mi_l12_batch *b, int n, const int32_t *slots_host, int close, void *state_dev, size_t state_stride,
                                 mp3mi_l12_slot_ticket *tickets_host);
int mp3mi_l12_batch_slots_import(mp3mi_l12_batch *b, int n, const int32_t *slots_host, const void *state_dev, size_t state_stride,
                                 const mp3mi_l12_slot_ticket *tickets_host);

/* The feeder: any number of samples per call.  A per-slot call wants a full call of samples from every open slot; real streams
 * arrive in packets of 160 or 960 samples, in bursts, in whatever a decoder upstream hands over.  A feeder has n_lanes LANES in front
 * of the batch's n_streams slots, in any relation (fewer, as many, more).  A lane keeps a FIFO of samples ON THE DEVICE; the rows of
 * every tick are cut there (k12_feed, csrc/k_format.hip); a slot is lent to a lane for the ticks in which it encodes.  It touches no
 * encoding kernel: a tick ends in one mp3mi_l12_batch_encode_slots_kbps call on rows the feeder owns.  A frame is 384 (Layer I) or
 * 1152 (Layer II) samples per channel; a TICK is tick_frames of them.
 *   mp3mi_l12_feed_create    a feeder for batch b -- on which no stream is open, and which has no feeder yet -- that encodes tick_frames
 *                        frames (1 .. the batch's max_frames) per encoding lane and tick and takes up to max_push (>= 1) samples per
 *                        lane and call.  n_lanes >= 1; max_rows in 1 .. n_lanes: the most lanes that may push in one tick (it sizes
 *                        the upload blocks); ring_samples: the pending samples per channel a lane's FIFO holds, at least tick_frames *
 *                        frame + max_push, 0: exactly that.  A lane that is ready but waits for a slot keeps taking pushes until its
 *                        FIFO is full, so a server sizes it for the wait it accepts.
 *   mp3mi_l12_feed_capacity  the pending samples per channel a lane's FIFO holds (ring_samples, or the least).  A lane's ring on the
 *                        device is 1792 samples per channel longer: the samples a stream has encoded last stay there, and they are all
 *                        a stream of these layers carries from call to call -- so a stream that sits out a tick leaves its slot
 *                        without a copy, and comes back to any slot by one copy out of its own ring.
 *   mp3mi_l12_feed_n_lanes   the lanes; mp3mi_l12_feed_lanes takes arrays of that many entries.
 *   mp3mi_l12_feed_tick      the pushes come as ROWS: row r is lane row_lane_host[r] (strictly increasing, each in 0 .. n_lanes-1;
 *                        n_rows in 0 .. max_rows), its samples row r of pcm_dev, device, int16 [n_rows][pcm_pitch][channels] in WAV
 *                        order, pcm_pitch >= max_push: the lane brings the row's first n_push_host[r] samples per channel (0 ..
 *                        max_push).  ctl_host, n_push_host and kbps_host are HOST arrays indexed by row.  A lane that no row names
 *                        pushes nothing and has ctl 0; it may encode all the same (it drains, or gets a slot at last).  With n_rows
 *                        == 0 the four row arrays and pcm_dev may be NULL; with n_rows > 0 none of them may.  All host arrays are
 *                        copied before the call returns.
 *     ctl_host[r]   MP3MI_SLOT_START: a new stream begins in the lane with this call's first pushed sample, at kbps_host[r]: 0, or a
 *                   bitrate of the batch's layer that is not above the batch's ceiling (the rules of
 *                   mp3mi_l12_batch_encode_slots_kbps, checked here).  A stream open in the lane is abandoned with its pending
 *                   samples, as mp3mi_l12_batch_encode_slots abandons one.  The batch sees the START in the first tick in which the
 *                   lane encodes.
 *                   MP3MI_SLOT_END: this call's samples are the stream's last.  From here the lane DRAINS: tick_frames frames per
 *                   tick in which it encodes while more than tick_frames * frame samples are pending; in the first with that many or
 *                   fewer (0 too) the batch gets its END with exactly that count, and the lane closes.  START | END with few samples
 *                   is a one-call file.
 *     kbps_host[r]  of a row without START: 0, or the bitrate of the stream open in the lane once that is known (below).
 *     Ready.  A lane is READY when its pending samples and the pushed ones make a tick, or when it is ending (draining, with a tick or
 *     less pending).  A lane that is not ready delivers nothing; its samples stay pending, nothing of it is lost, and a stream it
 *     holds in the batch leaves its slot (it is parked) until the lane encodes again.
 *     Who encodes.  If no more than n_streams lanes are ready, all encode.  Otherwise the n_streams lanes encode whose current
 *     unbroken spell of being ready began in the earliest tick, ties going to the lower lane; a lane that encodes and is still ready
 *     begins a new spell in the next tick.  So no ready lane encodes twice while another that was ready before it has not encoded
 *     once.  A ready lane that gets no slot keeps its samples, delivers nothing, is parked if its stream is in a slot, and shows bit
 *     3 in mp3mi_l12_feed_lanes' flags until the tick in which it encodes.
 *     Where.  A chosen lane whose stream is in a slot keeps the slot.  Every other stream in a slot leaves it.  The other chosen
 *     lanes take the free slots -- those vacated in this very tick among them --, the lowest free slot going to the lowest lane: a
 *     parked stream is resumed there, a stream the batch has not seen STARTs there.  A START at kbps 0 means the create-time bitrate
 *     of the slot in which the stream first encodes; until then only kbps 0 may be passed with the lane's pushes.
 *     Output is by SLOT, as mp3mi_l12_batch_encode_slots writes it: out_dev [n_streams][out_stride], out_stride >=
 *     mp3mi_l12_batch_out_stride(b, tick_frames), and out_len_dev [n_streams].  slot_lane_host [n_streams] is filled before the call
 *     returns (host bookkeeping, no device wait): entry i is the lane that encodes in slot i in this tick, or -1, and out_len_dev[i]
 *     is 0 where it is -1.  A tick in which nothing encodes launches no encoding kernel and zeroes out_len_dev in stream order.
 *     The bytes a LANE delivers from a stream's START through the tick that closes it, gathered slot by slot through slot_lane_host
 *     and concatenated, are byte for byte what mp3mi_l12_batch_encode gives for the stream's samples as one stream of a ragged
 *     whole-file call at its bitrate -- however the samples were cut into pushes, however often the stream sat out a tick, and in
 *     whichever slots it encoded.
 *     MP3MI_ERR_ARG, with nothing enqueued and feeder and batch unchanged -- the check runs over all rows first --: n_rows outside
 *     0 .. max_rows; a row map out of order or out of range; a NULL row array or pcm_dev with n_rows > 0; a NULL out_dev,
 *     out_len_dev or slot_lane_host; unknown ctl bits; a push or an END on a closed lane without START; START, END or a push on a
 *     draining lane; n_push outside 0 .. max_push; pending + push above mp3mi_l12_feed_capacity (a waiting lane whose FIFO is full);
 *     pcm_pitch < max_push; out_stride too small; a kbps that breaks the rules above.
 *     The call waits for nothing but the fence of its own upload block (the tick four before, as a rule long through) and what the
 *     per-slot call itself waits for (its control block, two turns before): ticks may be issued back to back.
 *   mp3mi_l12_feed_lanes     host bookkeeping only, no wait: per lane the pending samples, the frames encoded so far (-1: closed) and
 *                        flags -- bit 0 parked, bit 1 draining, bit 2 started but not yet in the batch, bit 3 ready and waiting for
 *                        a slot.  Returns the number of lanes that are not closed.
 *   mp3mi_l12_feed_destroy   resets the batch (streams in lanes are abandoned) and detaches; mp3mi_l12_batch_destroy on a batch with
 *                        a feeder attached frees the feeder with it (do not destroy it afterwards).
 * While a feeder is attached the batch's streams are the feeder's: mp3mi_l12_batch_encode, _encode_next, _encode_slots(_kbps), _flush,
 * _reset, _slots_export, _slots_import, _set_mode, _set_error_protection and _set_header return MP3MI_ERR_ARG; mp3mi_l12_batch_sync,
 * _slot_frames, _slot_kbps and the timing accessors work as ever (a parked lane's slot reads as closed).  A batch that never gets a
 * feeder allocates, copies and launches exactly what it did without.  Not here: ticks on host buffers, a status query per lane. */
typedef struct mp3mi_l12_feed mp3mi_l12_feed;
int mp3mi_l12_feed_create(mp3mi_l12_feed **out, mp3mi_l12_batch *b, int n_lanes, int max_rows, int tick_frames, int max_push,
                          int ring_samples);
void mp3mi_l12_feed_destroy(mp3mi_l12_feed *f);
size_t mp3mi_l12_feed_capacity(const mp3mi_l12_feed *f);
int mp3mi_l12_feed_n_lanes(const mp3mi_l12_feed *f);
int mp3mi_l12_feed_tick(mp3mi_l12_feed *f, int n_rows, const int32_t *row_lane_host, const int16_t *pcm_dev, size_t pcm_pitch,
                        const uint8_t *ctl_host, const int32_t *n_push_host, const int32_t *kbps_host, uint8_t *out_dev, size_t out_stride,
                        uint32_t *out_len_dev, int32_t *slot_lane_host);
int mp3mi_l12_feed_lanes(const mp3mi_l12_feed *f, int32_t *pending_host, int64_t *frames_host, uint8_t *flags_host);

/* Self-test hook: k12_feed alone, as mp3mi_l12_feed_tick launches it (csrc/format_debug.cpp), on n_lanes rings [ring_pitch][channels]
 * of `cap` samples, n_push_rows push rows [push_pitch][channels], n_slots dense rows [row_pitch][channels] of row_samples samples and
 * the slots' two history rows, hist [n_slots][1792][channels] and fb_hist [n_slots][1056][channels]; pitches in samples per channel,
 * those of rings and rows multiples of 16 bytes.  desc: n_active descriptors of eight uint32 {head, pending, n_push, take, lane,
 * push_row, slot, resume}, resume 0 or 0x80000000 | n_hist.  The first `take` samples of ring[head .. head + pending) ++ push[0 ..
 * n_push) go to row `slot`; all n_push samples are appended to the ring at (head + pending) % cap; a resuming descriptor also writes
 * the slot's history rows: the n_hist samples before head with zeros in front, and the last 1056 of the same.  The arrays go up and
 * come back whole.  MP3MI_ERR_ARG, and nothing is launched, where a descriptor breaks a rule the tick keeps: head < cap; 1792 +
 * pending + n_push <= cap; take <= pending + n_push and <= row_samples; n_push <= push_pitch; lane, push_row and slot inside their
 * arrays; n_hist <= 1792 and no other bit in word 7; no lane twice, no push row of a pushing descriptor twice, no slot of a taking or
 * resuming descriptor twice. */
int mp3mi_debug_l12_feed(int channels, int n_active, int n_lanes, int n_push_rows, int n_slots, int cap, int row_samples,
                         const uint32_t *desc, int16_t *ring, size_t ring_pitch, int16_t *push, size_t push_pitch, int16_t *rows,
                         size_t row_pitch, int16_t *hist, int16_t *fb_hist);

/* Two-tier decisions (mp3mi.h, MP3MI_TEST_PHASE_EXACT | _PSY_EXACT | _CW_EXACT): force the exact tier; bytes must not change */
int mp3mi_l12_batch_set_test_flags(mp3mi_l12_batch *b, unsigned flags);

/* Stage seams of the LAST chunk of the last call for tests (oracle/stage_dump_l12.h): enable before encoding, then
 * fetch [n_streams][frames of that chunk] records of mp3mi_l12_frame_seams; returns bytes written or a negative error;
 * *first_frame receives the chunk's first frame. */
typedef struct mp3mi_l12_frame_seams {
    double ltmin[2][32];
    int32_t scalar[2][3][32], j_scale[3][32], scfsi[2][32], bit_alloc[2][32];
    int32_t mode, mode_ext, jsbound, sblimit, adb_left, crc, pad[2];
} mp3mi_l12_frame_seams;
void mp3mi_l12_batch_debug_enable(mp3mi_l12_batch *b, int on);
long mp3mi_l12_batch_debug_fetch(mp3mi_l12_batch *b, void *host_dst, size_t cap, int *first_frame, int *n_chunk_frames);

/* Self-test hook: k12_alloc alone, as the batch launches it (csrc/l12_alloc_debug.cpp; k_l12.hip is the product's), on n_streams x
 * n_frames frames of GIVEN subband samples sb[n_streams][n_frames][channels][parts][12][32] (parts 1 / 3: sb_sample of
 * src/musicin.c:622-626, 662-666, before k_filter's sign change, which the hook applies) and signal-to-mask ratios
 * ratio[n_streams][n_frames][passes][channels][32] (passes = layer: Layer II keeps the larger of its two).  One format per call --
 * layer, rate_hz, channels, mode (MP3MI_MODE_*), crc, hdr_flags (bit 3 copyright, bit 2 original, bits 1-0 emphasis) -- and a
 * bitrate per stream.  slot0 (0..17) is the phase of the first frame's first slot in k_filter's 18-slot granules.
 * Out: per stream the frames' bytes one behind the other and the file's last byte, out_len[n_streams], and
 * seams[n_streams][n_frames] records of mp3mi_l12_frame_seams.  MP3MI_ERR_ARG, and nothing is launched, outside the domain
 * k12_alloc takes on trust (derived in csrc/l12_alloc_debug.cpp): a sample that is not finite or above 2.0 in magnitude, a ratio
 * that is not finite, a format the batch would refuse, more than 4096 streams or 64 frames, out_stride below
 * n_frames * (the longest frame's bytes; 38 at least for two-channel Layer I) + 1.  MP3MI_ERR_NO_DEVICE without a GPU. */
int mp3mi_debug_l12_alloc(int layer, int rate_hz, int channels, int mode, int crc, int hdr_flags, int slot0, int n_streams,
                          int n_frames, const int32_t *kbps, const double *sb, const float *ratio, uint8_t *out, size_t out_stride,
                          uint32_t *out_len, void *seams);

/* milliseconds inside the kernels of all encode calls since create (HIP events on the batch's stream), and the calls */
int mp3mi_l12_batch_total_timing(mp3mi_l12_batch *b, double *all_kernels_ms, long *calls);
/* the same per kernel, HIP events around every launch: [0] k_fft12, [1] k12_psy, [2] k_filter,
 * [3] k12_alloc -- milliseconds and launches since create */
int mp3mi_l12_batch_kernel_timing(mp3mi_l12_batch *b, double ms[4], long launches[4]);

/* Host-buffer convenience wrapper (tests, smoke): pcm [n_streams][n_frames * frame * channels], n_samples may be NULL;
 * mode MP3MI_MODE_* or -1 = by the channel count. */
int mp3mi_l12_encode_host(int layer, int n_streams, int rate_hz, int channels, const int *kbps, int kbps_all, int mode,
                          int error_protection, const int16_t *pcm, const int32_t *n_samples, int n_frames,
                          uint8_t *out, size_t out_stride, uint32_t *out_len);

#ifdef __cplusplus
}
#endif
#endif
