// Host side of the batched encoder: owns the device buffers, cuts the frames of a call into
// chunks that fit the scratch budget, and enqueues the kernels of every chunk on TWO HIP streams:
//
//   front stream (low priority):  k_fft | k_cw k_part k_psy k_filter k_mdct (k_prep: the records k_mdct lists)   of chunk c+1
//   loop  stream (high priority): k_loop k_format                                   of chunk c
//
// k_loop keeps one wavefront per stream resident for a whole chunk (four per SIMD) and leaves room for
// one more wavefront per SIMD: the feed-forward kernels of the next chunk run there, behind a gate that
// lets k_loop become resident first -- all but the FFTs, which take a whole CU's LDS per workgroup and run
// between two k_loop launches.  The three buffers that cross from the front stream to the loop stream
// (psy, xr, prep) are double-buffered; events order producer/consumer.  Calls overlap the same way.
//
//   k_fft     (stream, granule, channel)  psy FFTs                 feed-forward
//   k_psy     (stream, channel)           thresholds / block type  serial over granules
//   k_fbmdct  (stream, channel, granules) filterbank + MDCT        feed-forward, needs block type
//   k_loop    (stream)                    iteration loop           serial over frames
//   k_format  (stream, frame)             bitstream formatting     independent per frame
//
// Mirrors the Layer III case of the reference's frame loop (src/musicin.c:708-788) for every
// stream at once.  No CPU fallback: every entry point returns an error when HIP cannot run.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "host_util.h"
#include "mp3mi.h"

size_t mp3mi_psy_state_size(void);

// What a stream carries from call to call: one record per slot in each of these regions.  mp3mi_batch::carried is the ONE list
// of them (carried_init, once the buffers exist), in the order of a parked stream's state record -- that order is part of the
// slot-state format (park_tables).  Whoever clears, starts, parks or resumes streams walks it.
//   loop: the HIP stream that owns the region, the only one it is read or written on (encode_impl): the psy state and the PCM
//         history belong to the front stream, whose feed-forward kernels do not wait for the loop stream; everything k_loop,
//         k_format and k_stream_tail carry belongs to the loop stream
//   zero: a fresh stream needs its record zeroed (what the reference's function statics and the caller's buffers hold when its
//         main() starts).  Not carry's contents -- carry_len says how much of them counts -- and not the live bitrate words:
//         rates_restore and k_slot_rate see to those
struct carried_region {
    void *base;
    size_t bytes; // per slot
    bool loop, zero;
};
enum { N_CARRIED = 8 };

// The control block of a per-slot call:
//   fabs int64[S] | n_samples int32[S] | START list int32[S] | ctl uint8[S] | row map int32[S] (host-buffer calls, n_rows used) |
//   by position in the START list: bits per frame int32[S] | bitrate index int32[S] (k_slot_rate)
// The offsets are computed once (batch_build); at() gives the typed pointers of a block from its base -- of the staging copy and
// of the device copy alike.
struct ctl_block {
    int64_t *fabs;       // [S] index of the call's first frame in the stream of each slot
    int32_t *n_samples;  // [S] valid samples per channel of each slot in the call
    int32_t *list;       // [n_start] the slots that START
    uint8_t *ctl;        // [S] MP3MI_SLOT_DEV_* bits
    int32_t *rows;       // [n_rows] row_slot of a host-buffer call with a row map
    int32_t *rate_bits, *rate_index; // [n_start] of the streams that START, by position in `list`
};
struct ctl_layout {
    size_t n_samples, list, ctl, rows, rate_bits, rate_index; // byte offsets (fabs: 0)
    size_t base_bytes; // the block without the bitrates: all that goes up while no call writes the live bitrate arrays
    size_t bytes;      // the whole block
    void init(size_t S)
    {
        n_samples = 8 * S; list = n_samples + 4 * S; ctl = list + 4 * S;
        rows = (ctl + S + 3) & ~(size_t) 3;
        rate_bits = rows + 4 * S; rate_index = rate_bits + 4 * S;
        base_bytes = (rate_bits + 255) & ~(size_t) 255;
        bytes = (rate_index + 4 * S + 255) & ~(size_t) 255;
    }
    ctl_block at(uint8_t *p) const
    {
        return {(int64_t *) p, (int32_t *) (p + n_samples), (int32_t *) (p + list), p + ctl, (int32_t *) (p + rows), (int32_t *) (p + rate_bits),
                (int32_t *) (p + rate_index)};
    }
};

// The batch, in this order: what it was created as; the two HIP streams and the fences between them and between calls; the
// per-chunk scratch; what a stream carries (carried); the two stream-position bookkeepings; the two upload rings (control block,
// park list); host-buffer calls; timing.  Ownership: every device and pinned buffer is allocated through dev_alloc / pinned_alloc,
// which note it in `owned`, and mp3mi_batch_destroy frees what was noted -- a new buffer needs no line there.  (One exception,
// host_io::io_slot::out_rows, which is freed and reallocated as calls grow: by hand.)  Events are destroyed by name.
struct mp3mi_batch {
    int device;              // the HIP device everything of this batch lives on (current at create time)
    int n_streams, rate_idx, rate_hz, channels, max_frames, chunk_frames;
    std::vector<int> bits_per_frame_h, bitrate_index_h, kbps_h; // as created, per stream index
    int max_frame_bytes, ceil_kbps; // of the largest bitrate the batch was created with: what the output rows are sized for
    struct owned_buf { void *p; bool pinned; };
    std::vector<owned_buf> owned; // every buffer of dev_alloc / pinned_alloc, in the order of allocation
    hipStream_t stream;      // front stream: feed-forward kernels (and the initial memsets)
    hipStream_t lstream;     // loop stream: k_loop + k_format
    // A batch of more streams than k_loop holds resident is cut into PARTS (contiguous stream ranges); a part's frames of
    // one chunk are an "item", and the items go through the two HIP streams one after the other (encode_impl).
    // Per (double-buffer slot, part), index slot * n_parts + part:
    std::vector<hipEvent_t> ev_front; // the item's front kernels are done
    std::vector<fence> ev_loop;       // its k_loop is done (the slot's region of this part may be overwritten): the region's last reader is a k_loop that may still run
    int n_parts, part_streams;
    fence ev_done;           // everything of the previous encode call is done
    hipEvent_t ev_hist;      // the front stream's last work of a call (the PCM history hand-over) is enqueued
    // The last k_loop of a call is HELD on the device (k_hold, k_loop.hip) until the next call's first transforms are through:
    // hold_flag is one word of host memory mapped into the device's address space, hold_seq the ticket of the hold in
    // force (tickets only grow), held = a hold is in force that neither a next call nor the host has let go yet
    unsigned *hold_flag_h, *hold_flag_d;
    unsigned hold_seq;
    bool held, hold_calls;
    int slot_base;           // parity of the double-buffer slot the next call's chunk 0 takes
    unsigned *gate_count;    // start census of k_loop's wavefronts (device memory, only ever grows)
    unsigned gate_total;     // census value once every wavefront launched so far has started
    unsigned gate_first;     // ... the same (kept for the gate's target: the census once the LAST launch is resident)
    int *place_order, *place_cost; // k_loop stream placement (mp3mi_loop_place), NULL = off
    unsigned *place_zero;    // taken[n] + simd_slots + simd_idx + ticket + scan, zeroed before every k_loop
    int n_simd;
    unsigned *voided;        // device counter: streams whose file a call voided (the reference dies on them), since the last sync
    int32_t *status_dev;     // [S]: what mp3mi_batch_stream_status copies out; between a flush and the next encode / reset it HOLDS the ended streams' status
    bool status_kept;        // status_dev holds the status of the streams the last flush ended (their state is reset)
    int prep_exact;          // MP3MI_TEST_PREP_EXACT: k_prep over every record, its second tier only, instead of k_mdct's tail (tests)
    int test_flags;          // mp3mi_geom::test_flags
    int hdr_flags;           // copyright << 3 | original << 2 | emphasis (src/l3bitstream.c:330-334)
    int hdr_mode;            // header mode field: 0 stereo, 2 dual channel, 3 mono (src/common.h:233-236)
    int crc;                 // error protection (-e): zero CRC word after the header, as the reference writes it
    int last_slot;
    mp3mi_tables *T;
    // The LIVE bitrate arrays, [S] each, which k_loop, k_format and k_stream_tail read per stream (one allocation, rate_live: bits
    // per frame | bitrate index), and the create-time values beside them (rate_create, same layout).  A per-slot call may START a
    // stream at another bitrate (mp3mi_batch_encode_slots_kbps): k_slot_rate writes the live arrays, rates_restore copies the
    // create-time ones back.  Both run on the LOOP stream only, and the host never writes the live arrays after create: every
    // reader runs on the loop stream, so a write is in order behind the readers of the call before (a held k_loop among them) and
    // ahead of the readers of the call that issued it.
    int32_t *rate_live, *rate_create;
    int32_t *bits_per_frame, *bitrate_index; // rate_live, rate_live + S
    std::vector<int32_t> slot_kbps_h;  // the bitrate of the stream open in each slot; of a closed slot: kbps_h
    bool rate_dirty;                   // the live arrays may differ from the create-time ones
    float *energy_l, *energy_s, *hist6, *fft_bins;
    double *cw_mid, *xr[2], *sbs, *sb_dbg, *part_eb;
    mp3mi_cw_fixlist *cw_fix; // the (granule, channel) records whose unpredictability needs its second tier (k_part)
    float *part_cb;
    mp3mi_psy_out *psy[2];
    mp3mi_loop_prep *prep[2];
    mp3mi_prep_fixlist *prep_fix; // the records k_mdct's tail could not decide (k_prep works through the list); front stream only
    int16_t *ix;
    mp3mi_frame_side *side;
    // what a stream carries from call to call (whole-file calls clear it, streaming calls continue from it): `carried` lists it all
    void *psy_state, *loop_state;
    int16_t *pcm_hist;       // [S][MP3MI_PCM_HIST][C]: the samples before the next call's first
    int64_t *out_base;       // [S]: file bytes delivered so far
    uint8_t *carry;          // [S][MP3MI_CARRY_BYTES]: file bytes formatted but not final yet
    int32_t *carry_len;      // [S]
    carried_region carried[N_CARRIED];
    // streaming: where the streams are -- the whole-batch counter of encode_next / flush (book.frames_all: frames of every stream
    // encoded since the last reset) and the slots of mp3mi_batch_encode_slots (host_util.h)
    slot_book book;
    bool fresh;              // reset since the last encode (or never encoded): state buffers are zero
    int debug, last_nf;
    // the control block of a per-slot call (ctl_layout), twice, taken in turn by the per-slot calls: an entry's fence is recorded
    // behind the last reader of its device copy, and the host waits for it before it writes the staging again (the per-slot call
    // two before: ctl_take)
    ctl_layout ctl_at;
    typedef upload_ring<uint8_t, 2> ctl_ring;
    ctl_ring ctl;
    hipEvent_t ev_ctl_up;    // the front stream has uploaded the block (or the park list) of the call
    // parking (mp3mi_batch_slots_export / _import): the slot list of such a call -- int32[S] --, a ring of four by call, apart from
    // the control block's two so that a tick, a park and a resume issued in a row do not wait for each other; an entry's fence is
    // recorded behind the last reader of its device copy, and the host waits for it before it writes the staging again (the park
    // call four before).  Each entry is created with its first turn: a batch that never parks holds none of it.
    typedef upload_ring<int32_t, 4> park_ring;
    park_ring park;
    // Host-buffer calls (mp3mi_batch_encode_host_async): the call's PCM goes up and its file bytes come down chunk by
    // chunk on two copy streams of their own, beside the kernels; two calls may be in flight, so the device copies of
    // PCM and output exist twice (slot = call number & 1).  Created with the first such call.
    struct host_io {
        bool ready;
        hipStream_t h2d, d2h;
        size_t out_stride;
        struct io_slot {
            int16_t *pcm;             // [S][max_frames * 1152][C]
            uint8_t *out;             // [S][out_stride]
            uint32_t *len;            // [S]
            fence pcm_free, out_free; // the slot's PCM has been read by its last kernel / its output by its last copy
            std::vector<hipEvent_t> ev_fmt;     // per chunk: the chunk's formatter is done
            std::vector<hipEvent_t> t_up, t_dn; // per chunk two events around the copy (the second is what consumers wait for)
            // per-slot calls on host buffers with a row map (mp3mi_batch_encode_slots_host_async): the caller's rows are DENSE, one
            // per live slot; they cross PCIe as they are, into and out of dense device buffers, and k_rows_in / k_rows_out
            // (k_format.hip) move them to and from the rows per slot above.  Created with the first such call of a slot.
            int16_t *pcm_rows;        // [n_rows][max_frames * 1152][C]
            uint8_t *out_rows;        // [n_rows][the caller's out_stride]; NOT in mp3mi_batch::owned: host_rows_init regrows it
            size_t out_rows_cap;      // bytes
            uint32_t *len_rows;       // [n_rows]
            std::vector<hipEvent_t> ev_in; // per chunk: the chunk's columns are in the slot rows (k_rows_in, on the upload stream)
            unsigned hold_of;         // the ticket of the call hold the slot's call left in force (0: none)
            int n_chunks;
            double bytes_up, bytes_dn;
            bool pending;
        } slot[2];
        unsigned call_no;
        double tot_up_bytes, tot_dn_bytes, tot_up_ms, tot_dn_ms;
        long tot_calls;
    } hio;
    // HIP-event timing of the calls: two sets taken in turn, so that a call can be issued while the one before still
    // runs; a set is read out (harvested) when its turn comes again -- which also keeps the host at most two calls
    // ahead of the device -- or when the timing is asked for
    struct timing_set {
        hipEvent_t ev0, ev1;
        std::vector<hipEvent_t> loop_ev;
        int launches; // bracketed spans (one per chunk)
        int kernels;  // k_loop launches inside them
        bool pending;
    } ts[2];
    unsigned call_no;
    float last_loop_ms, last_all_ms;
    int last_launches;
    double tot_loop_ms, tot_all_ms;
    long tot_launches, tot_calls;
    // a feeder in front of the batch (feed.h, mp3mi_feed_create): while one is attached, the calls that start, move or end streams
    // and the header settings are the feeder's alone (feed_locked); feed_call: the feeder is making such a call
    struct mp3mi_feed *feed;
    bool feed_call;
    bool feed_host_call; // ... for a tick on host buffers, whose samples are still crossing PCIe: neither joined nor held (encode_impl)
};
static void feed_drop(struct mp3mi_feed *f); // (feed.h, at the end of this file)
static hipError_t feed_host_sync(struct mp3mi_feed *f); // (the feeder's own copy streams, where it has made ticks on host buffers)
static inline bool feed_locked(const mp3mi_batch *b) { return b && b->feed && !b->feed_call; }

// Device and pinned buffers of a batch: allocated here and nowhere else, so that mp3mi_batch_destroy knows them all
template <typename T> static hipError_t dev_alloc(mp3mi_batch *b, T **p, size_t bytes)
{
    const hipError_t e = hipMalloc((void **) p, bytes);
    if (e == hipSuccess) b->owned.push_back({*p, false});
    return e;
}
template <typename T> static hipError_t pinned_alloc(mp3mi_batch *b, T **p, size_t bytes, unsigned flags)
{
    const hipError_t e = hipHostMalloc((void **) p, bytes, flags);
    if (e == hipSuccess) b->owned.push_back({*p, true});
    return e;
}
// A ring entry: staging, device copy, fence -- in this order
template <typename E> static hipError_t ring_entry_create(mp3mi_batch *b, E &en, size_t bytes)
{
    hipError_t e = pinned_alloc(b, &en.stage, bytes, 0);
    if (e == hipSuccess) e = dev_alloc(b, &en.dev, bytes);
    if (e == hipSuccess) e = en.free.create();
    return e;
}

// What a bitrate means for a stream of sampling-frequency code ri: its index in the header and the frame's size, slots per frame
// never padded (src/musicin.c:562-581).  False for anything but an MPEG-1 Layer III bitrate (src/common.c:118-125, 460-481) --
// the check of mp3mi_batch_create_ex and of a per-slot call's kbps_host alike.
static bool rate_of_kbps(int ri, int k, int *bitrate_index, int *bits_per_frame)
{
    const int bi = bitrate_index_of(3, k);
    if (!bi || ri < 0 || ri > 2) return false;
    *bitrate_index = bi;
    *bits_per_frame = frame_bits(1152, ri, k, 8);
    return true;
}

#if !defined(MP3MI_SOURCE_HASH)
#define MP3MI_SOURCE_HASH "unknown"
#endif
extern "C" const char *mp3mi_source_hash(void) { return MP3MI_SOURCE_HASH; }

extern "C" const char *mp3mi_version(void)
{
#if defined(MP3MI_EMU)
    return "libmp3mi 0.1 (TEST BUILD: wave emulator, not the product)";
#else
    return "libmp3mi 0.1 (gfx950 HIP)";
#endif
}

static_assert(offsetof(mp3mi_loop_prep, peak) == MP3MI_LOOP_PREP_HEAD, "mp3mi_batch_debug_fetch hands out the head of a prep record");
static_assert((int) MP3MI_STREAM_ABORT_GLOBAL_GAIN == MP3MI_DEV_ABORT_GLOBAL_GAIN && (int) MP3MI_STREAM_ABORT_HUFF_BITS == MP3MI_DEV_ABORT_HUFF_BITS &&
                  (int) MP3MI_STREAM_ABORT_FLUSH_SLOT == MP3MI_DEV_ABORT_FLUSH_SLOT,
              "status codes of mp3mi.h and mp3mi_dev.h");

extern "C" void mp3mi_batch_destroy(mp3mi_batch *b);

// The host lets the held k_loop of the last call go (mp3mi_batch::held): whoever is about to WAIT for that call's results,
// or to put work on the front stream that waits for it, calls this first.
static void hold_release(mp3mi_batch *b)
{
    if (!b->held) return;
    // (this hold, not the ones before it: k_hold reads the word of ITS ticket -- a ring of eight, so that a release the device
    // has not looked at yet is not overwritten by the next one: the host runs ahead of the device through chains of calls
    // that never wait, e.g. encode_next / flush / encode_next / flush)
    __atomic_store_n(b->hold_flag_h + 1 + (b->hold_seq & 7u), b->hold_seq, __ATOMIC_RELEASE);
    b->held = false;
}

extern "C" void mp3mi_batch_options_default(mp3mi_batch_options *o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->struct_size = (uint32_t) sizeof(*o);
    o->abi = MP3MI_OPTIONS_ABI;
    o->dropin_lookahead = o->call_hold = -1;
}

// The one place the library reads its environment (mp3mi.h): the knobs of tools/ and tests/.
extern "C" void mp3mi_batch_options_from_env(mp3mi_batch_options *o)
{
    if (!o) return;
    mp3mi_batch_options_default(o);
    const char *e;
    auto on = [](const char *v) { return v && atoi(v) != 0; };
    if ((e = getenv("MP3MI_SCRATCH_MB")) && atol(e) > 0) o->scratch_mb = (uint32_t) atol(e);
    if ((e = getenv("MP3MI_CHUNK_FRAMES")) && atol(e) > 0) o->chunk_frames = (int32_t) atol(e);
    if (on(getenv("MP3MI_NOISE_EXACT"))) o->test_flags |= MP3MI_TEST_NOISE_EXACT;
    if (on(getenv("MP3MI_PHASE_EXACT"))) o->test_flags |= MP3MI_TEST_PHASE_EXACT;
    if (on(getenv("MP3MI_PSY_EXACT"))) o->test_flags |= MP3MI_TEST_PSY_EXACT;
    if (on(getenv("MP3MI_QUANT_EXACT"))) o->test_flags |= MP3MI_TEST_QUANT_EXACT;
    if (on(getenv("MP3MI_PREP_EXACT"))) o->test_flags |= MP3MI_TEST_PREP_EXACT;
    if (on(getenv("MP3MI_CW_EXACT"))) o->test_flags |= MP3MI_TEST_CW_EXACT;
    if ((e = getenv("MP3MI_CALL_HOLD"))) o->call_hold = atoi(e) != 0;
    if (on(getenv("MP3MI_DROPIN_STATS"))) o->dropin_stats = 1;
    if ((e = getenv("MP3MI_DROPIN_LOOKAHEAD")) && atoi(e) >= 0 && atoi(e) <= 4) o->dropin_lookahead = atoi(e);
}

// MP3MI_TEST_* flags as the kernels and the scheduler take them (checked by the caller)
static void set_test_flags(mp3mi_batch *b, unsigned flags)
{
    b->test_flags = (int) (flags & 15u) | ((flags & MP3MI_TEST_CW_EXACT) ? 16 : 0) | ((flags & MP3MI_TEST_PREP_LIST) ? 32 : 0);
    b->prep_exact = (flags & MP3MI_TEST_PREP_EXACT) ? 1 : 0;
}

// The list of what a stream carries (carried_region), once the buffers exist
static void carried_init(mp3mi_batch *b)
{
    const size_t C = (size_t) b->channels;
    const carried_region r[N_CARRIED] = {{b->psy_state, mp3mi_psy_state_size() * C, false, true},
                                         {b->pcm_hist, sizeof(int16_t) * MP3MI_PCM_HIST * C, false, true},
                                         {b->loop_state, sizeof(mp3mi_loop_state), true, true},
                                         {b->out_base, sizeof(int64_t), true, true}, // (0: a flush before the first encode delivers nothing)
                                         {b->carry, MP3MI_CARRY_BYTES, true, false},
                                         {b->carry_len, sizeof(int32_t), true, true},
                                         {b->bits_per_frame, sizeof(int32_t), true, false},  // (the live bitrate words last: an import leaves them
                                         {b->bitrate_index, sizeof(int32_t), true, false}};  // out where the arrays hold nothing but create-time values)
    for (int k = 0; k < N_CARRIED; k++) b->carried[k] = r[k];
}

// Fills *b step by step; on any failure the caller destroys the partially built object (every pointer and handle
// starts out null, and mp3mi_batch_destroy skips what was never created; so does every counter and flag: only what is not zero
// is set here).  The arguments are mp3mi_batch_create_ex's, checked there.
static int batch_build(mp3mi_batch *b, int n_streams, int rate_hz, int channels, const int *kbps, int kbps_all, int max_frames,
                       const mp3mi_batch_options &opt)
{
    const int ri = rate_idx_of(rate_hz);
    CHK(hipGetDevice(&b->device));
    b->n_streams = n_streams; b->rate_idx = ri; b->rate_hz = rate_hz; b->channels = channels;
    b->max_frames = max_frames;
    b->bits_per_frame_h.resize(n_streams);
    b->bitrate_index_h.resize(n_streams);
    b->kbps_h.resize(n_streams);
    for (int s = 0; s < n_streams; s++) {
        const int k = kbps ? kbps[s] : kbps_all;
        (void) rate_of_kbps(ri, k, &b->bitrate_index_h[s], &b->bits_per_frame_h[s]);
        b->kbps_h[s] = k;
        if (k > b->ceil_kbps) b->ceil_kbps = k;
        if (b->bits_per_frame_h[s] / 8 > b->max_frame_bytes) b->max_frame_bytes = b->bits_per_frame_h[s] / 8;
    }
    b->slot_kbps_h.assign(b->kbps_h.begin(), b->kbps_h.end());
    // chunk size from a scratch budget (bytes per frame and stream of the per-chunk buffers)
    const size_t per_gc = MP3MI_HBLK_P * 4 + MP3MI_PART_P * 12 + 3 * MP3MI_HBLK_S * 4 + MP3MI_FFT_BINS * 4 + 50 * 8 + 12 * 4 +
                          2 * (sizeof(mp3mi_psy_out) + sizeof(mp3mi_loop_prep) + 576 * 8) + 576 * 8 + 576 * 2;
    const size_t per_frame = per_gc * 2 * (size_t) channels + sizeof(mp3mi_frame_side);
    const size_t budget = (size_t) (opt.scratch_mb ? opt.scratch_mb : 32768u) << 20;
    long cf = (long) (budget / (per_frame * (size_t) n_streams));
    if (cf < 1) cf = 1;
    if (cf > max_frames) cf = max_frames;
    if (opt.chunk_frames > 0 && opt.chunk_frames < cf) cf = opt.chunk_frames;
    if ((size_t) n_streams * 2 * (size_t) cf * (size_t) channels > MP3MI_CW_MAX_REC) return MP3MI_ERR_ARG; // (k_cw's 32-bit item index; such a chunk's buffers would be a terabyte)
    b->chunk_frames = (int) cf;

    std::vector<char> Th_store(sizeof(mp3mi_tables)); // host copy of the tables, released on every path
    mp3mi_tables *Th = (mp3mi_tables *) Th_store.data();
    { const int trc = tables_rc(mp3mi_build_tables(Th, ri)); if (trc != MP3MI_OK) return trc; }
    const size_t S = (size_t) n_streams, ngc = S * 2 * (size_t) cf * (size_t) channels;
    {
        int least = 0, greatest = 0;
        CHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        CHK(hipStreamCreateWithPriority(&b->stream, hipStreamDefault, least));
        CHK(hipStreamCreateWithPriority(&b->lstream, hipStreamDefault, greatest));
    }
    {   // parts: as few as hold the batch with at most mp3mi_loop_resident() streams each, equal in size (a multiple of 64)
        const int resident = mp3mi_loop_resident();
        const int np = (n_streams + resident - 1) / resident;
        const int ps = ((n_streams + np - 1) / np + 63) / 64 * 64;
        b->part_streams = ps;
        b->n_parts = (n_streams + ps - 1) / ps;
        b->ev_front.assign(2 * (size_t) b->n_parts, (hipEvent_t) 0);
        b->ev_loop.assign(2 * (size_t) b->n_parts, fence());
        for (size_t i = 0; i < b->ev_front.size(); i++) {
            CHK(hipEventCreateWithFlags(&b->ev_front[i], hipEventDisableTiming));
            CHK(b->ev_loop[i].create());
        }
    }
    CHK(b->ev_done.create());
    CHK(hipEventCreateWithFlags(&b->ev_hist, hipEventDisableTiming));
    set_test_flags(b, opt.test_flags);
    b->hdr_mode = (channels == 1) ? 3 : 0;
    b->hold_calls = opt.call_hold != 0;
    if (b->hold_calls) {
        CHK(pinned_alloc(b, &b->hold_flag_h, 64, hipHostMallocMapped));
        for (int i = 0; i < 16; i++) b->hold_flag_h[i] = 0;
        CHK(hipHostGetDevicePointer((void **) &b->hold_flag_d, b->hold_flag_h, 0));
    }
    CHK(dev_alloc(b, &b->gate_count, 2 * sizeof(unsigned))); // [0] start census, [1] frames finished in this launch
    CHK(hipMemset(b->gate_count, 0, 2 * sizeof(unsigned)));
    CHK(dev_alloc(b, &b->voided, sizeof(unsigned)));
    CHK(hipMemset(b->voided, 0, sizeof(unsigned)));
    CHK(dev_alloc(b, &b->status_dev, sizeof(int32_t) * S));
    {
        hipDeviceProp_t prop;
        int dev = 0;
        CHK(hipGetDevice(&dev));
        CHK(hipGetDeviceProperties(&prop, dev));
        b->n_simd = prop.multiProcessorCount * 4;
        if (n_streams >= 2 * b->n_simd) { // placement only matters when SIMDs hold several streams
            CHK(dev_alloc(b, &b->place_order, sizeof(int) * S));
            CHK(dev_alloc(b, &b->place_cost, sizeof(int) * S));
            CHK(dev_alloc(b, &b->place_zero, sizeof(unsigned) * (S + 2 * MP3MI_PLACE_KEYS + 2)));
        }
    }
    CHK(dev_alloc(b, &b->T, sizeof(mp3mi_tables)));
    CHK(hipMemcpy(b->T, Th, sizeof(mp3mi_tables), hipMemcpyHostToDevice));
    CHK(dev_alloc(b, &b->rate_live, 2 * sizeof(int32_t) * S));
    CHK(dev_alloc(b, &b->rate_create, 2 * sizeof(int32_t) * S));
    b->bits_per_frame = b->rate_live;
    b->bitrate_index = b->rate_live + n_streams;
    for (int32_t *dst : {b->rate_live, b->rate_create}) {
        CHK(hipMemcpy(dst, b->bits_per_frame_h.data(), sizeof(int32_t) * S, hipMemcpyHostToDevice));
        CHK(hipMemcpy(dst + n_streams, b->bitrate_index_h.data(), sizeof(int32_t) * S, hipMemcpyHostToDevice));
    }
    CHK(dev_alloc(b, &b->energy_l, ngc * MP3MI_HBLK_P * sizeof(float)));
    CHK(dev_alloc(b, &b->part_eb, ngc * MP3MI_PART_P * sizeof(double)));
#if defined(MP3MI_ULP_CENSUS) // (diagnostic build: two shadow copies behind the sums, mp3mi_geom::census_cb_stride)
    CHK(dev_alloc(b, &b->part_cb, 3 * ngc * MP3MI_PART_P * sizeof(float)));
    CHK(hipMemset(b->part_cb, 0, 3 * ngc * MP3MI_PART_P * sizeof(float)));
#else
    CHK(dev_alloc(b, &b->part_cb, ngc * MP3MI_PART_P * sizeof(float)));
#endif
    CHK(dev_alloc(b, &b->energy_s, ngc * 3 * MP3MI_HBLK_S * sizeof(float)));
    CHK(dev_alloc(b, &b->hist6, ngc * 12 * sizeof(float)));
    CHK(dev_alloc(b, &b->fft_bins, ngc * MP3MI_FFT_BINS * sizeof(float)));
    CHK(dev_alloc(b, &b->cw_mid, ngc * 50 * sizeof(double)));
    CHK(dev_alloc(b, &b->cw_fix, mp3mi_cw_fixlist_bytes(ngc)));
    CHK(hipMemset(b->cw_fix, 0, sizeof(mp3mi_cw_fixlist)));
    CHK(dev_alloc(b, &b->prep_fix, mp3mi_prep_fixlist_bytes(ngc)));
    CHK(hipMemset(b->prep_fix, 0, sizeof(mp3mi_prep_fixlist)));
    for (int i = 0; i < 2; i++) {
        CHK(dev_alloc(b, &b->xr[i], ngc * 576 * sizeof(double)));
        CHK(dev_alloc(b, &b->psy[i], ngc * sizeof(mp3mi_psy_out)));
        CHK(dev_alloc(b, &b->prep[i], ngc * sizeof(mp3mi_loop_prep)));
    }
    CHK(dev_alloc(b, &b->sbs, (ngc + S * channels) * 576 * sizeof(double)));
    CHK(dev_alloc(b, &b->ix, ngc * 576 * sizeof(int16_t)));
    CHK(dev_alloc(b, &b->side, S * (size_t) cf * sizeof(mp3mi_frame_side)));
    CHK(dev_alloc(b, &b->psy_state, mp3mi_psy_state_size() * S * channels));
    CHK(dev_alloc(b, &b->loop_state, sizeof(mp3mi_loop_state) * S));
    CHK(dev_alloc(b, &b->pcm_hist, sizeof(int16_t) * MP3MI_PCM_HIST * (size_t) channels * S));
    CHK(dev_alloc(b, &b->out_base, sizeof(int64_t) * S));
    CHK(dev_alloc(b, &b->carry, (size_t) MP3MI_CARRY_BYTES * S));
    CHK(dev_alloc(b, &b->carry_len, sizeof(int32_t) * S));
    carried_init(b);
    // (zero state from the start: a per-slot call runs every slot's stream through the kernels, the closed ones on silence, and a
    // slot that never had a stream must hold a valid -- fresh -- encoder state for that)
    for (const carried_region &r : b->carried)
        if (r.zero) CHK(hipMemset(r.base, 0, r.bytes * S));
    b->book.init(n_streams);
    b->ctl_at.init(S);
    for (mp3mi_batch::ctl_ring::entry &en : b->ctl.e) CHK(ring_entry_create(b, en, b->ctl_at.bytes));
    CHK(hipEventCreateWithFlags(&b->ev_ctl_up, hipEventDisableTiming));
    for (mp3mi_batch::timing_set &ts : b->ts) {
        CHK(hipEventCreate(&ts.ev0));
        CHK(hipEventCreate(&ts.ev1));
    }
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_create(mp3mi_batch **out, int n_streams, int rate_hz, int channels, const int *kbps,
                                  int kbps_all, int max_frames)
{
    mp3mi_batch_options opt;
    mp3mi_batch_options_from_env(&opt); // once per batch; nothing else in the library reads the environment
    return mp3mi_batch_create_ex(out, n_streams, rate_hz, channels, kbps, kbps_all, max_frames, &opt);
}

extern "C" int mp3mi_batch_create_ex(mp3mi_batch **out, int n_streams, int rate_hz, int channels, const int *kbps,
                                     int kbps_all, int max_frames, const mp3mi_batch_options *opt_in)
{
    if (!out) return MP3MI_ERR_ARG;
    *out = NULL;
    mp3mi_batch_options opt;
    mp3mi_batch_options_default(&opt);
    if (opt_in) {
        if (opt_in->struct_size != sizeof(opt) || opt_in->abi != MP3MI_OPTIONS_ABI) return MP3MI_ERR_ARG; // another version of the header
        opt = *opt_in;
        if ((opt.test_flags & ~(unsigned) (MP3MI_TEST_ALL_EXACT | MP3MI_TEST_PREP_LIST)) || opt.chunk_frames < 0 || opt.dropin_lookahead < -1 ||
            opt.dropin_lookahead > 4 || (opt.dropin_stats != 0 && opt.dropin_stats != 1) || opt.call_hold < -1 || opt.call_hold > 1)
            return MP3MI_ERR_ARG;
    }
    // argument errors first: they are the caller's, whatever the machine
    if (rate_idx_of(rate_hz) < 0) return MP3MI_ERR_ARG; // src/l3psy.c:170-176 exits on anything else
    if (n_streams <= 0 || max_frames <= 0 || (channels != 1 && channels != 2)) return MP3MI_ERR_ARG;
    for (int s = 0; s < n_streams; s++) {
        int bi, bits;
        if (!rate_of_kbps(rate_idx_of(rate_hz), kbps ? kbps[s] : kbps_all, &bi, &bits)) return MP3MI_ERR_ARG;
        if (!kbps) break;
    }
    if (!have_device()) {
        fprintf(stderr, "mp3mi: no HIP device available -- this library has no CPU path\n");
        return MP3MI_ERR_NO_DEVICE;
    }
    mp3mi_batch *b = new mp3mi_batch(); // value-initialised: every pointer, handle and counter starts at zero
    const int rc = batch_build(b, n_streams, rate_hz, channels, kbps, kbps_all, max_frames, opt);
    if (rc != MP3MI_OK) {
        mp3mi_batch_destroy(b); // frees whatever was allocated before the failure
        return rc;
    }
    *out = b; // published only when complete
    return MP3MI_OK;
}

extern "C" void mp3mi_batch_destroy(mp3mi_batch *b)
{
    if (!b) return;
    device_scope ds(b->device);
    hold_release(b);
    mp3mi_batch::host_io &H = b->hio;
    for (hipStream_t st : {b->stream, b->lstream, H.h2d, H.d2h}) // (whatever exists, also after a build that failed half-way)
        if (st) hipStreamSynchronize(st);
    // the buffers: what dev_alloc / pinned_alloc noted, the last first, and the one kept by hand
    for (size_t i = b->owned.size(); i-- > 0;) {
        if (b->owned[i].pinned) hipHostFree(b->owned[i].p);
        else hipFree(b->owned[i].p);
    }
    for (mp3mi_batch::host_io::io_slot &io : H.slot)
        if (io.out_rows) hipFree(io.out_rows);
    // the fences, then the plain events
    b->ev_done.destroy();
    for (fence &f : b->ev_loop) f.destroy();
    for (mp3mi_batch::ctl_ring::entry &en : b->ctl.e) en.free.destroy();
    for (mp3mi_batch::park_ring::entry &en : b->park.e) en.free.destroy();
    std::vector<hipEvent_t> evs = {b->ev_hist, b->ev_ctl_up, b->ts[0].ev0, b->ts[0].ev1, b->ts[1].ev0, b->ts[1].ev1};
    for (const std::vector<hipEvent_t> *v : {&b->ev_front, &b->ts[0].loop_ev, &b->ts[1].loop_ev}) evs.insert(evs.end(), v->begin(), v->end());
    for (mp3mi_batch::host_io::io_slot &io : H.slot) {
        io.pcm_free.destroy();
        io.out_free.destroy();
        for (const std::vector<hipEvent_t> *v : {&io.ev_fmt, &io.t_up, &io.t_dn, &io.ev_in}) evs.insert(evs.end(), v->begin(), v->end());
    }
    for (hipEvent_t e : evs)
        if (e) hipEventDestroy(e);
    for (hipStream_t st : {H.h2d, H.d2h, b->stream, b->lstream})
        if (st) hipStreamDestroy(st);
    if (b->feed) feed_drop(b->feed); // (its buffers were the batch's: freed above)
    delete b;
}

// The least out_stride a call of n_frames takes: whole frames, the byte under construction that close writes, and -- for
// streaming calls -- the bytes an earlier call formatted but could not deliver yet, which lead the row
static size_t min_out_stride(const mp3mi_batch *b, int n_frames, bool streaming)
{
    return (size_t) n_frames * (size_t) b->max_frame_bytes + 1 + (streaming ? MP3MI_CARRY_BYTES : 0);
}

extern "C" size_t mp3mi_batch_out_stride(const mp3mi_batch *b, int n_frames) { return (min_out_stride(b, n_frames, true) + 255) & ~(size_t) 255; }

extern "C" void mp3mi_batch_debug_enable(mp3mi_batch *b, int on) { b->debug = on; }

extern "C" int mp3mi_batch_set_test_flags(mp3mi_batch *b, unsigned flags)
{
    if (!b || (flags & ~(unsigned) (MP3MI_TEST_ALL_EXACT | MP3MI_TEST_PREP_LIST))) return MP3MI_ERR_ARG;
    set_test_flags(b, flags);
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_set_header(mp3mi_batch *b, int copyright, int original, int emphasis)
{
    if (feed_locked(b)) return MP3MI_ERR_ARG;
    if (!b || (copyright & ~1) || (original & ~1) || (emphasis & ~3)) return MP3MI_ERR_ARG;
    b->hdr_flags = (copyright << 3) | (original << 2) | emphasis;
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_set_mode(mp3mi_batch *b, int mode)
{
    if (feed_locked(b)) return MP3MI_ERR_ARG;
    if (!b) return MP3MI_ERR_ARG;
    // -m s / d / m of the reference's driver (src/musicin.c:226-234); joint stereo is refused for Layer III by the
    // reference itself (src/musicin.c:548-552), and the mode has to fit the channel count
    const bool ok = (b->channels == 2 && (mode == MP3MI_MODE_STEREO || mode == MP3MI_MODE_DUAL_CHANNEL)) || (b->channels == 1 && mode == MP3MI_MODE_MONO);
    if (!ok) return MP3MI_ERR_ARG;
    b->hdr_mode = mode;
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_set_error_protection(mp3mi_batch *b, int on)
{
    if (feed_locked(b)) return MP3MI_ERR_ARG;
    if (!b || (on & ~1)) return MP3MI_ERR_ARG;
    b->crc = on;
    return MP3MI_OK;
}

struct host_call { // a call on host buffers (mp3mi_batch_encode_host_async): where the PCM comes from and the results go
    const int16_t *pcm;
    uint8_t *out;
    size_t out_stride;
    uint32_t *out_len;
    int slot;
    // a per-slot call with a row map: the caller's buffers hold n_rows dense rows, row r belongs to slot rows_host[r]
    // (rows_host NULL: a row per stream, no map); rows_dev is the map's copy in the call's control block (slots_impl)
    int n_rows;
    const int32_t *rows_host, *rows_dev;
};
struct slot_call { // a per-slot call (mp3mi_batch_encode_slots)
    mp3mi_batch::ctl_ring::entry *blk; // its control block: the ring entry the call took
    ctl_block dev;        // ... and the fields of the device copy
    int n_start;
    bool set_rates;       // the START slots' bitrates go into the live arrays (dev.rate_bits / rate_index); false: the arrays hold
                          // the create-time values and stay as they are
    bool any_continue;    // a stream that earlier calls began goes on in the call: its carried bytes lead its row
};
static int encode_impl(mp3mi_batch *b, const int16_t *pcm_dev, const int32_t *n_samples_dev, int n_frames, uint8_t *out_dev,
                       size_t out_stride, uint32_t *out_len_dev, bool whole_file, const host_call *hc = NULL, const slot_call *sc = NULL);

// reads a timing set out (waits for its call to finish)
static int harvest_timing(mp3mi_batch *b, int k)
{
    mp3mi_batch::timing_set &ts = b->ts[k];
    if (!ts.pending) return MP3MI_OK;
    CHK(hipEventSynchronize(ts.ev1));
    float tot = 0, loop = 0;
    CHK(hipEventElapsedTime(&tot, ts.ev0, ts.ev1));
    for (int c = 0; c < ts.launches; c++) {
        float ms = 0;
        CHK(hipEventElapsedTime(&ms, ts.loop_ev[2 * c], ts.loop_ev[2 * c + 1]));
        loop += ms;
    }
    b->last_loop_ms = loop; b->last_all_ms = tot; b->last_launches = ts.kernels;
    b->tot_loop_ms += loop; b->tot_all_ms += tot; b->tot_launches += ts.kernels; b->tot_calls++;
    ts.pending = false;
    return MP3MI_OK;
}

// Every stream is over, or starts afresh: back to the create-time bitrates where a per-slot call has written others
// (mp3mi_batch::rate_dirty).  On the LOOP stream, like every write of the live arrays: in order behind the last reader of the
// streams that end -- the k_loop, k_format and k_stream_tail of the call before, which may still run there, held even -- and
// ahead of every reader of the streams that begin.  (Not on the front stream, where the rest of a reset goes: the copy would
// have to wait for ev_done, and ev_done to be recorded behind the last reader on every path that leads here.)
static int rates_restore(mp3mi_batch *b)
{
    if (!b->rate_dirty) return MP3MI_OK;
    CHK(hipMemcpyAsync(b->rate_live, b->rate_create, 2 * sizeof(int32_t) * (size_t) b->n_streams, hipMemcpyDeviceToDevice, b->lstream));
    b->slot_kbps_h.assign(b->kbps_h.begin(), b->kbps_h.end());
    b->rate_dirty = false;
    return MP3MI_OK;
}

// Fresh encoder state for every stream: what the reference's function statics and the caller's buffers hold when
// its main() starts (all zero).  Enqueued on the front stream behind whatever is still running.
static int reset_impl(mp3mi_batch *b)
{
    if (rates_restore(b) != MP3MI_OK) return MP3MI_ERR_HIP;
    CHK(b->ev_done.wait_on(b->stream)); // the previous call's kernels may still be running on the loop stream
    for (const carried_region &r : b->carried) // (all on the front stream, the loop stream's regions too: behind ev_done)
        if (r.zero) CHK(hipMemsetAsync(r.base, 0, r.bytes * (size_t) b->n_streams, b->stream));
    b->book.close();
    b->fresh = true;
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_reset(mp3mi_batch *b)
{
    if (feed_locked(b)) return MP3MI_ERR_ARG;
    if (!b) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    b->status_kept = false; // an explicit reset starts new streams: what a flush kept of the ones it ended goes with them
    hold_release(b); // (the front stream is about to wait for the call before)
    return reset_impl(b);
}

extern "C" int mp3mi_batch_encode(mp3mi_batch *b, const int16_t *pcm_dev, int n_frames, uint8_t *out_dev,
                                  size_t out_stride, uint32_t *out_len_dev)
{
    if (feed_locked(b)) return MP3MI_ERR_ARG;
    return encode_impl(b, pcm_dev, NULL, n_frames, out_dev, out_stride, out_len_dev, true);
}

extern "C" int mp3mi_batch_encode_ragged(mp3mi_batch *b, const int16_t *pcm_dev, const int32_t *n_samples_dev, int n_frames,
                                         uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev)
{
    if (!n_samples_dev || feed_locked(b)) return MP3MI_ERR_ARG;
    return encode_impl(b, pcm_dev, n_samples_dev, n_frames, out_dev, out_stride, out_len_dev, true);
}

// ---- per-slot streaming (mp3mi_batch_encode_slots) ----
// Writes the staging copy of the control block this per-slot call takes (waits for the per-slot call two before, whose kernels
// read the device copy of the same parity and whose upload read this staging)
static int ctl_take(mp3mi_batch *b, mp3mi_batch::ctl_ring::entry **blk)
{
    *blk = &b->ctl.take();
    CHK((*blk)->free.sync());
    return MP3MI_OK;
}

// The rules of a per-slot call (f: slot_book::now): the book's, which all three layers share, then Layer III's own of the bitrate -- a
// STARTing stream's (0: the slot's create-time one) is a Layer III bitrate that fits the rows; any other slot's is 0, or what the
// open stream has
static bool slots_rules_ok(const mp3mi_batch *b, const int64_t *f, int n_frames, const uint8_t *ctl_host, const int32_t *n_samples_host,
                           const int32_t *kbps_host)
{
    if (!b->book.rules_ok(f, n_frames, 1152, ctl_host, n_samples_host)) return false;
    for (int s = 0; kbps_host && s < b->n_streams; s++) {
        const bool open = f[s] >= 0, start = ctl_host[s] & MP3MI_SLOT_START;
        const int32_t k = kbps_host[s];
        int bi, bits;
        if (start ? (k != 0 && (k > b->ceil_kbps || !rate_of_kbps(b->rate_idx, k, &bi, &bits))) : (k != 0 && !(open && k == b->slot_kbps_h[s])))
            return false;
    }
    return true;
}

// ctl_host / n_samples_host are per SLOT; hc: the call's buffers are the host-buffer copies of hc->slot, and the caller's are hc's
static int slots_impl(mp3mi_batch *b, const int16_t *pcm_dev, int n_frames, const uint8_t *ctl_host, const int32_t *n_samples_host,
                      const int32_t *kbps_host, uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev, host_call *hc = NULL)
{
    if (!b || !pcm_dev || !ctl_host || !out_dev || !out_len_dev || n_frames <= 0 || n_frames > b->max_frames) return MP3MI_ERR_ARG;
    if (out_stride < min_out_stride(b, n_frames, true)) return MP3MI_ERR_ARG;
    const int S = b->n_streams;
    std::vector<int64_t> f((size_t) S);
    b->book.now(f.data());
    // every rule first: a call that breaks one leaves the batch as it was
    if (!slots_rules_ok(b, f.data(), n_frames, ctl_host, n_samples_host, kbps_host)) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    slot_call sc;
    if (ctl_take(b, &sc.blk) != MP3MI_OK) return MP3MI_ERR_HIP;
    const ctl_block st = b->ctl_at.at(sc.blk->stage); // the staging copy: written here
    sc.dev = b->ctl_at.at(sc.blk->dev);
    if (hc && hc->rows_host) {
        memcpy(st.rows, hc->rows_host, sizeof(int32_t) * (size_t) hc->n_rows);
        hc->rows_dev = sc.dev.rows;
    }
    std::vector<int32_t> kb(b->slot_kbps_h);
    bool other_rate = false; // a stream STARTs at another bitrate than its slot was created with
    sc.n_start = b->book.fill(f.data(), n_frames, 1152, ctl_host, n_samples_host, st.fabs, st.n_samples, st.ctl, st.list);
    for (int i = 0; i < sc.n_start; i++) { // the bitrates of the streams that START, in the order of the list
        const int s = st.list[i];
        kb[s] = (kbps_host && kbps_host[s]) ? kbps_host[s] : b->kbps_h[s];
        int bi = 0, bits = 0;
        (void) rate_of_kbps(b->rate_idx, kb[s], &bi, &bits); // (checked: slots_rules_ok, create)
        st.rate_bits[i] = bits;
        st.rate_index[i] = bi;
        other_rate |= kb[s] != b->kbps_h[s];
    }
    sc.any_continue = false;
    for (int s = 0; s < S; s++) {
        if (f[s] >= 0 && !(ctl_host[s] & MP3MI_SLOT_START)) sc.any_continue = true;
        if (ctl_host[s] & MP3MI_SLOT_END) kb[s] = b->kbps_h[s]; // the stream takes its bitrate with it
    }
    // the START slots' bitrates go into the live arrays (encode_impl) once any slot of the batch may hold another than its
    // create-time one -- a START with kbps 0, or without kbps_host, then brings its slot back; a batch that never saw another
    // bitrate launches what it always launched
    sc.set_rates = b->rate_dirty || other_rate;
    const int rc = encode_impl(b, pcm_dev, NULL, n_frames, out_dev, out_stride, out_len_dev, false, hc, &sc);
    if (rc != MP3MI_OK) return rc;
    b->ctl.next();
    b->slot_kbps_h.swap(kb);
    b->rate_dirty |= other_rate;
    b->book.advance(f.data(), ctl_host, n_frames);
    b->book.settle(f.data());
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_encode_slots_kbps(mp3mi_batch *b, const int16_t *pcm_dev, int n_frames, const uint8_t *ctl_host,
                                             const int32_t *n_samples_host, const int32_t *kbps_host, uint8_t *out_dev, size_t out_stride,
                                             uint32_t *out_len_dev)
{
    if (feed_locked(b)) return MP3MI_ERR_ARG;
    return slots_impl(b, pcm_dev, n_frames, ctl_host, n_samples_host, kbps_host, out_dev, out_stride, out_len_dev);
}

extern "C" int mp3mi_batch_encode_slots(mp3mi_batch *b, const int16_t *pcm_dev, int n_frames, const uint8_t *ctl_host,
                                        const int32_t *n_samples_host, uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev)
{
    return mp3mi_batch_encode_slots_kbps(b, pcm_dev, n_frames, ctl_host, n_samples_host, NULL, out_dev, out_stride, out_len_dev);
}

extern "C" int mp3mi_batch_slot_kbps(const mp3mi_batch *b, int32_t *kbps_host)
{
    if (!b || !kbps_host) return MP3MI_ERR_ARG;
    memcpy(kbps_host, b->slot_kbps_h.data(), sizeof(int32_t) * (size_t) b->n_streams);
    return b->ceil_kbps;
}

extern "C" int mp3mi_batch_slot_frames(const mp3mi_batch *b, int64_t *frames_host)
{
    if (!b || !frames_host) return MP3MI_ERR_ARG;
    b->book.now(frames_host);
    return b->book.count_open();
}

extern "C" int mp3mi_batch_encode_next(mp3mi_batch *b, const int16_t *pcm_dev, int n_frames, uint8_t *out_dev,
                                       size_t out_stride, uint32_t *out_len_dev)
{
    if (feed_locked(b)) return MP3MI_ERR_ARG;
    if (b && b->book.on) {
        // per-slot bookkeeping in force: with no stream open every slot starts (the whole-batch start: state cleared for all);
        // otherwise the open streams go on and the other slots stay closed
        if (b->book.any_open()) {
            std::vector<uint8_t> ctl((size_t) b->n_streams, 0);
            return slots_impl(b, pcm_dev, n_frames, ctl.data(), NULL, NULL, out_dev, out_stride, out_len_dev);
        }
        if (!pcm_dev || !out_dev || !out_len_dev || n_frames <= 0 || n_frames > b->max_frames || out_stride < min_out_stride(b, n_frames, true))
            return MP3MI_ERR_ARG; // (before the bookkeeping changes)
        b->book.close();
        b->fresh = false;
    }
    return encode_impl(b, pcm_dev, NULL, n_frames, out_dev, out_stride, out_len_dev, false);
}

// What a call is to the kernels beyond the frames of a chunk, and its geometry (mp3mi_geom) for frames [f0, f0 + nf) -- a chunk;
// 0, 0: no frames, a flush -- and the n streams from s0: the whole batch's (s0 = 0, n = n_streams), or a PART's, which is the
// whole batch's with every per-stream pointer advanced to the part's first stream.
struct call_shape {
    int n_frames;
    const int32_t *n_samples; // device, per stream (mp3mi_geom::n_samples), or NULL
    long fabs0;               // frames of every stream before the call (a per-slot call: 0, and ...)
    const int64_t *fabs_s;    // ... device, per slot (mp3mi_geom::fabs_s), with
    const uint8_t *slot_ctl;  // device, per slot: MP3MI_SLOT_DEV_* (mp3mi_geom::slot_ctl); both NULL otherwise
    bool whole_file;
};
struct item_view { // an ITEM of a call: the frames of one chunk of one part of the streams (encode_impl)
    mp3mi_geom g;      // of the part: n_streams, n_samples / hist / out_base advanced
    int slot, ev;      // double-buffer slot of the chunk; index of the (slot, part) events
    size_t s0, rec0;   // first stream; (granule, channel) records of the chunk before the part
};
static mp3mi_geom call_geom(const mp3mi_batch *b, const call_shape &c, int f0, int nf, size_t s0, int n)
{
    mp3mi_geom g = mp3mi_make_geom(n, b->channels, b->rate_idx, c.n_frames, f0, nf);
    g.test_flags = b->test_flags;
    g.n_samples = c.n_samples ? c.n_samples + s0 : NULL;
    g.hdr_flags |= b->hdr_flags;
    g.hdr_mode = b->hdr_mode;
    g.crc = b->crc;
    g.fabs0 = c.fabs0;
    g.fabs_s = c.fabs_s ? c.fabs_s + s0 : NULL;
    g.slot_ctl = c.slot_ctl ? c.slot_ctl + s0 : NULL;
    g.hist = b->pcm_hist + s0 * MP3MI_PCM_HIST * (size_t) b->channels;
    g.out_base = c.whole_file ? NULL : b->out_base + s0;
    g.whole_file = c.whole_file ? 1 : 0;
#if defined(MP3MI_ULP_CENSUS)
    g.census_cb_stride = (size_t) b->n_streams * 2 * (size_t) b->chunk_frames * (size_t) b->channels * MP3MI_PART_P;
#endif
    return g;
}

extern "C" int mp3mi_batch_flush(mp3mi_batch *b, uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev)
{
    if (!b || !out_dev || !out_len_dev || out_stride < min_out_stride(b, 0, true) || feed_locked(b)) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    hold_release(b);
    const int S = b->n_streams;
    call_shape cs = {0, NULL, b->book.frames_all, NULL, NULL, false};
    mp3mi_batch::ctl_ring::entry *blk = NULL;
    if (b->book.on) { // some slots open, not all at the same frame (slot_book::settle), or none: end the open ones
        if (!b->book.any_open()) { // nothing to end; the ended streams' status stays in their slots -- and the book stays on
            CHK(hipMemsetAsync(out_len_dev, 0, sizeof(uint32_t) * (size_t) S, b->lstream));
            return MP3MI_OK;
        }
        if (ctl_take(b, &blk) != MP3MI_OK) return MP3MI_ERR_HIP;
        memset(blk->stage, 0, b->ctl_at.base_bytes); // (k_stream_tail reads fabs_s and ctl only)
        const ctl_block st = b->ctl_at.at(blk->stage), dev = b->ctl_at.at(blk->dev);
        for (int s = 0; s < S; s++) {
            const bool open = b->book.at(s) >= 0;
            st.fabs[s] = open ? b->book.at(s) : 0;
            st.ctl[s] = open ? MP3MI_SLOT_DEV_ACTIVE : 0;
        }
        CHK(hipMemcpyAsync(blk->dev, blk->stage, b->ctl_at.base_bytes, hipMemcpyHostToDevice, b->lstream));
        cs.fabs0 = 0;
        cs.fabs_s = dev.fabs;
        cs.slot_ctl = dev.ctl;
    } else if (b->fresh) { // nothing was encoded since the reset: no file body (the reference would write one byte; see mp3mi.h)
        CHK(hipMemsetAsync(out_len_dev, 0, sizeof(uint32_t) * (size_t) S, b->lstream));
        return MP3MI_OK;
    }
    // the tail of either kind of flush
    const int words = (int) (sizeof(mp3mi_loop_state) / 4);
    mp3mi_launch_stream_tail(call_geom(b, cs, 0, 0, 0, S), 1, (int32_t *) b->loop_state, words, b->bits_per_frame, out_dev, out_stride, b->out_base,
                             b->carry, b->carry_len, out_len_dev, b->voided, b->lstream); // behind the last call's k_format
    CHK(hipGetLastError());
    // the streams' status words go with the state the reset clears: keep what mp3mi_batch_stream_status is asked for
    // after the flush (until the next encode starts new streams)
    mp3mi_launch_status_gather(S, (const int32_t *) b->loop_state, words, b->status_dev, b->lstream);
    CHK(hipGetLastError());
    if (blk) {
        CHK(blk->free.record(b->lstream));
        b->ctl.next();
    }
    b->status_kept = true;
    CHK(b->ev_done.record(b->lstream));
    return reset_impl(b); // the streams are over: the next encode_next starts new ones
}

// ---- parking and resuming streams (mp3mi_batch_slots_export / mp3mi_batch_slots_import) ----
// Everything a stream carries from call to call is a record per slot in the regions of mp3mi_batch::carried.  The state record
// of a parked stream holds them one after the other, in that order, each at a multiple of 16 bytes; front / loop: the regions
// by the HIP stream that owns them (encode_impl), with their offsets.  Returns the record's size.
static size_t park_tables(const mp3mi_batch *b, mp3mi_park_table *front, mp3mi_park_table *loop)
{
    if (front) memset(front, 0, sizeof(*front));
    if (loop) memset(loop, 0, sizeof(*loop));
    uint32_t off = 0;
    for (const carried_region &c : b->carried) {
        mp3mi_park_table *t = c.loop ? loop : front;
        if (t && t->n < MP3MI_PARK_REGIONS) t->r[t->n++] = {c.base, (uint32_t) c.bytes, off};
        off += ((uint32_t) c.bytes + 15u) & ~15u;
    }
    return off;
}
static_assert(MP3MI_PARK_REGIONS >= N_CARRIED - 2, "the loop stream's regions of a parked stream");

// k_slot_begin over the regions of one HIP stream that a fresh stream needs zeroed (at most three per launch: the kernel's arguments)
static void slot_begin(const mp3mi_batch *b, bool loop, const int32_t *list, int n_list)
{
    mp3mi_slot_region r[3] = {{NULL, 0}, {NULL, 0}, {NULL, 0}};
    int k = 0;
    for (const carried_region &c : b->carried)
        if (c.zero && c.loop == loop && k < 3) r[k++] = {c.base, c.bytes};
    mp3mi_launch_slot_begin(list, n_list, r[0], r[1], r[2], loop ? b->lstream : b->stream);
}

extern "C" size_t mp3mi_batch_slot_state_bytes(const mp3mi_batch *b) { return b ? park_tables(b, NULL, NULL) : 0; }

// What export and import ask of their arguments alike (state_bytes: park_tables)
static bool park_args_ok(const mp3mi_batch *b, int n, const int32_t *slots_host, const void *state_dev, size_t state_stride, const void *tickets,
                         size_t state_bytes)
{
    if (!b || !slots_host || !state_dev || !tickets || n < 1 || n > b->n_streams) return false;
    if (state_stride < state_bytes || state_stride % 16 != 0 || (uintptr_t) state_dev % 16 != 0) return false;
    std::vector<char> seen((size_t) b->n_streams, 0);
    for (int i = 0; i < n; i++) {
        const int32_t s = slots_host[i];
        if (s < 0 || s >= b->n_streams || seen[s]) return false;
        seen[s] = 1;
    }
    return true;
}

// The launches of an export (to_state) or an import: the slot list goes up on the front stream, like a per-slot call's control
// block, and each stream moves the regions it owns -- the next call's feed-forward kernels do not wait for the loop stream, so
// the psy state and the PCM history are read and written on the front stream only; everything k_loop, k_format and
// k_stream_tail carry, the live bitrate words among them, on the loop stream only, behind the k_loop of the call before
// (held or not: nothing here lets a hold go, the next call's first transforms do as ever, and neither launch waits for the
// other stream's kernels).  An import's writes are also behind a reset's memsets, which run on the front stream (ev_ctl_up).
static int park_run(mp3mi_batch *b, int n, const int32_t *slots_host, const mp3mi_park_table &front, const mp3mi_park_table &loop,
                    void *state_dev, size_t state_stride, int to_state)
{
    mp3mi_batch::park_ring::entry &en = b->park.take();
    if (!en.stage) CHK(ring_entry_create(b, en, sizeof(int32_t) * (size_t) b->n_streams));
    // Whether the readers of the entry are through (four park calls ago: as a rule long since, and then the host neither waits
    // nor lets a held k_loop go, which would cost the next call its place beside that k_loop)
    if (!en.free.done()) {
        hold_release(b); // (the host is about to wait for work that may be queued behind the held k_loop)
        CHK(en.free.sync());
    }
    memcpy(en.stage, slots_host, sizeof(int32_t) * (size_t) n);
    CHK(hipMemcpyAsync(en.dev, en.stage, sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, b->stream));
    CHK(hipEventRecord(b->ev_ctl_up, b->stream));
    mp3mi_launch_slot_park(en.dev, n, front, state_dev, state_stride, to_state, b->stream);
    CHK(hipGetLastError());
    CHK(hipEventRecord(b->ev_hist, b->stream));
    CHK(hipStreamWaitEvent(b->lstream, b->ev_ctl_up, 0));
    if (!to_state && b->status_kept) {
        // the last flush ended every stream and reset the state: the ended streams' status goes back into their slots now, as with a
        // per-slot call, so that the call after this one does not write it over the status the resumed streams bring along
        mp3mi_launch_status_scatter(b->n_streams, (int32_t *) b->loop_state, (int) (sizeof(mp3mi_loop_state) / 4), b->status_dev, b->lstream);
        CHK(hipGetLastError());
        b->status_kept = false;
    }
    mp3mi_launch_slot_park(en.dev, n, loop, state_dev, state_stride, to_state, b->lstream);
    CHK(hipGetLastError());
    CHK(hipStreamWaitEvent(b->lstream, b->ev_hist, 0)); // both readers of the list are ahead of the entry's fence; ev_done covers both streams
    CHK(en.free.record(b->lstream));
    b->park.next();
    CHK(b->ev_done.record(b->lstream));
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_slots_export(mp3mi_batch *b, int n, const int32_t *slots_host, int close, void *state_dev, size_t state_stride,
                                        mp3mi_slot_ticket *tickets_host)
{
    if (!b || feed_locked(b)) return MP3MI_ERR_ARG;
    mp3mi_park_table front, loop;
    const size_t state_bytes = park_tables(b, &front, &loop);
    if (!park_args_ok(b, n, slots_host, state_dev, state_stride, tickets_host, state_bytes)) return MP3MI_ERR_ARG;
    std::vector<int64_t> f((size_t) b->n_streams);
    b->book.now(f.data());
    for (int i = 0; i < n; i++)
        if (f[slots_host[i]] < 0) return MP3MI_ERR_ARG; // no stream open there
    ON_DEVICE(b);
    for (int i = 0; i < n; i++) { // all of it host bookkeeping: no wait
        const int32_t s = slots_host[i];
        mp3mi_slot_ticket &t = tickets_host[i];
        memset(&t, 0, sizeof(t));
        t.magic = MP3MI_SLOT_TICKET_MAGIC;
        t.version = MP3MI_SLOT_TICKET_VERSION;
        t.state_bytes = (uint64_t) state_bytes;
        t.rate_hz = b->rate_hz;
        t.channels = b->channels;
        t.hdr_mode = b->hdr_mode;
        t.hdr_flags = b->hdr_flags;
        t.error_protection = b->crc;
        t.kbps = b->slot_kbps_h[s];
        t.frames = f[s];
    }
    const int rc = park_run(b, n, slots_host, front, loop, state_dev, state_stride, 1);
    if (rc != MP3MI_OK) return rc;
    if (close) {
        // (the whole-batch bookkeeping cannot say "all but these": the per-slot one takes over; slot_book::settle hands back as ever)
        for (int i = 0; i < n; i++) {
            const int32_t s = slots_host[i];
            f[s] = -1;
            b->slot_kbps_h[s] = b->kbps_h[s]; // the stream takes its bitrate with it
        }
    }
    b->book.settle(f.data());
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_slots_import(mp3mi_batch *b, int n, const int32_t *slots_host, const void *state_dev, size_t state_stride,
                                        const mp3mi_slot_ticket *tickets_host)
{
    if (!b || feed_locked(b)) return MP3MI_ERR_ARG;
    mp3mi_park_table front, loop;
    const size_t state_bytes = park_tables(b, &front, &loop);
    if (!park_args_ok(b, n, slots_host, state_dev, state_stride, tickets_host, state_bytes)) return MP3MI_ERR_ARG;
    std::vector<int64_t> f((size_t) b->n_streams);
    b->book.now(f.data());
    bool other_rate = false; // a stream arrives at another bitrate than its slot was created with
    for (int i = 0; i < n; i++) {
        const int32_t s = slots_host[i];
        const mp3mi_slot_ticket &t = tickets_host[i];
        int bi, bits;
        if (f[s] >= 0) return MP3MI_ERR_ARG; // a stream is open there
        if (t.magic != MP3MI_SLOT_TICKET_MAGIC || t.version != MP3MI_SLOT_TICKET_VERSION || t.state_bytes != (uint64_t) state_bytes) return MP3MI_ERR_ARG;
        if (t.rate_hz != b->rate_hz || t.channels != b->channels || t.hdr_mode != b->hdr_mode || t.hdr_flags != b->hdr_flags ||
            t.error_protection != b->crc)
            return MP3MI_ERR_ARG;
        if (t.kbps > b->ceil_kbps || !rate_of_kbps(b->rate_idx, t.kbps, &bi, &bits) || t.frames < 0) return MP3MI_ERR_ARG;
        other_rate |= t.kbps != b->kbps_h[s];
    }
    ON_DEVICE(b);
    // the streams' bitrate words go into the live arrays once any slot of the batch may hold another bitrate than its create-time
    // one -- the rule of a START (slots_impl); otherwise the arrays already hold what the records hold
    if (!(b->rate_dirty || other_rate)) loop.n -= 2;
    const int rc = park_run(b, n, slots_host, front, loop, const_cast<void *>(state_dev), state_stride, 0);
    if (rc != MP3MI_OK) return rc;
    for (int i = 0; i < n; i++) {
        const int32_t s = slots_host[i];
        f[s] = tickets_host[i].frames;
        b->slot_kbps_h[s] = tickets_host[i].kbps;
    }
    b->rate_dirty |= other_rate;
    // the per-slot bookkeeping from here on, also on a batch nothing has run on yet: no later call takes the "first call clears
    // every stream's state" branch of encode_impl over the resumed streams (slot_book::settle hands back only with every slot open)
    b->fresh = false;
    b->book.settle(f.data());
    return MP3MI_OK;
}

// One call of encode_impl, as its stages (below, in the order of their calls) share it: the caller's arguments, the call's shape,
// its cut into chunks and items, its timing set.  (Built behind fresh_start, which decides the shape's fabs0.)
struct encode_call {
    mp3mi_batch *b;
    const int16_t *pcm_dev; uint8_t *out_dev; size_t out_stride; uint32_t *out_len_dev; // the device buffers the kernels read and write
    bool whole_file;
    const host_call *hc; // NULL: the caller's buffers are those
    const slot_call *sc; // NULL: no per-slot call
    call_shape cs;
    int nchunks, cfr, P, n_items; // chunks, frames of a chunk, parts, items = nchunks * P
    size_t pcm_pitch;
    mp3mi_batch::timing_set *ts;
    bool joined; // the first item runs beside the held k_loop of the call before (join_or_release)
    size_t psy_state_bytes, loop_state_bytes;
    item_view view(int k) const
    {
        item_view v;
        const int c = k / P, part = k % P, S = b->n_streams;
        const int f0 = c * cfr;
        const int nf = (cs.n_frames - f0 < cfr) ? cs.n_frames - f0 : cfr;
        v.s0 = (size_t) part * (size_t) b->part_streams;
        const int n = S - (int) v.s0 < b->part_streams ? S - (int) v.s0 : b->part_streams;
        v.g = call_geom(b, cs, f0, nf, v.s0, n);
        v.slot = (c + b->slot_base) & 1;
        v.ev = v.slot * P + part;
        v.rec0 = v.s0 * 2 * (size_t) nf * (size_t) b->channels;
        return v;
    }
    // A part larger than the resident wavefronts (on the emulator, whose single CU holds 16) keeps every SIMD full to its end,
    // so the feed-forward kernels of the next item find no freed slots beside it, only cycles to take: there the item's
    // stage Y waits for the k_loop before it, and nothing of stage X runs beside that k_loop.
    bool y_after(const item_view &iv) const { return iv.g.n_streams > mp3mi_loop_resident(); }
    // (A per-slot call on host buffers does not join: its first transforms wait for the tick's PCM to cross PCIe, and a
    // k_loop held for that long -- a tick is one chunk, so the held launch is the whole tick before -- leaves the chip idle
    // during the upload: 29.7 ms per 4096 x 32 tick against 16.4 resident.  Let go at once, that k_loop runs beside the upload.)
    bool waits_for_upload() const { return (hc && sc) || b->feed_host_call; } // (a feeder's tick on host buffers: the same upload, the same rule)
};

static int fresh_start(mp3mi_batch *b, bool whole_file, const slot_call *sc)
{
    if (!(whole_file || (!sc && b->book.frames_all == 0 && !b->fresh))) return MP3MI_OK;
    for (const carried_region &r : b->carried) // (each region on the stream that owns it)
        if (r.zero) CHK(hipMemsetAsync(r.base, 0, r.bytes * (size_t) b->n_streams, r.loop ? b->lstream : b->stream));
    // streams that per-slot calls began at bitrates of their own end here.  (The host mirror is reset with the copy's enqueue, not
    // with the call's success: a HIP error further down leaves a call half enqueued, like any MP3MI_ERR_HIP of this function,
    // and no entry point recovers a batch from that, so the mirror is not rolled back.)
    if (rates_restore(b) != MP3MI_OK) return MP3MI_ERR_HIP;
    b->book.frames_all = 0;
    return MP3MI_OK;
}

static int control_block(const encode_call &c, bool kept) // (kept: status_dev still holds the status of the streams the last flush ended)
{
    mp3mi_batch *b = c.b;
    const slot_call *sc = c.sc;
    if (sc) {
        // the control block goes up on the front stream, ahead of everything of the call that reads it; the START slots' state is
        // cleared on the stream that owns it: psy state and PCM history before the call's first transform, the loop state, the
        // file position and the carry length before carry_in and the call's first k_loop
        // (the bitrates behind it travel only where k_slot_rate will read them: otherwise the copy is the size it always had)
        CHK(hipMemcpyAsync(sc->blk->dev, sc->blk->stage, sc->set_rates ? b->ctl_at.bytes : b->ctl_at.base_bytes, hipMemcpyHostToDevice, b->stream));
        CHK(hipEventRecord(b->ev_ctl_up, b->stream));
        slot_begin(b, false, sc->dev.list, sc->n_start);
        CHK(hipGetLastError());
        CHK(hipStreamWaitEvent(b->lstream, b->ev_ctl_up, 0));
        if (kept) { // the last flush ended every stream and reset the state: the ended streams' status stays until their slot STARTs
            mp3mi_launch_status_scatter(b->n_streams, (int32_t *) b->loop_state, (int) (sizeof(mp3mi_loop_state) / 4), b->status_dev, b->lstream);
            CHK(hipGetLastError());
        }
        slot_begin(b, true, sc->dev.list, sc->n_start);
        CHK(hipGetLastError());
        if (sc->set_rates) { // ... and their bitrates: here, behind the readers of the call before and ahead of this call's first
            mp3mi_launch_slot_rate(sc->dev.list, sc->n_start, sc->dev.rate_bits, sc->dev.rate_index, b->bits_per_frame, b->bitrate_index, b->lstream);
            CHK(hipGetLastError());
        }
    }
    if (!c.whole_file && (sc ? sc->any_continue : c.cs.fabs0 > 0)) { // the bytes earlier calls formatted but could not deliver lead the rows
        mp3mi_launch_carry_in(b->n_streams, b->carry, b->carry_len, c.out_dev, c.out_stride, b->lstream);
        CHK(hipGetLastError());
    }
    return MP3MI_OK;
}

static int timing_setup(const encode_call &c)
{
    mp3mi_batch *b = c.b;
    if (harvest_timing(b, (int) (b->call_no & 1)) != MP3MI_OK) return MP3MI_ERR_HIP; // (the call before the last one)
    mp3mi_batch::timing_set &ts = *c.ts;
    CHK(grow_events(ts.loop_ev, 2 * (size_t) c.n_items, 0));
    ts.launches = c.n_items;
    ts.kernels = 0;
    CHK(hipEventRecord(ts.ev0, b->stream));
    return MP3MI_OK;
}

// The whole call's PCM, chunk by chunk, in order on the upload stream: a 2-D copy per chunk (every stream's samples of
// the chunk's frames; the layout on the device is the caller's).  The chunk's first kernel waits for its copy, so chunk
// c + 1 crosses PCIe while chunk c is encoded -- and, with calls issued back to back, the next call's first chunk
// while this call's last one is.
// A per-slot call with a row map: the caller's rows are dense, one per live slot.  They cross as they are, into the
// dense device buffer, and behind each chunk's copy k_rows_in spreads the chunk's columns into the slot rows the
// kernels read -- on the upload stream, so a chunk's rows are in place while the chunk before is encoded.  (The map is
// in the control block, which the front stream uploads: ev_ctl_up.)
static int upload_chunks(const encode_call &c)
{
    mp3mi_batch *b = c.b;
    const size_t C = (size_t) b->channels, pcm_pitch = c.pcm_pitch;
    mp3mi_batch::host_io &H = b->hio;
    mp3mi_batch::host_io::io_slot &io = H.slot[c.hc->slot];
    const bool mapped = c.hc->rows_dev != NULL;
    const size_t R = mapped ? (size_t) c.hc->n_rows : (size_t) b->n_streams;
    CHK(io.pcm_free.wait_on(H.h2d)); // (the kernels of the call two before this one)
    for (std::vector<hipEvent_t> *v : {&io.t_up, &io.t_dn}) CHK(grow_events(*v, 2 * (size_t) c.nchunks, 0));
    for (std::vector<hipEvent_t> *v : {&io.ev_fmt, &io.ev_in}) CHK(grow_events(*v, (size_t) c.nchunks, hipEventDisableTiming));
    io.n_chunks = c.nchunks;
    io.bytes_up = io.bytes_dn = 0.0;
    if (mapped) CHK(hipStreamWaitEvent(H.h2d, b->ev_ctl_up, 0));
    for (int k = 0; k < c.nchunks; k++) {
        const int f0 = k * c.cfr, nf = (c.cs.n_frames - f0 < c.cfr) ? c.cs.n_frames - f0 : c.cfr;
        const size_t off = (size_t) f0 * 1152 * C, width = (size_t) nf * 1152 * C * sizeof(int16_t);
        int16_t *dst = mapped ? io.pcm_rows : io.pcm;
        CHK(hipEventRecord(io.t_up[2 * k], H.h2d));
        CHK(hipMemcpy2DAsync(dst + off, pcm_pitch * sizeof(int16_t), c.hc->pcm + off, pcm_pitch * sizeof(int16_t), width, R,
                             hipMemcpyHostToDevice, H.h2d));
        CHK(hipEventRecord(io.t_up[2 * k + 1], H.h2d));
        io.bytes_up += (double) width * (double) R;
        if (mapped) {
            mp3mi_launch_rows_in(c.hc->rows_dev, c.hc->n_rows, io.pcm_rows, io.pcm, pcm_pitch * sizeof(int16_t), off * sizeof(int16_t), width, H.h2d);
            CHK(hipGetLastError());
            CHK(hipEventRecord(io.ev_in[k], H.h2d));
        }
    }
    return MP3MI_OK;
}

// which: 1 the FFTs, 2 k_cw, the partition sums (k_part) and k_psy (passed on as mp3mi_launch_fft's which, whose bit 1 is k_cw)
static int stage_x(const encode_call &c, int k, int which)
{
    mp3mi_batch *b = c.b;
    const item_view v = c.view(k);
    const size_t r = v.rec0;
    if (c.hc && (which & 1) && k % c.P == 0) // the chunk's PCM is up (and in its slots' rows)
        CHK(hipStreamWaitEvent(b->stream, c.hc->rows_dev ? b->hio.slot[c.hc->slot].ev_in[k / c.P] : b->hio.slot[c.hc->slot].t_up[2 * (k / c.P) + 1], 0));
    mp3mi_launch_fft(b->T, v.g, c.pcm_dev + v.s0 * c.pcm_pitch, b->energy_l + r * MP3MI_HBLK_P, b->energy_s + r * 3 * MP3MI_HBLK_S,
                     b->fft_bins + r * MP3MI_FFT_BINS, b->cw_mid + r * 50, b->hist6 + r * 12, b->stream, which);
    CHK(hipGetLastError());
    if (which & 2) {
        // the k_loop that read this region of the slot last (two chunks ago, maybe in the call before)
        CHK(b->ev_loop[v.ev].wait_on(b->stream));
        mp3mi_launch_psy(b->T, v.g, b->energy_l + r * MP3MI_HBLK_P, b->energy_s + r * 3 * MP3MI_HBLK_S, b->cw_mid + r * 50, b->hist6 + r * 12,
                         b->fft_bins + r * MP3MI_FFT_BINS, b->cw_fix, (char *) b->psy_state + v.s0 * c.psy_state_bytes, b->part_eb + r * MP3MI_PART_P,
                         b->part_cb + r * MP3MI_PART_P, b->psy[v.slot] + r, b->stream);
        CHK(hipGetLastError());
    }
    return MP3MI_OK;
}

// The call before this one may have left its last k_loop HELD (k_hold): this call's first item then takes the place
// "the next item" has inside a call -- its transforms run now, in front of that k_loop, the hold is let go behind them,
// and the rest of the item runs beside that k_loop, behind the gate, like every item after it.
static int join_or_release(encode_call &c)
{
    mp3mi_batch *b = c.b;
    if (!(b->held && !c.y_after(c.view(0)) && !c.waits_for_upload())) {
        hold_release(b);
        return stage_x(c, 0, 3);
    }
    if (stage_x(c, 0, 1) != MP3MI_OK) return MP3MI_ERR_HIP;
    mp3mi_launch_hold_release(b->hold_flag_d, b->hold_seq, b->stream);
    CHK(hipGetLastError());
    b->held = false;
    c.joined = true;
    return MP3MI_OK;
}

// ---- front stream: everything that does not depend on the bit reservoir ----
static int item_front(const encode_call &c, int k, const item_view &v)
{
    mp3mi_batch *b = c.b;
    const mp3mi_geom &g = v.g;
    const size_t r = v.rec0, C = (size_t) b->channels;
    const bool follows = k >= 1 || c.joined; // a k_loop runs (or is about to) that this item's kernels go beside
    // what of stage X runs beside k_loop: all but the FFTs -- k_cw, k_part, k_psy are small in registers and LDS, the
    // item's FFTs were done before that launch started, and the region k_psy writes was read last by the launch before
    // it: 238.2 vs 247.2 ms per 4096 x 383 step with them between the launches.
    const bool beside = !c.y_after(v);
    if (k >= 1 && !beside) { // (the k_loop before this item's: view(k - 1))
        const item_view pv = c.view(k - 1);
        CHK(b->ev_loop[pv.ev].wait_on(b->stream));
    } else if (follows) // this item's kernels run behind k_loop(k - 1), once that is resident (<= 300 us)
        mp3mi_launch_gate(b->gate_count, b->gate_first - 16u, 30000u, b->stream);
    if (beside && follows && stage_x(c, k, 2) != MP3MI_OK) return MP3MI_ERR_HIP;
    mp3mi_launch_filter(b->T, g, c.pcm_dev + v.s0 * c.pcm_pitch, b->sbs + v.s0 * (size_t) (g.n_gran + 1) * C * 576,
                        b->debug ? b->sb_dbg + r * 576 : NULL, b->stream);
    CHK(hipGetLastError());
    // k_mdct's tail also computes the loop's stateless head and lists the records it could not decide; k_prep works
    // through the list (MP3MI_TEST_PREP_EXACT: through every record, the reference's way)
    CHK(hipMemsetAsync(&b->prep_fix->count, 0, sizeof(unsigned), b->stream));
    mp3mi_launch_mdct(b->T, g, b->psy[v.slot] + r, b->sbs + v.s0 * (size_t) (g.n_gran + 1) * C * 576, b->xr[v.slot] + r * 576,
                      b->prep[v.slot] + r, b->prep_fix, b->stream);
    CHK(hipGetLastError());
    mp3mi_launch_prep(b->T, g, b->xr[v.slot] + r * 576, b->psy[v.slot] + r, b->prep[v.slot] + r, b->prep_exact ? NULL : b->prep_fix, b->prep_exact, b->stream);
    CHK(hipGetLastError());
    if (k + 1 < c.n_items) {
        // (The next item's transforms take whole CUs' LDS: they run BETWEEN two k_loop launches.  Nothing but the queue behind
        // a busy chip sees to that -- this item's kernels take longer than the k_loop they run beside -- and an explicit wait
        // for that k_loop's end costs 1.4 ms per step, because the transforms then no longer slip in as its last CUs drain:
        // profiles/r05_experiments.txt, E7.)
        if (stage_x(c, k + 1, c.y_after(c.view(k + 1)) ? 3 : 1) != MP3MI_OK) return MP3MI_ERR_HIP;
    }
    CHK(hipEventRecord(b->ev_front[v.ev], b->stream));
    return MP3MI_OK;
}

// The call's file bytes, behind its last formatter -- a streaming call's behind its k_stream_tail, which settles the lengths
// -- as ONE copy: rows of the caller's stride when that is the device
// buffer's (mp3mi_batch_out_stride(b, max_frames): a plain copy, which the DMA engines take), a 2-D copy
// otherwise.  (A window of columns per chunk -- the bytes that became final with it -- was measured first: the
// runtime runs such rectangles as copy KERNELS, 11 ms each beside the encoder's own, and the step lost 56 ms;
// profiles/r04_experiments.txt.  With calls issued back to back this copy runs beside the next call's kernels.)
// With a row map k_rows_out gathers the listed slots' bytes and lengths into dense rows of the caller's stride first, so
// that the copy is plain whatever the stride and moves the live rows only.
static int download(const encode_call &c)
{
    mp3mi_batch *b = c.b;
    const size_t S = (size_t) b->n_streams, out_stride = c.out_stride;
    mp3mi_batch::host_io &H = b->hio;
    mp3mi_batch::host_io::io_slot &io = H.slot[c.hc->slot];
    const bool mapped = c.hc->rows_dev != NULL;
    const size_t R = mapped ? (size_t) c.hc->n_rows : S;
    const size_t row = mapped ? c.hc->out_stride : (c.hc->out_stride < out_stride ? c.hc->out_stride : out_stride);
    if (mapped) {
        mp3mi_launch_rows_out(c.hc->rows_dev, c.hc->n_rows, c.out_dev, out_stride, c.out_len_dev, io.out_rows, c.hc->out_stride, io.len_rows, b->lstream);
        CHK(hipGetLastError());
    }
    CHK(hipEventRecord(io.ev_fmt[0], b->lstream));
    CHK(hipStreamWaitEvent(H.d2h, io.ev_fmt[0], 0));
    CHK(hipEventRecord(io.t_dn[0], H.d2h));
    if (mapped)
        CHK(hipMemcpyAsync(c.hc->out, io.out_rows, c.hc->out_stride * R, hipMemcpyDeviceToHost, H.d2h));
    else if (c.hc->out_stride == out_stride)
        CHK(hipMemcpyAsync(c.hc->out, c.out_dev, out_stride * S, hipMemcpyDeviceToHost, H.d2h));
    else
        CHK(hipMemcpy2DAsync(c.hc->out, c.hc->out_stride, c.out_dev, out_stride, row, S, hipMemcpyDeviceToHost, H.d2h));
    CHK(hipMemcpyAsync(c.hc->out_len, mapped ? io.len_rows : c.out_len_dev, sizeof(uint32_t) * R, hipMemcpyDeviceToHost, H.d2h));
    CHK(hipEventRecord(io.t_dn[1], H.d2h));
    io.bytes_dn += (double) row * (double) R;
    CHK(io.out_free.record(H.d2h));
    return MP3MI_OK;
}

// ---- loop stream: the serial search and the formatter ----
static int item_loop(const encode_call &c, int k, const item_view &v)
{
    mp3mi_batch *b = c.b;
    const mp3mi_geom &g = v.g;
    const size_t r = v.rec0;
    // (what k_loop needs of its own stream is prepared AHEAD of the wait for the front stream -- in the shadow of the transforms that
    // run between two k_loop launches, not behind them: the ranking of the part's streams by their cost in the chunk before,
    // 0.19 ms for 4096 streams, and the two counters' reset)
    mp3mi_loop_place place = {NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0};
    if (b->place_order) { // rank the part's streams by their cost in the previous chunk, hand the tables to k_loop
        mp3mi_launch_rank(b->place_cost + v.s0, b->place_order + v.s0, g.n_streams, b->lstream);
        CHK(hipGetLastError());
        CHK(hipMemsetAsync(b->place_zero, 0, sizeof(unsigned) * ((size_t) b->n_streams + 2 * MP3MI_PLACE_KEYS + 2), b->lstream));
        place.order = b->place_order + v.s0; place.cost = b->place_cost + v.s0; place.taken = b->place_zero;
        place.simd_slots = b->place_zero + b->n_streams; place.simd_idx = place.simd_slots + MP3MI_PLACE_KEYS;
        place.ticket = place.simd_idx + MP3MI_PLACE_KEYS; place.scan = place.ticket + 1;
        place.n_simd = b->n_simd;
    }
    CHK(hipMemsetAsync(b->gate_count + 1, 0, sizeof(unsigned), b->lstream));
    CHK(hipStreamWaitEvent(b->lstream, b->ev_front[v.ev], 0));
    if (b->hold_calls && k == c.n_items - 1 && !c.waits_for_upload()) { // (a per-slot call on host buffers is not held: the next one would not join, above)
        // the call's LAST k_loop: held until the next call's first transforms are through (its first item then runs beside
        // this launch), the host lets go (hold_release), or the bound has passed: 20 ms, more for chunks so long that what the
        // front stream still holds of this item plus the next call's transforms take longer (0.4 ms per frame of a chunk)
        b->hold_seq++;
        const unsigned hold_ticks = 100000u * (unsigned) (g.nf * 4 / 10 > 20 ? (g.nf * 4 / 10 < 200 ? g.nf * 4 / 10 : 200) : 20); // 100 MHz
        mp3mi_launch_hold(b->hold_flag_d, b->hold_seq, hold_ticks, b->lstream);
        CHK(hipGetLastError());
        b->held = true;
    }
    CHK(hipEventRecord(c.ts->loop_ev[2 * k], b->lstream));
    {
        const int n = g.n_streams;
        b->gate_total += (unsigned) n; // a wavefront per stream counts itself in
        b->gate_first = b->gate_total; // the census once this launch is resident: the next item's kernels start behind it
        mp3mi_launch_loop(b->T, g, b->xr[v.slot] + r * 576, b->psy[v.slot] + r, b->prep[v.slot] + r, b->bits_per_frame + v.s0,
                          (char *) b->loop_state + v.s0 * c.loop_state_bytes, b->ix + r * 576, b->side + v.s0 * (size_t) g.nf,
                          b->gate_count, place, b->lstream);
        CHK(hipGetLastError());
    }
    c.ts->kernels += 1;
    CHK(hipEventRecord(c.ts->loop_ev[2 * k + 1], b->lstream));
    CHK(b->ev_loop[v.ev].record(b->lstream));
    mp3mi_launch_format(b->T, g, b->ix + r * 576, b->side + v.s0 * (size_t) g.nf, b->bits_per_frame + v.s0, b->bitrate_index + v.s0,
                        c.out_dev + v.s0 * c.out_stride, c.out_stride, c.out_len_dev + v.s0, (int32_t *) ((char *) b->loop_state + v.s0 * c.loop_state_bytes),
                        (int) (c.loop_state_bytes / 4), b->voided, b->lstream);
    CHK(hipGetLastError());
    if (c.hc && c.whole_file && k == c.n_items - 1 && download(c) != MP3MI_OK) return MP3MI_ERR_HIP;
    b->last_nf = g.nf;
    b->last_slot = v.slot;
    return MP3MI_OK;
}

// hand over to the next call: PCM history (front stream: behind the last kernels that read the old one) and,
// for a streaming call, what became final / what waits (loop stream: behind the last k_format)
static int hand_over(const encode_call &c)
{
    mp3mi_batch *b = c.b;
    const mp3mi_geom g = call_geom(b, c.cs, 0, c.cs.n_frames < c.cfr ? c.cs.n_frames : c.cfr, 0, b->n_streams); // the whole batch's, of chunk 0
    mp3mi_launch_hist_save(g, c.pcm_dev, b->pcm_hist, b->stream);
    CHK(hipGetLastError());
    if (!c.whole_file) {
        mp3mi_launch_stream_tail(g, 0, (int32_t *) b->loop_state, (int) (sizeof(mp3mi_loop_state) / 4), b->bits_per_frame, c.out_dev,
                                 c.out_stride, b->out_base, b->carry, b->carry_len, c.out_len_dev, b->voided, b->lstream);
        CHK(hipGetLastError());
        if (c.hc && download(c) != MP3MI_OK) return MP3MI_ERR_HIP;
    }
    CHK(hipEventRecord(b->ev_hist, b->stream));
    CHK(hipStreamWaitEvent(b->lstream, b->ev_hist, 0)); // ev_done below then covers both streams
    if (c.hc) { // (lstream has just joined the front stream: every kernel that reads the slot's PCM is ahead of this)
        mp3mi_batch::host_io::io_slot &io = b->hio.slot[c.hc->slot];
        CHK(io.pcm_free.record(b->lstream));
        io.pending = true;
        io.hold_of = b->held ? b->hold_seq : 0u;
    }
    if (c.sc) CHK(c.sc->blk->free.record(b->lstream)); // (lstream has joined the front stream: every reader of this copy of the control block is ahead of this)
    b->slot_base = (b->slot_base + c.nchunks) & 1;
    if (c.whole_file) b->book.close(); // a whole-file call leaves finished streams behind
    else b->book.frames_all = c.sc ? 0 : c.cs.fabs0 + c.cs.n_frames; // (a per-slot call: slots_impl keeps the slots' frames)
    CHK(hipEventRecord(c.ts->ev1, b->lstream));
    c.ts->pending = true;
    b->call_no++;
    CHK(b->ev_done.record(b->lstream));
    CHK(hipGetLastError());
    return MP3MI_OK;
}

static int encode_impl(mp3mi_batch *b, const int16_t *pcm_dev, const int32_t *n_samples_dev, int n_frames, uint8_t *out_dev,
                       size_t out_stride, uint32_t *out_len_dev, bool whole_file, const host_call *hc, const slot_call *sc)
{
    if (!b || !pcm_dev || !out_dev || !out_len_dev || n_frames <= 0 || n_frames > b->max_frames) return MP3MI_ERR_ARG;
    if (out_stride < min_out_stride(b, n_frames, !whole_file)) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    const size_t C = (size_t) b->channels;
    if (b->debug && !b->sb_dbg) {
        const size_t ngc = (size_t) b->n_streams * 2 * (size_t) b->chunk_frames * C;
        CHK(dev_alloc(b, &b->sb_dbg, ngc * 576 * sizeof(double)));
    }
    // The call before this one may still be running.  Its kernels and this call's share nothing but the batch's own
    // buffers, and every one of those is either touched on ONE stream only (in-order: the FFT outputs, the subband
    // samples, the psy state and the PCM history on the front stream; ix, the side information, the loop state, the
    // carry and the caller's output on the loop stream) or double-buffered across the two (psy / xr / prep: the slots
    // go on alternating from call to call, and a slot's writer waits for the k_loop that read it last, ev_loop).  So
    // this call's feed-forward kernels start at once and fill the chip while the last k_loop of the call before -- 4096
    // wavefronts, serial, nothing beside them -- runs out: back-to-back calls lose no pipeline fill.
    // a whole-file call starts every stream afresh; a streaming call continues (the first one after create / reset /
    // flush / a whole-file call starts afresh too)
    if (fresh_start(b, whole_file, sc) != MP3MI_OK) return MP3MI_ERR_HIP;
    // (a per-slot call: every slot has its own frame index, in the control block; k_loop counts the frame of a status from the
    // call's first, and k_stream_tail places it in the stream)
    const long fabs0 = sc ? 0 : b->book.frames_all;
    if (sc) n_samples_dev = sc->dev.n_samples;
    const bool kept = b->status_kept;
    b->fresh = false;
    b->status_kept = false;
    const int nchunks = (n_frames + b->chunk_frames - 1) / b->chunk_frames;
    const int cfr = (n_frames + nchunks - 1) / nchunks; // equal chunks: a short last one would run without overlap
    const size_t pcm_pitch = (size_t) n_frames * 1152 * C; // int16 per stream in the caller's buffer
    encode_call c = {b, pcm_dev, out_dev, out_stride, out_len_dev, whole_file, hc, sc,
                     {n_frames, n_samples_dev, fabs0, sc ? sc->dev.fabs : NULL, sc ? sc->dev.ctl : NULL, whole_file},
                     nchunks, cfr, b->n_parts, nchunks * b->n_parts, pcm_pitch, &b->ts[b->call_no & 1], false,
                     mp3mi_psy_state_size() * C, sizeof(mp3mi_loop_state)};
    if (b->place_cost) CHK(hipMemsetAsync(b->place_cost, 0, sizeof(int) * (size_t) b->n_streams, b->lstream)); // first chunk: order = identity
    if (hc) CHK(b->hio.slot[hc->slot].out_free.wait_on(b->lstream)); // the call two before this one copied out of it
    CHK(hipMemsetAsync(out_dev, 0, out_stride * (size_t) b->n_streams, b->lstream)); // (behind the formatter of the call before: it may be the same buffer)
    if (control_block(c, kept) != MP3MI_OK || timing_setup(c) != MP3MI_OK) return MP3MI_ERR_HIP;
    // The unit of scheduling is an ITEM: the frames of one chunk of one PART of the streams (a batch of at most
    // mp3mi_loop_resident() streams -- 4096 on an MI355X -- is one part).  Items go through the pipeline one after the
    // other, chunk by chunk and within a chunk part by part, exactly as the chunks of a one-part batch do: every buffer
    // is stream-major, so an item is the same kernels with their pointers advanced to the part's first stream.
    //
    //   front stream:  FFT(k+1) | gate | k_cw k_part k_psy (k+1) | k_filter k_mdct k_prep (k+1) | FFT(k+2) ...
    //   loop stream:              k_rank k_loop(k) ................................................ k_format(k)
    //
    // Two kinds of front-end kernels cannot share the chip with k_loop as it starts: k_fft takes a whole CU's LDS per
    // workgroup, and k_psy's wavefronts live long (serial over granules), so whichever is in flight when a k_loop is
    // launched keeps its workgroups from starting.  The FFTs of item k+1 therefore run BETWEEN two k_loop launches; all
    // the rest of item k+1 runs beside k_loop(k), behind a gate that lets k_loop become resident first, in the order of
    // how little each loses at one wavefront per SIMD; what does not fit beside k_loop (the tail of k_mdct, k_prep)
    // runs behind it, alone and fast.  (Until round 3 the feed-forward kernels ran over ALL streams of a chunk and only
    // k_loop was cut into parts, with a hand-made assignment of kernels to parts for two and for four parts; with three
    // parts k_psy was still running when the second part started and that part took 65 ms instead of 37:
    // profiles/r03_experiments.txt.  12 288 / 16 384 / 20 000 streams: 5.8 -> ... M frames/s.)
    if (hc && upload_chunks(c) != MP3MI_OK) return MP3MI_ERR_HIP;
    if (join_or_release(c) != MP3MI_OK) return MP3MI_ERR_HIP;
    for (int k = 0; k < c.n_items; k++) {
        const item_view v = c.view(k);
        if (item_front(c, k, v) != MP3MI_OK || item_loop(c, k, v) != MP3MI_OK) return MP3MI_ERR_HIP;
    }
    return hand_over(c);
}

extern "C" int mp3mi_batch_sync(mp3mi_batch *b)
{
    if (!b) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    hold_release(b);
    CHK(hipStreamSynchronize(b->stream));
    CHK(hipStreamSynchronize(b->lstream));
    if (b->hio.ready) { // host-buffer calls: the results are in the caller's memory when this returns
        CHK(hipStreamSynchronize(b->hio.h2d));
        CHK(hipStreamSynchronize(b->hio.d2h));
    }
    if (b->feed) CHK(feed_host_sync(b->feed)); // (ticks on host buffers: the same promise)
    CHK(hipGetLastError());
    // streams whose file was voided since the last sync: the reference dies on those inputs (mp3mi.h)
    unsigned voided = 0;
    CHK(hipMemcpy(&voided, b->voided, sizeof(voided), hipMemcpyDeviceToHost));
    if (voided) {
        CHK(hipMemset(b->voided, 0, sizeof(unsigned)));
        return MP3MI_ERR_REFERENCE_ABORT;
    }
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_stream_status(mp3mi_batch *b, int32_t *status_host)
{
    if (!b || !status_host) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    hold_release(b);
    // (the state of the most recent streams: a whole-file call leaves it behind, the next call's reset clears it; a
    // flush gathers it before its reset)
    if (!b->status_kept) {
        mp3mi_launch_status_gather(b->n_streams, (const int32_t *) b->loop_state, (int) (sizeof(mp3mi_loop_state) / 4), b->status_dev, b->lstream);
        CHK(hipGetLastError());
    }
    CHK(hipStreamSynchronize(b->stream));
    CHK(hipStreamSynchronize(b->lstream));
    CHK(hipMemcpy(status_host, b->status_dev, sizeof(int32_t) * (size_t) b->n_streams, hipMemcpyDeviceToHost));
    int n = 0;
    for (int s = 0; s < b->n_streams; s++) n += status_host[s] != 0;
    return n;
}

extern "C" int mp3mi_batch_debug_cw_fixups(mp3mi_batch *b, int *n_listed, int *n_records)
{
    if (!b || !n_listed || !n_records) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    hold_release(b);
    mp3mi_cw_fixlist h;
    CHK(hipMemcpy(&h, b->cw_fix, sizeof(h), hipMemcpyDeviceToHost));
    *n_listed = (int) h.count;
    *n_records = (int) h.cap;
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_debug_prep_fixups(mp3mi_batch *b, int *n_listed)
{
    if (!b || !n_listed) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    hold_release(b);
    mp3mi_prep_fixlist h;
    if (hipStreamSynchronize(b->stream) != hipSuccess) return MP3MI_ERR_HIP;
    CHK(hipMemcpy(&h, b->prep_fix, sizeof(h), hipMemcpyDeviceToHost));
    *n_listed = (int) h.count;
    return MP3MI_OK;
}

// both timing sets read out, the older first (waits for the calls issued so far)
static int harvest_all(mp3mi_batch *b)
{
    ON_DEVICE(b);
    hold_release(b);
    if (harvest_timing(b, (int) (b->call_no & 1)) != MP3MI_OK || harvest_timing(b, (int) ((b->call_no - 1) & 1)) != MP3MI_OK) return MP3MI_ERR_HIP;
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_last_timing(mp3mi_batch *b, float *loop_kernel_ms, float *all_kernels_ms, int *launches)
{
    if (!b || !b->ev_done.recorded || b->call_no == 0) return MP3MI_ERR_ARG; // nothing has been encoded yet
    if (harvest_all(b) != MP3MI_OK) return MP3MI_ERR_HIP;
    if (loop_kernel_ms) *loop_kernel_ms = b->last_loop_ms;
    if (all_kernels_ms) *all_kernels_ms = b->last_all_ms;
    if (launches) *launches = b->last_launches;
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_total_timing(mp3mi_batch *b, double *loop_kernel_ms, double *all_kernels_ms, long *launches, long *calls)
{
    if (!b) return MP3MI_ERR_ARG;
    if (harvest_all(b) != MP3MI_OK) return MP3MI_ERR_HIP;
    if (loop_kernel_ms) *loop_kernel_ms = b->tot_loop_ms;
    if (all_kernels_ms) *all_kernels_ms = b->tot_all_ms;
    if (launches) *launches = b->tot_launches;
    if (calls) *calls = b->tot_calls;
    return MP3MI_OK;
}

extern "C" long mp3mi_batch_debug_fetch(mp3mi_batch *b, int what, void *host_dst, size_t cap)
{
    if (!b || !host_dst) return MP3MI_ERR_ARG;
    const size_t ngc = (size_t) b->n_streams * 2 * (size_t) b->last_nf * (size_t) b->channels;
    const void *src = NULL;
    size_t n = 0;
    switch (what) {
    case 0: src = b->psy[b->last_slot]; n = ngc * sizeof(mp3mi_psy_out); break;
    case 1: src = b->xr[b->last_slot]; n = ngc * 576 * sizeof(double); break;
    case 2: src = b->ix; n = ngc * 576 * sizeof(int16_t); break;
    case 3: src = b->side; n = (size_t) b->n_streams * (size_t) b->last_nf * sizeof(mp3mi_frame_side); break;
    case 4: src = b->sb_dbg; n = ngc * 576 * sizeof(double); break;
    case 5: src = b->prep[b->last_slot]; n = ngc * MP3MI_LOOP_PREP_HEAD; break;
    // the transforms' outputs as k_fft hands them to k_cw / k_part / k_psy (the direct FFT seam: oracle/fft_seam.h)
    case 6: src = b->energy_l; n = ngc * MP3MI_HBLK_P * sizeof(float); break;
    case 7: src = b->energy_s; n = ngc * 3 * MP3MI_HBLK_S * sizeof(float); break;
    case 8: src = b->fft_bins; n = ngc * MP3MI_FFT_BINS * sizeof(float); break;
    default: return MP3MI_ERR_ARG;
    }
    if (!src || n > cap) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    hold_release(b);
    if (hipStreamSynchronize(b->stream) != hipSuccess || hipStreamSynchronize(b->lstream) != hipSuccess) return MP3MI_ERR_HIP;
    if (what == 5) { // the records' heads, side by side (what follows the head is k_loop's alone: mp3mi_dev.h)
        char *tmp = (char *) malloc(ngc * sizeof(mp3mi_loop_prep));
        if (!tmp) return MP3MI_ERR_NOMEM;
        const bool ok = hipMemcpy(tmp, src, ngc * sizeof(mp3mi_loop_prep), hipMemcpyDeviceToHost) == hipSuccess;
        for (size_t i = 0; ok && i < ngc; i++) memcpy((char *) host_dst + i * MP3MI_LOOP_PREP_HEAD, tmp + i * sizeof(mp3mi_loop_prep), MP3MI_LOOP_PREP_HEAD);
        free(tmp);
        return ok ? (long) n : MP3MI_ERR_HIP;
    }
    if (hipMemcpy(host_dst, src, n, hipMemcpyDeviceToHost) != hipSuccess) return MP3MI_ERR_HIP;
    return (long) n;
}

// ---- host buffers in, host buffers out, overlapped with the encode ("end-to-end with PCIe") ----
// What the reference's driver does per frame with get_audio / read_samples (src/encode.c:123-269) and fwrite: here the
// PCM of a whole call crosses PCIe chunk by chunk on a copy stream while the chunks before it are encoded, and the
// file bytes come back behind each chunk's formatter (encode_impl).
static int host_io_harvest(mp3mi_batch *b, int sl)
{
    mp3mi_batch::host_io &H = b->hio;
    mp3mi_batch::host_io::io_slot &io = H.slot[sl];
    if (!io.pending) return MP3MI_OK;
    const int n = io.n_chunks;
    CHK(hipEventSynchronize(io.t_dn[1]));
    CHK(hipEventSynchronize(io.t_up[2 * n - 1]));
    float ms = 0;
    for (int c = 0; c < n; c++) {
        CHK(hipEventElapsedTime(&ms, io.t_up[2 * c], io.t_up[2 * c + 1]));
        H.tot_up_ms += ms;
    }
    CHK(hipEventElapsedTime(&ms, io.t_dn[0], io.t_dn[1]));
    H.tot_dn_ms += ms;
    H.tot_up_bytes += io.bytes_up;
    H.tot_dn_bytes += io.bytes_dn;
    H.tot_calls++;
    io.pending = false;
    return MP3MI_OK;
}

// The copy streams with the first host-buffer call, a slot's device copies with the first call that uses the slot: a
// one-shot call (mp3mi_encode_host) pays for one slot, the second exists once two calls are in flight.  What a failed
// allocation leaves behind is freed by mp3mi_batch_destroy.
static int host_io_init(mp3mi_batch *b, int sl)
{
    mp3mi_batch::host_io &H = b->hio;
    const size_t S = (size_t) b->n_streams;
    if (!H.ready) {
        H.out_stride = mp3mi_batch_out_stride(b, b->max_frames);
        if (!H.h2d) CHK(hipStreamCreateWithFlags(&H.h2d, hipStreamNonBlocking));
        if (!H.d2h) CHK(hipStreamCreateWithFlags(&H.d2h, hipStreamNonBlocking));
        H.ready = true;
    }
    mp3mi_batch::host_io::io_slot &io = H.slot[sl];
    if (!io.pcm) CHK(dev_alloc(b, &io.pcm, S * (size_t) b->max_frames * 1152 * (size_t) b->channels * sizeof(int16_t)));
    if (!io.out) CHK(dev_alloc(b, &io.out, S * H.out_stride));
    if (!io.len) CHK(dev_alloc(b, &io.len, S * sizeof(uint32_t)));
    if (!io.pcm_free.ev) CHK(io.pcm_free.create());
    if (!io.out_free.ev) CHK(io.out_free.create());
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_encode_host_async(mp3mi_batch *b, const int16_t *pcm_host, int n_frames, uint8_t *out_host, size_t out_stride,
                                             uint32_t *out_len_host)
{
    if (!b || !pcm_host || !out_host || !out_len_host || n_frames <= 0 || n_frames > b->max_frames || feed_locked(b)) return MP3MI_ERR_ARG;
    if (out_stride < min_out_stride(b, n_frames, false)) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    mp3mi_batch::host_io &H = b->hio;
    const int sl = (int) (H.call_no & 1);
    if (host_io_init(b, sl) != MP3MI_OK) return MP3MI_ERR_HIP;
    if (host_io_harvest(b, sl) != MP3MI_OK) return MP3MI_ERR_HIP; // (waits for the call two before this one: at most two in flight)
    const host_call hc = {pcm_host, out_host, out_stride, out_len_host, sl};
    const int rc = encode_impl(b, H.slot[sl].pcm, NULL, n_frames, H.slot[sl].out, H.out_stride, H.slot[sl].len, true, &hc);
    if (rc == MP3MI_OK) H.call_no++; // (a call that failed took no slot)
    return rc;
}

// The dense device buffers of a call with a row map (mp3mi_batch::host_io::pcm_rows): PCM and lengths for as many rows as there
// are slots; the output rows have the caller's stride, so that buffer grows with the largest call so far (behind the slot's
// last download -- the host has waited for it: host_io_harvest).
static int host_rows_init(mp3mi_batch *b, int sl, size_t out_stride)
{
    mp3mi_batch::host_io::io_slot &io = b->hio.slot[sl];
    const size_t S = (size_t) b->n_streams;
    if (!io.pcm_rows) CHK(dev_alloc(b, &io.pcm_rows, S * (size_t) b->max_frames * 1152 * (size_t) b->channels * sizeof(int16_t)));
    if (!io.len_rows) CHK(dev_alloc(b, &io.len_rows, S * sizeof(uint32_t)));
    if (io.out_rows_cap < S * out_stride) { // (by hand, not dev_alloc: the one buffer that is freed before the batch is)
        if (io.out_rows) {
            CHK(io.out_free.sync());
            CHK(hipFree(io.out_rows));
            io.out_rows = NULL;
            io.out_rows_cap = 0;
        }
        CHK(hipMalloc((void **) &io.out_rows, S * out_stride));
        io.out_rows_cap = S * out_stride;
    }
    return MP3MI_OK;
}

// mp3mi_batch_encode_slots with host buffers that hold a row per LIVE slot: the arrays by row become arrays by slot (a slot no
// row names must be closed and stays so), the per-slot call's rules are checked on those, and the call runs as the per-slot
// call on the host-buffer copies of the batch, with the row map between the dense rows and the rows per slot (encode_impl).
extern "C" int mp3mi_batch_encode_slots_kbps_host_async(mp3mi_batch *b, const int16_t *pcm_host, int n_frames, int n_rows, const int32_t *row_slot_host,
                                                        const uint8_t *ctl_host, const int32_t *n_samples_host, const int32_t *kbps_host,
                                                        uint8_t *out_host, size_t out_stride, uint32_t *out_len_host)
{
    if (!b || !pcm_host || !ctl_host || !out_host || !out_len_host || n_frames <= 0 || n_frames > b->max_frames || feed_locked(b)) return MP3MI_ERR_ARG;
    const int S = b->n_streams;
    if (n_rows < 1 || n_rows > S || (!row_slot_host && n_rows != S)) return MP3MI_ERR_ARG;
    if (out_stride < mp3mi_batch_out_stride(b, n_frames)) return MP3MI_ERR_ARG;
    std::vector<int64_t> f((size_t) S);
    b->book.now(f.data());
    std::vector<uint8_t> ctl_s;
    std::vector<int32_t> ns_s, kbps_s;
    const uint8_t *ctl = ctl_host;
    const int32_t *ns = n_samples_host, *kbps = kbps_host;
    if (row_slot_host) {
        ctl_s.assign((size_t) S, 0);
        if (n_samples_host) ns_s.assign((size_t) S, 0);
        if (kbps_host) kbps_s.assign((size_t) S, 0);
        std::vector<char> named((size_t) S, 0);
        for (int r = 0; r < n_rows; r++) {
            const int32_t s = row_slot_host[r];
            if (s < 0 || s >= S || (r > 0 && s <= row_slot_host[r - 1])) return MP3MI_ERR_ARG;
            if (f[s] < 0 && !(ctl_host[r] & MP3MI_SLOT_START)) return MP3MI_ERR_ARG; // a row carries a stream: open or starting
            named[s] = 1;
            ctl_s[s] = ctl_host[r];
            if (n_samples_host) ns_s[s] = n_samples_host[r];
            if (kbps_host) kbps_s[s] = kbps_host[r];
        }
        for (int s = 0; s < S; s++)
            if (f[s] >= 0 && !named[s]) return MP3MI_ERR_ARG; // an open stream goes on (or ends) in every call
        ctl = ctl_s.data();
        ns = n_samples_host ? ns_s.data() : NULL;
        kbps = kbps_host ? kbps_s.data() : NULL;
    }
    if (!slots_rules_ok(b, f.data(), n_frames, ctl, ns, kbps)) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    mp3mi_batch::host_io &H = b->hio;
    const int sl = (int) (H.call_no & 1);
    if (host_io_init(b, sl) != MP3MI_OK) return MP3MI_ERR_HIP;
    if (host_io_harvest(b, sl) != MP3MI_OK) return MP3MI_ERR_HIP; // (waits for the call two before this one: at most two in flight)
    if (row_slot_host && host_rows_init(b, sl, out_stride) != MP3MI_OK) return MP3MI_ERR_HIP;
    host_call hc = {pcm_host, out_host, out_stride, out_len_host, sl, n_rows, row_slot_host, NULL};
    const int rc = slots_impl(b, H.slot[sl].pcm, n_frames, ctl, ns, kbps, H.slot[sl].out, H.out_stride, H.slot[sl].len, &hc);
    if (rc == MP3MI_OK) H.call_no++; // (a call that failed took no slot)
    return rc;
}

extern "C" int mp3mi_batch_encode_slots_host_async(mp3mi_batch *b, const int16_t *pcm_host, int n_frames, int n_rows, const int32_t *row_slot_host,
                                                   const uint8_t *ctl_host, const int32_t *n_samples_host, uint8_t *out_host, size_t out_stride,
                                                   uint32_t *out_len_host)
{
    return mp3mi_batch_encode_slots_kbps_host_async(b, pcm_host, n_frames, n_rows, row_slot_host, ctl_host, n_samples_host, NULL, out_host,
                                                    out_stride, out_len_host);
}

// Waits for the results of ONE host-buffer call: the latest (0) or the one before (1).  Only the call hold that very call left
// in force is let go -- a later call's stays, so a server collects tick t while tick t + 1 keeps its place in the pipeline.
extern "C" int mp3mi_batch_host_wait(mp3mi_batch *b, int calls_back)
{
    if (!b || calls_back < 0 || calls_back > 1) return MP3MI_ERR_ARG;
    mp3mi_batch::host_io &H = b->hio;
    if (!H.ready || H.call_no <= (unsigned) calls_back) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    const int sl = (int) ((H.call_no - 1u - (unsigned) calls_back) & 1u);
    if (b->held && H.slot[sl].hold_of == b->hold_seq) hold_release(b);
    CHK(hipEventSynchronize(H.slot[sl].t_dn[1]));
    return MP3MI_OK;
}

extern "C" int mp3mi_batch_host_io_stats(mp3mi_batch *b, mp3mi_host_io_stats *st)
{
    if (!b || !st) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    memset(st, 0, sizeof(*st));
    if (!b->hio.ready) return MP3MI_OK;
    hold_release(b);
    if (host_io_harvest(b, 0) != MP3MI_OK || host_io_harvest(b, 1) != MP3MI_OK) return MP3MI_ERR_HIP;
    st->calls = b->hio.tot_calls;
    st->h2d_bytes = b->hio.tot_up_bytes; st->d2h_bytes = b->hio.tot_dn_bytes;
    st->h2d_ms = b->hio.tot_up_ms; st->d2h_ms = b->hio.tot_dn_ms;
    return MP3MI_OK;
}

// page-locked host memory for the calls above (a caller that does not link HIP itself)
extern "C" void *mp3mi_host_alloc(size_t bytes)
{
    void *p = NULL;
    if (!have_device() || hipHostMalloc(&p, bytes, 0) != hipSuccess) return NULL;
    return p;
}
extern "C" void mp3mi_host_free(void *p) { if (p) (void) hipHostFree(p); }

static int encode_host_impl(int n_streams, int rate_hz, int channels, const int *kbps, int kbps_all, const int16_t *pcm,
                            const int32_t *n_samples, int n_frames, int hdr, uint8_t *out, size_t out_stride, uint32_t *out_len)
{
    mp3mi_batch *b = NULL;
    int rc = mp3mi_batch_create(&b, n_streams, rate_hz, channels, kbps, kbps_all, n_frames);
    if (rc != MP3MI_OK) return rc;
    if (hdr >= 0) rc = mp3mi_batch_set_header(b, (hdr >> 3) & 1, (hdr >> 2) & 1, hdr & 3);
    if (rc == MP3MI_OK && !n_samples) { // whole streams: the overlapped host path (pageable buffers here: staged by the runtime)
        rc = mp3mi_batch_encode_host_async(b, pcm, n_frames, out, out_stride, out_len);
        if (rc == MP3MI_OK) rc = mp3mi_batch_sync(b); // (MP3MI_ERR_REFERENCE_ABORT: done, the outputs are delivered -- mp3mi.h)
    } else if (rc == MP3MI_OK) { // a ragged batch: device copies of the call's buffers, freed before the batch goes
        const size_t S = (size_t) n_streams;
        hook_bufs D;
        int16_t *pcm_d = D.copy_of(pcm, S * (size_t) n_frames * 1152 * (size_t) channels);
        uint8_t *out_d = D.raw<uint8_t>(out_stride * S);
        uint32_t *len_d = D.raw<uint32_t>(S);
        int32_t *ns_d = D.copy_of(n_samples, S);
        rc = D.rc();
        if (rc == MP3MI_OK) rc = mp3mi_batch_encode_ragged(b, pcm_d, ns_d, n_frames, out_d, out_stride, len_d);
        if (rc == MP3MI_OK) rc = mp3mi_batch_sync(b);
        // MP3MI_ERR_REFERENCE_ABORT means "done, and some stream is an input the reference dies on": that stream's out_len is
        // 0 and every other stream's output is valid (mp3mi.h), so the results are delivered and the code is kept
        if ((rc == MP3MI_OK || rc == MP3MI_ERR_REFERENCE_ABORT) && !(D.fetch(out, out_d, out_stride * S) && D.fetch(out_len, len_d, S)))
            rc = MP3MI_ERR_HIP;
    }
    mp3mi_batch_destroy(b);
    return rc;
}

extern "C" int mp3mi_encode_host(int n_streams, int rate_hz, int channels, const int *kbps, int kbps_all,
                                 const int16_t *pcm, int n_frames, uint8_t *out, size_t out_stride,
                                 uint32_t *out_len)
{
    return encode_host_impl(n_streams, rate_hz, channels, kbps, kbps_all, pcm, NULL, n_frames, -1, out, out_stride, out_len);
}

extern "C" int mp3mi_encode_host_ex(int n_streams, int rate_hz, int channels, const int *kbps, int kbps_all,
                                    const int16_t *pcm, const int32_t *n_samples, int n_frames, int copyright,
                                    int original, int emphasis, uint8_t *out, size_t out_stride, uint32_t *out_len)
{
    if ((copyright & ~1) || (original & ~1) || (emphasis & ~3)) return MP3MI_ERR_ARG;
    return encode_host_impl(n_streams, rate_hz, channels, kbps, kbps_all, pcm, n_samples, n_frames,
                            (copyright << 3) | (original << 2) | emphasis, out, out_stride, out_len);
}

// ---- the feeder: a device FIFO per slot in front of the batch (mp3mi_feed_*) ----
#include "feed.h"
