/* Internal host-side declarations shared by the translation units of libmp3mi.so. */
#ifndef MP3MI_HOST_H
#define MP3MI_HOST_H

#include <stddef.h>
#include "mp3mi_dev.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tables_host.cpp: fill the table block for MPEG-1 sampling_frequency code rate_idx
 * (0 = 44.1 kHz, 1 = 48 kHz, 2 = 32 kHz).  Returns 0 on success. */
int mp3mi_build_tables(mp3mi_tables *T, int rate_idx);
/* hashes of the table members as this host builds them (test / pin generation; tables_host.cpp) */
int mp3mi_tables_digest(int rate_idx, uint64_t *hashes, const char **names, int cap);
/* the mirror identities of the 32 x 32 matrixing coefficients that k_filter's shared products rest on, bit for bit
 * (tables_host.cpp; every table build runs it, and mp3mi_build_tables reports a violation as -8 like a damaged blob): 0, or -14 */
int mp3mi_filt_mirror_check(const double *filt);

#ifdef __cplusplus
}

/* kernel launchers (one per .hip file); all take device pointers */
struct mp3mi_geom {
#if defined(MP3MI_ULP_CENSUS)
    size_t census_cb_stride; /* diagnostic build: the shadow sums of census site UC_CW_REACH sit this many floats (and twice as many) behind cb_all */
#endif
    int n_streams, channels, rate_idx;
    int n_frames;       /* frames per stream in this call (PCM extent = n_frames*1152 per channel) */
    int f0, nf;         /* frames [f0, f0+nf) form the current chunk */
    int g0, n_gran;     /* granules [g0, g0+n_gran) of the chunk: 2*f0, 2*nf for the batch path */
    int hdr_mode;       /* header mode field (src/common.h:233-236): 0 stereo, 2 dual, 3 mono */
    int hdr_flags;      /* bit 3 copyright, bit 2 original, bits 1-0 emphasis, bits 5-4 mode_ext */
    int crc;            /* error protection on: protection bit 0 and the 16-bit CRC word after the header -- which the
                           reference never computes for Layer III and writes as 0 (src/l3bitstream.c:312, 338-342); side
                           info grows by 16 bits (src/musicin.c:744-746) */
    const int32_t *n_samples; /* device, [n_streams]: valid samples per channel of each stream (ragged batch), or NULL: all n_frames*1152.
                                 Samples beyond it read as zero and frames beyond ceil(n/1152) are not encoded (src/encode.c:162-166) */
    /* streaming (mp3mi_batch_encode_next): the call continues streams that earlier calls began */
    long fabs0;         /* frames of every stream encoded by earlier calls = index of the call's first frame in its stream */
    const int16_t *hist; /* device, [n_streams][MP3MI_PCM_HIST][channels]: the samples before the call's first one (zeros at the
                           start of a stream), or NULL: nothing precedes the call */
    const int64_t *out_base; /* device, [n_streams]: file position of byte 0 of the stream's output row, or NULL: 0 */
    int whole_file;     /* the call is the whole stream: k_format also finishes the file (length incl. flush + close) */
    long pcm_pitch;     /* samples per channel in a stream's row of the PCM buffer; 0 = n_frames * 1152 (Layers I / II frames are
                           not 1152 samples: l12_batch.cpp sets it for k_filter) */
    int test_flags;     /* bit 0: k_loop takes the exact (sequential) noise sums only (MP3MI_NOISE_EXACT=1, tests);
                           bit 1: k_cw takes the correctly rounded atan2 only (MP3MI_PHASE_EXACT=1, tests);
                           bit 2: k_psy takes dm_log / dm_exp only (MP3MI_PSY_EXACT=1, tests);
                           bit 3: k_loop's quantiser takes the exact table search only (MP3MI_QUANT_EXACT=1, tests);
                           bit 4: k_cw takes the correctly rounded sines and cosines for every record (MP3MI_CW_EXACT=1, tests) */
    /* per-slot streaming (mp3mi_batch_encode_slots): streams of one batch begin and end in different calls */
    const int64_t *fabs_s;   /* device, [n_streams]: index of the call's first frame in the stream open in each slot, or NULL: fabs0 for all */
    const uint8_t *slot_ctl; /* device, [n_streams]: MP3MI_SLOT_* bits of the call, or NULL: every stream continues */
};
/* slot_ctl bits: the slot begins a stream with the call, ends it with the call, takes part in the call at all (a stream is open
   in it or begins); k_stream_tail leaves a slot without MP3MI_SLOT_DEV_ACTIVE alone */
#define MP3MI_SLOT_DEV_START 1
#define MP3MI_SLOT_DEV_END 2
#define MP3MI_SLOT_DEV_ACTIVE 4

static inline mp3mi_geom mp3mi_make_geom(int n_streams, int channels, int rate_idx, int n_frames, int f0, int nf)
{
    mp3mi_geom g;
    g.n_streams = n_streams; g.channels = channels; g.rate_idx = rate_idx; g.n_frames = n_frames;
    g.f0 = f0; g.nf = nf; g.g0 = 2 * f0; g.n_gran = 2 * nf;
    g.hdr_mode = (channels == 1) ? 3 : 0;
    g.hdr_flags = 0;
    g.crc = 0;
    g.fabs0 = 0; g.hist = NULL; g.out_base = NULL; g.whole_file = 1;
    g.test_flags = 0;
    g.pcm_pitch = 0;
    g.n_samples = NULL;
    g.fabs_s = NULL; g.slot_ctl = NULL;
#if defined(MP3MI_ULP_CENSUS)
    g.census_cb_stride = 0;
#endif
    return g;
}

/* records (granule, channel) of one launch at most: k_cw numbers 56 items a record in 32 bits (k_fft.hip); batch
 * creation refuses a chunk beyond it -- its per-chunk buffers would take more than a terabyte */
#define MP3MI_CW_MAX_REC ((size_t) 1 << 26)
void mp3mi_launch_fft(const mp3mi_tables *T, const mp3mi_geom &g, const int16_t *pcm,
                      float *energy_l, float *energy_s, float *bins, double *cw_mid, float *hist6, hipStream_t st, int which = 3);
/* records whose unpredictability needs its second tier (k_part lists them, k_cw_fix and k_part's second run work
 * through the list); device memory, mp3mi_cw_fixlist_bytes(records) */
struct mp3mi_cw_fixlist {
    unsigned count, cap, pad[2];
    unsigned list[1]; /* cap entries */
};
static inline size_t mp3mi_cw_fixlist_bytes(size_t n_rec) { return sizeof(mp3mi_cw_fixlist) + n_rec * sizeof(unsigned); }
void mp3mi_launch_cw_fix_reset(mp3mi_cw_fixlist *fix, unsigned cap, hipStream_t st);
void mp3mi_launch_cw_fix(const mp3mi_geom &g, const float *bins, double *cw_mid, float *hist6, const mp3mi_cw_fixlist *fix, hipStream_t st);
void mp3mi_launch_psy(const mp3mi_tables *T, const mp3mi_geom &g, const float *energy_l,
                      const float *energy_s, double *cw_mid, float *hist6, const float *bins, mp3mi_cw_fixlist *fix,
                      void *psy_state, double *eb_all, float *cb_all, mp3mi_psy_out *out, hipStream_t st, int which = 3);
/* the 32 new samples of a window_subband call, as a kernel argument (k_dropin.hip) */
struct mp3mi_dropin_samples { int16_t v[32]; };
void mp3mi_launch_filter(const mp3mi_tables *T, const mp3mi_geom &g, const int16_t *pcm, double *sbs, double *sb_dbg, hipStream_t st);
/* records whose loop-prep values k_mdct's tail could not decide (k_fbmdct.hip): k_prep works through the list;
 * device memory, mp3mi_prep_fixlist_bytes(records) */
struct mp3mi_prep_fixlist {
    unsigned count, pad[3];
    unsigned list[1]; /* one entry per record of a launch at most */
};
static inline size_t mp3mi_prep_fixlist_bytes(size_t n_rec) { return sizeof(mp3mi_prep_fixlist) + n_rec * sizeof(unsigned); }
/* prep / fix NULL: the spectrum only (fix->count is zeroed by the caller, on the same stream) */
void mp3mi_launch_mdct(const mp3mi_tables *T, const mp3mi_geom &g, const mp3mi_psy_out *psy, const double *sbs, double *xr,
                       mp3mi_loop_prep *prep, mp3mi_prep_fixlist *fix, hipStream_t st);
size_t mp3mi_sbs_bytes(const mp3mi_geom &g); /* subband samples between k_filter and k_mdct */
/* fix != NULL: the records it lists (a fixed small grid walks the list); NULL: every record of the launch */
void mp3mi_launch_prep(const mp3mi_tables *T, const mp3mi_geom &g, const double *xr,
                       const mp3mi_psy_out *psy, mp3mi_loop_prep *prep, const mp3mi_prep_fixlist *fix, int force_exact, hipStream_t st);
/* stream placement of k_loop (k_loop.hip: loop_place_stream); all pointers NULL = stream == blockIdx */
#define MP3MI_PLACE_KEYS 8192
struct mp3mi_loop_place {
    const int *order;      /* [n_streams] sorted position -> stream (k_rank) */
    int *cost;             /* [n_streams] cost of each stream in this launch (input of the next k_rank) */
    unsigned *taken;       /* [n_streams] zero before the launch */
    unsigned *simd_slots;  /* [MP3MI_PLACE_KEYS] zero before the launch: arrivals per SIMD */
    unsigned *simd_idx;    /* [MP3MI_PLACE_KEYS] zero before the launch: arrival ticket of the SIMD + 1 */
    unsigned *ticket, *scan; /* zero before the launch */
    int n_simd;            /* SIMDs of the device */
};
void mp3mi_launch_rank(const int *cost, int *order, int n, hipStream_t st);
void mp3mi_launch_loop(const mp3mi_tables *T, const mp3mi_geom &g, const double *xr,
                       const mp3mi_psy_out *psy, const mp3mi_loop_prep *prep, const int32_t *bits_per_frame,
                       void *loop_state, int16_t *ix, mp3mi_frame_side *side, unsigned *gate_count, mp3mi_loop_place place,
                       hipStream_t st);
/* bounded wait (one wavefront) until k_loop's start census reaches `target` -- see k_loop.hip */
int mp3mi_loop_resident(void);
void mp3mi_launch_gate(const unsigned *count, unsigned target, unsigned max_ticks, hipStream_t st);
void mp3mi_launch_hold(const unsigned *flag, unsigned ticket, unsigned max_ticks, hipStream_t st);
void mp3mi_launch_hold_release(unsigned *flag, unsigned ticket, hipStream_t st);
/* streaming plumbing around k_format (k_format.hip): the bytes of a stream that are not final yet -- the unfilled
   part of the bit reservoir's slots and the headers in between, at most MP3MI_CARRY_BYTES -- wait in `carry` */
#define MP3MI_CARRY_BYTES 2048
void mp3mi_launch_carry_in(int n_streams, const uint8_t *carry, const int32_t *carry_len, uint8_t *out, size_t out_stride, hipStream_t st);
/* what k_loop keeps of a stream between calls: the bit reservoir, the scfsi history and the region addresses */
typedef struct {
    int32_t ResvSize;
    int32_t sc_en_tot[2][2], sc_en[2][2][21], sc_xm[2][2][21], sc_xrmax[2][2];
    int32_t addr[2][2][3];
    int32_t ref_abort; /* 0, or MP3MI_DEV_ABORT_* | frame << 8 -- an input the reference dies on */
} mp3mi_loop_state;
static_assert(offsetof(mp3mi_loop_state, ref_abort) == sizeof(mp3mi_loop_state) - 4, "ref_abort is the last word: k_format and k_stream_tail find it there");
/* loop_state: the streams' mp3mi_loop_state records as words -- word 0 is ResvSize, the last word the
   stream's status (MP3MI_DEV_ABORT_*); voided: counts the streams whose file a call voided because of it */
void mp3mi_launch_stream_tail(const mp3mi_geom &g, int flush, int32_t *loop_state, int loop_state_words, const int32_t *bits_per_frame,
                              uint8_t *out, size_t out_stride, int64_t *out_base, uint8_t *carry, int32_t *carry_len, uint32_t *out_len,
                              unsigned *voided, hipStream_t st);
/* k_slot_begin: fresh state for the n_list slots of `list` (a call's MP3MI_SLOT_START slots): every region's record of each listed
   slot is zeroed -- bytes per slot a multiple of 4; regions with a NULL base are skipped */
struct mp3mi_slot_region { void *base; size_t bytes; };
void mp3mi_launch_slot_begin(const int32_t *list, int n_list, mp3mi_slot_region r0, mp3mi_slot_region r1, mp3mi_slot_region r2,
                             hipStream_t st);
/* k_slot_rate: bits_per_frame[list[i]] = bits[i], bitrate_index[list[i]] = index[i] for the n_list listed slots (the bitrates of the
   streams a call STARTs; list values are slots of the two live arrays, checked on the host) */
void mp3mi_launch_slot_rate(const int32_t *list, int n_list, const int32_t *bits, const int32_t *index, int32_t *bits_per_frame,
                            int32_t *bitrate_index, hipStream_t st);
/* k_slot_park: the listed slots' records of up to MP3MI_PARK_REGIONS regions to (to_state != 0) or from the caller's state
   records: record i, of list[i], at state + i * stride, region k of it at offset r[k].off (a multiple of 16; stride and state too).
   bytes: the region's record size per slot, a multiple of 4; a multiple of 16 moves as 16-byte accesses */
#define MP3MI_PARK_REGIONS 6
struct mp3mi_park_region { void *base; uint32_t bytes, off; };
struct mp3mi_park_table { mp3mi_park_region r[MP3MI_PARK_REGIONS]; int n; };
void mp3mi_launch_slot_park(const int32_t *list, int n_list, const mp3mi_park_table &t, void *state, size_t stride, int to_state, hipStream_t st);
/* per-slot streaming on host buffers: dense rows (one per live slot, row_slot[r] = its slot) to and from the rows per slot.
   k_rows_in: bytes [col0, col0 + width) of every dense PCM row into the same columns of its slot's row (all multiples of 16);
   k_rows_out: out_len[slot] bytes of every listed slot's output row and the length into dense rows of dense_stride, rest zeroed */
void mp3mi_launch_rows_in(const int32_t *row_slot, int n_rows, const int16_t *dense, int16_t *pcm, size_t pitch_bytes, size_t col0_bytes,
                          size_t width_bytes, hipStream_t st);
void mp3mi_launch_rows_out(const int32_t *row_slot, int n_rows, const uint8_t *out, size_t out_stride, const uint32_t *out_len, uint8_t *dense,
                           size_t dense_stride, uint32_t *dense_len, hipStream_t st);
/* k_feed (the feeder, mp3mi_feed_tick): per lane one descriptor of four uint32 {head, pending, n_push, take}, checked on the host
   (head < cap, pending + n_push <= cap, take <= pending + n_push, take samples fit a row, n_push samples lie in the push row).  The
   first `take` samples of ring[head .. head + pending) (wrapping at cap) ++ push[0 .. n_push) go to the lane's row; the pushed
   samples behind them are appended to the ring at their place in that stream.  Pitches in bytes; rings and rows 16-byte aligned
   with pitches that are multiples of 16; most_bytes: the longest copy of any lane (sizes the workgroups per lane) */
void mp3mi_launch_feed(const void *desc, int n_lanes, int16_t *ring, size_t ring_pitch_bytes, int cap, int channels, const int16_t *push,
                       size_t push_pitch_bytes, int16_t *rows, size_t row_pitch_bytes, size_t most_bytes, hipStream_t st);
/* k_feed_lanes (mp3mi_feed_tick_lanes): k_feed over the n_active lanes that move in a tick.  Per entry a descriptor of eight uint32
   {head, pending, n_push, take, lane, push_row, slot, 0}: the ring is ring + lane * pitch, the push row push + push_row * pitch, the
   row that is cut rows + slot * pitch (unused when take is 0).  The rules of k_feed per descriptor, and no lane, no slot of a
   taking entry and no push row of a pushing entry twice in a launch: checked on the host */
void mp3mi_launch_feed_lanes(const void *desc, int n_active, int16_t *ring, size_t ring_pitch_bytes, int cap, int channels, const int16_t *push,
                             size_t push_pitch_bytes, int16_t *rows, size_t row_pitch_bytes, size_t most_bytes, hipStream_t st);
/* k_feed_packed (mp3mi_feed_tick_lanes_host_async): k_feed_lanes on a PACKED push buffer and over a WORK LIST.  Word 5 of a
   descriptor is the push's first sample (of all channels) in `packed`, so a push begins at any even byte; the grid is 1-D over
   n_items work items of two uint32 {descriptor index, part | parts << 16}: workgroup `part` of the `parts` that share the
   descriptor's copies.  mp3mi_feed_work_list builds the list: a descriptor gets ceil(its longest copy / wg_bytes) workgroups, at
   least 1 and at most MP3MI_FEED_MAX_PARTS, whatever the other descriptors of the launch move.  work: room for
   2 * MP3MI_FEED_MAX_PARTS * n_active words; returns the items.  The product's wg_bytes is MP3MI_FEED_WG_BYTES */
#define MP3MI_FEED_MAX_PARTS 8
#define MP3MI_FEED_WG_BYTES ((size_t) 256 * 16 * 4) /* four stores per lane of the longest copy, as k_feed's grid */
static inline size_t mp3mi_feed_work_list(const uint32_t *desc, size_t n_active, size_t esz, size_t wg_bytes, uint32_t *work)
{
    size_t n_items = 0;
    for (size_t i = 0; i < n_active; i++) {
        const uint32_t n_push = desc[8 * i + 2], take = desc[8 * i + 3];
        const size_t longest = (size_t) (take > n_push ? take : n_push) * esz;
        size_t parts = (longest + wg_bytes - 1) / wg_bytes;
        parts = parts < 1 ? 1 : parts > MP3MI_FEED_MAX_PARTS ? MP3MI_FEED_MAX_PARTS : parts;
        for (size_t p = 0; p < parts; p++) {
            work[2 * n_items] = (uint32_t) i;
            work[2 * n_items + 1] = (uint32_t) (p | parts << 16);
            n_items++;
        }
    }
    return n_items;
}
void mp3mi_launch_feed_packed(const void *desc, const void *work, int n_items, int16_t *ring, size_t ring_pitch_bytes, int cap, int channels,
                              const int16_t *packed, int16_t *rows, size_t row_pitch_bytes, hipStream_t st);
/* k12_feed (mp3mi_l12_feed_tick): k_feed_lanes for Layers I and II, whose rings keep history.  A descriptor's word 7 is 0, or
   MP3MI_L12_FEED_RESUME | n_hist: then the kernel also writes rows `slot` of hist_a ([n_slots][len_a][channels]) and hist_b
   ([n_slots][len_b][channels], len_b <= len_a) -- the n_hist <= len_a samples before head with zeros in front, and the last len_b
   of the same.  All n_push samples are appended at (head + pending) % cap.  The rules of k_feed_lanes per descriptor and launch,
   with len_a + pending + n_push <= cap in place of pending + n_push <= cap: checked on the host.  most_bytes counts a resuming
   descriptor's len_a samples too */
#define MP3MI_L12_FEED_RESUME 0x80000000u
void mp3mi_launch_l12_feed(const void *desc, int n_active, int16_t *ring, size_t ring_pitch_bytes, int cap, int channels, const int16_t *push,
                           size_t push_pitch_bytes, int16_t *rows, size_t row_pitch_bytes, int16_t *hist_a, int len_a, int16_t *hist_b, int len_b,
                           size_t most_bytes, hipStream_t st);
/* status[s] = the status word of stream s (a gather out of the strided state records) */
void mp3mi_launch_status_gather(int n_streams, const int32_t *loop_state, int loop_state_words, int32_t *status, hipStream_t st);
/* the reverse, for the streams a flush ended: their status words go back into the cleared state records, marked as reported */
void mp3mi_launch_status_scatter(int n_streams, int32_t *loop_state, int loop_state_words, const int32_t *status, hipStream_t st);
void mp3mi_launch_hist_save(const mp3mi_geom &g, const int16_t *pcm, int16_t *hist, hipStream_t st);
/* loop_state / voided as for mp3mi_launch_stream_tail (a whole-file call ends the streams in k_format); NULL: no status */
void mp3mi_launch_format(const mp3mi_tables *T, const mp3mi_geom &g, const int16_t *ix,
                         const mp3mi_frame_side *side, const int32_t *bits_per_frame,
                         const int32_t *bitrate_index, uint8_t *out, size_t out_stride,
                         uint32_t *out_len, int32_t *loop_state, int loop_state_words, unsigned *voided, hipStream_t st);
/* Compute units of the CURRENT device (launch geometry of the persistent kernels).  Asked per call: batches of
   several devices may be driven from one process, by several threads (mp3mi.h, "Threads") -- no cached static. */
static inline int mp3mi_current_cu_count(void)
{
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    return n;
}
#endif

#endif
