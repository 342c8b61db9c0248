// Host side of the Layer I / II batch (include/mp3mi_l12.h): set-up as the reference's driver does it
// (src/musicin.c:528-581, src/common.c:291-347), scratch sizing, and one pipeline of kernels per chunk of frames:
//
//   k_fft12 -> k12_psy ;  k_filter ;  k12_alloc
//
// Frames are independent but for PCM history (l12_dev.h), so a chunk is just these four launches in stream order, and
// chunks follow each other on the batch's one HIP stream.  A per-slot call (mp3mi_l12_batch_encode_slots) puts its control block's
// upload and k12_slot_begin ahead of them on the same stream -- and k12_slot_rate, where a stream begins at another bitrate than its
// slot's (mp3mi_l12_batch_encode_slots_kbps); an export or an import (mp3mi_l12_batch_slots_export / _import) is a slot list's upload
// and one k12_slot_park there.  No CPU fallback.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "l12_host.h"
#include "mp3mi_l12.h"

static void l12_feed_drop(mp3mi_l12_feed *f); // (l12_feed.h, at the end of this file)

struct mp3mi_l12_batch {
    int device;
    int layer, n_streams, rate_idx, rate_hz, channels, max_frames, chunk_frames;
    int spf, spp, span, lb;
    int mode, crc, hdr_flags;
    unsigned test_flags;
    int debug;
    int max_frame_bytes;     // of the longest frame in an output row (l12_row_frame_bytes)
    std::vector<l12_stream_cfg> cfg_h; // as created
    // A bitrate per stream (mp3mi_l12_batch_encode_slots_kbps): kbps_h the slots' create-time bitrates and ceil_kbps the largest of
    // them; slot_kbps_h the bitrate of the stream open in each slot, kbps_h[s] where none is; dev_kbps_h the bitrate the device's
    // cfg[s] stands at.  cfg[s] is what slot_kbps_h says wherever a stream is open; elsewhere it may lag (rate_dirty: somewhere
    // dev_kbps_h differs from kbps_h) and is put right, by k12_slot_rate, where a stream next begins there.
    std::vector<int32_t> kbps_h, slot_kbps_h, dev_kbps_h;
    int ceil_kbps;
    bool rate_dirty;
    hipStream_t stream;
    hipEvent_t ev0, ev1;
    std::vector<hipEvent_t> kev; // five per chunk of the last call: around the four launches
    int kev_chunks;
    double kernel_ms[4];
    long kernel_launches[4];
    bool timing_open;
    double total_ms;
    long calls;
    mp3mi_tables *T3;          // window, FFT program, filterbank tables (shared with Layer III)
    mp3mi_tables_l12 *T;
    l12_stream_cfg *cfg;
    float *erp, *snr;
    double *sbs;
    l12_frame_dbg *dbg;
    int dbg_f0, dbg_nf;
    // streaming: PCM history of the streams in progress, two copies taken in turn (k12_hist_save is out of place)
    int16_t *hist[2], *fb_hist[2];
    int hist_cur;
    // where the streams are: the whole-batch counter of mp3mi_l12_batch_encode_next (book.frames_all: frames every stream has been
    // given since the last reset) and the slots of mp3mi_l12_batch_encode_slots (host_util.h)
    slot_book book;
    // the control block of a per-slot call (l12_ctl_block), twice, taken in turn: calls are issued back to back, and an entry's
    // fence is recorded behind the last kernel that reads its device copy -- the host waits for it before it writes the staging
    // again (the per-slot call two before).  Created with the first per-slot call: a batch that never makes one holds none of it.
    // An entry also carries the slot list of a park (mp3mi_l12_batch_slots_export / _import) and, behind the block, the entries
    // of k12_slot_rate (l12_rate_at) -- that part only from the first turn that needs it (ctl_cap: bytes an entry has).
    typedef upload_ring<uint8_t, 2> ctl_ring;
    ctl_ring ctl;
    size_t ctl_cap[2];
    // the feeder attached to the batch (mp3mi_l12_feed_create; l12_feed.h), NULL: none.  While one is, the batch's streams are the
    // feeder's: the calls that begin, move or end streams, or change what a frame's header says, are the feeder's alone (feed_call:
    // the call comes from it)
    mp3mi_l12_feed *feed;
    bool feed_call;
};
// A call the caller may not make while a feeder is attached
static inline bool l12_feeders_call(const mp3mi_l12_batch *b) { return b && b->feed && !b->feed_call; }

// The control block of a per-slot call, one array per slot after the other: what the kernels read of it (l12_geom) and the list of
// the slots the call STARTs (k12_slot_begin)
struct l12_ctl_block {
    int64_t *fabs;      // index of the call's first frame in the slot's stream
    int32_t *n_samples; // valid samples per channel
    int32_t *list;      // the START slots, n_start of them
    uint8_t *ctl;       // MP3MI_SLOT_DEV_*
};
static size_t l12_ctl_bytes(int S) { return (size_t) S * (sizeof(int64_t) + 2 * sizeof(int32_t) + 1); }
static l12_ctl_block l12_ctl_at(uint8_t *p, int S)
{
    l12_ctl_block c;
    c.fabs = (int64_t *) p;
    c.n_samples = (int32_t *) (c.fabs + S);
    c.list = c.n_samples + S;
    c.ctl = (uint8_t *) (c.list + S);
    return c;
}
// Behind the control block, at a multiple of 16 bytes: what k12_slot_rate reads, room for an entry per slot
static size_t l12_rate_off(int S) { return (l12_ctl_bytes(S) + 15) / 16 * 16; }
static size_t l12_rate_bytes(int S) { return (size_t) S * sizeof(l12_rate_entry); }
static l12_rate_entry *l12_rate_at(uint8_t *p, int S) { return (l12_rate_entry *) (p + l12_rate_off(S)); }
static void l12_rate_set(l12_rate_entry *e, int slot, const l12_stream_cfg &c)
{
    memset(e, 0, sizeof(*e));
    e->cfg = c;
    e->slot = slot;
}
struct l12_slot_call { // a per-slot call: its control block on the device, and the ring entry it took
    l12_ctl_block dev;
    int n_start;
    int n_rate;         // slots whose cfg the call writes first (l12_rate_at of the entry)
    mp3mi_l12_batch::ctl_ring::entry *blk;
};

static size_t l12_per_frame_bytes(int layer, int channels, int spf)
{
    const size_t rec = (size_t) 3 * L12_ROW * sizeof(float) + 32 * sizeof(float);
    return (size_t) layer * channels * rec + (size_t) spf * 8 * channels;
}

extern "C" int mp3mi_l12_batch_create(mp3mi_l12_batch **out, int layer, int n_streams, int rate_hz, int channels,
                                      const int *kbps, int kbps_all, int max_frames, unsigned scratch_mb)
{
    if (!out) return MP3MI_ERR_ARG;
    *out = NULL;
    if ((layer != 1 && layer != 2) || n_streams < 1 || max_frames < 1 || (channels != 1 && channels != 2)) return MP3MI_ERR_ARG;
    const int ri = rate_idx_of(rate_hz);
    if (ri < 0) return MP3MI_ERR_ARG;
    if (!have_device()) {
        fprintf(stderr, "mp3mi: no usable HIP device -- this library has no CPU fallback\n");
        return MP3MI_ERR_NO_DEVICE;
    }
    mp3mi_l12_batch *b = new mp3mi_l12_batch();
    memset((void *) &b->stream, 0, sizeof(b->stream));
    b->layer = layer; b->n_streams = n_streams; b->rate_idx = ri; b->rate_hz = rate_hz; b->channels = channels;
    b->max_frames = max_frames;
    b->spf = l12_samples_per_frame(layer); b->spp = layer == 1 ? 384 : 576; b->span = layer == 1 ? 1024 : 1056;
    b->lb = layer == 1 ? 3 : 2;
    b->mode = channels == 1 ? MP3MI_MODE_MONO : MP3MI_MODE_STEREO;
    b->crc = 0; b->hdr_flags = 0; b->test_flags = 0; b->debug = 0;
    b->timing_open = false; b->total_ms = 0.0; b->calls = 0; b->kev_chunks = 0;
    for (int i = 0; i < 4; i++) { b->kernel_ms[i] = 0.0; b->kernel_launches[i] = 0; }
    b->ev0 = b->ev1 = 0; b->T3 = NULL; b->T = NULL; b->cfg = NULL;
    b->erp = b->snr = NULL; b->sbs = NULL; b->dbg = NULL; b->dbg_f0 = b->dbg_nf = 0;
    b->hist[0] = b->hist[1] = b->fb_hist[0] = b->fb_hist[1] = NULL; b->hist_cur = 0;
    b->book.init(n_streams);
    memset((void *) &b->ctl, 0, sizeof(b->ctl));
    b->ctl_cap[0] = b->ctl_cap[1] = 0;
    b->ceil_kbps = 0; b->rate_dirty = false;
    b->feed = NULL; b->feed_call = false;
    if (hipGetDevice(&b->device) != hipSuccess) { delete b; return MP3MI_ERR_HIP; }
    b->cfg_h.resize((size_t) n_streams);
    b->max_frame_bytes = 0;
    for (int s = 0; s < n_streams; s++) {
        l12_stream_cfg &c = b->cfg_h[(size_t) s];
        if (!l12_stream_cfg_of(layer, rate_hz, ri, channels, kbps ? kbps[s] : kbps_all, &c)) { delete b; return MP3MI_ERR_ARG; }
        const int fb = (int) l12_row_frame_bytes(layer, channels, c.frame_bits);
        if (fb > b->max_frame_bytes) b->max_frame_bytes = fb;
        b->kbps_h.push_back(kbps ? kbps[s] : kbps_all);
        if (b->kbps_h.back() > b->ceil_kbps) b->ceil_kbps = b->kbps_h.back();
    }
    b->slot_kbps_h = b->kbps_h;
    b->dev_kbps_h = b->kbps_h;
    const size_t budget = (size_t) (scratch_mb ? scratch_mb : 32768u) << 20;
    // per stream the chunk's buffers also hold the lb warm-up passes and three extra filterbank granules, whatever its length
    const size_t per_stream_fixed = (size_t) b->lb * channels * ((size_t) 3 * L12_ROW * sizeof(float) + 32 * sizeof(float)) + (size_t) 4 * channels * 576 * sizeof(double);
    const size_t per_stream_budget = budget / (size_t) n_streams;
    long cf = per_stream_budget > per_stream_fixed ? (long) ((per_stream_budget - per_stream_fixed) / l12_per_frame_bytes(layer, channels, b->spf)) : 1;
    if (cf < 1) cf = 1;
    if (cf > max_frames) cf = max_frames;
    b->chunk_frames = (int) cf;

    int rc = MP3MI_OK;
    auto build = [&]() -> int {
        std::vector<char> t3_store(sizeof(mp3mi_tables)), t12_store(sizeof(mp3mi_tables_l12));
        mp3mi_tables *T3h = (mp3mi_tables *) t3_store.data();
        mp3mi_tables_l12 *T12h = (mp3mi_tables_l12 *) t12_store.data();
        int trc = tables_rc(mp3mi_build_tables(T3h, ri));
        if (trc == MP3MI_OK) trc = tables_rc(mp3mi_build_tables_l12(T12h, ri, layer));
        if (trc != MP3MI_OK) return trc;
        for (int s = 0; s < n_streams; s++)
            if (layer == 2 && b->cfg_h[(size_t) s].sblimit != T12h->sblimit[b->cfg_h[(size_t) s].table]) return MP3MI_ERR_TABLES;
        CHK(hipStreamCreate(&b->stream));
        CHK(hipEventCreate(&b->ev0));
        CHK(hipEventCreate(&b->ev1));
        CHK(hipMalloc((void **) &b->T3, sizeof(mp3mi_tables)));
        CHK(hipMalloc((void **) &b->T, sizeof(mp3mi_tables_l12)));
        CHK(hipMalloc((void **) &b->cfg, sizeof(l12_stream_cfg) * (size_t) n_streams));
        CHK(hipMemcpy(b->T3, T3h, sizeof(mp3mi_tables), hipMemcpyHostToDevice));
        CHK(hipMemcpy(b->T, T12h, sizeof(mp3mi_tables_l12), hipMemcpyHostToDevice));
        CHK(hipMemcpy(b->cfg, b->cfg_h.data(), sizeof(l12_stream_cfg) * (size_t) n_streams, hipMemcpyHostToDevice));
        const size_t np = (size_t) cf * layer + (size_t) b->lb, nrec = (size_t) n_streams * np * (size_t) channels;
        const size_t ngran = ((size_t) cf * (size_t) (b->spf / 32) + 17) / 18 + 3; // granules of 18 slots k_filter may be asked for
        CHK(hipMalloc((void **) &b->erp, nrec * 3 * L12_ROW * sizeof(float)));
        CHK(hipMalloc((void **) &b->snr, nrec * 32 * sizeof(float)));
        CHK(hipMalloc((void **) &b->sbs, (size_t) n_streams * ngran * (size_t) channels * 576 * sizeof(double)));
        return MP3MI_OK;
    };
    rc = build();
    if (rc != MP3MI_OK) { mp3mi_l12_batch_destroy(b); return rc; }
    *out = b;
    return MP3MI_OK;
}

extern "C" void mp3mi_l12_batch_destroy(mp3mi_l12_batch *b)
{
    if (!b) return;
    {
        device_scope sc(b->device);
        if (b->stream) (void) hipStreamSynchronize(b->stream);
        if (b->feed) l12_feed_drop(b->feed); // (a batch that goes with its feeder attached)
        (void) hipFree(b->T3); (void) hipFree(b->T); (void) hipFree(b->cfg); (void) hipFree(b->erp);
        (void) hipFree(b->snr); (void) hipFree(b->sbs); (void) hipFree(b->dbg);
        for (int i = 0; i < 2; i++) { (void) hipFree(b->hist[i]); (void) hipFree(b->fb_hist[i]); }
        for (mp3mi_l12_batch::ctl_ring::entry &en : b->ctl.e) {
            if (en.stage) (void) hipHostFree(en.stage);
            (void) hipFree(en.dev);
            en.free.destroy();
        }
        if (b->ev0) (void) hipEventDestroy(b->ev0);
        if (b->ev1) (void) hipEventDestroy(b->ev1);
        for (hipEvent_t e : b->kev) (void) hipEventDestroy(e);
        if (b->stream) (void) hipStreamDestroy(b->stream);
    }
    delete b;
}

extern "C" int mp3mi_l12_batch_set_mode(mp3mi_l12_batch *b, int mode)
{
    if (!b || mode < 0 || mode > 3 || l12_feeders_call(b)) return MP3MI_ERR_ARG;
    if ((b->channels == 1) != (mode == MP3MI_MODE_MONO)) return MP3MI_ERR_ARG;
    b->mode = mode;
    return MP3MI_OK;
}
extern "C" int mp3mi_l12_batch_set_error_protection(mp3mi_l12_batch *b, int on)
{
    if (!b || l12_feeders_call(b)) return MP3MI_ERR_ARG;
    b->crc = on != 0;
    return MP3MI_OK;
}
extern "C" int mp3mi_l12_batch_set_header(mp3mi_l12_batch *b, int copyright, int original, int emphasis)
{
    if (!b || emphasis < 0 || emphasis > 3 || l12_feeders_call(b)) return MP3MI_ERR_ARG;
    b->hdr_flags = ((copyright != 0) << 3) | ((original != 0) << 2) | emphasis;
    return MP3MI_OK;
}
extern "C" int mp3mi_l12_batch_set_test_flags(mp3mi_l12_batch *b, unsigned flags)
{
    if (!b) return MP3MI_ERR_ARG;
    b->test_flags = flags;
    return MP3MI_OK;
}
extern "C" size_t mp3mi_l12_batch_out_stride(const mp3mi_l12_batch *b, int n_frames)
{
    if (!b || n_frames < 0) return 0;
    return ((size_t) n_frames * (size_t) b->max_frame_bytes + 1 + 255) / 256 * 256;
}
extern "C" void mp3mi_l12_batch_debug_enable(mp3mi_l12_batch *b, int on) { if (b) b->debug = on != 0; }

static int l12_close_timing(mp3mi_l12_batch *b)
{
    if (!b->timing_open) return MP3MI_OK;
    float ms = 0.0f;
    CHK(hipEventSynchronize(b->ev1));
    CHK(hipEventElapsedTime(&ms, b->ev0, b->ev1));
    b->total_ms += (double) ms;
    for (int c = 0; c < b->kev_chunks; c++)
        for (int k = 0; k < 4; k++) {
            CHK(hipEventElapsedTime(&ms, b->kev[(size_t) c * 5 + k], b->kev[(size_t) c * 5 + k + 1]));
            b->kernel_ms[k] += (double) ms;
            b->kernel_launches[k]++;
        }
    b->kev_chunks = 0;
    b->timing_open = false;
    return MP3MI_OK;
}

// The PCM history of a streaming batch: allocated and zeroed with the first streaming call
static int l12_hist_ensure(mp3mi_l12_batch *b)
{
    const size_t S = (size_t) b->n_streams, C = (size_t) b->channels;
    for (int i = 0; i < 2; i++) {
        if (b->hist[i] && b->fb_hist[i]) continue;
        if (!b->hist[i]) CHK(hipMalloc((void **) &b->hist[i], sizeof(int16_t) * L12_PCM_HIST * C * S));
        if (!b->fb_hist[i]) CHK(hipMalloc((void **) &b->fb_hist[i], sizeof(int16_t) * MP3MI_PCM_HIST * C * S));
        CHK(hipMemsetAsync(b->hist[i], 0, sizeof(int16_t) * L12_PCM_HIST * C * S, b->stream));
        CHK(hipMemsetAsync(b->fb_hist[i], 0, sizeof(int16_t) * MP3MI_PCM_HIST * C * S, b->stream));
    }
    return MP3MI_OK;
}

// The control block this call takes, its entry created with its first turn; the host waits for the per-slot call two before,
// whose kernels read the device copy and whose upload read the staging it is about to write.  with_rates: the turn needs room for
// the entry's rate entries too (l12_rate_at) -- an entry that was created without is created anew, once its readers are through
static int l12_ctl_take(mp3mi_l12_batch *b, mp3mi_l12_batch::ctl_ring::entry **blk, bool with_rates = false)
{
    mp3mi_l12_batch::ctl_ring::entry &en = b->ctl.take();
    size_t &cap = b->ctl_cap[b->ctl.calls % 2u];
    const size_t bytes = with_rates ? l12_rate_off(b->n_streams) + l12_rate_bytes(b->n_streams) : l12_ctl_bytes(b->n_streams);
    if (!en.free.ev) CHK(en.free.create());
    CHK(en.free.sync());
    if (cap < bytes) {
        if (en.stage) CHK(hipHostFree(en.stage));
        en.stage = NULL;
        CHK(hipFree(en.dev));
        en.dev = NULL;
        cap = 0;
        CHK(hipHostMalloc((void **) &en.stage, bytes, 0));
        CHK(hipMalloc((void **) &en.dev, bytes));
        cap = bytes;
    }
    *blk = &en;
    return MP3MI_OK;
}

// The n_rate rate entries of a turn go up and k12_slot_rate writes cfg from them: on the batch's stream, ahead of the k12_alloc that
// follows
static int l12_rates_write(mp3mi_l12_batch *b, mp3mi_l12_batch::ctl_ring::entry *blk, int n_rate)
{
    const int S = b->n_streams;
    CHK(hipMemcpyAsync(l12_rate_at(blk->dev, S), l12_rate_at(blk->stage, S), sizeof(l12_rate_entry) * (size_t) n_rate, hipMemcpyHostToDevice, b->stream));
    mp3mi_launch_l12_slot_rate(l12_rate_at(blk->dev, S), n_rate, b->cfg, b->stream);
    CHK(hipGetLastError());
    return MP3MI_OK;
}

// Every stream is over: the slots are closed and at their create-time bitrates again (cfg follows where streams next begin)
static void l12_streams_over(mp3mi_l12_batch *b)
{
    b->book.close();
    if (b->rate_dirty) b->slot_kbps_h = b->kbps_h;
}

// Every stream starts afresh (a whole-file call, an encode_next with no stream open), at its slot's create-time bitrate: cfg goes
// back to it where it stands at another -- those slots alone, in a turn of the control ring of its own.  A batch that never saw
// another bitrate does nothing here.
static int l12_rates_restore(mp3mi_l12_batch *b)
{
    if (!b->rate_dirty) return MP3MI_OK;
    const int S = b->n_streams;
    mp3mi_l12_batch::ctl_ring::entry *blk;
    { const int rc = l12_ctl_take(b, &blk, true); if (rc != MP3MI_OK) return rc; }
    l12_rate_entry *st = l12_rate_at(blk->stage, S);
    int n = 0;
    for (int s = 0; s < S; s++)
        if (b->dev_kbps_h[(size_t) s] != b->kbps_h[(size_t) s]) l12_rate_set(&st[n++], s, b->cfg_h[(size_t) s]);
    { const int rc = l12_rates_write(b, blk, n); if (rc != MP3MI_OK) return rc; }
    CHK(blk->free.record(b->stream));
    b->ctl.next();
    b->dev_kbps_h = b->kbps_h;
    b->slot_kbps_h = b->kbps_h;
    b->rate_dirty = false;
    return MP3MI_OK;
}

// sc: the call is a per-slot one (l12_slots_impl), its control block written to the staging of sc->blk
static int l12_encode_impl(mp3mi_l12_batch *b, const int16_t *pcm_dev, const int32_t *n_samples_dev, int n_frames,
                           uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev, bool whole_file, const l12_slot_call *sc = NULL)
{
    if (!b || !pcm_dev || !out_dev || !out_len_dev || n_frames < 1 || n_frames > b->max_frames || l12_feeders_call(b)) return MP3MI_ERR_ARG;
    if (out_stride < mp3mi_l12_batch_out_stride(b, n_frames)) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    { const int rc = l12_close_timing(b); if (rc != MP3MI_OK) return rc; }
    const int S = b->n_streams, C = b->channels, layer = b->layer;
    if (b->debug && !b->dbg) CHK(hipMalloc((void **) &b->dbg, sizeof(l12_frame_dbg) * (size_t) S * (size_t) b->chunk_frames));
    CHK(hipEventRecord(b->ev0, b->stream));
    CHK(grow_events(b->kev, 5 * (size_t) ((n_frames + b->chunk_frames - 1) / b->chunk_frames), 0));
    // equal chunks (as batch.cpp cuts a Layer III call): a short remainder -- 191 + 191 + 1 frames of the 383-frame bench call --
    // costs four full launches over all streams and recomputes the warm-up passes for one frame
    const int nchunks = (n_frames + b->chunk_frames - 1) / b->chunk_frames, cfr = (n_frames + nchunks - 1) / nchunks;
    if (!sc && (whole_file || b->book.frames_all == 0)) { const int rc = l12_rates_restore(b); if (rc != MP3MI_OK) return rc; }
    if (sc) {
        // the control block goes up on the batch's one stream, ahead of its readers; the slots that START begin from silence
        { const int rc = l12_hist_ensure(b); if (rc != MP3MI_OK) return rc; }
        CHK(hipMemcpyAsync(sc->blk->dev, sc->blk->stage, l12_ctl_bytes(S), hipMemcpyHostToDevice, b->stream));
        if (sc->n_rate > 0) { const int rc = l12_rates_write(b, sc->blk, sc->n_rate); if (rc != MP3MI_OK) return rc; }
        mp3mi_launch_l12_slot_begin(sc->dev.list, sc->n_start, C, b->hist[b->hist_cur], b->fb_hist[b->hist_cur], b->stream);
    }
    int chunk = 0;
    for (int f0 = 0; f0 < n_frames; f0 += cfr, chunk++) {
        hipEvent_t *ke = &b->kev[(size_t) chunk * 5];
        const int nf = n_frames - f0 < cfr ? n_frames - f0 : cfr;
        l12_geom g;
        memset(&g, 0, sizeof(g));
        g.n_streams = S; g.channels = C; g.layer = layer; g.rate_idx = b->rate_idx;
        g.n_frames = n_frames; g.f0 = f0; g.nf = nf;
        g.lb = b->lb; g.np = nf * layer + b->lb;
        g.spf = b->spf; g.spp = b->spp; g.span = b->span;
        g.actual_mode = b->mode; g.crc = b->crc; g.hdr_flags = b->hdr_flags; g.test_flags = (int) b->test_flags;
        g.n_samples = sc ? sc->dev.n_samples : n_samples_dev;
        g.whole_file = whole_file ? 1 : 0;
        g.fabs0 = (whole_file || sc) ? 0 : b->book.frames_all;
        g.hist = (!whole_file && b->book.frames_all > 0) ? b->hist[b->hist_cur] : NULL; // (nothing precedes a stream's first call: zeros)
        if (sc) { // every slot has its own position, and always a history: k12_slot_begin has zeroed the rows of the streams that begin
            g.fabs_s = sc->dev.fabs;
            g.slot_ctl = sc->dev.ctl;
            g.hist = b->hist[b->hist_cur];
        }
        // the filterbank slots of the chunk: frame f's slot u is slot (spf / 32) f + u of the stream, Layer I's two slots
        // EARLIER (get_audio holds 64 samples back, src/encode.c:224-247); k_filter computes whole 18-slot granules
        const long slots = b->spf / 32, first = slots * f0 - (layer == 1 ? 2 : 0), last = slots * (f0 + nf) - 1 - (layer == 1 ? 2 : 0);
        const long gf = first >= 0 ? first / 18 : -((-first + 17) / 18), gl = last >= 0 ? last / 18 : -((-last + 17) / 18);
        g.g0 = (int) gf + 1;                 // granule g0 - 1 is "granule slot 0" of k_filter
        g.n_gran = (int) (gl - gf);          // granules [g0, g0 + n_gran) follow it
        g.slot0 = (int) (first - 18 * gf);
        mp3mi_geom fg = mp3mi_make_geom(S, C, b->rate_idx, n_frames, f0, nf);
        fg.g0 = g.g0; fg.n_gran = g.n_gran;
        fg.pcm_pitch = (long) n_frames * b->spf;
        fg.n_samples = g.n_samples;
        fg.fabs0 = g.fabs0;
        fg.fabs_s = g.fabs_s;
        fg.hist = g.hist ? b->fb_hist[b->hist_cur] : NULL;
        CHK(hipEventRecord(ke[0], b->stream));
        mp3mi_launch_fft12(b->T3, g, pcm_dev, b->erp, b->stream);
        CHK(hipEventRecord(ke[1], b->stream));
        mp3mi_launch_l12_psy(b->T, g, b->erp, b->snr, b->stream);
        CHK(hipEventRecord(ke[2], b->stream));
        mp3mi_launch_filter(b->T3, fg, pcm_dev, b->sbs, NULL, b->stream);
        CHK(hipEventRecord(ke[3], b->stream));
        mp3mi_launch_l12_alloc(b->T, g, b->cfg, b->sbs, b->snr, out_dev, out_stride, out_len_dev, b->debug ? b->dbg : NULL, b->stream);
        CHK(hipEventRecord(ke[4], b->stream));
        b->dbg_f0 = f0; b->dbg_nf = nf;
    }
    if (!whole_file) { // the samples the next call will need from before its first
        l12_geom g;
        memset(&g, 0, sizeof(g));
        g.n_streams = S; g.channels = C; g.n_frames = n_frames; g.spf = b->spf;
        { const int rc = l12_hist_ensure(b); if (rc != MP3MI_OK) return rc; }
        if (!sc && b->book.frames_all == 0) { // a stream's first call: what precedes it is silence (the reference's zero-filled buffers)
            CHK(hipMemsetAsync(b->hist[b->hist_cur], 0, sizeof(int16_t) * L12_PCM_HIST * (size_t) C * (size_t) S, b->stream));
            CHK(hipMemsetAsync(b->fb_hist[b->hist_cur], 0, sizeof(int16_t) * MP3MI_PCM_HIST * (size_t) C * (size_t) S, b->stream));
        }
        mp3mi_launch_l12_hist_save(g, pcm_dev, b->hist[b->hist_cur], b->hist[b->hist_cur ^ 1], b->fb_hist[b->hist_cur], b->fb_hist[b->hist_cur ^ 1], b->stream);
        b->hist_cur ^= 1;
        if (sc) CHK(sc->blk->free.record(b->stream)); // behind the last reader of the control block
        else b->book.frames_all += n_frames;          // (a per-slot call: l12_slots_impl keeps the slots' frames)
    } else l12_streams_over(b);
    CHK(hipEventRecord(b->ev1, b->stream));
    b->kev_chunks = chunk;
    b->timing_open = true;
    b->calls++;
    CHK(hipGetLastError());
    return MP3MI_OK;
}

extern "C" int mp3mi_l12_batch_encode(mp3mi_l12_batch *b, const int16_t *pcm_dev, const int32_t *n_samples_dev, int n_frames,
                                      uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev)
{
    return l12_encode_impl(b, pcm_dev, n_samples_dev, n_frames, out_dev, out_stride, out_len_dev, true);
}

// ---- per-slot streaming (mp3mi_l12_batch_encode_slots) ----
// A bitrate a stream of this batch may have: one of the layer's, as create takes them, not above the ceiling that sized the rows
static bool l12_kbps_ok(const mp3mi_l12_batch *b, int32_t kbps, l12_stream_cfg *c)
{
    return kbps <= b->ceil_kbps && l12_stream_cfg_of(b->layer, b->rate_hz, b->rate_idx, b->channels, kbps, c);
}

static int l12_slots_impl(mp3mi_l12_batch *b, const int16_t *pcm_dev, int n_frames, const uint8_t *ctl_host, const int32_t *n_samples_host,
                          const int32_t *kbps_host, uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev)
{
    if (!b || !pcm_dev || !ctl_host || !out_dev || !out_len_dev || n_frames < 1 || n_frames > b->max_frames || l12_feeders_call(b)) return MP3MI_ERR_ARG;
    if (out_stride < mp3mi_l12_batch_out_stride(b, n_frames)) return MP3MI_ERR_ARG;
    const int S = b->n_streams;
    std::vector<int64_t> f((size_t) S);
    b->book.now(f.data());
    // every rule first: a call that breaks one leaves the batch as it was
    if (!b->book.rules_ok(f.data(), n_frames, b->spf, ctl_host, n_samples_host)) return MP3MI_ERR_ARG;
    bool other_rate = false; // a stream STARTs at another bitrate than its slot was created with
    for (int s = 0; kbps_host && s < S; s++) { // a STARTing stream's bitrate (0: the slot's own); any other slot's is 0, or what the open stream has
        const bool open = f[s] >= 0, start = ctl_host[s] & MP3MI_SLOT_START;
        const int32_t k = kbps_host[s];
        l12_stream_cfg c;
        if (k != 0 && (start ? !l12_kbps_ok(b, k, &c) : !(open && k == b->slot_kbps_h[(size_t) s]))) return MP3MI_ERR_ARG;
        other_rate |= start && k != 0 && k != b->kbps_h[(size_t) s];
    }
    ON_DEVICE(b);
    // cfg is written for the START slots where it stands at another bitrate than the stream's -- never on a batch that has not
    // seen another bitrate than its slots' own, which takes its turn and launches as it always did
    const bool rates = b->rate_dirty || other_rate;
    l12_slot_call sc;
    if (l12_ctl_take(b, &sc.blk, rates) != MP3MI_OK) return MP3MI_ERR_HIP;
    const l12_ctl_block st = l12_ctl_at(sc.blk->stage, S); // the staging copy: the caller's two arrays are copied here
    sc.dev = l12_ctl_at(sc.blk->dev, S);
    sc.n_start = b->book.fill(f.data(), n_frames, b->spf, ctl_host, n_samples_host, st.fabs, st.n_samples, st.ctl, st.list);
    sc.n_rate = 0;
    std::vector<int32_t> kb, dk; // the books behind the call, kept only where they can change
    if (rates) { kb = b->slot_kbps_h; dk = b->dev_kbps_h; }
    for (int i = 0; rates && i < sc.n_start; i++) {
        const int s = st.list[i];
        l12_stream_cfg c;
        kb[(size_t) s] = (kbps_host && kbps_host[s]) ? kbps_host[s] : b->kbps_h[(size_t) s];
        if (dk[(size_t) s] == kb[(size_t) s]) continue;
        (void) l12_stream_cfg_of(b->layer, b->rate_hz, b->rate_idx, b->channels, kb[(size_t) s], &c); // (checked above, or at create)
        l12_rate_set(&l12_rate_at(sc.blk->stage, S)[sc.n_rate++], s, c);
        dk[(size_t) s] = kb[(size_t) s];
    }
    for (int s = 0; rates && s < S; s++)
        if (ctl_host[s] & MP3MI_SLOT_END) kb[(size_t) s] = b->kbps_h[(size_t) s]; // the stream takes its bitrate with it
    const int rc = l12_encode_impl(b, pcm_dev, NULL, n_frames, out_dev, out_stride, out_len_dev, false, &sc);
    if (rc != MP3MI_OK) return rc;
    b->ctl.next();
    if (rates) {
        b->slot_kbps_h.swap(kb);
        b->dev_kbps_h.swap(dk);
        b->rate_dirty = b->dev_kbps_h != b->kbps_h;
    }
    b->book.advance(f.data(), ctl_host, n_frames);
    b->book.settle(f.data());
    return MP3MI_OK;
}

extern "C" int mp3mi_l12_batch_encode_slots_kbps(mp3mi_l12_batch *b, const int16_t *pcm_dev, int n_frames, const uint8_t *ctl_host,
                                                 const int32_t *n_samples_host, const int32_t *kbps_host, uint8_t *out_dev,
                                                 size_t out_stride, uint32_t *out_len_dev)
{
    return l12_slots_impl(b, pcm_dev, n_frames, ctl_host, n_samples_host, kbps_host, out_dev, out_stride, out_len_dev);
}

extern "C" int mp3mi_l12_batch_encode_slots(mp3mi_l12_batch *b, const int16_t *pcm_dev, int n_frames, const uint8_t *ctl_host,
                                            const int32_t *n_samples_host, uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev)
{
    return mp3mi_l12_batch_encode_slots_kbps(b, pcm_dev, n_frames, ctl_host, n_samples_host, NULL, out_dev, out_stride, out_len_dev);
}

extern "C" int mp3mi_l12_batch_slot_kbps(const mp3mi_l12_batch *b, int32_t *kbps_host)
{
    if (!b || !kbps_host) return MP3MI_ERR_ARG;
    memcpy(kbps_host, b->slot_kbps_h.data(), sizeof(int32_t) * (size_t) b->n_streams);
    return b->ceil_kbps;
}

// ---- parking and resuming streams (mp3mi_l12_batch_slots_export / _import) ----
// A stream carries its two rows of PCM history and nothing else: the state record is the row of hist and behind it the row of
// fb_hist, both of the copy the NEXT call reads (hist_cur); frames and bitrate travel in the ticket.  One turn of the control ring
// takes the slot list up, one k12_slot_park moves the rows, on the batch's one stream -- behind every call before, ahead of every
// call after; the host waits for nothing but the turn's own fence (the turn two before).
extern "C" size_t mp3mi_l12_batch_slot_state_bytes(const mp3mi_l12_batch *b)
{
    return b ? (size_t) b->channels * (L12_PCM_HIST + MP3MI_PCM_HIST) * sizeof(int16_t) : 0;
}

// The host halves of an export with close and of an import, for the public calls and for the feeder (l12_feed.h), which parks a
// stream by the first alone and resumes it by the second and its own kernel.  f: the slots as slot_book::now gives them; the caller
// settles the book.  Leave: the stream open in slot s is gone without a flush and takes its bitrate with it (cfg follows at the
// slot's next START).  Enter: a stream at `frames` frames and kbps is open in closed slot s, and cfg[s] stands at kbps -- the
// caller has sent a rate entry up where it lagged (l12_cfg_lags) and settles rate_dirty.
static inline void l12_book_leave(mp3mi_l12_batch *b, int64_t *f, size_t s)
{
    f[s] = -1;
    b->slot_kbps_h[s] = b->kbps_h[s];
}
static inline bool l12_cfg_lags(const mp3mi_l12_batch *b, size_t s, int32_t kbps) { return kbps != b->dev_kbps_h[s]; }
static inline void l12_book_enter(mp3mi_l12_batch *b, int64_t *f, size_t s, int64_t frames, int32_t kbps)
{
    f[s] = frames;
    b->slot_kbps_h[s] = b->dev_kbps_h[s] = kbps;
}

// What export and import ask of their arguments alike
static bool l12_park_args_ok(const mp3mi_l12_batch *b, int n, const int32_t *slots_host, const void *state_dev, size_t state_stride,
                             const void *tickets)
{
    if (!b || !slots_host || !state_dev || !tickets || n < 1 || n > b->n_streams || l12_feeders_call(b)) return false;
    if (state_stride < mp3mi_l12_batch_slot_state_bytes(b) || state_stride % 16 != 0 || (uintptr_t) state_dev % 16 != 0) return false;
    std::vector<char> seen((size_t) b->n_streams, 0);
    for (int i = 0; i < n; i++) {
        const int32_t s = slots_host[i];
        if (s < 0 || s >= b->n_streams || seen[(size_t) s]) return false;
        seen[(size_t) s] = 1;
    }
    return true;
}

// The turn of an export (to_state) or an import: n_rate > 0 -- an import of streams at other bitrates than cfg holds for their
// slots -- has the entry's rate entries written by fill_rates before they go up
template <typename F> static int l12_park_run(mp3mi_l12_batch *b, int n, const int32_t *slots_host, void *state_dev, size_t state_stride,
                                              int to_state, int n_rate, F fill_rates)
{
    mp3mi_l12_batch::ctl_ring::entry *blk;
    { const int rc = l12_ctl_take(b, &blk, n_rate > 0); if (rc != MP3MI_OK) return rc; }
    { const int rc = l12_hist_ensure(b); if (rc != MP3MI_OK) return rc; } // (an import as a fresh batch's first call)
    memcpy(blk->stage, slots_host, sizeof(int32_t) * (size_t) n);
    CHK(hipMemcpyAsync(blk->dev, blk->stage, sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, b->stream));
    mp3mi_launch_l12_slot_park((const int32_t *) blk->dev, n, b->channels, b->hist[b->hist_cur], b->fb_hist[b->hist_cur], state_dev,
                               state_stride, to_state, b->stream);
    CHK(hipGetLastError());
    if (n_rate > 0) {
        fill_rates(l12_rate_at(blk->stage, b->n_streams));
        const int rc = l12_rates_write(b, blk, n_rate);
        if (rc != MP3MI_OK) return rc;
    }
    CHK(blk->free.record(b->stream));
    b->ctl.next();
    return MP3MI_OK;
}

extern "C" int mp3mi_l12_batch_slots_export(mp3mi_l12_batch *b, int n, const int32_t *slots_host, int close, void *state_dev,
                                            size_t state_stride, mp3mi_l12_slot_ticket *tickets_host)
{
    static_assert(sizeof(mp3mi_l12_slot_ticket) == 56, "the ticket of mp3mi_l12.h has no padding");
    if (!l12_park_args_ok(b, n, slots_host, state_dev, state_stride, tickets_host)) return MP3MI_ERR_ARG;
    std::vector<int64_t> f((size_t) b->n_streams);
    b->book.now(f.data());
    for (int i = 0; i < n; i++)
        if (f[(size_t) slots_host[i]] < 0) return MP3MI_ERR_ARG; // no stream open there
    ON_DEVICE(b);
    const int rc = l12_park_run(b, n, slots_host, state_dev, state_stride, 1, 0, [](l12_rate_entry *) {});
    if (rc != MP3MI_OK) return rc;
    for (int i = 0; i < n; i++) { // all of it host bookkeeping: no wait
        const size_t s = (size_t) slots_host[i];
        mp3mi_l12_slot_ticket &t = tickets_host[i];
        memset(&t, 0, sizeof(t));
        t.magic = MP3MI_L12_SLOT_TICKET_MAGIC;
        t.version = MP3MI_L12_SLOT_TICKET_VERSION;
        t.state_bytes = (uint64_t) mp3mi_l12_batch_slot_state_bytes(b);
        t.layer = b->layer;
        t.rate_hz = b->rate_hz;
        t.channels = b->channels;
        t.hdr_mode = b->mode;
        t.hdr_flags = b->hdr_flags;
        t.error_protection = b->crc;
        t.kbps = b->slot_kbps_h[s];
        t.frames = f[s];
        if (close) l12_book_leave(b, f.data(), s);
    }
    // (the whole-batch counter cannot say "all but these": the per-slot bookkeeping takes over; slot_book::settle hands back as ever)
    b->book.settle(f.data());
    return MP3MI_OK;
}

extern "C" int mp3mi_l12_batch_slots_import(mp3mi_l12_batch *b, int n, const int32_t *slots_host, const void *state_dev, size_t state_stride,
                                            const mp3mi_l12_slot_ticket *tickets_host)
{
    if (!l12_park_args_ok(b, n, slots_host, state_dev, state_stride, tickets_host)) return MP3MI_ERR_ARG;
    const int S = b->n_streams;
    std::vector<int64_t> f((size_t) S);
    b->book.now(f.data());
    std::vector<l12_stream_cfg> val((size_t) n);
    int n_rate = 0; // streams that arrive at another bitrate than cfg holds for their slots
    for (int i = 0; i < n; i++) {
        const size_t s = (size_t) slots_host[i];
        const mp3mi_l12_slot_ticket &t = tickets_host[i];
        if (f[s] >= 0) return MP3MI_ERR_ARG; // a stream is open there
        if (t.magic != MP3MI_L12_SLOT_TICKET_MAGIC || t.version != MP3MI_L12_SLOT_TICKET_VERSION ||
            t.state_bytes != (uint64_t) mp3mi_l12_batch_slot_state_bytes(b))
            return MP3MI_ERR_ARG;
        if (t.layer != b->layer || t.rate_hz != b->rate_hz || t.channels != b->channels || t.hdr_mode != b->mode ||
            t.hdr_flags != b->hdr_flags || t.error_protection != b->crc || t.reserved != 0)
            return MP3MI_ERR_ARG;
        if (!l12_kbps_ok(b, t.kbps, &val[(size_t) i]) || t.frames < 0) return MP3MI_ERR_ARG;
        n_rate += l12_cfg_lags(b, s, t.kbps);
    }
    ON_DEVICE(b);
    // cfg of a resumed stream is rebuilt here, from the ticket's checked bitrate: nothing of a device record is used as an index
    const int rc = l12_park_run(b, n, slots_host, const_cast<void *>(state_dev), state_stride, 0, n_rate, [&](l12_rate_entry *rt) {
        for (int i = 0; i < n; i++)
            if (l12_cfg_lags(b, (size_t) slots_host[i], tickets_host[i].kbps)) l12_rate_set(rt++, slots_host[i], val[(size_t) i]);
    });
    if (rc != MP3MI_OK) return rc;
    for (int i = 0; i < n; i++) l12_book_enter(b, f.data(), (size_t) slots_host[i], tickets_host[i].frames, tickets_host[i].kbps);
    if (n_rate > 0) b->rate_dirty = b->dev_kbps_h != b->kbps_h;
    // the per-slot bookkeeping from here on, also on a batch nothing has run on yet (slot_book::settle hands back only with every
    // slot open at one frame count, and then the whole-batch path continues them from the same history)
    b->book.settle(f.data());
    return MP3MI_OK;
}

extern "C" int mp3mi_l12_batch_slot_frames(const mp3mi_l12_batch *b, int64_t *frames_host)
{
    if (!b || !frames_host) return MP3MI_ERR_ARG;
    b->book.now(frames_host);
    return b->book.count_open();
}

extern "C" int mp3mi_l12_batch_encode_next(mp3mi_l12_batch *b, const int16_t *pcm_dev, int n_frames, uint8_t *out_dev, size_t out_stride,
                                           uint32_t *out_len_dev)
{
    if (l12_feeders_call(b)) return MP3MI_ERR_ARG;
    if (b && b->book.on) {
        // per-slot bookkeeping in force: with no stream open every slot starts (the whole-batch start); otherwise the open streams
        // go on and the other slots stay closed
        if (b->book.any_open()) {
            std::vector<uint8_t> ctl((size_t) b->n_streams, 0);
            return l12_slots_impl(b, pcm_dev, n_frames, ctl.data(), NULL, NULL, out_dev, out_stride, out_len_dev);
        }
        if (!pcm_dev || !out_dev || !out_len_dev || n_frames < 1 || n_frames > b->max_frames || out_stride < mp3mi_l12_batch_out_stride(b, n_frames))
            return MP3MI_ERR_ARG; // (before the bookkeeping changes)
        b->book.close();
    }
    return l12_encode_impl(b, pcm_dev, NULL, n_frames, out_dev, out_stride, out_len_dev, false);
}

extern "C" int mp3mi_l12_batch_flush(mp3mi_l12_batch *b, uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev)
{
    if (!b || !out_dev || !out_len_dev || out_stride < 1 || l12_feeders_call(b)) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    const uint8_t *slot_ctl = NULL;
    mp3mi_l12_batch::ctl_ring::entry *blk = NULL;
    if (b->book.on) { // some slots open, not all at the same frame (slot_book::settle), or none: the open ones end, the others deliver nothing
        const int S = b->n_streams;
        if (l12_ctl_take(b, &blk) != MP3MI_OK) return MP3MI_ERR_HIP;
        const l12_ctl_block st = l12_ctl_at(blk->stage, S), dev = l12_ctl_at(blk->dev, S);
        for (int s = 0; s < S; s++) st.ctl[s] = b->book.at(s) >= 0 ? MP3MI_SLOT_DEV_ACTIVE : 0;
        CHK(hipMemcpyAsync(dev.ctl, st.ctl, (size_t) S, hipMemcpyHostToDevice, b->stream)); // (k12_flush reads nothing else of the block)
        slot_ctl = dev.ctl;
    }
    mp3mi_launch_l12_flush(b->n_streams, slot_ctl, out_dev, out_stride, out_len_dev, b->stream);
    if (blk) {
        CHK(blk->free.record(b->stream));
        b->ctl.next();
    }
    l12_streams_over(b);
    CHK(hipGetLastError());
    return MP3MI_OK;
}

extern "C" int mp3mi_l12_batch_reset(mp3mi_l12_batch *b)
{
    if (!b || l12_feeders_call(b)) return MP3MI_ERR_ARG;
    l12_streams_over(b);
    return MP3MI_OK;
}

extern "C" int mp3mi_l12_batch_sync(mp3mi_l12_batch *b)
{
    if (!b) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    CHK(hipStreamSynchronize(b->stream));
    return l12_close_timing(b);
}

extern "C" int mp3mi_l12_batch_total_timing(mp3mi_l12_batch *b, double *all_kernels_ms, long *calls)
{
    if (!b) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    CHK(hipStreamSynchronize(b->stream));
    { const int rc = l12_close_timing(b); if (rc != MP3MI_OK) return rc; }
    if (all_kernels_ms) *all_kernels_ms = b->total_ms;
    if (calls) *calls = b->calls;
    return MP3MI_OK;
}

extern "C" int mp3mi_l12_batch_kernel_timing(mp3mi_l12_batch *b, double ms[4], long launches[4])
{
    if (!b || !ms || !launches) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    CHK(hipStreamSynchronize(b->stream));
    { const int rc = l12_close_timing(b); if (rc != MP3MI_OK) return rc; }
    for (int i = 0; i < 4; i++) { ms[i] = b->kernel_ms[i]; launches[i] = b->kernel_launches[i]; }
    return MP3MI_OK;
}

extern "C" long mp3mi_l12_batch_debug_fetch(mp3mi_l12_batch *b, void *host_dst, size_t cap, int *first_frame, int *n_chunk_frames)
{
    static_assert(sizeof(mp3mi_l12_frame_seams) == sizeof(l12_frame_dbg), "seam record of mp3mi_l12.h and l12_dev.h");
    if (!b || !host_dst || !b->dbg) return MP3MI_ERR_ARG;
    ON_DEVICE(b);
    CHK(hipStreamSynchronize(b->stream));
    const size_t bytes = sizeof(l12_frame_dbg) * (size_t) b->n_streams * (size_t) b->dbg_nf;
    if (cap < bytes) return MP3MI_ERR_ARG;
    CHK(hipMemcpy(host_dst, b->dbg, bytes, hipMemcpyDeviceToHost));
    if (first_frame) *first_frame = b->dbg_f0;
    if (n_chunk_frames) *n_chunk_frames = b->dbg_nf;
    return (long) bytes;
}

extern "C" int mp3mi_l12_encode_host(int layer, int n_streams, int rate_hz, int channels, const int *kbps, int kbps_all, int mode,
                                     int error_protection, const int16_t *pcm, const int32_t *n_samples, int n_frames,
                                     uint8_t *out, size_t out_stride, uint32_t *out_len)
{
    if (!pcm || !out || !out_len || n_frames < 1 || n_streams < 1) return MP3MI_ERR_ARG;
    mp3mi_l12_batch *b = NULL;
    int rc = mp3mi_l12_batch_create(&b, layer, n_streams, rate_hz, channels, kbps, kbps_all, n_frames, 0);
    if (rc != MP3MI_OK) return rc;
    if (mode >= 0) rc = mp3mi_l12_batch_set_mode(b, mode);
    if (rc == MP3MI_OK) rc = mp3mi_l12_batch_set_error_protection(b, error_protection);
    if (rc != MP3MI_OK || out_stride < mp3mi_l12_batch_out_stride(b, n_frames)) { mp3mi_l12_batch_destroy(b); return MP3MI_ERR_ARG; }
    const size_t S = (size_t) n_streams;
    {
        hook_bufs D; // (the call's device copies: freed before the batch goes)
        int16_t *pcm_d = D.copy_of(pcm, S * (size_t) n_frames * (size_t) l12_samples_per_frame(layer) * (size_t) channels);
        uint8_t *out_d = D.raw<uint8_t>(out_stride * S);
        uint32_t *len_d = D.raw<uint32_t>(S);
        int32_t *ns_d = n_samples ? D.copy_of(n_samples, S) : D.raw<int32_t>(S);
        rc = D.rc();
        if (rc == MP3MI_OK) rc = mp3mi_l12_batch_encode(b, pcm_d, n_samples ? ns_d : NULL, n_frames, out_d, out_stride, len_d);
        if (rc == MP3MI_OK) rc = mp3mi_l12_batch_sync(b);
        if (rc == MP3MI_OK && !(D.fetch(out, out_d, out_stride * S) && D.fetch(out_len, len_d, S))) rc = MP3MI_ERR_HIP;
    }
    mp3mi_l12_batch_destroy(b);
    return rc;
}

#include "l12_feed.h"
