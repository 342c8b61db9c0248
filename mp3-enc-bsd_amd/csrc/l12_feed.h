// The feeder of Layers I and II (include/mp3mi_l12.h, mp3mi_l12_feed_*): lanes in front of the slots of a Layer I / II batch, a device
// FIFO per lane, so that a stream may bring any number of samples per call.  Part of l12_batch.cpp's translation unit (included at
// its end).  The contract -- rows, lane states, the scheduler, the flags -- is that of the Layer III feeder with lanes (feed.h,
// mp3mi_feed_tick_lanes), restated here for a batch of one HIP stream; what a parked stream costs is not.
//
// The ring is the record.  A stream of these layers carries nothing from call to call but PCM history: the last L12_PCM_HIST
// samples before the next call's first and the last MP3MI_PCM_HIST of the same (k12_hist_save; the state record of
// mp3mi_l12_batch_slots_export is exactly these two rows).  A lane's ring holds cap = capacity + L12_PCM_HIST samples per channel
// and the tick keeps L12_PCM_HIST + pending + n_push <= cap, so the L12_PCM_HIST samples behind the read position `head` are never
// overwritten: whatever the stream has encoded of them lies there, in time order.  Parking a stream is therefore host bookkeeping
// alone (l12_book_leave: the slot is closed without a flush, nothing is launched), and resuming it is one more pair of copies in
// the kernel that cuts the tick's rows (k12_feed, k_format.hip: ring -> the slot's rows of the batch's live history buffers, zeros
// in front of a stream younger than the rows) and l12_book_enter -- plus k12_slot_rate where cfg of the slot stands at another
// bitrate than the stream's.  No state records, no dense blocks, no tickets.
//
// Per lane on the device: ring [L][cap][C] int16.  Per slot: rows [S][tick_frames * frame][C], what the per-slot call of a tick
// reads, written by k12_feed only.  On the host (lane): head, pending, the stream's bitrate, flags, frames, the slot it holds.
//
// A tick, on the batch's ONE stream, all of it enqueued and none of it waited for:
//   upload of the descriptors | k12_feed | (k12_slot_rate: resumed streams whose slot's cfg lags) |
//   mp3mi_l12_batch_encode_slots_kbps on the feeder's rows: control block, k12_slot_rate and k12_slot_begin for the STARTs,
//   k_fft12, k12_psy, k_filter, k12_alloc, k12_hist_save
// Orderings it rests on.  (1) k12_feed is the rows' only writer and the per-slot call of the same tick their only reader, behind it
// on the same stream; the next tick's k12_feed is behind that reader: one copy of the rows is enough.  (2) k12_feed writes the
// resumed slots' rows of hist[hist_cur] / fb_hist[hist_cur], the pair the per-slot call that follows READS (it writes the other
// pair and flips); it runs behind the k12_hist_save of the tick before, which wrote that pair -- stale rows for the slots that
// were closed then, overwritten here for those that resume, zeroed by k12_slot_begin for those that START.  (3) Within a launch
// no workgroup reads what another writes: per descriptor the spans read (history and pending: [head - n_hist, head + pending))
// and the span written (the append: [head + pending, head + pending + n_push)) are disjoint by the ring's rule, and no lane, no
// slot of a taking or resuming descriptor and no push row of a pushing one appears twice.  (4) The upload block of a tick is read
// by that tick's k12_feed alone; its fence is recorded behind it, and the host meets it four ticks later -- as a rule long through.
// The per-slot call and the rate turn take turns of the batch's control ring as any caller's would (l12_ctl_take).

#include <algorithm>
#include <utility>

struct mp3mi_l12_feed {
    mp3mi_l12_batch *b;
    int tick_frames, max_push, max_rows;
    int capacity, cap;            // pending samples per channel a lane holds; the ring's samples: capacity + L12_PCM_HIST
    int32_t full;                 // tick_frames * frame
    size_t ring_pitch, row_pitch; // bytes, multiples of 16
    int16_t *ring, *rows;
    struct lane {
        int32_t head, pending; // the ring's read position and fill, in samples per channel
        int32_t kbps;          // as given at START; from the first tick that encodes, the stream's bitrate
        bool open;             // a stream is in the lane: from the feeder's START to the tick that closes it
        bool parked;           // ... out of its slot, its history in the ring
        bool draining;         // ... END has been given
        bool waiting;          // ... the batch has not seen its START yet
        bool wait_slot;        // ready in the last tick and left without a slot
        bool seen, chosen;     // (within a tick) among the tick's lanes; encodes in this tick
        int64_t frames;        // frames encoded so far, -1: closed
        int32_t slot;          // the slot that holds the lane's stream (an abandoned one while `waiting`), -1: none
        int64_t since;         // the tick in which the lane's unbroken spell of being ready began, -1: none
    };
    std::vector<lane> lanes;
    int64_t tick_no;
    std::vector<int32_t> slot_lane; // [S]: the lane whose stream is open in the slot, -1: none
    std::vector<int32_t> hot;       // ascending: the lanes that are ready without a push (a tick pending, or draining)
    // what goes up per tick: descriptors of 32 bytes, for at most max_rows + S lanes that move; a ring of four with fences
    typedef upload_ring<uint8_t, 4> up_ring;
    up_ring up;
};

// the feeder's buffers, handles and the object (the device is through with them: the caller has waited); the batch is detached
static void l12_feed_drop(mp3mi_l12_feed *f)
{
    (void) hipFree(f->ring);
    (void) hipFree(f->rows);
    for (mp3mi_l12_feed::up_ring::entry &en : f->up.e) {
        if (en.stage) (void) hipHostFree(en.stage);
        (void) hipFree(en.dev);
        en.free.destroy();
    }
    f->b->feed = NULL;
    delete f;
}

extern "C" int mp3mi_l12_feed_create(mp3mi_l12_feed **out, mp3mi_l12_batch *b, int n_lanes, int max_rows, int tick_frames, int max_push,
                                     int ring_samples)
{
    if (!out) return MP3MI_ERR_ARG;
    *out = NULL;
    if (!b || b->feed || tick_frames < 1 || tick_frames > b->max_frames || max_push < 1 || b->book.any_open()) return MP3MI_ERR_ARG;
    if (n_lanes < 1 || max_rows < 1 || max_rows > n_lanes || ring_samples < 0) return MP3MI_ERR_ARG;
    const int64_t least = (int64_t) tick_frames * b->spf + max_push, capacity = ring_samples ? ring_samples : least;
    if (capacity < least || capacity + L12_PCM_HIST > INT32_MAX / 8) return MP3MI_ERR_ARG; // (a lane's bytes stay far inside 32 bits)
    ON_DEVICE(b);
    mp3mi_l12_feed *f = new mp3mi_l12_feed(); // value-initialised
    f->b = b;
    f->tick_frames = tick_frames;
    f->max_push = max_push;
    f->max_rows = max_rows;
    f->full = tick_frames * b->spf;
    f->capacity = (int) capacity;
    f->cap = (int) capacity + L12_PCM_HIST;
    b->feed = f; // (l12_feed_drop detaches)
    auto build = [&]() -> int {
        const size_t S = (size_t) b->n_streams, L = (size_t) n_lanes, esz = 2 * (size_t) b->channels;
        f->ring_pitch = ((size_t) f->cap * esz + 15) & ~(size_t) 15;
        f->row_pitch = (size_t) f->full * esz; // (a frame of one channel is 768 or 2304 bytes: multiples of 16)
        CHK(hipMalloc((void **) &f->ring, L * f->ring_pitch));
        CHK(hipMalloc((void **) &f->rows, S * f->row_pitch));
        CHK(hipMemset(f->rows, 0, S * f->row_pitch));
        const size_t up_bytes = 32 * ((size_t) max_rows + S);
        for (mp3mi_l12_feed::up_ring::entry &en : f->up.e) {
            CHK(hipHostMalloc((void **) &en.stage, up_bytes, 0));
            CHK(hipMalloc((void **) &en.dev, up_bytes));
            CHK(en.free.create());
        }
        return MP3MI_OK;
    };
    const int rc = build();
    if (rc != MP3MI_OK) {
        l12_feed_drop(f);
        return rc;
    }
    f->lanes.assign((size_t) n_lanes, mp3mi_l12_feed::lane());
    for (mp3mi_l12_feed::lane &l : f->lanes) {
        l.frames = l.since = -1;
        l.slot = -1;
    }
    f->slot_lane.assign((size_t) b->n_streams, -1);
    *out = f;
    return MP3MI_OK;
}

extern "C" void mp3mi_l12_feed_destroy(mp3mi_l12_feed *f)
{
    if (!f) return;
    mp3mi_l12_batch *b = f->b;
    device_scope ds(b->device);
    b->feed_call = true;
    (void) mp3mi_l12_batch_reset(b); // the streams in the slots are abandoned with the parked and the pending ones
    b->feed_call = false;
    (void) hipStreamSynchronize(b->stream);
    l12_feed_drop(f);
}

extern "C" size_t mp3mi_l12_feed_capacity(const mp3mi_l12_feed *f) { return f ? (size_t) f->capacity : 0; }
extern "C" int mp3mi_l12_feed_n_lanes(const mp3mi_l12_feed *f) { return f ? (int) f->lanes.size() : 0; }

extern "C" int mp3mi_l12_feed_lanes(const mp3mi_l12_feed *f, int32_t *pending_host, int64_t *frames_host, uint8_t *flags_host)
{
    if (!f || !pending_host || !frames_host || !flags_host) return MP3MI_ERR_ARG;
    int n = 0;
    for (size_t s = 0; s < f->lanes.size(); s++) {
        const mp3mi_l12_feed::lane &l = f->lanes[s];
        pending_host[s] = l.open ? l.pending : 0;
        frames_host[s] = l.open ? l.frames : -1;
        flags_host[s] = (uint8_t) (l.open ? (l.parked ? 1 : 0) | (l.draining ? 2 : 0) | (l.waiting ? 4 : 0) | (l.wait_slot ? 8 : 0) : 0);
        n += l.open;
    }
    return n;
}

// The resumed streams whose slots' cfg stands at another bitrate: a turn of the control ring of its own, rate entries alone, ahead
// of the per-slot call on the batch's stream (as l12_rates_restore does for the slots that go back to their create-time bitrates)
static int l12_feed_rates(mp3mi_l12_batch *b, const std::vector<int32_t> &slots, const std::vector<int32_t> &kbps)
{
    const int S = b->n_streams;
    mp3mi_l12_batch::ctl_ring::entry *blk;
    { const int rc = l12_ctl_take(b, &blk, true); if (rc != MP3MI_OK) return rc; }
    l12_rate_entry *st = l12_rate_at(blk->stage, S);
    for (size_t i = 0; i < slots.size(); i++) {
        l12_stream_cfg c;
        (void) l12_stream_cfg_of(b->layer, b->rate_hz, b->rate_idx, b->channels, kbps[i], &c); // (checked at the stream's START)
        l12_rate_set(&st[i], slots[i], c);
    }
    { const int rc = l12_rates_write(b, blk, (int) slots.size()); if (rc != MP3MI_OK) return rc; }
    CHK(blk->free.record(b->stream));
    b->ctl.next();
    return MP3MI_OK;
}

extern "C" int mp3mi_l12_feed_tick(mp3mi_l12_feed *f, int n_rows, const int32_t *row_lane_host, const int16_t *pcm_dev, size_t pcm_pitch,
                                   const uint8_t *ctl_host, const int32_t *n_push_host, const int32_t *kbps_host, uint8_t *out_dev,
                                   size_t out_stride, uint32_t *out_len_dev, int32_t *slot_lane_host)
{
    if (!f || !out_dev || !out_len_dev || !slot_lane_host) return MP3MI_ERR_ARG;
    mp3mi_l12_batch *b = f->b;
    if (n_rows < 0 || n_rows > f->max_rows || out_stride < mp3mi_l12_batch_out_stride(b, f->tick_frames)) return MP3MI_ERR_ARG;
    if (n_rows > 0 && (!row_lane_host || !pcm_dev || !ctl_host || !n_push_host || !kbps_host || pcm_pitch < (size_t) f->max_push)) return MP3MI_ERR_ARG;
    const int S = b->n_streams, L = (int) f->lanes.size(), spf = b->spf;
    const size_t esz = 2 * (size_t) b->channels;
    typedef mp3mi_l12_feed::lane lane;
    // ---- 1. the rules, over all rows, before anything changes state (a lane without a row pushes nothing and breaks none) ----
    for (int r = 0; r < n_rows; r++) {
        const int32_t ln = row_lane_host[r];
        if (ln < 0 || ln >= L || (r > 0 && ln <= row_lane_host[r - 1])) return MP3MI_ERR_ARG;
        const lane &l = f->lanes[ln];
        const int c = ctl_host[r];
        const int32_t n = n_push_host[r], k = kbps_host[r];
        if ((c & ~(MP3MI_SLOT_START | MP3MI_SLOT_END)) || n < 0 || n > f->max_push) return MP3MI_ERR_ARG;
        const bool start = c & MP3MI_SLOT_START, end = c & MP3MI_SLOT_END;
        if (l.open && l.draining && (start || end || n != 0)) return MP3MI_ERR_ARG; // its samples are all in
        if (!l.open && !start && (end || n != 0)) return MP3MI_ERR_ARG;
        l12_stream_cfg cfg;
        // (a stream that STARTed at kbps 0 has the create-time bitrate of the slot it first encodes in: known from then on)
        if (start ? (k != 0 && !l12_kbps_ok(b, k, &cfg)) : (k != 0 && !(l.open && l.kbps != 0 && k == l.kbps))) return MP3MI_ERR_ARG;
        if ((int64_t) (start ? 0 : l.pending) + n > f->capacity) return MP3MI_ERR_ARG;
    }
    // ---- 2. the lanes of this tick: the hot ones and the rows', ascending; who is ready ----
    struct cand { int32_t ln, row, n, have, head0, pend0; bool ready, closes; };
    std::vector<cand> cs;
    cs.reserve(f->hot.size() + (size_t) n_rows);
    std::vector<std::pair<int32_t, lane> > undo; // the lanes as they were, should a HIP call fail further down
    undo.reserve(f->hot.size() + (size_t) n_rows + (size_t) S);
    const std::vector<int32_t> slot_lane0(f->slot_lane);
    size_t n_ready = 0;
    for (size_t h = 0, r = 0; h < f->hot.size() || r < (size_t) n_rows;) {
        const int32_t lh = h < f->hot.size() ? f->hot[h] : INT32_MAX, lr = r < (size_t) n_rows ? row_lane_host[r] : INT32_MAX;
        cand c;
        memset(&c, 0, sizeof(c));
        c.ln = lh < lr ? lh : lr;
        c.row = lr == c.ln ? (int32_t) r : -1;
        h += lh == c.ln;
        r += lr == c.ln;
        lane &l = f->lanes[c.ln];
        undo.push_back(std::make_pair(c.ln, l));
        l.seen = true;
        const int ctl = c.row >= 0 ? ctl_host[c.row] : 0;
        c.n = c.row >= 0 ? n_push_host[c.row] : 0;
        if (ctl & MP3MI_SLOT_START) { // a new stream; one that is open in the lane is abandoned: its samples, its history -- and its slot,
            l.open = l.waiting = true; // where it has one, with this tick: to this lane's START if it is chosen, else it is vacated
            l.parked = l.draining = false;
            l.head = l.pending = 0;
            l.kbps = kbps_host[c.row];
            l.frames = 0;
        }
        if (!l.open) continue; // (a hot lane is open; a row on a closed lane without START brought nothing)
        if (ctl & MP3MI_SLOT_END) l.draining = true;
        c.head0 = l.head;
        c.pend0 = l.pending;
        c.have = l.pending + c.n;
        c.closes = l.draining && c.have <= f->full;
        c.ready = c.closes || c.have >= f->full;
        if (c.ready && l.since < 0) l.since = f->tick_no;
        if (!c.ready) l.since = -1;
        n_ready += c.ready;
        cs.push_back(c);
    }
    if (n_ready > (size_t) S) { // the S whose spells began first; ties to the lower lane
        std::vector<std::pair<int64_t, int32_t> > order;
        order.reserve(n_ready);
        for (const cand &c : cs)
            if (c.ready) order.push_back(std::make_pair(f->lanes[c.ln].since, c.ln));
        std::nth_element(order.begin(), order.begin() + S, order.end());
        for (int i = 0; i < S; i++) f->lanes[order[i].second].chosen = true;
    } else {
        for (const cand &c : cs)
            if (c.ready) f->lanes[c.ln].chosen = true;
    }
    // ---- 3. the slots: who stays, who leaves, who enters -- and the batch's books of those who move ----
    std::vector<int64_t> fr((size_t) S);
    b->book.now(fr.data());
    const slot_book book0(b->book);
    const std::vector<int32_t> slot_kbps0(b->slot_kbps_h), dev_kbps0(b->dev_kbps_h);
    const bool rate_dirty0 = b->rate_dirty;
    std::vector<int32_t> free_slots, rate_slots, rate_kbps;
    bool moved = false;
    for (int s = 0; s < S; s++) {
        const int32_t ln = f->slot_lane[s];
        if (ln >= 0 && !f->lanes[ln].chosen) { // sits out, waits for a slot, or was abandoned for a stream that does not encode now
            lane &l = f->lanes[ln];
            if (!l.seen) undo.push_back(std::make_pair(ln, l)); // (a lane of no row that is not hot)
            l.parked = !l.waiting;
            l.slot = -1;
            f->slot_lane[s] = -1;
            l12_book_leave(b, fr.data(), (size_t) s); // parked: closed without a flush, nothing launched
            moved = true;
        }
        if (f->slot_lane[s] < 0) free_slots.push_back(s);
    }
    std::vector<uint8_t> ctl((size_t) S, 0);
    std::vector<int32_t> ns((size_t) S, 0), kb((size_t) S, 0);
    std::vector<uint32_t> desc;
    desc.reserve(8 * cs.size());
    std::vector<int32_t> hot;
    for (int s = 0; s < S; s++) slot_lane_host[s] = -1;
    size_t most = 0, n_free = 0;
    bool any_ready = false;
    for (const cand &c : cs) {
        lane &l = f->lanes[c.ln];
        int32_t take = 0;
        uint32_t resume = 0;
        if (l.chosen) {
            take = c.closes ? c.have : f->full;
            if (l.slot < 0) { // the lowest free slot to the lowest lane
                l.slot = free_slots[n_free++];
                if (l.parked) { // resumed: open there at its frame count and bitrate, its history out of the ring
                    const int64_t done = l.frames * (int64_t) spf;
                    resume = MP3MI_L12_FEED_RESUME | (uint32_t) (done < L12_PCM_HIST ? done : L12_PCM_HIST);
                    if (l12_cfg_lags(b, (size_t) l.slot, l.kbps)) {
                        rate_slots.push_back(l.slot);
                        rate_kbps.push_back(l.kbps);
                    }
                    l12_book_enter(b, fr.data(), (size_t) l.slot, l.frames, l.kbps);
                    moved = true;
                }
            }
            const int32_t s = l.slot;
            any_ready = true;
            ctl[s] = (uint8_t) ((l.waiting ? MP3MI_SLOT_START : 0) | (c.closes ? MP3MI_SLOT_END : 0));
            ns[s] = take;
            kb[s] = l.waiting ? l.kbps : 0;
            if (l.waiting && l.kbps == 0) l.kbps = b->kbps_h[s];
            slot_lane_host[s] = c.ln;
            f->slot_lane[s] = c.closes ? -1 : c.ln;
            l.parked = l.waiting = l.wait_slot = false;
            l.since = -1; // a lane that is still ready begins a new spell in the next tick
            l.frames += c.closes ? (take + spf - 1) / spf : f->tick_frames;
        } else
            l.wait_slot = c.ready;
        if (c.n || take || resume) {
            const uint32_t d[8] = {(uint32_t) c.head0, (uint32_t) c.pend0, (uint32_t) c.n, (uint32_t) take,
                                   (uint32_t) c.ln, c.n ? (uint32_t) c.row : 0u, (uint32_t) ((take || resume) ? l.slot : 0), resume};
            desc.insert(desc.end(), d, d + 8);
            size_t longest = (size_t) (take > c.n ? take : c.n);
            if (resume && longest < L12_PCM_HIST) longest = L12_PCM_HIST;
            most = longest * esz > most ? longest * esz : most;
        }
        l.head = (int32_t) (((int64_t) c.head0 + take) % f->cap);
        l.pending = c.have - take;
        if (l.chosen && c.closes) {
            l.open = false;
            l.frames = -1;
            l.slot = -1;
        }
        l.chosen = false;
        if (l.open && (l.draining || l.pending >= f->full)) hot.push_back(c.ln);
    }
    for (const std::pair<int32_t, lane> &u : undo) f->lanes[u.first].seen = false;
    if (moved) {
        b->book.settle(fr.data());
        if (!rate_slots.empty()) b->rate_dirty = b->dev_kbps_h != b->kbps_h;
    }
    const size_t n_active = desc.size() / 8;
    auto fail = [&](int rc) { // the books as they were
        for (size_t i = undo.size(); i-- > 0;) f->lanes[undo[i].first] = undo[i].second;
        f->slot_lane = slot_lane0;
        b->book = book0;
        b->slot_kbps_h = slot_kbps0;
        b->dev_kbps_h = dev_kbps0;
        b->rate_dirty = rate_dirty0;
        b->feed_call = false;
        return rc;
    };
#define FCHK(call)                                                  \
    do {                                                            \
        if ((call) != hipSuccess) {                                 \
            fprintf(stderr, "mp3mi: %s failed (%s:%d)\n", #call, __FILE__, __LINE__); \
            return fail(MP3MI_ERR_HIP);                             \
        }                                                           \
    } while (0)
    device_scope ds(b->device);
    if (!ds.ok) return fail(MP3MI_ERR_HIP);
    // ---- 4. the descriptors go up; k12_feed over the lanes that move: rings, rows, and the history rows of the slots that resume ----
    if (n_active) {
        mp3mi_l12_feed::up_ring::entry &en = f->up.take();
        if (!en.free.done()) FCHK(en.free.sync()); // the one place this call can block: the entry's reader, four ticks ago
        if (l12_hist_ensure(b) != MP3MI_OK) return fail(MP3MI_ERR_HIP);
        memcpy(en.stage, desc.data(), 32 * n_active);
        FCHK(hipMemcpyAsync(en.dev, en.stage, 32 * n_active, hipMemcpyHostToDevice, b->stream));
        mp3mi_launch_l12_feed(en.dev, (int) n_active, f->ring, f->ring_pitch, f->cap, b->channels, pcm_dev, pcm_pitch * esz, f->rows, f->row_pitch,
                              b->hist[b->hist_cur], L12_PCM_HIST, b->fb_hist[b->hist_cur], MP3MI_PCM_HIST, most, b->stream);
        FCHK(hipGetLastError());
        FCHK(en.free.record(b->stream));
        f->up.next();
    }
    b->feed_call = true;
    int rc = MP3MI_OK;
    // ---- 5. cfg of the slots whose resumed stream runs at another bitrate; 6. one per-slot call on the feeder's rows ----
    if (!rate_slots.empty()) rc = l12_feed_rates(b, rate_slots, rate_kbps);
    if (rc == MP3MI_OK && any_ready)
        rc = mp3mi_l12_batch_encode_slots_kbps(b, f->rows, f->tick_frames, ctl.data(), ns.data(), kb.data(), out_dev, out_stride, out_len_dev);
    b->feed_call = false;
    if (rc != MP3MI_OK) return fail(rc);
    if (!any_ready) FCHK(hipMemsetAsync(out_len_dev, 0, sizeof(uint32_t) * (size_t) S, b->stream)); // nothing encodes: zeros, in stream order
#undef FCHK
    f->hot.swap(hot);
    f->tick_no++;
    return MP3MI_OK;
}
