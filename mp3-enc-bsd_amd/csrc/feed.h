// The feeder (include/mp3mi.h, mp3mi_feed_*): a device FIFO per slot in front of a Layer III slot batch, so that a stream may
// bring any number of samples per call.  Part of batch.cpp's translation unit (included at its end): it allocates through
// dev_alloc / pinned_alloc and asks hold_release and park_tables, but it DRIVES the batch through the public per-slot calls only --
// mp3mi_batch_slots_export, mp3mi_batch_slots_import, mp3mi_batch_encode_slots_kbps -- and so rests on their contracts.
//
// Per lane (= slot) on the device:
//   ring       [S][cap][C] int16, cap = tick_frames * 1152 + max_push: the samples pushed and not yet encoded
//   rows       [S][tick_frames * 1152][C]: what the per-slot call of a tick reads; written by k_feed only
//   rec_front, rec_loop   the parked stream's state record, in the two parts the batch's two HIP streams own (below)
// and on the host (lane): head, pending, the bitrate remembered at START, flags, frames, the parked stream's ticket.
//
// A tick, all of it enqueued and none of it waited for:
//   front stream   upload of {descriptors, park list, resume list} | k_feed | export: front regions | scatter -> rec_front |
//                  gather <- rec_front | import: front regions | the per-slot call's feed-forward kernels
//   loop stream    (waits for the upload) export: loop regions | scatter -> rec_loop | gather <- rec_loop | import: loop regions |
//                  the per-slot call's k_loop, k_format, k_stream_tail
// Every reader of the rows -- mp3mi_launch_fft, mp3mi_launch_filter, mp3mi_launch_hist_save (encode_impl) -- runs on the front
// stream, and so does k_feed, their only writer: tick t + 1's k_feed is in order behind tick t's readers, and one copy of the rows
// is enough.  The ring is touched by k_feed alone.
//
// Parked records.  mp3mi_batch_slots_export writes record i of its LIST at state + i * stride, and a lane that sits out may stay
// out for any number of ticks while others come and go: the records of a tick's list go through a dense scratch block and are
// scattered from there to (gathered from) a record per LANE, by k_slot_park with a one-region table -- the kernel that moves records
// between regions per slot and dense records anyway.  The front stream never waits for the loop stream (batch.cpp, park_run), so
// each stream moves the part of a record it wrote or will read: the state record lists the front stream's regions first
// (park_tables), which makes the parts the bytes below and from the first loop-stream region's offset.  That costs a tick one
// export, one import and four small launches however many lanes sit out, instead of a call per run of neighbouring lanes.

struct mp3mi_feed {
    mp3mi_batch *b;
    int tick_frames, max_push, cap; // cap: samples per channel of a lane's ring
    int32_t full;                   // tick_frames * 1152
    size_t owned0, owned1;          // the feeder's buffers in mp3mi_batch::owned: [owned0, owned1)
    size_t ring_pitch, row_pitch;   // bytes per lane, multiples of 16
    int16_t *ring, *rows;
    size_t state_bytes, front_bytes; // of a state record; the part the front stream owns
    uint8_t *rec_front, *rec_loop;   // [S][front_bytes], [S][state_bytes - front_bytes]
    uint8_t *park_block, *resume_block; // [S][state_bytes]: the records of this tick's export / import, by position in the list
    struct lane {
        int32_t head, pending; // the ring's read position and fill, in samples per channel
        int32_t kbps;          // as given at START (0: the slot's create-time bitrate)
        bool open;             // a stream is in the lane: from the feeder's START to the tick that closes it
        bool parked;           // ... exported out of its slot (ticket, rec_front / rec_loop)
        bool draining;         // ... END has been given
        bool waiting;          // ... the batch has not seen its START yet
        int64_t frames;        // frames encoded so far
        mp3mi_slot_ticket ticket;
    };
    std::vector<lane> lanes;
    // what goes up per tick: descriptors uint32[4 S] | park list int32[S] | resume list int32[S]; a ring of four with fences, like
    // the batch's park lists
    typedef upload_ring<uint8_t, 4> up_ring;
    up_ring up;
    hipEvent_t ev_up, ev_front;
};

static void feed_drop(mp3mi_feed *f) // the handles and the object; the buffers are the batch's (mp3mi_batch::owned)
{
    for (mp3mi_feed::up_ring::entry &en : f->up.e) en.free.destroy();
    for (hipEvent_t e : {f->ev_up, f->ev_front})
        if (e) hipEventDestroy(e);
    delete f;
}

// frees the feeder's buffers and takes them off the batch's list (the device is through with them: the caller has waited)
static void feed_release_buffers(mp3mi_feed *f)
{
    mp3mi_batch *b = f->b;
    for (size_t i = f->owned1; i-- > f->owned0;) {
        if (b->owned[i].pinned) hipHostFree(b->owned[i].p);
        else hipFree(b->owned[i].p);
    }
    b->owned.erase(b->owned.begin() + (long) f->owned0, b->owned.begin() + (long) f->owned1);
    f->owned1 = f->owned0;
}

static int feed_build(mp3mi_feed *f)
{
    mp3mi_batch *b = f->b;
    const size_t S = (size_t) b->n_streams, esz = 2 * (size_t) b->channels;
    mp3mi_park_table front, loop;
    f->state_bytes = park_tables(b, &front, &loop);
    f->front_bytes = loop.n > 0 ? loop.r[0].off : f->state_bytes;
    for (int k = 0; k < front.n; k++)
        if (front.r[k].off >= f->front_bytes) return MP3MI_ERR_ARG; // (the record's order is front stream first: carried_init)
    f->ring_pitch = ((size_t) f->cap * esz + 15) & ~(size_t) 15;
    f->row_pitch = (size_t) f->full * esz; // (a frame of one channel is 2304 bytes = 16 * 144)
    CHK(dev_alloc(b, &f->ring, S * f->ring_pitch));
    CHK(dev_alloc(b, &f->rows, S * f->row_pitch));
    CHK(hipMemset(f->rows, 0, S * f->row_pitch));
    CHK(dev_alloc(b, &f->rec_front, S * f->front_bytes));
    CHK(dev_alloc(b, &f->rec_loop, S * (f->state_bytes - f->front_bytes)));
    CHK(dev_alloc(b, &f->park_block, S * f->state_bytes));
    CHK(dev_alloc(b, &f->resume_block, S * f->state_bytes));
    for (mp3mi_feed::up_ring::entry &en : f->up.e) CHK(ring_entry_create(b, en, 24 * S));
    CHK(hipEventCreateWithFlags(&f->ev_up, hipEventDisableTiming));
    CHK(hipEventCreateWithFlags(&f->ev_front, hipEventDisableTiming));
    f->lanes.assign(S, mp3mi_feed::lane());
    for (mp3mi_feed::lane &l : f->lanes) l.frames = -1;
    return MP3MI_OK;
}

extern "C" int mp3mi_feed_create(mp3mi_feed **out, mp3mi_batch *b, int tick_frames, int max_push)
{
    if (!out) return MP3MI_ERR_ARG;
    *out = NULL;
    if (!b || b->feed || tick_frames < 1 || tick_frames > b->max_frames || max_push < 1 || b->book.any_open()) return MP3MI_ERR_ARG;
    if ((int64_t) tick_frames * 1152 + max_push > INT32_MAX / 8) return MP3MI_ERR_ARG; // (a lane's bytes stay far inside 32 bits)
    ON_DEVICE(b);
    mp3mi_feed *f = new mp3mi_feed(); // value-initialised
    f->b = b;
    f->tick_frames = tick_frames;
    f->max_push = max_push;
    f->full = tick_frames * 1152;
    f->cap = f->full + max_push;
    f->owned0 = f->owned1 = b->owned.size();
    const int rc = feed_build(f);
    f->owned1 = b->owned.size();
    if (rc != MP3MI_OK) {
        feed_release_buffers(f);
        feed_drop(f);
        return rc;
    }
    b->feed = f;
    *out = f;
    return MP3MI_OK;
}

extern "C" void mp3mi_feed_destroy(mp3mi_feed *f)
{
    if (!f) return;
    mp3mi_batch *b = f->b;
    device_scope ds(b->device);
    b->feed_call = true;
    (void) mp3mi_batch_reset(b); // the streams in the slots are abandoned with the parked and the pending ones
    b->feed_call = false;
    for (hipStream_t st : {b->stream, b->lstream}) hipStreamSynchronize(st);
    feed_release_buffers(f);
    b->feed = NULL;
    feed_drop(f);
}

extern "C" size_t mp3mi_feed_capacity(const mp3mi_feed *f) { return f ? (size_t) f->cap : 0; }

extern "C" int mp3mi_feed_lanes(const mp3mi_feed *f, int32_t *pending_host, int64_t *frames_host, uint8_t *flags_host)
{
    if (!f || !pending_host || !frames_host || !flags_host) return MP3MI_ERR_ARG;
    int n = 0;
    for (size_t s = 0; s < f->lanes.size(); s++) {
        const mp3mi_feed::lane &l = f->lanes[s];
        pending_host[s] = l.open ? l.pending : 0;
        frames_host[s] = l.open ? l.frames : -1;
        flags_host[s] = (uint8_t) (l.open ? (l.parked ? 1 : 0) | (l.draining ? 2 : 0) | (l.waiting ? 4 : 0) : 0);
        n += l.open;
    }
    return n;
}

extern "C" int mp3mi_feed_tick(mp3mi_feed *f, const int16_t *pcm_dev, size_t pcm_pitch, const uint8_t *ctl_host, const int32_t *n_push_host,
                               const int32_t *kbps_host, uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev)
{
    if (!f || !pcm_dev || !ctl_host || !out_dev || !out_len_dev) return MP3MI_ERR_ARG;
    mp3mi_batch *b = f->b;
    if (pcm_pitch < (size_t) f->max_push || out_stride < mp3mi_batch_out_stride(b, f->tick_frames)) return MP3MI_ERR_ARG;
    const int S = b->n_streams;
    const size_t esz = 2 * (size_t) b->channels;
    // ---- 1. the rules, over all lanes, before anything changes state; 2. who encodes ----
    std::vector<mp3mi_feed::lane> nl(f->lanes); // the lanes behind the tick
    std::vector<uint32_t> desc(4 * (size_t) S, 0u);
    std::vector<uint8_t> ctl((size_t) S, 0);
    std::vector<int32_t> ns((size_t) S, 0), kb((size_t) S, 0), park, resume;
    size_t most = 0;
    bool any_move = false, any_ready = false;
    for (int s = 0; s < S; s++) {
        mp3mi_feed::lane &l = nl[s];
        const int c = ctl_host[s];
        const int32_t n = n_push_host ? n_push_host[s] : 0, k = kbps_host ? kbps_host[s] : 0;
        if ((c & ~(MP3MI_SLOT_START | MP3MI_SLOT_END)) || n < 0 || n > f->max_push) return MP3MI_ERR_ARG;
        const bool start = c & MP3MI_SLOT_START, end = c & MP3MI_SLOT_END;
        if (l.open && l.draining && (start || end || n != 0)) return MP3MI_ERR_ARG; // its samples are all in
        if (!l.open && !start && (end || n != 0)) return MP3MI_ERR_ARG;
        int bi, bits;
        if (start ? (k != 0 && (k > b->ceil_kbps || !rate_of_kbps(b->rate_idx, k, &bi, &bits)))
                  : (k != 0 && !(l.open && k == (l.kbps ? l.kbps : b->kbps_h[s]))))
            return MP3MI_ERR_ARG;
        bool in_slot = l.open && !l.parked && !l.waiting; // a stream is open in the batch's slot
        if (start) { // a new stream; one that is open in the lane is abandoned with its pending samples and its parked record
            l.open = l.waiting = true;
            l.parked = l.draining = false;
            l.head = l.pending = 0;
            l.kbps = k;
            l.frames = 0;
        }
        if ((int64_t) l.pending + n > f->cap) return MP3MI_ERR_ARG;
        if (!l.open) continue;
        if (end) l.draining = true;
        const int32_t have = l.pending + n;
        const bool closes = l.draining && have <= f->full, ready = closes || have >= f->full;
        const int32_t take = !ready ? 0 : closes ? have : f->full;
        desc[4 * s] = (uint32_t) l.head; desc[4 * s + 1] = (uint32_t) l.pending; desc[4 * s + 2] = (uint32_t) n; desc[4 * s + 3] = (uint32_t) take;
        if (n || take) {
            const size_t longest = (size_t) (take > n ? take : n) * esz;
            most = longest > most ? longest : most;
            any_move = true;
        }
        l.head = (int32_t) (((int64_t) l.head + take) % f->cap);
        l.pending = have - take;
        if (ready) {
            any_ready = true;
            ctl[s] = (uint8_t) ((l.waiting ? MP3MI_SLOT_START : 0) | (closes ? MP3MI_SLOT_END : 0));
            ns[s] = take;
            kb[s] = l.waiting ? l.kbps : 0;
            if (l.parked) resume.push_back(s);
            l.parked = l.waiting = false;
            l.frames += closes ? (take + 1151) / 1152 : f->tick_frames;
            if (closes) { l.open = false; l.frames = -1; }
        } else if (in_slot) { // sits out (or was abandoned for a stream that is not ready): out of its slot
            park.push_back(s);
            l.parked = !start;
        }
    }
    ON_DEVICE(b);
    // ---- 3. / 4. the descriptors and the two lists go up; k_feed ----
    mp3mi_feed::up_ring::entry &en = f->up.take();
    const bool lists = !park.empty() || !resume.empty();
    int32_t *park_dev = (int32_t *) (en.dev + 16 * (size_t) S), *resume_dev = park_dev + S;
    if (any_move || lists) {
        // (the readers of the entry, four ticks ago: as a rule long through, and then the host neither waits nor lets a held k_loop go)
        if (!en.free.done()) {
            hold_release(b);
            CHK(en.free.sync());
        }
        memcpy(en.stage, desc.data(), 16 * (size_t) S);
        memset(en.stage + 16 * (size_t) S, 0, 8 * (size_t) S);
        if (!park.empty()) memcpy(en.stage + 16 * (size_t) S, park.data(), sizeof(int32_t) * park.size());
        if (!resume.empty()) memcpy(en.stage + 20 * (size_t) S, resume.data(), sizeof(int32_t) * resume.size());
        CHK(hipMemcpyAsync(en.dev, en.stage, 24 * (size_t) S, hipMemcpyHostToDevice, b->stream));
        if (any_move) {
            mp3mi_launch_feed(en.dev, S, f->ring, f->ring_pitch, f->cap, b->channels, pcm_dev, pcm_pitch * esz, f->rows, f->row_pitch, most, b->stream);
            CHK(hipGetLastError());
        }
        CHK(hipEventRecord(f->ev_up, b->stream));
        if (lists) CHK(hipStreamWaitEvent(b->lstream, f->ev_up, 0));
    }
    // the one-region tables of the records per lane: region bytes = the part's size, so lane s's part lies at base + s * bytes
    mp3mi_park_table tf, tl;
    memset(&tf, 0, sizeof(tf));
    memset(&tl, 0, sizeof(tl));
    tf.r[0] = {f->rec_front, (uint32_t) f->front_bytes, 0u};
    tl.r[0] = {f->rec_loop, (uint32_t) (f->state_bytes - f->front_bytes), (uint32_t) f->front_bytes};
    tf.n = f->front_bytes ? 1 : 0;
    tl.n = f->state_bytes > f->front_bytes ? 1 : 0;
    std::vector<mp3mi_slot_ticket> tk(park.size() > resume.size() ? park.size() : resume.size());
    int rc = MP3MI_OK;
    b->feed_call = true;
    // ---- 5. the lanes that sit out leave their slots ----
    if (!park.empty()) {
        rc = mp3mi_batch_slots_export(b, (int) park.size(), park.data(), 1, f->park_block, f->state_bytes, tk.data());
        if (rc == MP3MI_OK) {
            for (size_t i = 0; i < park.size(); i++) nl[park[i]].ticket = tk[i];
            mp3mi_launch_slot_park(park_dev, (int) park.size(), tf, f->park_block, f->state_bytes, 0, b->stream);
            mp3mi_launch_slot_park(park_dev, (int) park.size(), tl, f->park_block, f->state_bytes, 0, b->lstream);
            if (hipGetLastError() != hipSuccess) rc = MP3MI_ERR_HIP;
        }
    }
    // ---- 6. the parked lanes that are ready come back ----
    if (rc == MP3MI_OK && !resume.empty()) {
        for (size_t i = 0; i < resume.size(); i++) tk[i] = f->lanes[resume[i]].ticket;
        mp3mi_launch_slot_park(resume_dev, (int) resume.size(), tf, f->resume_block, f->state_bytes, 1, b->stream);
        mp3mi_launch_slot_park(resume_dev, (int) resume.size(), tl, f->resume_block, f->state_bytes, 1, b->lstream);
        if (hipGetLastError() != hipSuccess) rc = MP3MI_ERR_HIP;
        if (rc == MP3MI_OK) rc = mp3mi_batch_slots_import(b, (int) resume.size(), resume.data(), f->resume_block, f->state_bytes, tk.data());
    }
    // ---- 7. one per-slot call on the feeder's rows: the ready lanes; every other slot is closed ----
    if (rc == MP3MI_OK && any_ready)
        rc = mp3mi_batch_encode_slots_kbps(b, f->rows, f->tick_frames, ctl.data(), ns.data(), kb.data(), out_dev, out_stride, out_len_dev);
    b->feed_call = false;
    if (rc != MP3MI_OK) return rc;
    if (!any_ready) {
        // nothing encodes: no lengths but zeros, in stream order; and no next call's transforms will let a held k_loop go
        hold_release(b);
        CHK(hipMemsetAsync(out_len_dev, 0, sizeof(uint32_t) * (size_t) S, b->lstream));
    }
    if (any_move || lists) { // the entry's fence behind its readers on both streams
        CHK(hipEventRecord(f->ev_front, b->stream));
        CHK(hipStreamWaitEvent(b->lstream, f->ev_front, 0));
        CHK(en.free.record(b->lstream));
        f->up.next();
    }
    f->lanes.swap(nl);
    return MP3MI_OK;
}
