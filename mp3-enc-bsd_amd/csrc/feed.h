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
//
// The first half of this file is the feeder whose lane s IS slot s (mp3mi_feed_create, mp3mi_feed_tick), untouched by the second:
// more lanes than slots (mp3mi_feed_create_lanes, mp3mi_feed_tick_lanes), with the indirection lane -> slot, the scheduler and
// k_feed_lanes over the lanes that move.  They share the object, its buffers (feed_build: sized by lanes or by slots), the records
// per lane and mp3mi_feed_lanes / mp3mi_feed_destroy; each kind has its own tick, and the old one allocates and launches what it did.

#include <algorithm>
#include <utility>

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
        // more lanes than slots (below): the slot that holds the lane's stream (an abandoned one while `waiting`), -1: none; the
        // tick in which the lane's unbroken spell of being ready began, -1: it was not ready in the last tick, or encoded in it
        bool wait_slot;    // ready in the last tick and left without a slot
        bool seen, chosen; // (within a tick) among the tick's lanes; encodes in this tick
        int32_t slot;
        int64_t since;
    };
    std::vector<lane> lanes;
    // more lanes than slots (mp3mi_feed_create_lanes; the second half of this file)
    bool lanes_mode;
    int n_lanes, max_rows;
    int64_t tick_no;
    std::vector<int32_t> slot_lane; // [S]: the lane whose stream is open in the slot, -1: none
    std::vector<int32_t> hot;       // ascending: the lanes that are ready without a push (a tick pending, or draining)
    // what goes up per tick: descriptors uint32[4 S] | park list int32[S] | resume list int32[S]; a ring of four with fences, like
    // the batch's park lists
    typedef upload_ring<uint8_t, 4> up_ring;
    up_ring up;
    hipEvent_t ev_up, ev_front;
    // ticks on host buffers (mp3mi_feed_tick_lanes_host_async; the third part of this file): two copy streams and two tick slots of
    // the feeder's own, created with the first such tick and freed with the feeder (by hand, not through mp3mi_batch::owned, whose
    // range [owned0, owned1) is closed at create)
    struct host_ticks {
        bool ready;
        hipStream_t h2d, d2h;
        size_t dev_stride;            // mp3mi_batch_out_stride(b, tick_frames): of tick_slot::out
        struct tick_slot {
            int16_t *stage;           // the tick's packets back to back: max_rows * max_push samples of all channels
            uint8_t *out;             // [S][dev_stride]: what the per-slot call writes
            uint32_t *len;            // [S]
            uint8_t *out_rows;        // [n_out][the caller's out_stride]: grows with the caller's stride
            size_t out_rows_cap;      // bytes
            uint32_t *len_rows;       // [S]
            fence stage_free, out_free; // the staging has been read by k_feed_packed / the dense rows by the download
            hipEvent_t ev_enc;        // the loop stream has gathered the tick's rows (k_rows_out)
            hipEvent_t t_up[2], t_dn[2]; // around the upload and around the download (the second is what consumers wait for)
            bool pending, up, dn;     // a tick of this slot has not been harvested; it uploaded samples; it downloaded rows
            double bytes_up, bytes_dn;
        } slot[2];
        unsigned tick_no;             // host ticks issued
        double tot_up_bytes, tot_dn_bytes, tot_up_ms, tot_dn_ms;
        long tot_calls;
    } ht;
};

static void feed_host_free(mp3mi_feed *f);

static void feed_drop(mp3mi_feed *f) // the handles and the object; the buffers are the batch's (mp3mi_batch::owned)
{
    feed_host_free(f); // (but for those of the ticks on host buffers)
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

// n_lanes rings and records per lane; rows and the two dense record blocks per slot; up_bytes: an upload block
static int feed_build(mp3mi_feed *f, size_t n_lanes, size_t up_bytes)
{
    mp3mi_batch *b = f->b;
    const size_t S = (size_t) b->n_streams, L = n_lanes, esz = 2 * (size_t) b->channels;
    mp3mi_park_table front, loop;
    f->state_bytes = park_tables(b, &front, &loop);
    f->front_bytes = loop.n > 0 ? loop.r[0].off : f->state_bytes;
    for (int k = 0; k < front.n; k++)
        if (front.r[k].off >= f->front_bytes) return MP3MI_ERR_ARG; // (the record's order is front stream first: carried_init)
    f->ring_pitch = ((size_t) f->cap * esz + 15) & ~(size_t) 15;
    f->row_pitch = (size_t) f->full * esz; // (a frame of one channel is 2304 bytes = 16 * 144)
    CHK(dev_alloc(b, &f->ring, L * f->ring_pitch));
    CHK(dev_alloc(b, &f->rows, S * f->row_pitch));
    CHK(hipMemset(f->rows, 0, S * f->row_pitch));
    CHK(dev_alloc(b, &f->rec_front, L * f->front_bytes));
    CHK(dev_alloc(b, &f->rec_loop, L * (f->state_bytes - f->front_bytes)));
    CHK(dev_alloc(b, &f->park_block, S * f->state_bytes));
    CHK(dev_alloc(b, &f->resume_block, S * f->state_bytes));
    for (mp3mi_feed::up_ring::entry &en : f->up.e) CHK(ring_entry_create(b, en, up_bytes));
    CHK(hipEventCreateWithFlags(&f->ev_up, hipEventDisableTiming));
    CHK(hipEventCreateWithFlags(&f->ev_front, hipEventDisableTiming));
    f->lanes.assign(L, mp3mi_feed::lane());
    for (mp3mi_feed::lane &l : f->lanes) {
        l.frames = l.since = -1;
        l.slot = -1;
    }
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
    const int rc = feed_build(f, (size_t) b->n_streams, 24 * (size_t) b->n_streams);
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
    (void) feed_host_sync(f);
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
        flags_host[s] = (uint8_t) (l.open ? (l.parked ? 1 : 0) | (l.draining ? 2 : 0) | (l.waiting ? 4 : 0) | (l.wait_slot ? 8 : 0) : 0);
        n += l.open;
    }
    return n;
}

// Steps 5 and 6 of a tick, of either feeder: the streams that do not encode leave their slots, the parked lanes that encode enter
// free ones.  The SLOT lists go to the export and the import, the LANE lists -- park_dev / resume_dev: their device copies, in the
// tick's upload block -- to the scatter and the gather between the dense blocks and the records per lane (mp3mi_feed_tick: a lane
// is its slot, and the lists are the same).  after: the lanes behind the tick, which take the leaving streams' tickets.
static int feed_park_resume(mp3mi_feed *f, const std::vector<int32_t> &park_slots, const std::vector<int32_t> &park_lanes, const int32_t *park_dev,
                            const std::vector<int32_t> &resume_slots, const std::vector<int32_t> &resume_lanes, const int32_t *resume_dev,
                            std::vector<mp3mi_feed::lane> &after)
{
    mp3mi_batch *b = f->b;
    // the one-region tables of the records per lane: region bytes = the part's size, so lane l's part lies at base + l * bytes
    mp3mi_park_table tf, tl;
    memset(&tf, 0, sizeof(tf));
    memset(&tl, 0, sizeof(tl));
    tf.r[0] = {f->rec_front, (uint32_t) f->front_bytes, 0u};
    tl.r[0] = {f->rec_loop, (uint32_t) (f->state_bytes - f->front_bytes), (uint32_t) f->front_bytes};
    tf.n = f->front_bytes ? 1 : 0;
    tl.n = f->state_bytes > f->front_bytes ? 1 : 0;
    std::vector<mp3mi_slot_ticket> tk(park_lanes.size() > resume_lanes.size() ? park_lanes.size() : resume_lanes.size());
    int rc = MP3MI_OK;
    // ---- 5. the streams that do not encode leave their slots: the SLOT list to the export, the LANE list to the scatter ----
    if (!park_slots.empty()) {
        rc = mp3mi_batch_slots_export(b, (int) park_slots.size(), park_slots.data(), 1, f->park_block, f->state_bytes, tk.data());
        if (rc == MP3MI_OK) {
            for (size_t i = 0; i < park_lanes.size(); i++) after[park_lanes[i]].ticket = tk[i];
            mp3mi_launch_slot_park(park_dev, (int) park_lanes.size(), tf, f->park_block, f->state_bytes, 0, b->stream);
            mp3mi_launch_slot_park(park_dev, (int) park_lanes.size(), tl, f->park_block, f->state_bytes, 0, b->lstream);
            if (hipGetLastError() != hipSuccess) rc = MP3MI_ERR_HIP;
        }
    }
    // ---- 6. the parked lanes that encode enter the free slots -- slots this tick's export vacated among them ----
    if (rc == MP3MI_OK && !resume_slots.empty()) {
        for (size_t i = 0; i < resume_lanes.size(); i++) tk[i] = f->lanes[resume_lanes[i]].ticket;
        mp3mi_launch_slot_park(resume_dev, (int) resume_lanes.size(), tf, f->resume_block, f->state_bytes, 1, b->stream);
        mp3mi_launch_slot_park(resume_dev, (int) resume_lanes.size(), tl, f->resume_block, f->state_bytes, 1, b->lstream);
        if (hipGetLastError() != hipSuccess) rc = MP3MI_ERR_HIP;
        if (rc == MP3MI_OK)
            rc = mp3mi_batch_slots_import(b, (int) resume_slots.size(), resume_slots.data(), f->resume_block, f->state_bytes, tk.data());
    }
    return rc;
}

extern "C" int mp3mi_feed_tick(mp3mi_feed *f, const int16_t *pcm_dev, size_t pcm_pitch, const uint8_t *ctl_host, const int32_t *n_push_host,
                               const int32_t *kbps_host, uint8_t *out_dev, size_t out_stride, uint32_t *out_len_dev)
{
    if (!f || f->lanes_mode || !pcm_dev || !ctl_host || !out_dev || !out_len_dev) return MP3MI_ERR_ARG; // (lanes: mp3mi_feed_tick_lanes)
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
    b->feed_call = true;
    // ---- 5. the lanes that sit out leave their slots; 6. the parked lanes that are ready come back ----
    int rc = feed_park_resume(f, park, park, park_dev, resume, resume, resume_dev, nl);
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

// ---- more lanes than slots (mp3mi_feed_create_lanes, mp3mi_feed_tick_lanes) ----
// A lane is no longer a slot.  Rings, records per lane, tickets and the lane table are sized by n_lanes; the rows and the two dense
// record blocks stay sized by the batch's slots, since no more than n_streams streams encode, leave or enter in one tick.  On the
// host the feeder keeps lane -> slot (lane::slot) and slot -> lane (slot_lane), and the HOT list: the lanes that are ready whether
// or not they push (a tick pending, or draining).  A tick looks at the hot lanes, the lanes its rows name and the lanes in slots
// -- never at all lanes: with 100 of 100 000 lanes pushing it touches those 100, the few that wait and the slots.
//
// Who encodes: the ready lanes, and with more of them than slots the n_streams whose spell of being ready began first (lane::since;
// ties to the lower lane).  A lane that encodes ends its spell, so a lane that is ready all the time queues behind every lane that
// was ready before it: round robin.  Where: a chosen lane keeps the slot its stream is in; every other stream in a slot leaves
// (export with close, as a lane that sits out in mp3mi_feed_tick); the other chosen lanes take the free slots, lowest slot to
// lowest lane, by import (parked) or by the per-slot call's START (not yet in the batch).
//
// A slot vacated and refilled in ONE tick.  The launches of a tick are, on each of the batch's two HIP streams and in this order:
// the export's k_slot_park (slot regions -> park_block), the scatter (park_block -> the leaving lanes' records), the gather (the
// entering lanes' records -> resume_block), the import's k_slot_park (resume_block -> slot regions), the per-slot call with its
// k_slot_begin for the STARTs.  Each stream moves only the regions it owns (park_run), and a stream runs its launches in order:
// the import or the START that writes slot k's regions on a stream is behind the export that read them on THAT stream, which is all
// that "a record may be imported into the batch that exported it at once" (mp3mi.h) asks.  The leaving and the entering lanes of a
// tick are different lanes, so scatter and gather touch different records; park_block and resume_block are written and read in
// the same order tick after tick, each part on one stream only.  The rows are by slot and k_feed_lanes, their only writer, runs
// on the front stream behind the per-slot call of the tick before, their only reader -- as k_feed does.
//
// The upload block of a tick: park lanes int32[S] | resume lanes int32[S] | (to a multiple of 16) | descriptors 32 bytes each, for
// at most max_rows + S lanes that move (those that push, those that take).  The slot lists of export and import go up with those
// calls (park_run).  One copy per tick, of the lists and the descriptors in use.

//
// A tick on host buffers (below) sends two more things up in the same block, behind the descriptors: the work list of k_feed_packed,
// at most MP3MI_FEED_MAX_PARTS items of 8 bytes per descriptor, and the slots of the lanes that encode, int32[S], for k_rows_out.

static inline size_t feed_lists_bytes(const mp3mi_feed *f) { return (8 * (size_t) f->b->n_streams + 15) & ~(size_t) 15; }
static inline size_t feed_block_bytes(const mp3mi_feed *f)
{
    const size_t most_active = (size_t) f->max_rows + (size_t) f->b->n_streams;
    return feed_lists_bytes(f) + (32 + 8 * (size_t) MP3MI_FEED_MAX_PARTS) * most_active + 4 * (size_t) f->b->n_streams;
}

extern "C" int mp3mi_feed_create_lanes(mp3mi_feed **out, mp3mi_batch *b, int n_lanes, int max_rows, int tick_frames, int max_push, int ring_samples)
{
    if (!out) return MP3MI_ERR_ARG;
    *out = NULL;
    if (!b || b->feed || tick_frames < 1 || tick_frames > b->max_frames || max_push < 1 || b->book.any_open()) return MP3MI_ERR_ARG;
    if (n_lanes < 1 || max_rows < 1 || max_rows > n_lanes || ring_samples < 0) return MP3MI_ERR_ARG;
    const int64_t least = (int64_t) tick_frames * 1152 + max_push, cap = ring_samples ? ring_samples : least;
    if (cap < least || cap > INT32_MAX / 8) return MP3MI_ERR_ARG; // (a lane's bytes stay far inside 32 bits)
    ON_DEVICE(b);
    mp3mi_feed *f = new mp3mi_feed(); // value-initialised
    f->b = b;
    f->lanes_mode = true;
    f->n_lanes = n_lanes;
    f->max_rows = max_rows;
    f->tick_frames = tick_frames;
    f->max_push = max_push;
    f->full = tick_frames * 1152;
    f->cap = (int) cap;
    f->owned0 = f->owned1 = b->owned.size();
    const int rc = feed_build(f, (size_t) n_lanes, feed_block_bytes(f));
    f->owned1 = b->owned.size();
    if (rc != MP3MI_OK) {
        feed_release_buffers(f);
        feed_drop(f);
        return rc;
    }
    f->slot_lane.assign((size_t) b->n_streams, -1);
    b->feed = f;
    *out = f;
    return MP3MI_OK;
}

extern "C" int mp3mi_feed_n_lanes(const mp3mi_feed *f) { return f ? (int) f->lanes.size() : 0; }

// What a tick on host buffers adds to a tick (mp3mi_feed_tick_lanes_host_async, below): the caller's packed samples and their count,
// the caller's dense output with its stride, and the two lists it is told.  The tick itself -- the rules, who encodes and where, the
// lists, the parking, the per-slot call -- is feed_tick_lanes_impl for both kinds; hc == NULL is the tick on device buffers.
struct feed_host_call {
    const int16_t *pcm;
    size_t n_pushed;      // samples per channel of all rows
    uint8_t *out;
    size_t out_stride;
    uint32_t *out_len;
    int32_t *out_lane, *out_slot, *n_out;
};
static int feed_host_begin(mp3mi_feed *f, const feed_host_call *hc);

static int feed_tick_lanes_impl(mp3mi_feed *f, int n_rows, const int32_t *row_lane_host, const int16_t *pcm_dev, size_t pcm_pitch,
                                const uint8_t *ctl_host, const int32_t *n_push_host, const int32_t *kbps_host, uint8_t *out_dev, size_t out_stride,
                                uint32_t *out_len_dev, int32_t *slot_lane_host, const feed_host_call *hc)
{
    mp3mi_batch *b = f->b;
    const int S = b->n_streams, L = f->n_lanes;
    const size_t esz = 2 * (size_t) b->channels;
    typedef mp3mi_feed::lane lane;
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
        int bi, bits;
        // (a stream that STARTed at kbps 0 has the create-time bitrate of the slot it first encodes in: known from then on)
        if (start ? (k != 0 && (k > b->ceil_kbps || !rate_of_kbps(b->rate_idx, k, &bi, &bits))) : (k != 0 && !(l.open && l.kbps != 0 && k == l.kbps)))
            return MP3MI_ERR_ARG;
        if ((int64_t) (start ? 0 : l.pending) + n > f->cap) return MP3MI_ERR_ARG;
    }
    // (a tick on host buffers: its copy streams and the tick slot of its turn, whose buffers stand in for the caller's device ones;
    // row r's samples begin at sample first[r] of the slot's staging)
    std::vector<uint32_t> first;
    std::vector<int32_t> by_slot;
    if (hc) {
        const int rc = feed_host_begin(f, hc);
        if (rc != MP3MI_OK) return rc;
        mp3mi_feed::host_ticks::tick_slot &io = f->ht.slot[f->ht.tick_no & 1u];
        out_dev = io.out;
        out_stride = f->ht.dev_stride;
        out_len_dev = io.len;
        by_slot.assign((size_t) S, -1);
        slot_lane_host = by_slot.data();
        first.assign((size_t) n_rows, 0u);
        for (int r = 1; r < n_rows; r++) first[r] = first[r - 1] + (uint32_t) n_push_host[r - 1];
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
        if (ctl & MP3MI_SLOT_START) { // a new stream; one that is open in the lane is abandoned: its samples, its record -- and its slot,
            l.open = l.waiting = true; // where it has one, with this tick: to this lane's START if it is chosen, else by the export
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
    // ---- 3. the slots: who stays, who leaves, who enters ----
    std::vector<int32_t> park_slots, park_lanes, resume_slots, resume_lanes, free_slots;
    for (int s = 0; s < S; s++) {
        const int32_t ln = f->slot_lane[s];
        if (ln >= 0 && !f->lanes[ln].chosen) { // sits out, waits for a slot, or was abandoned for a stream that does not encode now
            lane &l = f->lanes[ln];
            if (!l.seen) undo.push_back(std::make_pair(ln, l)); // (a lane of no row that is not hot)
            park_slots.push_back(s);
            park_lanes.push_back(ln);
            l.parked = !l.waiting;
            l.slot = -1;
            f->slot_lane[s] = -1;
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
        if (l.chosen) {
            take = c.closes ? c.have : f->full;
            if (l.slot < 0) { // the lowest free slot to the lowest lane
                l.slot = free_slots[n_free++];
                if (l.parked) {
                    resume_slots.push_back(l.slot);
                    resume_lanes.push_back(c.ln);
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
            l.frames += c.closes ? (take + 1151) / 1152 : f->tick_frames;
        } else
            l.wait_slot = c.ready;
        if (c.n || take) {
            const uint32_t d[8] = {(uint32_t) c.head0, (uint32_t) c.pend0, (uint32_t) c.n, (uint32_t) take,
                                   (uint32_t) c.ln, c.n ? (hc ? first[c.row] : (uint32_t) c.row) : 0u, (uint32_t) (take ? l.slot : 0), 0u};
            desc.insert(desc.end(), d, d + 8);
            const size_t longest = (size_t) (take > c.n ? take : c.n) * esz;
            most = longest > most ? longest : most;
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
    const size_t n_active = desc.size() / 8;
    auto fail = [&](int rc) { // the books as they were
        for (size_t i = undo.size(); i-- > 0;) f->lanes[undo[i].first] = undo[i].second;
        f->slot_lane = slot_lane0;
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
    // ---- 4. the lists and the descriptors go up; k_feed_lanes over the lanes that move ----
    mp3mi_feed::up_ring::entry &en = f->up.take();
    const bool lists = !park_lanes.empty() || !resume_lanes.empty();
    const size_t lb = feed_lists_bytes(f);
    int32_t *park_dev = (int32_t *) en.dev, *resume_dev = park_dev + S;
    // (a tick on host buffers: the lanes that encode, ascending, and their slots -- told to the caller now, and the slots sent up
    // for k_rows_out behind the work list of k_feed_packed)
    mp3mi_feed::host_ticks::tick_slot *io = hc ? &f->ht.slot[f->ht.tick_no & 1u] : NULL;
    std::vector<uint32_t> work;
    size_t n_items = 0, n_out = 0;
    if (hc) {
        std::vector<std::pair<int32_t, int32_t> > enc;
        for (int s = 0; s < S; s++)
            if (slot_lane_host[s] >= 0) enc.push_back(std::make_pair(slot_lane_host[s], (int32_t) s));
        std::sort(enc.begin(), enc.end());
        n_out = enc.size();
        for (size_t i = 0; i < n_out; i++) {
            hc->out_lane[i] = enc[i].first;
            hc->out_slot[i] = enc[i].second;
        }
        *hc->n_out = (int32_t) n_out;
        work.resize(2 * (size_t) MP3MI_FEED_MAX_PARTS * n_active + 1);
        n_items = mp3mi_feed_work_list(desc.data(), n_active, esz, MP3MI_FEED_WG_BYTES, work.data());
    }
    if (n_active || lists || n_out) {
        // The one place this call can block: the entry's readers, four ticks ago.  As a rule they are long through, and then the host
        // neither waits nor lets a held k_loop go.  Where it must wait, the fence may be queued behind the held k_loop of the last
        // per-slot call, which spins on its flag until the host lets it go: the host does that FIRST and waits then, so the wait ends.
        if (!en.free.done()) {
            hold_release(b);
            FCHK(en.free.sync());
        }
        memset(en.stage, 0, lb);
        if (!park_lanes.empty()) memcpy(en.stage, park_lanes.data(), sizeof(int32_t) * park_lanes.size());
        if (!resume_lanes.empty()) memcpy(en.stage + 4 * (size_t) S, resume_lanes.data(), sizeof(int32_t) * resume_lanes.size());
        if (n_active) memcpy(en.stage + lb, desc.data(), 32 * n_active);
        const size_t work_at = lb + 32 * n_active, slots_at = work_at + 8 * n_items;
        if (n_items) memcpy(en.stage + work_at, work.data(), 8 * n_items);
        if (n_out) memcpy(en.stage + slots_at, hc->out_slot, sizeof(int32_t) * n_out);
        FCHK(hipMemcpyAsync(en.dev, en.stage, slots_at + sizeof(int32_t) * n_out, hipMemcpyHostToDevice, b->stream));
        if (hc && hc->n_pushed) { // the tick's packets, as they are: one copy on the feeder's upload stream, beside whatever runs
            FCHK(hipEventRecord(io->t_up[0], f->ht.h2d));
            FCHK(hipMemcpyAsync(io->stage, hc->pcm, hc->n_pushed * esz, hipMemcpyHostToDevice, f->ht.h2d));
            FCHK(hipEventRecord(io->t_up[1], f->ht.h2d));
            FCHK(hipStreamWaitEvent(b->stream, io->t_up[1], 0));
        }
        if (n_active && hc) {
            mp3mi_launch_feed_packed(en.dev + lb, en.dev + work_at, (int) n_items, f->ring, f->ring_pitch, f->cap, b->channels, io->stage, f->rows,
                                     f->row_pitch, b->stream);
            FCHK(hipGetLastError());
            if (hc->n_pushed) FCHK(io->stage_free.record(b->stream));
        } else if (n_active) {
            mp3mi_launch_feed_lanes(en.dev + lb, (int) n_active, f->ring, f->ring_pitch, f->cap, b->channels, pcm_dev, pcm_pitch * esz, f->rows,
                                    f->row_pitch, most, b->stream);
            FCHK(hipGetLastError());
        }
        FCHK(hipEventRecord(f->ev_up, b->stream));
        if (lists) FCHK(hipStreamWaitEvent(b->lstream, f->ev_up, 0));
    }
    b->feed_call = true;
    // ---- 5. the streams that do not encode leave their slots; 6. the parked lanes that encode enter the free slots ----
    int rc = feed_park_resume(f, park_slots, park_lanes, park_dev, resume_slots, resume_lanes, resume_dev, f->lanes);
    // ---- 7. one per-slot call on the feeder's rows: the chosen lanes' slots; every other slot is closed ----
    b->feed_host_call = hc != NULL;
    if (rc == MP3MI_OK && any_ready)
        rc = mp3mi_batch_encode_slots_kbps(b, f->rows, f->tick_frames, ctl.data(), ns.data(), kb.data(), out_dev, out_stride, out_len_dev);
    b->feed_call = b->feed_host_call = false;
    if (rc != MP3MI_OK) return fail(rc);
    if (!any_ready) {
        // nothing encodes: no lengths but zeros, in stream order; and no next call's transforms will let a held k_loop go
        hold_release(b);
        if (!hc) FCHK(hipMemsetAsync(out_len_dev, 0, sizeof(uint32_t) * (size_t) S, b->lstream)); // (a host tick downloads no row then)
    }
    if (n_out) {
        // the download, behind the per-slot call on the loop stream: the encoding slots' bytes and lengths into dense rows of the
        // caller's stride, by encoding lane (k_rows_out zeroes a row behind its length), and from there two plain copies on the
        // feeder's download stream
        mp3mi_launch_rows_out((const int32_t *) (en.dev + lb + 32 * n_active + 8 * n_items), (int) n_out, out_dev, out_stride, out_len_dev, io->out_rows,
                              hc->out_stride, io->len_rows, b->lstream);
        FCHK(hipGetLastError());
        FCHK(hipEventRecord(io->ev_enc, b->lstream));
        FCHK(hipStreamWaitEvent(f->ht.d2h, io->ev_enc, 0));
        FCHK(hipEventRecord(io->t_dn[0], f->ht.d2h));
        FCHK(hipMemcpyAsync(hc->out, io->out_rows, hc->out_stride * n_out, hipMemcpyDeviceToHost, f->ht.d2h));
        FCHK(hipMemcpyAsync(hc->out_len, io->len_rows, sizeof(uint32_t) * n_out, hipMemcpyDeviceToHost, f->ht.d2h));
        FCHK(hipEventRecord(io->t_dn[1], f->ht.d2h));
        FCHK(io->out_free.record(f->ht.d2h));
    }
    if (n_active || lists || n_out) { // the entry's fence behind its readers on both streams
        FCHK(hipEventRecord(f->ev_front, b->stream));
        FCHK(hipStreamWaitEvent(b->lstream, f->ev_front, 0));
        FCHK(en.free.record(b->lstream));
        f->up.next();
    }
#undef FCHK
    f->hot.swap(hot);
    f->tick_no++;
    if (hc) { // the tick has taken its slot
        io->pending = true;
        io->up = hc->n_pushed != 0;
        io->dn = n_out != 0;
        io->bytes_up = (double) (hc->n_pushed * esz);
        io->bytes_dn = (double) n_out * (double) (hc->out_stride + sizeof(uint32_t));
        f->ht.tick_no++;
    }
    return MP3MI_OK;
}

extern "C" int mp3mi_feed_tick_lanes(mp3mi_feed *f, int n_rows, const int32_t *row_lane_host, const int16_t *pcm_dev, size_t pcm_pitch,
                                     const uint8_t *ctl_host, const int32_t *n_push_host, const int32_t *kbps_host, uint8_t *out_dev,
                                     size_t out_stride, uint32_t *out_len_dev, int32_t *slot_lane_host)
{
    if (!f || !f->lanes_mode || !out_dev || !out_len_dev || !slot_lane_host) return MP3MI_ERR_ARG; // (no lanes: mp3mi_feed_tick)
    mp3mi_batch *b = f->b;
    if (n_rows < 0 || n_rows > f->max_rows || out_stride < mp3mi_batch_out_stride(b, f->tick_frames)) return MP3MI_ERR_ARG;
    if (n_rows > 0 && (!row_lane_host || !pcm_dev || !ctl_host || !n_push_host || !kbps_host || pcm_pitch < (size_t) f->max_push)) return MP3MI_ERR_ARG;
    return feed_tick_lanes_impl(f, n_rows, row_lane_host, pcm_dev, pcm_pitch, ctl_host, n_push_host, kbps_host, out_dev, out_stride, out_len_dev,
                                slot_lane_host, NULL);
}

// ---- ticks on host buffers (mp3mi_feed_tick_lanes_host_async, mp3mi_feed_host_wait, mp3mi_feed_host_io_stats) ----
// A server has its packets in host memory and writes MP3 bytes from host memory.  The tick is the tick above; what differs is where
// the samples come from and where the bytes go.
//   upload stream (the feeder's)    the tick's packets, PACKED -- sum(n_push) samples, one copy -- into the tick slot's staging | event
//   front stream                    the upload block (lists, descriptors, work list, encoding slots) | waits for that event |
//                                   k_feed_packed: staging -> rings and rows | ... the tick as above, the per-slot call writing the
//                                   tick slot's out [S][device stride] and len [S]
//   loop stream                     ... behind the per-slot call's k_stream_tail: k_rows_out, the encoding slots' rows -> dense rows
//                                   of the caller's stride, by encoding lane | event
//   download stream (the feeder's)  waits for that event | dense rows -> out_host, lengths -> out_len_host: n_out of each
// Orderings the tick rests on.  The rings and the rows are written by k_feed_packed and k_feed_lanes alike on the front stream only,
// so device ticks and host ticks may alternate.  A tick slot -- staging, out, len, dense rows -- is used by every second host tick;
// before the slot is used again the HOST has seen the fences of its last tick (staging read, rows downloaded), so no stream waits
// for another on that account.  That wait is the one place a host tick may block beyond the upload block's; as there, the fences
// are queried first, and only when one is not through does the host let a held k_loop go, and then wait: the download is queued
// behind the tick's per-slot call, whose last k_loop may be the one that is held.
static void feed_host_free(mp3mi_feed *f)
{
    mp3mi_feed::host_ticks &H = f->ht;
    for (hipStream_t st : {H.h2d, H.d2h})
        if (st) hipStreamSynchronize(st);
    for (mp3mi_feed::host_ticks::tick_slot &io : H.slot) {
        for (void *p : {(void *) io.stage, (void *) io.out, (void *) io.len, (void *) io.out_rows, (void *) io.len_rows})
            if (p) hipFree(p);
        io.stage_free.destroy();
        io.out_free.destroy();
        for (hipEvent_t e : {io.ev_enc, io.t_up[0], io.t_up[1], io.t_dn[0], io.t_dn[1]})
            if (e) hipEventDestroy(e);
    }
    for (hipStream_t st : {H.h2d, H.d2h})
        if (st) hipStreamDestroy(st);
    memset(&H, 0, sizeof(H));
}

// everything the host ticks put on the feeder's own streams is through (mp3mi_batch_sync, behind the batch's streams)
static hipError_t feed_host_sync(mp3mi_feed *f)
{
    for (hipStream_t st : {f->ht.h2d, f->ht.d2h})
        if (st) {
            const hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

// The host has seen the end of the slot's last tick: its copies are through, and their times and bytes are booked.
static int feed_host_harvest(mp3mi_feed *f, int sl)
{
    mp3mi_feed::host_ticks &H = f->ht;
    mp3mi_feed::host_ticks::tick_slot &io = H.slot[sl];
    if (!io.pending) return MP3MI_OK;
    if (!(io.stage_free.done() && io.out_free.done())) {
        hold_release(f->b);
        CHK(io.stage_free.sync());
        CHK(io.out_free.sync());
    }
    float ms = 0;
    if (io.up) {
        CHK(hipEventSynchronize(io.t_up[1])); // (ahead of stage_free: at once)
        CHK(hipEventElapsedTime(&ms, io.t_up[0], io.t_up[1]));
        H.tot_up_ms += ms;
    }
    if (io.dn) {
        CHK(hipEventSynchronize(io.t_dn[1]));
        CHK(hipEventElapsedTime(&ms, io.t_dn[0], io.t_dn[1]));
        H.tot_dn_ms += ms;
    }
    H.tot_up_bytes += io.bytes_up;
    H.tot_dn_bytes += io.bytes_dn;
    H.tot_calls++;
    io.pending = false;
    // (the fences stand for THAT tick: one that uploads or downloads nothing must not find them)
    io.stage_free.recorded = io.out_free.recorded = false;
    return MP3MI_OK;
}

// The copy streams with the first host tick, a tick slot's buffers with the first tick that takes it; then the slot's last tick is
// waited for (at most two host ticks in flight), and the dense rows grow to the caller's stride.  What a failure leaves behind
// goes with the feeder.
static int feed_host_begin(mp3mi_feed *f, const feed_host_call *hc)
{
    mp3mi_batch *b = f->b;
    mp3mi_feed::host_ticks &H = f->ht;
    const size_t S = (size_t) b->n_streams, esz = 2 * (size_t) b->channels;
    if ((uint64_t) f->max_rows * (uint64_t) f->max_push > (uint64_t) UINT32_MAX) return MP3MI_ERR_ARG; // (a push's first sample is a descriptor word)
    ON_DEVICE(b);
    if (!H.ready) {
        H.dev_stride = mp3mi_batch_out_stride(b, f->tick_frames);
        if (!H.h2d) CHK(hipStreamCreateWithFlags(&H.h2d, hipStreamNonBlocking));
        if (!H.d2h) CHK(hipStreamCreateWithFlags(&H.d2h, hipStreamNonBlocking));
        H.ready = true;
    }
    const int sl = (int) (H.tick_no & 1u);
    mp3mi_feed::host_ticks::tick_slot &io = H.slot[sl];
    if (!io.stage) CHK(hipMalloc((void **) &io.stage, (size_t) f->max_rows * (size_t) f->max_push * esz));
    if (!io.out) CHK(hipMalloc((void **) &io.out, S * H.dev_stride));
    if (!io.len) CHK(hipMalloc((void **) &io.len, S * sizeof(uint32_t)));
    if (!io.len_rows) CHK(hipMalloc((void **) &io.len_rows, S * sizeof(uint32_t)));
    if (!io.stage_free.ev) CHK(io.stage_free.create());
    if (!io.out_free.ev) CHK(io.out_free.create());
    if (!io.ev_enc) CHK(hipEventCreateWithFlags(&io.ev_enc, hipEventDisableTiming));
    for (hipEvent_t *e : {&io.t_up[0], &io.t_up[1], &io.t_dn[0], &io.t_dn[1]})
        if (!*e) CHK(hipEventCreate(e));
    if (feed_host_harvest(f, sl) != MP3MI_OK) return MP3MI_ERR_HIP;
    if (io.out_rows_cap < S * hc->out_stride) { // (behind the slot's last download: harvested above)
        if (io.out_rows) {
            CHK(hipFree(io.out_rows));
            io.out_rows = NULL;
            io.out_rows_cap = 0;
        }
        CHK(hipMalloc((void **) &io.out_rows, S * hc->out_stride));
        io.out_rows_cap = S * hc->out_stride;
    }
    return MP3MI_OK;
}

extern "C" int mp3mi_feed_tick_lanes_host_async(mp3mi_feed *f, int n_rows, const int32_t *row_lane_host, const int16_t *pcm_host,
                                                const uint8_t *ctl_host, const int32_t *n_push_host, const int32_t *kbps_host, uint8_t *out_host,
                                                size_t out_stride, uint32_t *out_len_host, int32_t *out_lane_host, int32_t *out_slot_host,
                                                int32_t *n_out_host)
{
    if (!f || !f->lanes_mode || !out_host || !out_len_host || !out_lane_host || !out_slot_host || !n_out_host) return MP3MI_ERR_ARG;
    mp3mi_batch *b = f->b;
    if (n_rows < 0 || n_rows > f->max_rows || out_stride < mp3mi_batch_out_stride(b, f->tick_frames)) return MP3MI_ERR_ARG;
    if (n_rows > 0 && (!row_lane_host || !ctl_host || !n_push_host || !kbps_host)) return MP3MI_ERR_ARG;
    size_t n_pushed = 0;
    for (int r = 0; r < n_rows; r++) {
        if (n_push_host[r] < 0 || n_push_host[r] > f->max_push) return MP3MI_ERR_ARG;
        n_pushed += (size_t) n_push_host[r];
    }
    if (n_pushed && !pcm_host) return MP3MI_ERR_ARG;
    const feed_host_call hc = {pcm_host, n_pushed, out_host, out_stride, out_len_host, out_lane_host, out_slot_host, n_out_host};
    return feed_tick_lanes_impl(f, n_rows, row_lane_host, NULL, 0, ctl_host, n_push_host, kbps_host, NULL, 0, NULL, NULL, &hc);
}

// Waits for the upload and the download of ONE host tick: the latest (0) or the one before (1).  No call hold is let go (the ticket
// rule of mp3mi_batch_host_wait: only the hold that very tick left in force).  A host tick leaves none (mp3mi_batch::feed_host_call),
// and what it waits for was enqueued with the tick, ahead of whatever a later device tick holds: a later tick's hold stays, and a
// server collects tick t while tick t + 1 keeps its place in the pipeline.
extern "C" int mp3mi_feed_host_wait(mp3mi_feed *f, int ticks_back)
{
    if (!f || ticks_back < 0 || ticks_back > 1) return MP3MI_ERR_ARG;
    mp3mi_feed::host_ticks &H = f->ht;
    if (!H.ready || H.tick_no <= (unsigned) ticks_back) return MP3MI_ERR_ARG;
    mp3mi_batch *b = f->b;
    ON_DEVICE(b);
    mp3mi_feed::host_ticks::tick_slot &io = H.slot[(H.tick_no - 1u - (unsigned) ticks_back) & 1u];
    if (!io.pending || (io.stage_free.done() && io.out_free.done())) return MP3MI_OK;
    if (io.up) CHK(hipEventSynchronize(io.t_up[1]));
    if (io.dn) CHK(hipEventSynchronize(io.t_dn[1]));
    return MP3MI_OK;
}

extern "C" int mp3mi_feed_host_io_stats(mp3mi_feed *f, mp3mi_host_io_stats *st)
{
    if (!f || !st) return MP3MI_ERR_ARG;
    ON_DEVICE(f->b);
    memset(st, 0, sizeof(*st));
    if (!f->ht.ready) return MP3MI_OK;
    if (feed_host_harvest(f, 0) != MP3MI_OK || feed_host_harvest(f, 1) != MP3MI_OK) return MP3MI_ERR_HIP;
    st->calls = f->ht.tot_calls;
    st->h2d_bytes = f->ht.tot_up_bytes; st->d2h_bytes = f->ht.tot_dn_bytes;
    st->h2d_ms = f->ht.tot_up_ms; st->d2h_ms = f->ht.tot_dn_ms;
    return MP3MI_OK;
}
