// TEST INFRASTRUCTURE (CPU only): what the host side ENQUEUES -- kernel launches, copies, memsets, event records and waits, with
// their streams, in order -- for a fixed script of calls on emulated batches, printed to stdout (hipemu_trace, hipemu_trace.h).  No
// sanitizer, nothing loaded into Python, no expected output: the program is built twice, against two versions of csrc/ (the
// Makefile's CSRC), and the two outputs are compared with diff.  A host-side change that means to leave the sequence alone -- a
// refactor of encode_impl (batch.cpp) or of a feeder's tick (feed.h) -- shows an empty diff; DESIGN.md says how.
//
// The script reaches every branch of encode_impl that decides what is enqueued, at the smallest shapes that do:
//   S = 3    one part, no placement tables, every item beside the k_loop before it; call hold on, and again with it off
//   S = 12   placement tables (n_streams >= 2 * n_simd; the emulator has 4 SIMDs)
//   S = 65   two parts, of 64 streams and of 1; a part larger than the resident wavefronts (16 here): y_after
// all mono, chunk_frames = 1: a call of 3 frames is three chunks (the double-buffer parity flips from call to call), a call of 1
// frame chains hold to hold.  On the S = 3 batches: whole-file, encode_next x 3, flush, encode_next; per-slot calls (START of all,
// continue with an END, an END beside a START at another bitrate, export / import of a slot); two whole-file calls on host buffers
// back to back, at the device buffer's output stride (plain copy) and at a larger one (2-D copy); per-slot calls on host buffers
// without and with a row map; and, with the hold on, both feeders, with lanes that sit out (park) and come back (resume): device
// ticks and a host tick.  On the larger batches a short script (short_calls).
// Build and run: make -C tests/hipemu -f enqueue_trace.mk enqueue_trace
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <vector>
#include "hipemu_trace.h"
#include "mp3mi.h"

// the trace's state (hipemu_trace.h): where it goes, and the numbers of the streams and events created so far
namespace hipemu_tr {
FILE *to = NULL;
static int n_streams = 0, n_events = 0;
static std::map<hipEvent_t, int> event_of;
hipStream_t new_stream(const char *how)
{
    const int n = ++n_streams;
    HIPEMU_TRACE("%s  stream %d\n", how, n);
    return (hipStream_t) (uintptr_t) n;
}
void new_event(const char *how, hipEvent_t e)
{
    event_of[e] = ++n_events;
    HIPEMU_TRACE("%s  event %d\n", how, n_events);
}
void drop_event(hipEvent_t e) { event_of.erase(e); }
int event_no(hipEvent_t e)
{
    const std::map<hipEvent_t, int>::const_iterator it = event_of.find(e);
    return it == event_of.end() ? 0 : it->second;
}
}
void hipemu_trace(FILE *to) { hipemu_tr::to = to; }

#define OK(call)                                                                     \
    do {                                                                             \
        const long rc_ = (long) (call);                                              \
        if (rc_ != MP3MI_OK) { fprintf(stderr, "enqueue_trace: %s returned %ld (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)

static const int RATE = 44100, NF = 3, FULL = 1152, MAX_PUSH = 1500;
static const uint8_t ST = MP3MI_SLOT_START, EN = MP3MI_SLOT_END;

struct rig {
    mp3mi_batch *b;
    int S, C;
    size_t stride; // mp3mi_batch_out_stride(b, NF): the host-buffer calls' device stride too (NF = max_frames)
    std::vector<int16_t> pcm;
    std::vector<uint8_t> out;
    std::vector<uint32_t> len;
};

static void say(const char *what) { printf("## %s\n", what); }

static int whole_batch_calls(rig &r)
{
    int16_t *pcm = r.pcm.data();
    uint8_t *out = r.out.data();
    uint32_t *len = r.len.data();
    say("whole-file call, 3 frames");
    OK(mp3mi_batch_encode(r.b, pcm, 3, out, r.stride, len));
    say("encode_next, 3 frames: starts afresh behind the whole-file call");
    OK(mp3mi_batch_encode_next(r.b, pcm, 3, out, r.stride, len));
    say("encode_next, 1 frame");
    OK(mp3mi_batch_encode_next(r.b, pcm, 1, out, r.stride, len));
    say("encode_next, 1 frame: hold to hold");
    OK(mp3mi_batch_encode_next(r.b, pcm, 1, out, r.stride, len));
    say("flush");
    OK(mp3mi_batch_flush(r.b, out, r.stride, len));
    say("encode_next, 1 frame, behind the flush");
    OK(mp3mi_batch_encode_next(r.b, pcm, 1, out, r.stride, len));
    say("flush, sync");
    OK(mp3mi_batch_flush(r.b, out, r.stride, len));
    OK(mp3mi_batch_sync(r.b));
    return 0;
}

static int slot_calls(rig &r)
{
    const size_t S = (size_t) r.S;
    int16_t *pcm = r.pcm.data();
    uint8_t *out = r.out.data();
    uint32_t *len = r.len.data();
    std::vector<uint8_t> ctl(S, ST);
    std::vector<int32_t> kbps(S, 0);
    say("per-slot call, 1 frame: every slot STARTs (the flush before it kept the ended streams' status)");
    OK(mp3mi_batch_encode_slots(r.b, pcm, 1, ctl.data(), NULL, out, r.stride, len));
    ctl.assign(S, 0);
    ctl[1] = EN;
    say("per-slot call, 3 frames: all go on, slot 1 ENDs");
    OK(mp3mi_batch_encode_slots(r.b, pcm, 3, ctl.data(), NULL, out, r.stride, len));
    ctl[0] = EN;
    ctl[1] = ST;
    kbps[1] = 64;
    say("per-slot call, 1 frame: slot 0 ENDs, slot 1 STARTs at another bitrate");
    OK(mp3mi_batch_encode_slots_kbps(r.b, pcm, 1, ctl.data(), NULL, kbps.data(), out, r.stride, len));
    {
        const size_t sb = mp3mi_batch_slot_state_bytes(r.b);
        std::vector<uint8_t> state(sb + 16);
        void *at = (void *) (((uintptr_t) state.data() + 15) & ~(uintptr_t) 15);
        mp3mi_slot_ticket t;
        int32_t slot = 2;
        say("export of slot 2 (closed), import into slot 0");
        OK(mp3mi_batch_slots_export(r.b, 1, &slot, 1, at, sb, &t));
        slot = 0;
        OK(mp3mi_batch_slots_import(r.b, 1, &slot, at, sb, &t));
    }
    ctl.assign(S, 0);
    say("per-slot call, 1 frame: the open streams go on");
    OK(mp3mi_batch_encode_slots(r.b, pcm, 1, ctl.data(), NULL, out, r.stride, len));
    say("flush of the open slots, sync");
    OK(mp3mi_batch_flush(r.b, out, r.stride, len));
    OK(mp3mi_batch_sync(r.b));
    return 0;
}

static int host_calls(rig &r)
{
    const size_t S = (size_t) r.S, wide = r.stride + 64;
    std::vector<uint8_t> out2(wide * S);
    std::vector<uint32_t> len2(S);
    say("whole-file call on host buffers, 3 frames, the device buffer's stride: plain copy");
    OK(mp3mi_batch_encode_host_async(r.b, r.pcm.data(), 3, r.out.data(), r.stride, r.len.data()));
    say("... and back to back at a larger stride: 2-D copy");
    OK(mp3mi_batch_encode_host_async(r.b, r.pcm.data(), 3, out2.data(), wide, len2.data()));
    say("host_wait for each, sync");
    OK(mp3mi_batch_host_wait(r.b, 1));
    OK(mp3mi_batch_host_wait(r.b, 0));
    OK(mp3mi_batch_sync(r.b));
    std::vector<uint8_t> ctl(S, ST | EN);
    ctl[0] = ctl[2] = ST;
    say("per-slot call on host buffers, no row map, 1 frame: every slot STARTs, all but slots 0 and 2 END");
    OK(mp3mi_batch_encode_slots_kbps_host_async(r.b, r.pcm.data(), 1, r.S, NULL, ctl.data(), NULL, NULL, r.out.data(), r.stride, r.len.data()));
    const int32_t rows[3] = {0, 1, 2}, kbps[3] = {0, 64, 0};
    const uint8_t ctl3[3] = {0, ST, EN};
    say("per-slot call on host buffers with a row map, 3 frames: slot 0 goes on, slot 1 STARTs at another bitrate, slot 2 ENDs");
    OK(mp3mi_batch_encode_slots_kbps_host_async(r.b, r.pcm.data(), 3, 3, rows, ctl3, NULL, kbps, out2.data(), wide, len2.data()));
    say("per-slot call on device buffers behind it, 1 frame");
    ctl.assign(S, 0);
    OK(mp3mi_batch_encode_slots(r.b, r.pcm.data(), 1, ctl.data(), NULL, r.out.data(), r.stride, r.len.data()));
    say("flush, sync");
    OK(mp3mi_batch_flush(r.b, r.out.data(), r.stride, r.len.data()));
    OK(mp3mi_batch_sync(r.b));
    return 0;
}

// the feeder whose lane is its slot: lanes sit out (park) and come back (resume)
static int feeder_slots(rig &r)
{
    const size_t S = (size_t) r.S, stride1 = mp3mi_batch_out_stride(r.b, 1);
    mp3mi_feed *f = NULL;
    std::vector<int16_t> push((size_t) MAX_PUSH * r.C * S);
    for (size_t s = 0; s < S; s++) mp3mi_synth_pcm(push.data() + (size_t) MAX_PUSH * r.C * s, MAX_PUSH, r.C, RATE, (uint32_t) (300 + s), 0x6D70336Du);
    say("feeder (lane = slot): create");
    OK(mp3mi_feed_create(&f, r.b, 1, MAX_PUSH));
    std::vector<uint8_t> ctl(S, ST);
    std::vector<int32_t> n(S, FULL);
    say("tick: every lane STARTs with a full tick");
    OK(mp3mi_feed_tick(f, push.data(), MAX_PUSH, ctl.data(), n.data(), NULL, r.out.data(), stride1, r.len.data()));
    ctl.assign(S, 0);
    n.assign(S, 7);
    n[0] = FULL;
    say("tick: lane 0 encodes, the others sit out");
    OK(mp3mi_feed_tick(f, push.data(), MAX_PUSH, ctl.data(), n.data(), NULL, r.out.data(), stride1, r.len.data()));
    n.assign(S, FULL);
    n[0] = 0;
    say("tick: lane 0 sits out, the others come back");
    OK(mp3mi_feed_tick(f, push.data(), MAX_PUSH, ctl.data(), n.data(), NULL, r.out.data(), stride1, r.len.data()));
    say("tick: nobody pushes, nobody encodes");
    n.assign(S, 0);
    OK(mp3mi_feed_tick(f, push.data(), MAX_PUSH, ctl.data(), n.data(), NULL, r.out.data(), stride1, r.len.data()));
    say("sync, destroy");
    OK(mp3mi_batch_sync(r.b));
    mp3mi_feed_destroy(f);
    return 0;
}

// more lanes than slots (S = 3, five lanes): device ticks and a host tick, each with lanes that leave and lanes that enter
static int feeder_lanes(rig &r)
{
    const size_t S = (size_t) r.S, stride1 = mp3mi_batch_out_stride(r.b, 1);
    mp3mi_feed *f = NULL;
    std::vector<int16_t> push((size_t) MAX_PUSH * r.C * 4);
    for (size_t k = 0; k < 4; k++) mp3mi_synth_pcm(push.data() + (size_t) MAX_PUSH * r.C * k, MAX_PUSH, r.C, RATE, (uint32_t) (400 + k), 0x6D70336Du);
    std::vector<int32_t> slot_lane(S), out_lane(S), out_slot(S);
    int32_t n_out = 0;
    say("feeder (five lanes): create");
    OK(mp3mi_feed_create_lanes(&f, r.b, 5, 4, 1, MAX_PUSH, FULL + MAX_PUSH + 700));
    {
        const int32_t rows[4] = {0, 1, 2, 3}, n[4] = {FULL, FULL, FULL, FULL}, kbps[4] = {0, 64, 0, 0};
        const uint8_t ctl[4] = {ST, ST, ST, ST};
        say("device tick: four lanes START with a full tick on three slots, lane 3 waits");
        OK(mp3mi_feed_tick_lanes(f, 4, rows, push.data(), MAX_PUSH, ctl, n, kbps, r.out.data(), stride1, r.len.data(), slot_lane.data()));
    }
    {
        const int32_t rows[2] = {0, 4}, n[2] = {7, FULL}, kbps[2] = {0, 0};
        const uint8_t ctl[2] = {0, ST};
        say("device tick: lanes 0, 1, 2 sit out, lane 3 and lane 4 START in the slots they leave");
        OK(mp3mi_feed_tick_lanes(f, 2, rows, push.data(), MAX_PUSH, ctl, n, kbps, r.out.data(), stride1, r.len.data(), slot_lane.data()));
    }
    {
        const int32_t rows[2] = {0, 1}, n[2] = {FULL, FULL}, kbps[2] = {0, 0};
        const uint8_t ctl[2] = {0, 0};
        std::vector<int16_t> packed((size_t) 2 * FULL * r.C);
        memcpy(packed.data(), push.data(), sizeof(int16_t) * packed.size());
        std::vector<uint8_t> out(stride1 * S);
        std::vector<uint32_t> len(S);
        say("host tick: lanes 0 and 1 come back, lanes 3 and 4 sit out");
        OK(mp3mi_feed_tick_lanes_host_async(f, 2, rows, packed.data(), ctl, n, kbps, out.data(), stride1, len.data(), out_lane.data(), out_slot.data(), &n_out));
        say("device tick behind it: nobody pushes");
        OK(mp3mi_feed_tick_lanes(f, 0, NULL, NULL, 0, NULL, NULL, NULL, r.out.data(), stride1, r.len.data(), slot_lane.data()));
        say("host_wait, sync");
        OK(mp3mi_feed_host_wait(f, 0));
        OK(mp3mi_batch_sync(r.b));
    }
    say("destroy");
    mp3mi_feed_destroy(f);
    return 0;
}

// The larger batches: what placement tables, a second part and a part larger than the resident wavefronts change, and no more --
// the emulator runs a stream's frame in about 0.1 s.  Streaming calls that chain hold to hold, per-slot calls with a live slot in
// each part, and host-buffer calls, whose chunks wait for their upload once per chunk and download behind the last part.
static int short_calls(rig &r)
{
    const size_t S = (size_t) r.S;
    int16_t *pcm = r.pcm.data();
    uint8_t *out = r.out.data();
    uint32_t *len = r.len.data();
    say("encode_next, 1 frame");
    OK(mp3mi_batch_encode_next(r.b, pcm, 1, out, r.stride, len));
    say("encode_next, 1 frame: hold to hold");
    OK(mp3mi_batch_encode_next(r.b, pcm, 1, out, r.stride, len));
    say("flush");
    OK(mp3mi_batch_flush(r.b, out, r.stride, len));
    std::vector<uint8_t> ctl(S, 0);
    ctl[0] = ctl[S - 1] = ST;
    say("per-slot call, 1 frame: the first and the last slot START");
    OK(mp3mi_batch_encode_slots(r.b, pcm, 1, ctl.data(), NULL, out, r.stride, len));
    ctl.assign(S, 0);
    say("per-slot call, 2 frames: they go on");
    OK(mp3mi_batch_encode_slots(r.b, pcm, 2, ctl.data(), NULL, out, r.stride, len));
    say("flush of the open slots");
    OK(mp3mi_batch_flush(r.b, out, r.stride, len));
    say("whole-file call on host buffers, 2 frames");
    OK(mp3mi_batch_encode_host_async(r.b, pcm, 2, out, r.stride, len));
    const int32_t rows[2] = {0, (int32_t) S - 1};
    const uint8_t ctl2[2] = {ST, ST};
    say("per-slot call on host buffers with a row map, 1 frame: the first and the last slot START");
    OK(mp3mi_batch_encode_slots_kbps_host_async(r.b, pcm, 1, 2, rows, ctl2, NULL, NULL, out, r.stride, len));
    say("flush, sync");
    OK(mp3mi_batch_flush(r.b, out, r.stride, len));
    OK(mp3mi_batch_sync(r.b));
    return 0;
}

static int run(int S, int C, int hold, bool all)
{
    printf("#### S = %d, %d channel(s), call hold %s\n", S, C, hold ? "on" : "off");
    mp3mi_batch_options opt;
    mp3mi_batch_options_default(&opt);
    opt.chunk_frames = 1;
    opt.call_hold = hold;
    rig r;
    r.b = NULL;
    r.S = S;
    r.C = C;
    OK(mp3mi_batch_create_ex(&r.b, S, RATE, C, NULL, 128, NF, &opt));
    const size_t row = (size_t) NF * 1152 * (size_t) C;
    r.stride = mp3mi_batch_out_stride(r.b, NF);
    r.pcm.resize(row * (size_t) S);
    r.out.resize(r.stride * (size_t) S);
    r.len.resize((size_t) S);
    for (int s = 0; s < S; s++) mp3mi_synth_pcm(r.pcm.data() + row * (size_t) s, NF * 1152, C, RATE, (uint32_t) s, 0x6D70336Du);
    if (all ? (whole_batch_calls(r) || slot_calls(r) || host_calls(r) || (hold && (feeder_slots(r) || feeder_lanes(r)))) : short_calls(r)) return 1;
    say("destroy");
    mp3mi_batch_destroy(r.b);
    return 0;
}

int main(void)
{
    hipemu_trace(stdout);
    if (run(3, 1, 1, true) || run(3, 1, 0, true) || run(12, 1, 1, false) || run(65, 1, 1, false)) return 1;
    hipemu_trace(NULL);
    fprintf(stderr, "enqueue_trace: ok\n");
    return 0;
}
