// TEST INFRASTRUCTURE (CPU only): a feeder in front of a Layer III slot batch (mp3mi_feed_*, include/mp3mi.h) under a host
// sanitizer -- batch.cpp with feed.h, k_format.hip with k_feed and k_slot_park, the emulator and this program are instrumented, so an
// index out of a ring, a row, a descriptor block or a record is a report, and so is a buffer or an event that mp3mi_feed_destroy
// or mp3mi_batch_destroy forgets (the emulator's device memory is calloc, its events are new).  A dozen ticks with lanes that sit
// out and come back, every refused call, and destroy in both orders: the feeder first, and the batch with the feeder attached.
// Checks return codes, lengths and the lanes' books; parity is the suite's business (tests/test_feed.py).
// Build and run: make -C tests/hipemu -f feed.mk feed
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mp3mi.h"

#define OK(call)                                                                     \
    do {                                                                             \
        const long rc_ = (long) (call);                                              \
        if (rc_ != MP3MI_OK) { fprintf(stderr, "feed: %s returned %ld (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)
#define BAD(call)                                                                    \
    do {                                                                             \
        const long rc_ = (long) (call);                                              \
        if (rc_ != MP3MI_ERR_ARG) { fprintf(stderr, "feed: %s returned %ld, not MP3MI_ERR_ARG (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)
#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "feed: %s does not hold (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

static const int S = 4, RATE = 44100;
static const uint8_t ST = MP3MI_SLOT_START, EN = MP3MI_SLOT_END;

// (the emulator runs every lane of a workgroup as a fiber, and under the sanitizer a tick that encodes takes seconds: four lanes, one
// frame a tick and a dozen ticks are what shows the paths)
static int run(int C, int tick, int max_push, bool feeder_first)
{
    const int full = tick * 1152, burst = full < max_push ? full : max_push;
    mp3mi_batch *b = NULL;
    mp3mi_feed *f = NULL, *g = NULL;
    OK(mp3mi_batch_create(&b, S, RATE, C, NULL, 128, tick));
    BAD(mp3mi_feed_create(&f, b, 0, max_push));
    BAD(mp3mi_feed_create(&f, b, tick + 1, max_push));
    BAD(mp3mi_feed_create(&f, b, tick, 0));
    BAD(mp3mi_feed_create(&f, NULL, tick, max_push));
    BAD(mp3mi_feed_create(NULL, b, tick, max_push));
    OK(mp3mi_feed_create(&f, b, tick, max_push));
    BAD(mp3mi_feed_create(&g, b, tick, max_push)); // one feeder per batch
    EXPECT(g == NULL && mp3mi_feed_capacity(f) == (size_t) (full + max_push) && mp3mi_feed_capacity(NULL) == 0);
    // exact sizes, on the heap: a byte past a row's end is a report
    const size_t pitch = (size_t) max_push, stride = mp3mi_batch_out_stride(b, tick);
    std::vector<int16_t> pcm(pitch * C * S);
    std::vector<uint8_t> out(stride * S);
    std::vector<uint32_t> len(S);
    int32_t pend[S];
    int64_t fr[S];
    uint8_t fl[S];
    for (int s = 0; s < S; s++) mp3mi_synth_pcm(pcm.data() + pitch * C * s, max_push, C, RATE, (uint32_t) (400 + s), 0x6D70336Du);
#define TICK(ctl, n, kbps) mp3mi_feed_tick(f, pcm.data(), pitch, ctl, n, kbps, out.data(), stride, len.data())
    const uint8_t none[S] = {0, 0, 0, 0};
    {   // lane 0 STARTs with a tick, lane 1 with a few samples, lane 3 is a one-call file
        const uint8_t ctl[S] = {ST, ST, 0, (uint8_t) (ST | EN)};
        const int32_t n[S] = {burst, 7, 0, 333}, kbps[S] = {0, 64, 0, 96};
        OK(TICK(ctl, n, kbps));
        OK(mp3mi_batch_sync(b));
        EXPECT(len[0] + len[3] > 0 && len[1] == 0 && len[2] == 0);
        EXPECT(mp3mi_feed_lanes(f, pend, fr, fl) == 2 && pend[1] == 7 && fl[1] == 4 && fr[0] == (burst == full ? tick : 0) && fr[3] == -1);
    }
    // ticks with lanes that sit out and come back: lane 0 in packets of 960, lane 1 in bursts, lane 2 STARTs late
    for (int t = 0; t < (feeder_first ? 12 : 4); t++) {
        uint8_t ctl[S] = {0, 0, (uint8_t) (t == 3 ? ST : 0), 0};
        int32_t n[S] = {960, (t % 3 == 2) ? max_push : 1, t >= 3 ? burst : 0, 0};
        OK(mp3mi_feed_lanes(f, pend, fr, fl) < 0 ? -1 : 0);
        for (int s = 0; s < S; s++) // (never above the capacity: the burst waits a tick where it would not fit)
            if (pend[s] + n[s] > full + max_push) n[s] = 0;
        OK(TICK(ctl, n, NULL));
        if (t % 4 == 3) OK(mp3mi_batch_sync(b)); // (else back to back)
    }
    OK(mp3mi_batch_sync(b));
    EXPECT(mp3mi_feed_lanes(f, pend, fr, fl) == 3);
    {   // every refused tick leaves the feeder alone
        int32_t p0[S], p1[S];
        int64_t f1[S];
        uint8_t g0[S], g1[S];
        mp3mi_feed_lanes(f, p0, fr, g0);
        const uint8_t unknown[S] = {0, 4, 0, 0}, end_closed[S] = {0, 0, 0, EN}, start3[S] = {0, 0, 0, ST};
        const int32_t neg[S] = {-1, 0, 0, 0}, over[S] = {max_push + 1, 0, 0, 0}, closed_push[S] = {0, 0, 0, 5}, zero[S] = {0, 0, 0, 0};
        const int32_t k_bad[S] = {0, 0, 0, 100}, k_high[S] = {0, 0, 0, 160}, k_other[S] = {32, 0, 0, 0};
        BAD(TICK(unknown, zero, NULL));
        BAD(TICK(end_closed, zero, NULL));
        BAD(TICK(none, closed_push, NULL));
        BAD(TICK(none, neg, NULL));
        BAD(TICK(none, over, NULL));
        BAD(TICK(start3, zero, k_bad));
        BAD(TICK(start3, zero, k_high));
        BAD(TICK(none, zero, k_other));
        BAD(TICK(NULL, zero, NULL));
        BAD(mp3mi_feed_tick(NULL, pcm.data(), pitch, none, zero, NULL, out.data(), stride, len.data()));
        BAD(mp3mi_feed_tick(f, NULL, pitch, none, zero, NULL, out.data(), stride, len.data()));
        BAD(mp3mi_feed_tick(f, pcm.data(), pitch - 1, none, zero, NULL, out.data(), stride, len.data()));
        BAD(mp3mi_feed_tick(f, pcm.data(), pitch, none, zero, NULL, NULL, stride, len.data()));
        BAD(mp3mi_feed_tick(f, pcm.data(), pitch, none, zero, NULL, out.data(), stride - 1, len.data()));
        BAD(mp3mi_feed_tick(f, pcm.data(), pitch, none, zero, NULL, out.data(), stride, NULL));
        BAD(mp3mi_feed_lanes(f, NULL, fr, fl));
        // the attached batch refuses what is the feeder's
        mp3mi_slot_ticket tk;
        const int32_t slot0[1] = {0};
        std::vector<uint8_t> rec(mp3mi_batch_slot_state_bytes(b) + 16);
        void *rec16 = (void *) (((uintptr_t) rec.data() + 15) & ~(uintptr_t) 15);
        BAD(mp3mi_batch_encode(b, pcm.data(), tick, out.data(), stride, len.data()));
        BAD(mp3mi_batch_encode_next(b, pcm.data(), tick, out.data(), stride, len.data()));
        BAD(mp3mi_batch_encode_slots(b, pcm.data(), tick, none, NULL, out.data(), stride, len.data()));
        BAD(mp3mi_batch_flush(b, out.data(), stride, len.data()));
        BAD(mp3mi_batch_reset(b));
        BAD(mp3mi_batch_slots_export(b, 1, slot0, 1, rec16, mp3mi_batch_slot_state_bytes(b), &tk));
        BAD(mp3mi_batch_slots_import(b, 1, slot0, rec16, mp3mi_batch_slot_state_bytes(b), &tk));
        BAD(mp3mi_batch_set_header(b, 0, 0, 0));
        BAD(mp3mi_batch_set_mode(b, C == 1 ? MP3MI_MODE_MONO : MP3MI_MODE_STEREO));
        BAD(mp3mi_batch_set_error_protection(b, 0));
        EXPECT(mp3mi_feed_lanes(f, p1, f1, g1) == 3 && !memcmp(p0, p1, sizeof(p0)) && !memcmp(fr, f1, sizeof(f1)) && !memcmp(g0, g1, sizeof(g0)));
    }
    {   // lanes 0 and 2 END; a draining lane takes nothing more; lane 1 is abandoned for a new stream
        const uint8_t ctl[S] = {EN, ST, EN, 0};
        const int32_t n[S] = {100, 50, 0, 0};
        OK(TICK(ctl, n, NULL));
        for (int k = 0; k < 8 && mp3mi_feed_lanes(f, pend, fr, fl) > 1; k++) {
            const uint8_t again[S] = {EN, 0, 0, 0};
            if (fl[0] & 2) BAD(TICK(again, NULL, NULL));
            OK(TICK(none, NULL, NULL));
        }
        OK(mp3mi_batch_sync(b));
        EXPECT(mp3mi_feed_lanes(f, pend, fr, fl) == 1 && pend[1] == 50 && fl[1] == 4);
    }
    if (feeder_first) {
        mp3mi_feed_destroy(f);
        mp3mi_feed_destroy(NULL);
        // detached: the batch is the caller's again, and takes a new feeder
        OK(mp3mi_batch_set_header(b, 0, 0, 0));
        OK(mp3mi_batch_reset(b));
        OK(mp3mi_feed_create(&f, b, tick, max_push));
        const uint8_t ctl[S] = {ST, 0, 0, 0};
        const int32_t n[S] = {max_push, 0, 0, 0};
        OK(TICK(ctl, n, NULL));
        mp3mi_feed_destroy(f);
    } else {
        const uint8_t ctl[S] = {ST, 0, ST, 0};
        const int32_t n[S] = {max_push, 0, 3, 0};
        OK(TICK(ctl, n, NULL)); // (work in flight, a lane waiting, one parked or open: all of it goes with the batch)
    }
    mp3mi_batch_destroy(b);
    return 0;
}

int main(void)
{
    if (run(2, 1, 1500, true)) return 1;
    if (run(1, 1, 1000, false)) return 1;
    printf("feed: ok\n");
    return 0;
}
