// TEST INFRASTRUCTURE (CPU only): a feeder with more lanes than slots (mp3mi_feed_create_lanes / mp3mi_feed_tick_lanes,
// include/mp3mi.h) under a host sanitizer -- batch.cpp with feed.h, k_format.hip with k_feed_lanes and k_slot_park, the emulator and
// this program are instrumented, so an index out of a ring, a row, an upload block, a record per lane or the dense record blocks is a
// report, and so is a buffer or an event that mp3mi_feed_destroy or mp3mi_batch_destroy forgets.  Feeders with fewer, as many and
// more lanes than the batch has slots; ticks in which lanes wait for a slot, move to another slot, and take a slot that was vacated
// in the same tick (by a START and by an import); every refused call; destroy in both orders.  Checks return codes, slot_lane_host,
// lengths and the lanes' books; parity is the suite's business (tests/test_feed_lanes.py).
// Build and run: make -C tests/hipemu -f feed_lanes.mk feed_lanes
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mp3mi.h"

#define OK(call)                                                                     \
    do {                                                                             \
        const long rc_ = (long) (call);                                              \
        if (rc_ != MP3MI_OK) { fprintf(stderr, "feed_lanes: %s returned %ld (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)
#define BAD(call)                                                                    \
    do {                                                                             \
        const long rc_ = (long) (call);                                              \
        if (rc_ != MP3MI_ERR_ARG) { fprintf(stderr, "feed_lanes: %s returned %ld, not MP3MI_ERR_ARG (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)
#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "feed_lanes: %s does not hold (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

static const int S = 2, C = 2, RATE = 44100, TICK = 1, FULL = 1152, MAX_PUSH = 1500, MAX_L = 5;
static const uint8_t ST = MP3MI_SLOT_START, EN = MP3MI_SLOT_END;

struct rig {
    mp3mi_batch *b;
    mp3mi_feed *f;
    int L, max_rows;
    size_t pitch, stride;
    std::vector<int16_t> pcm; // exact sizes, on the heap: a byte past a row's end is a report
    std::vector<uint8_t> out;
    std::vector<uint32_t> len;
    int32_t slot_lane[S];
    int32_t pend[MAX_L];
    int64_t fr[MAX_L];
    uint8_t fl[MAX_L];
};

static int tick(rig &r, int n_rows, const int32_t *rows, const uint8_t *ctl, const int32_t *n, const int32_t *kbps)
{
    return mp3mi_feed_tick_lanes(r.f, n_rows, rows, r.pcm.data(), r.pitch, ctl, n, kbps, r.out.data(), r.stride, r.len.data(), r.slot_lane);
}

// what every accepted tick leaves: a lane or -1 per slot, no lane twice, no bytes without a lane
static int settled(rig &r)
{
    OK(mp3mi_batch_sync(r.b));
    for (int s = 0; s < S; s++) {
        EXPECT(r.slot_lane[s] >= -1 && r.slot_lane[s] < r.L);
        EXPECT(r.slot_lane[s] >= 0 || r.len[s] == 0);
    }
    EXPECT(r.slot_lane[0] < 0 || r.slot_lane[0] != r.slot_lane[1]);
    EXPECT(mp3mi_feed_lanes(r.f, r.pend, r.fr, r.fl) >= 0);
    return 0;
}

static int run(int L, bool feeder_first)
{
    rig r;
    r.b = NULL;
    r.f = NULL;
    r.L = L;
    r.max_rows = L < 3 ? L : 3;
    mp3mi_feed *g = NULL;
    OK(mp3mi_batch_create(&r.b, S, RATE, C, NULL, 128, TICK));
    BAD(mp3mi_feed_create_lanes(&r.f, r.b, 0, 1, TICK, MAX_PUSH, 0));
    BAD(mp3mi_feed_create_lanes(&r.f, r.b, L, 0, TICK, MAX_PUSH, 0));
    BAD(mp3mi_feed_create_lanes(&r.f, r.b, L, L + 1, TICK, MAX_PUSH, 0));
    BAD(mp3mi_feed_create_lanes(&r.f, r.b, L, 1, 0, MAX_PUSH, 0));
    BAD(mp3mi_feed_create_lanes(&r.f, r.b, L, 1, TICK + 1, MAX_PUSH, 0));
    BAD(mp3mi_feed_create_lanes(&r.f, r.b, L, 1, TICK, 0, 0));
    BAD(mp3mi_feed_create_lanes(&r.f, r.b, L, 1, TICK, MAX_PUSH, FULL + MAX_PUSH - 1));
    BAD(mp3mi_feed_create_lanes(&r.f, r.b, L, 1, TICK, MAX_PUSH, -5));
    BAD(mp3mi_feed_create_lanes(&r.f, NULL, L, 1, TICK, MAX_PUSH, 0));
    BAD(mp3mi_feed_create_lanes(NULL, r.b, L, 1, TICK, MAX_PUSH, 0));
    const int ring = L > S ? FULL + MAX_PUSH + 700 : 0;
    OK(mp3mi_feed_create_lanes(&r.f, r.b, L, r.max_rows, TICK, MAX_PUSH, ring));
    BAD(mp3mi_feed_create_lanes(&g, r.b, L, 1, TICK, MAX_PUSH, 0)); // one feeder per batch
    BAD(mp3mi_feed_create(&g, r.b, TICK, MAX_PUSH));
    EXPECT(g == NULL && mp3mi_feed_n_lanes(r.f) == L && mp3mi_feed_n_lanes(NULL) == 0);
    EXPECT(mp3mi_feed_capacity(r.f) == (size_t) (ring ? ring : FULL + MAX_PUSH));
    r.pitch = (size_t) MAX_PUSH;
    r.stride = mp3mi_batch_out_stride(r.b, TICK);
    r.pcm.resize(r.pitch * C * (size_t) r.max_rows);
    r.out.resize(r.stride * S);
    r.len.resize(S);
    for (int k = 0; k < r.max_rows; k++) mp3mi_synth_pcm(r.pcm.data() + r.pitch * C * k, MAX_PUSH, C, RATE, (uint32_t) (500 + k), 0x6D70336Du);
    const int32_t zero3[3] = {0, 0, 0};
    if (L == 5) {
        {   // three lanes START with a tick on two slots: lane 2 waits
            const int32_t rows[3] = {0, 1, 2}, n[3] = {FULL, FULL, FULL}, kbps[3] = {0, 64, 96};
            const uint8_t ctl[3] = {ST, ST, ST};
            OK(tick(r, 3, rows, ctl, n, kbps));
            if (settled(r)) return 1;
            EXPECT(r.slot_lane[0] == 0 && r.slot_lane[1] == 1 && r.len[0] + r.len[1] > 0 && r.fl[2] == (4 | 8) && r.pend[2] == FULL);
        }
        {   // lanes 0 and 1 sit out, lanes 3 and 4 START: lane 2 STARTs in the slot lane 0 leaves in this tick, lane 4 waits
            const int32_t rows[3] = {2, 3, 4}, n[3] = {7, FULL, FULL};
            const uint8_t ctl[3] = {0, ST, ST};
            OK(tick(r, 3, rows, ctl, n, zero3));
            if (settled(r)) return 1;
            EXPECT(r.slot_lane[0] == 2 && r.slot_lane[1] == 3 && r.fl[0] == 1 && r.fl[1] == 1 && r.fl[4] == (4 | 8) && r.pend[2] == 7);
        }
        {   // lanes 0 and 1 are ready again: lane 4, ready for longest, and lane 0 encode; lane 0 resumes in slot 0 and lane 4 STARTs in slot 1,
            // both vacated in this tick (the lowest free slot to the lowest lane)
            const int32_t rows[2] = {0, 1}, n[2] = {FULL, MAX_PUSH};
            const uint8_t ctl[2] = {0, 0};
            OK(tick(r, 2, rows, ctl, n, zero3));
            if (settled(r)) return 1;
            EXPECT(r.slot_lane[0] == 0 && r.slot_lane[1] == 4 && r.fl[1] == (1 | 8) && r.fl[2] == 1 && r.fl[3] == 1 && r.fr[0] == 2);
        }
        {   // back to back, no sync: lane 1, which ran in slot 1, resumes in slot 0; then a tick in which nobody is ready
            const int32_t rows[1] = {3}, n[1] = {960};
            const uint8_t ctl[1] = {0};
            OK(tick(r, 1, rows, ctl, n, zero3));
            EXPECT(r.slot_lane[0] == 1 && r.slot_lane[1] == -1);
            OK(tick(r, 1, rows, ctl, n, zero3)); // lane 1 has MAX_PUSH - FULL left ... and lane 3 960 + 960: ready
            EXPECT(r.slot_lane[0] == 3 && r.slot_lane[1] == -1);
            OK(mp3mi_feed_tick_lanes(r.f, 0, NULL, NULL, 0, NULL, NULL, NULL, r.out.data(), r.stride, r.len.data(), r.slot_lane));
            if (settled(r)) return 1;
            EXPECT(r.slot_lane[0] == -1 && r.slot_lane[1] == -1 && r.len[0] == 0 && r.len[1] == 0);
        }
    } else {
        // every lane STARTs with a packet, then brings a tick, then a packet: with two lanes on two slots nobody waits
        for (int t = 0; t < 3; t++) {
            const int32_t rows[2] = {0, 1}, n[2] = {t == 1 ? FULL : 960, t == 1 ? FULL : 960}, kbps[2] = {0, t == 0 ? 64 : 0};
            const uint8_t ctl[2] = {(uint8_t) (t == 0 ? ST : 0), (uint8_t) (t == 0 ? ST : 0)};
            OK(tick(r, L, rows, ctl, n, kbps));
            if (t != 1 && settled(r)) return 1;
        }
        EXPECT(r.slot_lane[0] == 0 && r.slot_lane[1] == (L == 2 ? 1 : -1) && r.fr[0] == 2 && r.fl[0] == 0);
    }
    {   // every refused tick leaves the feeder alone
        int32_t p0[MAX_L], p1[MAX_L];
        int64_t f0[MAX_L], f1[MAX_L];
        uint8_t g0[MAX_L], g1[MAX_L];
        const int open0 = mp3mi_feed_lanes(r.f, p0, f0, g0);
        const int32_t row0[1] = {0}, rowL[1] = {L}, rowm[1] = {-1}, two[2] = {0, 0}, n0[2] = {0, 0}, neg[1] = {-1}, over[1] = {MAX_PUSH + 1};
        const int32_t full_ring[1] = {(int32_t) mp3mi_feed_capacity(r.f) - p0[0] + 1}, k_bad[1] = {100}, k_high[1] = {160}, k_other[1] = {32};
        const uint8_t none[2] = {0, 0}, unknown[1] = {4}, start[1] = {ST};
        BAD(tick(r, 1, row0, unknown, n0, n0));
        BAD(tick(r, 1, row0, none, neg, n0));
        BAD(tick(r, 1, row0, none, over, n0));
        if (full_ring[0] <= MAX_PUSH) BAD(tick(r, 1, row0, none, full_ring, n0));
        BAD(tick(r, 1, row0, start, n0, k_bad));
        BAD(tick(r, 1, row0, start, n0, k_high));
        BAD(tick(r, 1, row0, none, n0, k_other));
        BAD(tick(r, 1, rowL, none, n0, n0));
        BAD(tick(r, 1, rowm, none, n0, n0));
        if (r.max_rows >= 2) BAD(tick(r, 2, two, none, n0, n0)); // the row map does not increase
        BAD(tick(r, r.max_rows + 1, row0, none, n0, n0));
        BAD(tick(r, -1, row0, none, n0, n0));
        BAD(tick(r, 1, NULL, none, n0, n0));
        BAD(tick(r, 1, row0, NULL, n0, n0));
        BAD(tick(r, 1, row0, none, NULL, n0));
        BAD(tick(r, 1, row0, none, n0, NULL));
        BAD(mp3mi_feed_tick_lanes(NULL, 1, row0, r.pcm.data(), r.pitch, none, n0, n0, r.out.data(), r.stride, r.len.data(), r.slot_lane));
        BAD(mp3mi_feed_tick_lanes(r.f, 1, row0, NULL, r.pitch, none, n0, n0, r.out.data(), r.stride, r.len.data(), r.slot_lane));
        BAD(mp3mi_feed_tick_lanes(r.f, 1, row0, r.pcm.data(), r.pitch - 1, none, n0, n0, r.out.data(), r.stride, r.len.data(), r.slot_lane));
        BAD(mp3mi_feed_tick_lanes(r.f, 1, row0, r.pcm.data(), r.pitch, none, n0, n0, NULL, r.stride, r.len.data(), r.slot_lane));
        BAD(mp3mi_feed_tick_lanes(r.f, 1, row0, r.pcm.data(), r.pitch, none, n0, n0, r.out.data(), r.stride - 1, r.len.data(), r.slot_lane));
        BAD(mp3mi_feed_tick_lanes(r.f, 1, row0, r.pcm.data(), r.pitch, none, n0, n0, r.out.data(), r.stride, NULL, r.slot_lane));
        BAD(mp3mi_feed_tick_lanes(r.f, 1, row0, r.pcm.data(), r.pitch, none, n0, n0, r.out.data(), r.stride, r.len.data(), NULL));
        // the other kind's tick, and what the attached batch refuses
        const uint8_t ctl_all[MAX_L] = {0, 0, 0, 0, 0};
        BAD(mp3mi_feed_tick(r.f, r.pcm.data(), r.pitch, ctl_all, NULL, NULL, r.out.data(), r.stride, r.len.data()));
        BAD(mp3mi_batch_encode_next(r.b, r.pcm.data(), TICK, r.out.data(), r.stride, r.len.data()));
        BAD(mp3mi_batch_flush(r.b, r.out.data(), r.stride, r.len.data()));
        BAD(mp3mi_batch_reset(r.b));
        BAD(mp3mi_batch_set_header(r.b, 0, 0, 0));
        BAD(mp3mi_feed_lanes(r.f, NULL, f1, g1));
        EXPECT(mp3mi_feed_lanes(r.f, p1, f1, g1) == open0 && !memcmp(p0, p1, sizeof(int32_t) * L) && !memcmp(f0, f1, sizeof(int64_t) * L) &&
               !memcmp(g0, g1, (size_t) L));
    }
    if (feeder_first) {
        // every open lane ENDs (at most max_rows a tick) and drains; a draining lane takes nothing more
        for (int k = 0; k < 12 && mp3mi_feed_lanes(r.f, r.pend, r.fr, r.fl) > 0; k++) {
            int32_t rows[3], n[3] = {33, 0, 1};
            uint8_t ctl[3] = {EN, EN, EN};
            int n_rows = 0;
            for (int i = 0; i < L && n_rows < r.max_rows; i++)
                if (r.fr[i] >= 0 && !(r.fl[i] & 2)) rows[n_rows++] = i;
            for (int i = 0; i < n_rows; i++)
                if (r.pend[rows[i]] + n[i] > (int32_t) mp3mi_feed_capacity(r.f)) n[i] = 0;
            OK(tick(r, n_rows, rows, ctl, n, zero3));
            if (n_rows) {
                const uint8_t again[1] = {EN};
                if (mp3mi_feed_lanes(r.f, r.pend, r.fr, r.fl) > 0 && r.fr[rows[0]] >= 0) BAD(tick(r, 1, rows, again, zero3, zero3));
            }
        }
        if (settled(r)) return 1;
        EXPECT(mp3mi_feed_lanes(r.f, r.pend, r.fr, r.fl) == 0);
        mp3mi_feed_destroy(r.f);
        // detached: the batch is the caller's again, and takes a feeder of the other kind
        OK(mp3mi_batch_set_header(r.b, 0, 0, 0));
        OK(mp3mi_batch_reset(r.b));
        OK(mp3mi_feed_create(&r.f, r.b, TICK, MAX_PUSH));
        BAD(mp3mi_feed_tick_lanes(r.f, 0, NULL, NULL, 0, NULL, NULL, NULL, r.out.data(), r.stride, r.len.data(), r.slot_lane));
        mp3mi_feed_destroy(r.f);
    } else {
        const int32_t rows[1] = {L - 1}, n[1] = {MAX_PUSH};
        const uint8_t ctl[1] = {ST};
        OK(tick(r, 1, rows, ctl, n, zero3)); // (work in flight, lanes waiting, parked and open: all of it goes with the batch)
    }
    mp3mi_batch_destroy(r.b);
    return 0;
}

int main(void)
{
    if (run(5, true)) return 1;  // more lanes than slots
    if (run(2, false)) return 1; // as many
    if (run(1, true)) return 1;  // fewer
    printf("feed_lanes: ok\n");
    return 0;
}
