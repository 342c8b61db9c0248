// TEST INFRASTRUCTURE (CPU only): a feeder's ticks on host buffers (mp3mi_feed_tick_lanes_host_async, mp3mi_feed_host_wait,
// mp3mi_feed_host_io_stats, include/mp3mi.h) under a host sanitizer -- batch.cpp with feed.h, k_format.hip with k_feed_packed and
// k_rows_out, the emulator and this program are instrumented, so an index out of the packed staging, the work list, the upload block,
// the tick slot's rows or the dense rows is a report, and so is a buffer, a stream or an event of the host ticks that
// mp3mi_feed_destroy or mp3mi_batch_destroy forgets.  Every buffer the caller brings lies on the heap with exactly the stated size:
// the packed samples sum(n_push) * channels, the rows n_streams * out_stride, the lengths and the two lists n_streams.  Host ticks
// with lanes that wait, move and refill a slot in the tick that vacated it; a regrow of the dense rows by a larger stride; refused
// calls; alternation with device ticks; destroy with ticks in flight, feeder first and batch first.  Checks return codes, the lists,
// the canaries behind n_out, the statistics and the lanes' books; parity is the suite's business (tests/test_feed_host.py).
// Build and run: make -C tests/hipemu -f feed_host.mk feed_host
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mp3mi.h"

#define OK(call)                                                                     \
    do {                                                                             \
        const long rc_ = (long) (call);                                              \
        if (rc_ != MP3MI_OK) { fprintf(stderr, "feed_host: %s returned %ld (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)
#define BAD(call)                                                                    \
    do {                                                                             \
        const long rc_ = (long) (call);                                              \
        if (rc_ != MP3MI_ERR_ARG) { fprintf(stderr, "feed_host: %s returned %ld, not MP3MI_ERR_ARG (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)
#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "feed_host: %s does not hold (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

static const int S = 2, C = 2, RATE = 44100, TICK = 1, FULL = 1152, MAX_PUSH = 1500, L = 5, MAX_ROWS = 3;
static const uint8_t ST = MP3MI_SLOT_START, EN = MP3MI_SLOT_END, CANARY = 0xA5;

// the buffers of one host tick, each of exactly the size the contract states; kept until the tick has been waited for
struct tick_bufs {
    std::vector<int16_t> pcm;
    std::vector<uint8_t> out;
    std::vector<uint32_t> len;
    std::vector<int32_t> lane, slot;
    int32_t n_out;
    size_t stride;
};

struct rig {
    mp3mi_batch *b;
    mp3mi_feed *f;
    size_t stride;
    double up, dn;
    long ticks;
    std::vector<tick_bufs *> kept;
    ~rig() { for (tick_bufs *t : kept) delete t; }
};

static int host_tick(rig &r, int n_rows, const int32_t *rows, const uint8_t *ctl, const int32_t *n, const int32_t *kbps, size_t stride, tick_bufs **out)
{
    tick_bufs *t = new tick_bufs();
    r.kept.push_back(t);
    size_t all = 0;
    for (int k = 0; k < n_rows; k++) all += (size_t) n[k];
    t->pcm.resize(all * C);
    for (size_t at = 0, k = 0; k < (size_t) n_rows; at += (size_t) n[k] * C, k++)
        if (n[k]) mp3mi_synth_pcm(t->pcm.data() + at, n[k], C, RATE, (uint32_t) (600 + rows[k]), 0x6D70336Du);
    t->stride = stride;
    t->out.assign(stride * S, CANARY);
    t->len.assign(S, 0xDEADBEEFu);
    t->lane.assign(S, -9);
    t->slot.assign(S, -9);
    t->n_out = -9;
    OK(mp3mi_feed_tick_lanes_host_async(r.f, n_rows, rows, all ? t->pcm.data() : NULL, ctl, n, kbps, t->out.data(), stride, t->len.data(), t->lane.data(),
                                        t->slot.data(), &t->n_out));
    EXPECT(t->n_out >= 0 && t->n_out <= S);
    for (int i = 0; i < S; i++) EXPECT(i < t->n_out ? (t->lane[i] >= 0 && t->lane[i] < L && t->slot[i] >= 0 && t->slot[i] < S) : (t->lane[i] == -9 && t->slot[i] == -9));
    EXPECT(t->n_out < 2 || (t->lane[0] < t->lane[1] && t->slot[0] != t->slot[1]));
    r.up += (double) (all * C * 2);
    r.dn += (double) t->n_out * (double) (stride + 4);
    r.ticks++;
    *out = t;
    return 0;
}

// a tick that has been waited for: rows zero behind their lengths, canaries from n_out on
static int delivered(const tick_bufs *t)
{
    for (int i = 0; i < S; i++) {
        const uint8_t *row = t->out.data() + (size_t) i * t->stride;
        if (i < t->n_out) {
            EXPECT(t->len[i] <= t->stride);
            for (size_t k = t->len[i]; k < t->stride; k++) EXPECT(row[k] == 0);
        } else {
            EXPECT(t->len[i] == 0xDEADBEEFu);
            for (size_t k = 0; k < t->stride; k++) EXPECT(row[k] == CANARY);
        }
    }
    return 0;
}

static int stats_exact(rig &r)
{
    mp3mi_host_io_stats st;
    OK(mp3mi_feed_host_io_stats(r.f, &st));
    EXPECT(st.calls == r.ticks && st.h2d_bytes == r.up && st.d2h_bytes == r.dn);
    return 0;
}

static int run(bool feeder_first)
{
    rig r;
    r.b = NULL;
    r.f = NULL;
    r.up = r.dn = 0;
    r.ticks = 0;
    OK(mp3mi_batch_create(&r.b, S, RATE, C, NULL, 128, TICK));
    OK(mp3mi_feed_create_lanes(&r.f, r.b, L, MAX_ROWS, TICK, MAX_PUSH, FULL + MAX_PUSH + 700));
    r.stride = mp3mi_batch_out_stride(r.b, TICK);
    BAD(mp3mi_feed_host_wait(r.f, 0)); // no host tick yet
    if (stats_exact(r)) return 1;
    const int32_t zero3[3] = {0, 0, 0};
    tick_bufs *t0, *t1, *t2, *t3;
    {   // three lanes START with a tick on two slots: lane 2 waits
        const int32_t rows[3] = {0, 1, 2}, n[3] = {FULL, FULL, FULL}, kbps[3] = {0, 64, 96};
        const uint8_t ctl[3] = {ST, ST, ST};
        if (host_tick(r, 3, rows, ctl, n, kbps, r.stride, &t0)) return 1;
        EXPECT(t0->n_out == 2 && t0->lane[0] == 0 && t0->lane[1] == 1 && t0->slot[0] == 0 && t0->slot[1] == 1);
        BAD(mp3mi_feed_host_wait(r.f, 1)); // none before it
    }
    {   // a packet, a row of no samples and two STARTs: lanes 0 and 1 sit out, lane 2 STARTs in the slot lane 0 leaves in this tick, lane 4 waits
        const int32_t rows[3] = {2, 3, 4}, n[3] = {7, 0, FULL};
        const uint8_t ctl[3] = {0, ST, ST};
        if (host_tick(r, 3, rows, ctl, n, zero3, r.stride, &t1)) return 1;
        EXPECT(t1->n_out == 2 && t1->lane[0] == 2 && t1->lane[1] == 4 && t1->slot[0] == 0 && t1->slot[1] == 1);
    }
    {   // the third tick in a row waits for the first by itself; a LARGER stride, no multiple of 16: the dense rows grow
        const int32_t rows[2] = {0, 1}, n[2] = {FULL, MAX_PUSH};
        const uint8_t ctl[2] = {0, 0};
        if (host_tick(r, 2, rows, ctl, n, zero3, r.stride + 40, &t2)) return 1;
        EXPECT(t2->n_out == 2 && t2->lane[0] == 0 && t2->lane[1] == 1);
        if (delivered(t0)) return 1;
        OK(mp3mi_feed_host_wait(r.f, 1));
        if (delivered(t1)) return 1;
        EXPECT(t0->len[0] + t0->len[1] > 0);
    }
    {   // refused calls: nothing is told, nothing is written, the books stay
        int32_t p0[L], p1[L];
        int64_t f0[L], f1[L];
        uint8_t g0[L], g1[L];
        const int open0 = mp3mi_feed_lanes(r.f, p0, f0, g0);
        tick_bufs b;
        b.pcm.assign(8 * C, 1);
        b.out.assign(r.stride * S, CANARY);
        b.len.assign(S, 0xDEADBEEFu);
        b.lane.assign(S, -9);
        b.slot.assign(S, -9);
        b.n_out = -9;
        const int32_t row3[1] = {3}, n8[1] = {8}, n0[1] = {0}, over[1] = {MAX_PUSH + 1}, rowL[1] = {L}, k_bad[1] = {100};
        const uint8_t none[1] = {0}, start[1] = {ST}, unknown[1] = {4};
#define TICK_WITH(pcm, out, len, lane, slot, nout, ctl, n, kbps, row, stride) \
    mp3mi_feed_tick_lanes_host_async(r.f, 1, row, pcm, ctl, n, kbps, out, stride, len, lane, slot, nout)
        BAD(TICK_WITH(NULL, b.out.data(), b.len.data(), b.lane.data(), b.slot.data(), &b.n_out, none, n8, n0, row3, r.stride)); // a push, no samples
        BAD(TICK_WITH(b.pcm.data(), NULL, b.len.data(), b.lane.data(), b.slot.data(), &b.n_out, none, n8, n0, row3, r.stride));
        BAD(TICK_WITH(b.pcm.data(), b.out.data(), NULL, b.lane.data(), b.slot.data(), &b.n_out, none, n8, n0, row3, r.stride));
        BAD(TICK_WITH(b.pcm.data(), b.out.data(), b.len.data(), NULL, b.slot.data(), &b.n_out, none, n8, n0, row3, r.stride));
        BAD(TICK_WITH(b.pcm.data(), b.out.data(), b.len.data(), b.lane.data(), NULL, &b.n_out, none, n8, n0, row3, r.stride));
        BAD(TICK_WITH(b.pcm.data(), b.out.data(), b.len.data(), b.lane.data(), b.slot.data(), NULL, none, n8, n0, row3, r.stride));
        BAD(TICK_WITH(b.pcm.data(), b.out.data(), b.len.data(), b.lane.data(), b.slot.data(), &b.n_out, none, n8, n0, row3, r.stride - 1));
        BAD(TICK_WITH(b.pcm.data(), b.out.data(), b.len.data(), b.lane.data(), b.slot.data(), &b.n_out, unknown, n8, n0, row3, r.stride));
        BAD(TICK_WITH(b.pcm.data(), b.out.data(), b.len.data(), b.lane.data(), b.slot.data(), &b.n_out, none, over, n0, row3, r.stride));
        BAD(TICK_WITH(b.pcm.data(), b.out.data(), b.len.data(), b.lane.data(), b.slot.data(), &b.n_out, none, n8, n0, rowL, r.stride));
        BAD(TICK_WITH(b.pcm.data(), b.out.data(), b.len.data(), b.lane.data(), b.slot.data(), &b.n_out, start, n8, k_bad, row3, r.stride));
        BAD(TICK_WITH(b.pcm.data(), b.out.data(), b.len.data(), b.lane.data(), b.slot.data(), &b.n_out, none, n8, n0, NULL, r.stride));
        BAD(mp3mi_feed_tick_lanes_host_async(NULL, 0, NULL, NULL, NULL, NULL, NULL, b.out.data(), r.stride, b.len.data(), b.lane.data(), b.slot.data(), &b.n_out));
        BAD(mp3mi_feed_tick_lanes_host_async(r.f, MAX_ROWS + 1, row3, b.pcm.data(), none, n0, n0, b.out.data(), r.stride, b.len.data(), b.lane.data(),
                                             b.slot.data(), &b.n_out));
#undef TICK_WITH
        BAD(mp3mi_feed_host_wait(r.f, 2));
        BAD(mp3mi_feed_host_wait(r.f, -1));
        BAD(mp3mi_feed_host_wait(NULL, 0));
        BAD(mp3mi_feed_host_io_stats(r.f, NULL));
        EXPECT(b.n_out == -9 && b.lane[0] == -9 && b.slot[1] == -9 && b.len[0] == 0xDEADBEEFu);
        for (size_t k = 0; k < b.out.size(); k++) EXPECT(b.out[k] == CANARY);
        EXPECT(mp3mi_feed_lanes(r.f, p1, f1, g1) == open0 && !memcmp(p0, p1, sizeof(p0)) && !memcmp(f0, f1, sizeof(f0)) && !memcmp(g0, g1, sizeof(g0)));
    }
    OK(mp3mi_feed_host_wait(r.f, 0));
    if (delivered(t2)) return 1;
    if (stats_exact(r)) return 1;
    {   // a device tick between host ticks: the rings and the rows are the same ones
        std::vector<int16_t> pcm((size_t) MAX_PUSH * C * 1);
        std::vector<uint8_t> out(r.stride * S);
        std::vector<uint32_t> len(S);
        int32_t slot_lane[S];
        mp3mi_synth_pcm(pcm.data(), MAX_PUSH, C, RATE, 700, 0x6D70336Du);
        const int32_t rows[1] = {2}, n[1] = {FULL};
        const uint8_t ctl[1] = {0};
        OK(mp3mi_feed_tick_lanes(r.f, 1, rows, pcm.data(), MAX_PUSH, ctl, n, zero3, out.data(), r.stride, len.data(), slot_lane));
        OK(mp3mi_batch_sync(r.b));
        EXPECT(slot_lane[0] >= 0 || slot_lane[1] >= 0);
    }
    {   // a host tick without rows and without samples (nobody is ready: nothing comes down); then one in which rows push nothing
        if (host_tick(r, 0, NULL, NULL, NULL, NULL, r.stride, &t3)) return 1;
        OK(mp3mi_batch_sync(r.b)); // (mp3mi_batch_sync waits for the host ticks' copies too)
        if (delivered(t3)) return 1;
        const int32_t rows[2] = {0, 3}, n[2] = {0, 0};
        const uint8_t ctl[2] = {0, 0};
        const double up = r.up;
        if (host_tick(r, 2, rows, ctl, n, zero3, r.stride, &t3)) return 1;
        EXPECT(r.up == up);
        OK(mp3mi_feed_host_wait(r.f, 0));
        if (delivered(t3)) return 1;
        if (stats_exact(r)) return 1;
    }
    {   // two host ticks in flight when everything goes: lanes END, others wait, parked records and staging are in use
        const int32_t rows[3] = {0, 1, 3}, n[3] = {33, 0, 960};
        const uint8_t ctl[3] = {EN, EN, 0};
        if (host_tick(r, 3, rows, ctl, n, zero3, r.stride, &t3)) return 1;
        const int32_t rows2[1] = {4}, n2[1] = {MAX_PUSH};
        const uint8_t ctl2[1] = {0};
        if (host_tick(r, 1, rows2, ctl2, n2, zero3, r.stride + 40, &t3)) return 1;
    }
    if (feeder_first) {
        mp3mi_feed_destroy(r.f);
        // detached: the batch is the caller's again, and a new feeder starts without host ticks
        OK(mp3mi_batch_reset(r.b));
        OK(mp3mi_feed_create_lanes(&r.f, r.b, 2, 2, TICK, MAX_PUSH, 0));
        BAD(mp3mi_feed_host_wait(r.f, 0));
        mp3mi_feed_destroy(r.f);
        OK(mp3mi_feed_create(&r.f, r.b, TICK, MAX_PUSH)); // the other kind of feeder refuses the call
        tick_bufs b;
        b.out.assign(r.stride * S, CANARY);
        b.len.assign(S, 0);
        b.lane.assign(S, -9);
        b.slot.assign(S, -9);
        BAD(mp3mi_feed_tick_lanes_host_async(r.f, 0, NULL, NULL, NULL, NULL, NULL, b.out.data(), r.stride, b.len.data(), b.lane.data(), b.slot.data(), &b.n_out));
        mp3mi_feed_destroy(r.f);
    }
    mp3mi_batch_destroy(r.b); // (with the feeder attached, and its ticks in flight, unless it went first)
    return 0;
}

int main(void)
{
    if (run(true)) return 1;
    if (run(false)) return 1;
    printf("feed_host: ok\n");
    return 0;
}
