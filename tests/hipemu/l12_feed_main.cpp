// TEST INFRASTRUCTURE (CPU only): the feeder of a Layer I and of a Layer II batch (mp3mi_l12_feed_*) under a host sanitizer -- the host
// side, the emulator, this program and the kernel files a tick runs are instrumented, so an index out of a descriptor block, a ring,
// a row or a history row is a report, and so is a buffer that mp3mi_l12_feed_destroy or mp3mi_l12_batch_destroy forgets (the
// emulator's device memory is calloc, its events are new).  Five lanes over two slots: ticks in which lanes wait for a slot, leave
// one, resume in another -- at another bitrate than the slot's, too -- and drain; one refused tick and one refused batch call;
// destroy in both orders.  The push rows and the output are heap blocks of exact size.  Checks return codes and the books; parity is
// the suite's business (tests/test_l12_feed.py).  Build and run: make -C tests/hipemu -f l12_feed.mk l12_feed
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mp3mi.h"
#include "mp3mi_l12.h"

#define OK(call)                                                                     \
    do {                                                                             \
        const long rc_ = (long) (call);                                              \
        if (rc_ != MP3MI_OK) { fprintf(stderr, "l12_feed: %s returned %ld (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)
#define BAD(call)                                                                    \
    do {                                                                             \
        const long rc_ = (long) (call);                                              \
        if (rc_ != MP3MI_ERR_ARG) { fprintf(stderr, "l12_feed: %s returned %ld, not MP3MI_ERR_ARG (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)
#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "l12_feed: %s does not hold (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

static const int S = 2, LANES = 5, RATE = 44100, C = 2;
static const uint8_t ST = MP3MI_SLOT_START, EN = MP3MI_SLOT_END;

static int layer(int layer, int feeder_first)
{
    const int spf = layer == 1 ? 384 : 1152, top = layer == 1 ? 448 : 384;
    const int create[S] = {128, top};
    mp3mi_l12_batch *b = NULL;
    mp3mi_l12_feed *f = NULL, *g = NULL;
    OK(mp3mi_l12_batch_create(&b, layer, S, RATE, C, create, 0, 2, 0));
    BAD(mp3mi_l12_feed_create(&f, b, LANES, LANES + 1, 1, spf, 0));
    OK(mp3mi_l12_feed_create(&f, b, LANES, 3, 1, spf, 2 * spf + 7)); // (a ring whose length is no multiple of 8 samples)
    BAD(mp3mi_l12_feed_create(&g, b, LANES, 3, 1, spf, 0));
    EXPECT(mp3mi_l12_feed_capacity(f) == (size_t) (2 * spf + 7) && mp3mi_l12_feed_n_lanes(f) == LANES);
    const size_t pitch = (size_t) spf, stride = mp3mi_l12_batch_out_stride(b, 1);
    std::vector<int16_t> pcm(3 * pitch * C); // three rows of exactly max_push samples
    std::vector<uint8_t> out(stride * S);
    std::vector<uint32_t> len(S);
    int32_t sl[S], pend[LANES];
    int64_t fr[LANES], sfr[S];
    uint8_t fl[LANES];
    for (int r = 0; r < 3; r++) mp3mi_synth_pcm(pcm.data() + pitch * C * r, spf, C, RATE, (uint32_t) (500 + r), 0x6D70336Du);
#define TICK(n, rows, ctl, ns, kb) mp3mi_l12_feed_tick(f, n, rows, pcm.data(), pitch, ctl, ns, kb, out.data(), stride, len.data(), sl)
    {   // lanes 0, 2 and 4 START with a tick each, at three bitrates: two encode, lane 4 waits for a slot
        const int32_t rows[3] = {0, 2, 4}, ns[3] = {spf, spf, spf}, kb[3] = {64, 0, top};
        const uint8_t ctl[3] = {ST, ST, ST};
        OK(TICK(3, rows, ctl, ns, kb));
        EXPECT(sl[0] == 0 && sl[1] == 2);
        EXPECT(mp3mi_l12_feed_lanes(f, pend, fr, fl) == 3 && fl[4] == (4 | 8) && pend[4] == spf && fr[0] == 1);
    }
    {   // one refused tick (a push on a closed lane beside a good row) and one refused batch call: nothing changes
        const int32_t rows[2] = {0, 1}, ns[2] = {5, 5}, kb[2] = {0, 0};
        const uint8_t ctl[2] = {0, 0};
        BAD(TICK(2, rows, ctl, ns, kb));
        BAD(mp3mi_l12_batch_reset(b));
        BAD(mp3mi_l12_batch_set_error_protection(b, 1));
        EXPECT(mp3mi_l12_feed_lanes(f, pend, fr, fl) == 3 && pend[0] == 0 && fl[4] == (4 | 8));
    }
    {   // lane 0 sits out and leaves slot 0, which lane 4 takes with its START -- at another bitrate than lane 0 left there
        const int32_t rows[2] = {0, 2}, ns[2] = {spf / 2, spf}, kb[2] = {64, 0};
        const uint8_t ctl[2] = {0, 0};
        OK(TICK(2, rows, ctl, ns, kb));
        EXPECT(sl[0] == 4 && sl[1] == 2);
        EXPECT(mp3mi_l12_batch_slot_frames(b, sfr) == 2 && sfr[0] == 1 && sfr[1] == 2);
        EXPECT(mp3mi_l12_feed_lanes(f, pend, fr, fl) == 3 && fl[0] == 1 && fl[4] == 0);
    }
    for (int t = 0; t < 6; t++) {
        // t 0: lane 4 ENDs with nothing pending and waits, parked; lane 0 resumes in slot 0, whose cfg stands at lane 4's bitrate.
        // t 1: lane 0 sits out again; lane 4 resumes there and closes.  t 2: lanes 0 and 2 END; lane 0 resumes once more.  Then nothing
        const int32_t rows[3] = {0, 2, 4}, ns[3] = {t < 2 ? spf / 2 + 1 : 0, t < 2 ? spf : 0, 0}, kb[3] = {0, 0, 0};
        const uint8_t ctl[3] = {(uint8_t) (t == 2 ? EN : 0), (uint8_t) (t == 2 ? EN : 0), (uint8_t) (t == 0 ? EN : 0)};
        OK(TICK(t <= 2 ? (t == 0 ? 3 : 2) : 0, rows, ctl, ns, kb));
        if (t == 0) EXPECT(sl[0] == 0 && sl[1] == 2);
        if (t == 1) EXPECT(sl[0] == 4 && sl[1] == 2);
        if (t == 2) EXPECT(sl[0] == 0 && sl[1] == 2);
        if (t > 2) EXPECT(sl[0] == -1 && sl[1] == -1);
    }
    OK(mp3mi_l12_batch_sync(b));
    EXPECT(mp3mi_l12_feed_lanes(f, pend, fr, fl) == 0);
    {   // streams left open -- in a slot, parked and waiting -- when the feeder or the batch goes
        const int32_t rows[3] = {1, 2, 3}, ns[3] = {spf, spf, spf}, kb[3] = {0, 0, 0}, one[1] = {1}, none[1] = {0};
        const uint8_t ctl[3] = {ST, ST, ST}, z[1] = {0};
        OK(TICK(3, rows, ctl, ns, kb));
        OK(TICK(1, one, z, none, none));
        EXPECT(mp3mi_l12_feed_lanes(f, pend, fr, fl) == 3);
    }
#undef TICK
    if (feeder_first) {
        mp3mi_l12_feed_destroy(f);
        EXPECT(mp3mi_l12_batch_slot_frames(b, sfr) == 0);
        OK(mp3mi_l12_batch_reset(b)); // the batch is the caller's again
    }
    mp3mi_l12_batch_destroy(b); // (with the feeder attached: it goes with the batch)
    return 0;
}

int main(void)
{
    if (layer(1, 1) != 0 || layer(2, 0) != 0 || layer(1, 0) != 0) return 1;
    printf("l12_feed ok: Layer I and Layer II feeders through waits, resumes and drains, destroyed in both orders\n");
    return 0;
}
