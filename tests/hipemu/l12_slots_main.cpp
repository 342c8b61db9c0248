// TEST INFRASTRUCTURE (CPU only): a Layer I and a Layer II batch through per-slot calls (mp3mi_l12_batch_encode_slots) with churn,
// calls that break a rule, flush, reset and destroy, under a host sanitizer -- the host side, the emulator, this program and the
// three kernels files a per-slot call runs are instrumented, so an index out of a control block, a history row or an output row
// is a report, and so is a buffer or an event that mp3mi_l12_batch_destroy forgets (the emulator's device memory is calloc, its
// events are new).  Checks return codes, lengths and the slots' frames; parity is the suite's business (tests/test_l12_slots.py).
// Build and run: make -C tests/hipemu -f l12_slots.mk l12_slots
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
        if (rc_ != MP3MI_OK) { fprintf(stderr, "l12_slots: %s returned %ld (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)
#define BAD(call)                                                                    \
    do {                                                                             \
        const long rc_ = (long) (call);                                              \
        if (rc_ != MP3MI_ERR_ARG) { fprintf(stderr, "l12_slots: %s returned %ld, not MP3MI_ERR_ARG (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)
#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "l12_slots: %s does not hold (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

static const int S = 5, RATE = 44100, C = 2;
static const uint8_t ST = MP3MI_SLOT_START, EN = MP3MI_SLOT_END;

static int layer(int layer, int nf, unsigned scratch_mb)
{
    const int spf = layer == 1 ? 384 : 1152, full = nf * spf;
    mp3mi_l12_batch *b = NULL;
    OK(mp3mi_l12_batch_create(&b, layer, S, RATE, C, NULL, layer == 1 ? 32 : 128, nf, scratch_mb));
    const size_t row = (size_t) full * C, stride = mp3mi_l12_batch_out_stride(b, nf);
    // exact sizes, on the heap: a byte past a row's end is a report
    std::vector<int16_t> pcm(row * S);
    std::vector<uint8_t> out(stride * S);
    std::vector<uint32_t> len(S);
    int64_t fr[S];
    for (int s = 0; s < S; s++) mp3mi_synth_pcm(pcm.data() + row * s, full, C, RATE, (uint32_t) (200 + s), 0x6D70336Du);
#define SLOTS(ctl, ns) mp3mi_l12_batch_encode_slots(b, pcm.data(), nf, ctl, ns, out.data(), stride, len.data())

    EXPECT(mp3mi_l12_batch_slot_frames(b, fr) == 0);
    {   // slots 0, 2 and the last START; the others stay closed
        const uint8_t ctl[S] = {ST, 0, ST, 0, ST};
        OK(SLOTS(ctl, NULL));
        OK(mp3mi_l12_batch_sync(b));
        EXPECT(len[1] == 0 && len[3] == 0 && len[0] > 0 && len[4] > 0);
        EXPECT(mp3mi_l12_batch_slot_frames(b, fr) == 3 && fr[0] == nf && fr[1] == -1 && fr[4] == nf);
    }
    {   // calls that break a rule leave the batch alone
        const uint8_t unknown[S] = {0, 4, 0, 0, 0}, end_closed[S] = {0, EN, 0, 0, 0}, none[S] = {0, 0, 0, 0, 0}, end0[S] = {EN, 0, 0, 0, 0};
        const int32_t short_ns[S] = {full - 1, 0, full, 0, full}, closed_ns[S] = {full, 1, full, 0, full}, over_ns[S] = {full + 1, 0, full, 0, full};
        BAD(SLOTS(unknown, NULL));
        BAD(SLOTS(end_closed, NULL));
        BAD(SLOTS(none, short_ns));
        BAD(SLOTS(none, closed_ns));
        BAD(SLOTS(end0, over_ns));
        BAD(SLOTS(NULL, NULL));
        BAD(mp3mi_l12_batch_encode_slots(b, NULL, nf, none, NULL, out.data(), stride, len.data()));
        BAD(mp3mi_l12_batch_encode_slots(b, pcm.data(), nf + 1, none, NULL, out.data(), stride, len.data()));
        BAD(mp3mi_l12_batch_encode_slots(b, pcm.data(), nf, none, NULL, out.data(), stride - 1, len.data()));
        BAD(mp3mi_l12_batch_slot_frames(b, NULL));
        EXPECT(mp3mi_l12_batch_slot_frames(b, fr) == 3 && fr[0] == nf);
    }
    {   // churn, back to back without a sync (both entries of the control ring, and the first again): slot 0 ENDs on a partial
        // frame, slot 1 is a one-call file, slot 2 goes on, slot 3 STARTs and ENDs with nothing, the last slot STARTs over its stream
        const uint8_t ctl[S] = {EN, (uint8_t) (ST | EN), 0, (uint8_t) (ST | EN), ST};
        const int32_t ns[S] = {full - 7, full, full, 0, full};
        OK(SLOTS(ctl, ns));
        const uint8_t ctl2[S] = {ST, 0, EN, 0, 0};
        const int32_t ns2[S] = {full, 0, 0, 0, full};
        OK(SLOTS(ctl2, ns2));
        const uint8_t ctl3[S] = {0, ST, 0, ST, EN};
        const int32_t ns3[S] = {full, full, 0, full, 1};
        OK(SLOTS(ctl3, ns3));
        OK(mp3mi_l12_batch_sync(b));
        EXPECT(len[2] == 0 && len[0] > 0 && len[4] > 1);
        EXPECT(mp3mi_l12_batch_slot_frames(b, fr) == 3 && fr[0] == 2 * nf && fr[1] == nf && fr[2] == -1 && fr[3] == nf && fr[4] == -1);
    }
    OK(mp3mi_l12_batch_encode_next(b, pcm.data(), nf, out.data(), stride, len.data())); // continues the open slots
    OK(mp3mi_l12_batch_flush(b, out.data(), stride, len.data()));                        // ends them
    OK(mp3mi_l12_batch_sync(b));
    EXPECT(len[0] == 1 && len[1] == 1 && len[2] == 0 && len[3] == 1 && len[4] == 0);
    EXPECT(mp3mi_l12_batch_slot_frames(b, fr) == 0);
    OK(mp3mi_l12_batch_encode_next(b, pcm.data(), nf, out.data(), stride, len.data())); // starts every slot
    {   // every slot ENDs: all closed under the per-slot bookkeeping; the flush then delivers nothing
        const uint8_t ctl[S] = {EN, EN, EN, EN, EN};
        const int32_t ns[S] = {0, 1, full, spf, spf + 1};
        OK(SLOTS(ctl, ns));
        OK(mp3mi_l12_batch_flush(b, out.data(), stride, len.data()));
        OK(mp3mi_l12_batch_sync(b));
        for (int s = 0; s < S; s++) EXPECT(len[s] == 0);
    }
    {
        const uint8_t ctl[S] = {ST, ST, 0, 0, 0};
        OK(SLOTS(ctl, NULL));
        OK(mp3mi_l12_batch_reset(b));
        EXPECT(mp3mi_l12_batch_slot_frames(b, fr) == 0);
        OK(SLOTS(ctl, NULL)); // left open at destroy
    }
#undef SLOTS
    mp3mi_l12_batch_destroy(b);
    return 0;
}

int main(void)
{
    // Layer I at 32 kbps, two channels: the frames that outgrow their slots; 1 MiB of scratch over five slots: chunks of 7 and 3
    // frames, two per call
    if (layer(1, 8, 1) != 0 || layer(2, 4, 1) != 0) return 1;
    printf("l12_slots ok: Layer I and Layer II batches driven through per-slot calls and destroyed\n");
    return 0;
}
