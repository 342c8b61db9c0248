// TEST INFRASTRUCTURE (CPU only): a Layer I and a Layer II batch through a bitrate per stream (mp3mi_l12_batch_encode_slots_kbps),
// export, import and continue (mp3mi_l12_batch_slots_export / _import), the import that is a fresh batch's first call, one refused call
// of each kind, and destroy, under a host sanitizer -- the host side, the emulator, this program and the kernel files such calls run
// are instrumented, so an index out of a slot list, a rate block, a history row or a state record is a report, and so is a buffer the
// grown control ring or mp3mi_l12_batch_destroy forgets (the emulator's device memory is calloc, its events are new).  The state
// records are heap blocks of exactly n * stride bytes.  Checks return codes and the books; parity is the suite's business
// (tests/test_l12_slot_park.py).  Build and run: make -C tests/hipemu -f l12_park.mk l12_park
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
        if (rc_ != MP3MI_OK) { fprintf(stderr, "l12_park: %s returned %ld (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)
#define BAD(call)                                                                    \
    do {                                                                             \
        const long rc_ = (long) (call);                                              \
        if (rc_ != MP3MI_ERR_ARG) { fprintf(stderr, "l12_park: %s returned %ld, not MP3MI_ERR_ARG (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)
#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "l12_park: %s does not hold (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

static const int S = 5, RATE = 44100, C = 2;
static const uint8_t ST = MP3MI_SLOT_START, EN = MP3MI_SLOT_END;

static int layer(int layer, int nf, unsigned scratch_mb)
{
    const int spf = layer == 1 ? 384 : 1152, full = nf * spf, top = layer == 1 ? 448 : 384, low = layer == 1 ? 32 : 64;
    const int create[S] = {128, 128, 128, 128, top};
    mp3mi_l12_batch *b = NULL, *fresh = NULL;
    OK(mp3mi_l12_batch_create(&b, layer, S, RATE, C, create, 0, nf, scratch_mb));
    OK(mp3mi_l12_batch_create(&fresh, layer, 2, RATE, C, NULL, top, nf, scratch_mb));
    const size_t row = (size_t) full * C, stride = mp3mi_l12_batch_out_stride(b, nf), sb = mp3mi_l12_batch_slot_state_bytes(b);
    EXPECT(sb == (size_t) C * 5696 && mp3mi_l12_batch_slot_state_bytes(fresh) == sb);
    // exact sizes, on the heap (aligned_alloc: multiples of 16): a byte past a row's or a record's end is a report
    std::vector<int16_t> pcm(row * S);
    std::vector<uint8_t> out(stride * S);
    std::vector<uint32_t> len(S);
    uint8_t *rec = (uint8_t *) aligned_alloc(16, 3 * sb);
    EXPECT(rec != NULL);
    mp3mi_l12_slot_ticket tk[3];
    int64_t fr[S];
    int32_t kb[S];
    for (int s = 0; s < S; s++) mp3mi_synth_pcm(pcm.data() + row * s, full, C, RATE, (uint32_t) (300 + s), 0x6D70336Du);
#define SLOTS(bb, ctl, ns, k) mp3mi_l12_batch_encode_slots_kbps(bb, pcm.data(), nf, ctl, ns, k, out.data(), mp3mi_l12_batch_out_stride(bb, nf), len.data())

    {   // slots 0 .. 2 START, at the lowest bitrate, the slot's own and the ceiling; a call without an array goes on (the grown ring entry
        // beside the one that was never grown)
        const uint8_t ctl[S] = {ST, ST, ST, 0, 0}, none[S] = {0, 0, 0, 0, 0};
        const int32_t k[S] = {low, 0, top, 0, 0};
        OK(SLOTS(b, ctl, NULL, k));
        OK(SLOTS(b, none, NULL, NULL));
        OK(SLOTS(b, none, NULL, k)); // (the persistent array: the open streams' own bitrates)
        EXPECT(mp3mi_l12_batch_slot_kbps(b, kb) == top && kb[0] == low && kb[1] == 128 && kb[2] == top && kb[3] == 128 && kb[4] == top);
        EXPECT(mp3mi_l12_batch_slot_frames(b, fr) == 3 && fr[0] == 3 * nf && fr[3] == -1);
    }
    {   // one refusal per call
        const uint8_t st3[S] = {0, 0, 0, ST, 0}, none[S] = {0, 0, 0, 0, 0};
        const int32_t over[S] = {0, 0, 0, top + 32, 0}, odd[S] = {0, 0, 0, 100, 0}, other[S] = {128, 0, 0, 0, 0};
        const int32_t twice[2] = {0, 0}, closed[1] = {3}, open1[1] = {1}, far[1] = {S};
        BAD(SLOTS(b, st3, NULL, over));
        BAD(SLOTS(b, st3, NULL, odd));
        BAD(SLOTS(b, none, NULL, other));
        BAD(mp3mi_l12_batch_slots_export(b, 2, twice, 1, rec, sb, tk));
        BAD(mp3mi_l12_batch_slots_export(b, 1, closed, 1, rec, sb, tk));
        BAD(mp3mi_l12_batch_slots_export(b, 1, far, 1, rec, sb, tk));
        BAD(mp3mi_l12_batch_slots_export(b, 1, open1, 1, rec + 8, sb, tk));
        BAD(mp3mi_l12_batch_slots_export(b, 1, open1, 1, rec, sb - 16, tk));
        BAD(mp3mi_l12_batch_slot_kbps(b, NULL));
        EXPECT(mp3mi_l12_batch_slot_frames(b, fr) == 3 && fr[1] == 3 * nf);
    }
    {   // slots 0 and 2 leave, slot 1 is copied; back to back with the call that reuses slot 0 and the imports -- the ring's fences
        const int32_t leave[2] = {2, 0}, snap[1] = {1}, into[2] = {3, 2}, first[2] = {1, 0};
        OK(mp3mi_l12_batch_slots_export(b, 2, leave, 1, rec, sb, tk));
        OK(mp3mi_l12_batch_slots_export(b, 1, snap, 0, rec + 2 * sb, sb, tk + 2));
        EXPECT(tk[0].kbps == top && tk[1].kbps == low && tk[2].kbps == 128 && tk[0].frames == 3 * nf && tk[2].reserved == 0);
        EXPECT(mp3mi_l12_batch_slot_kbps(b, kb) == top && kb[0] == 128 && kb[2] == 128);
        const uint8_t ctl[S] = {(uint8_t) (ST | EN), 0, 0, 0, 0};
        const int32_t ns[S] = {full - 1, full, 0, 0, 0};
        OK(SLOTS(b, ctl, ns, NULL)); // slot 0 at its own bitrate again: cfg is put back
        // refused imports: an open slot, a ticket with a field altered, a bitrate above the ceiling of the other batch
        mp3mi_l12_slot_ticket bad = tk[0];
        bad.reserved = 1;
        BAD(mp3mi_l12_batch_slots_import(b, 1, snap, rec, sb, tk));
        BAD(mp3mi_l12_batch_slots_import(b, 1, into, rec, sb, &bad));
        bad = tk[0];
        bad.kbps = top + 32;
        BAD(mp3mi_l12_batch_slots_import(b, 1, into, rec, sb, &bad));
        BAD(mp3mi_l12_batch_slots_import(b, 1, into, rec, sb + 8, tk));
        OK(mp3mi_l12_batch_slots_import(b, 2, into, rec, sb, tk));          // the two that left, into other slots
        OK(mp3mi_l12_batch_sync(b));                                        // (another batch reads the records next)
        OK(mp3mi_l12_batch_slots_import(fresh, 2, first, rec + sb, sb, tk + 1)); // the fresh batch's first call: no history buffers yet
        EXPECT(mp3mi_l12_batch_slot_kbps(b, kb) == top && kb[3] == top && kb[2] == low);
        EXPECT(mp3mi_l12_batch_slot_frames(b, fr) == 3 && fr[3] == 3 * nf && fr[2] == 3 * nf && fr[1] == 4 * nf && fr[0] == -1);
        EXPECT(mp3mi_l12_batch_slot_frames(fresh, fr) == 2 && fr[0] == 3 * nf);
        EXPECT(mp3mi_l12_batch_slot_kbps(fresh, kb) == top && kb[1] == low && kb[0] == 128);
    }
    {   // continue everywhere; the fresh batch hands over to the whole-batch path (both slots at one frame) and ends by its flush
        const uint8_t ctl[S] = {0, EN, EN, 0, 0};
        const int32_t ns[S] = {0, 7, 0, full, 0};
        OK(SLOTS(b, ctl, ns, NULL));
        OK(mp3mi_l12_batch_encode_next(fresh, pcm.data(), nf, out.data(), mp3mi_l12_batch_out_stride(fresh, nf), len.data()));
        OK(mp3mi_l12_batch_flush(fresh, out.data(), mp3mi_l12_batch_out_stride(fresh, nf), len.data()));
        OK(mp3mi_l12_batch_sync(fresh));
        EXPECT(len[0] == 1 && len[1] == 1);
        EXPECT(mp3mi_l12_batch_slot_kbps(fresh, kb) == top && kb[0] == top && kb[1] == top);
        // every stream afresh after other bitrates: cfg goes back in a turn of its own
        OK(mp3mi_l12_batch_encode_next(fresh, pcm.data(), nf, out.data(), mp3mi_l12_batch_out_stride(fresh, nf), len.data()));
        OK(mp3mi_l12_batch_encode(b, pcm.data(), NULL, nf, out.data(), stride, len.data()));
        OK(mp3mi_l12_batch_sync(b));
        EXPECT(mp3mi_l12_batch_slot_frames(b, fr) == 0 && len[0] > 1);
        const int32_t again[1] = {4};
        OK(mp3mi_l12_batch_slots_import(b, 1, again, rec, sb, tk)); // left open at destroy
    }
#undef SLOTS
    mp3mi_l12_batch_destroy(fresh);
    mp3mi_l12_batch_destroy(b);
    free(rec);
    return 0;
}

int main(void)
{
    // Layer I down to 32 kbps, two channels: the frames that outgrow their slots.  Short calls: the instrumented kernels are slow, and
    // what is looked at here is the host side and the two small kernels, whose work does not depend on a call's length
    if (layer(1, 2, 0) != 0 || layer(2, 1, 0) != 0) return 1;
    printf("l12_park ok: Layer I and Layer II batches through bitrates per stream, export and import, and destroyed\n");
    return 0;
}
