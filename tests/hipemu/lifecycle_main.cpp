// TEST INFRASTRUCTURE (CPU only): one batch of each kind through every entry point that allocates, so that a host sanitizer sees
// what the host side owns -- the wave emulator's device memory is calloc and its events are new, so a buffer or an event that
// mp3mi_batch_destroy forgets is a leak report.  Checks return codes only; parity is the suite's business.
// Build and run: make -C tests/hipemu lifecycle
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
        if (rc_ != MP3MI_OK) { fprintf(stderr, "lifecycle: %s returned %ld (line %d)\n", #call, rc_, __LINE__); return 1; } \
    } while (0)

static const int S = 3, RATE = 44100, C = 2, NF = 2;

static int layer3(void)
{
    mp3mi_batch_options opt;
    mp3mi_batch_options_default(&opt);
    opt.chunk_frames = 1; // two chunks per call: both halves of every double buffer
    mp3mi_batch *b = NULL;
    OK(mp3mi_batch_create_ex(&b, S, RATE, C, NULL, 128, NF, &opt));
    const size_t row = (size_t) NF * 1152 * C, stride = mp3mi_batch_out_stride(b, NF);
    // (the emulator's device memory is host memory: the page-locked allocator serves for both sides)
    int16_t *pcm = (int16_t *) mp3mi_host_alloc(sizeof(int16_t) * row * S);
    uint8_t *out = (uint8_t *) mp3mi_host_alloc(stride * S);
    uint32_t *len = (uint32_t *) mp3mi_host_alloc(sizeof(uint32_t) * S);
    if (!pcm || !out || !len) return 1;
    for (int s = 0; s < S; s++) mp3mi_synth_pcm(pcm + row * s, NF * 1152, C, RATE, (uint32_t) s, 0x6D70336Du);

    OK(mp3mi_batch_encode(b, pcm, NF, out, stride, len)); // a whole-file call
    OK(mp3mi_batch_sync(b));
    OK(mp3mi_batch_encode_next(b, pcm, NF, out, stride, len)); // streaming
    OK(mp3mi_batch_flush(b, out, stride, len));
    OK(mp3mi_batch_sync(b));
    {   // a per-slot call: slot 0 STARTs at another bitrate than the batch's
        const uint8_t ctl[S] = {MP3MI_SLOT_START, 0, 0};
        const int32_t kbps[S] = {64, 0, 0};
        OK(mp3mi_batch_encode_slots_kbps(b, pcm, NF, ctl, NULL, kbps, out, stride, len));
    }
    {   // a per-slot call on host buffers with a row map: slot 0 goes on, slot 1 STARTs, slot 2 has no row
        const int32_t rows[2] = {0, 1};
        const uint8_t ctl[2] = {0, MP3MI_SLOT_START};
        OK(mp3mi_batch_encode_slots_host_async(b, pcm, NF, 2, rows, ctl, NULL, out, stride, len));
        OK(mp3mi_batch_host_wait(b, 0));
    }
    {   // slot 0's stream is parked (closed) and resumed in slot 2
        const size_t sb = mp3mi_batch_slot_state_bytes(b);
        void *state = mp3mi_host_alloc(sb);
        if (!state) return 1;
        mp3mi_slot_ticket t;
        int32_t slot = 0;
        OK(mp3mi_batch_slots_export(b, 1, &slot, 1, state, sb, &t));
        slot = 2;
        OK(mp3mi_batch_slots_import(b, 1, &slot, state, sb, &t));
        OK(mp3mi_batch_sync(b));
        mp3mi_host_free(state);
    }
    OK(mp3mi_batch_flush(b, out, stride, len));
    OK(mp3mi_batch_sync(b));
    mp3mi_batch_destroy(b);
    mp3mi_host_free(pcm);
    mp3mi_host_free(out);
    mp3mi_host_free(len);
    return 0;
}

static int layer2(void)
{
    mp3mi_l12_batch *b = NULL;
    OK(mp3mi_l12_batch_create(&b, 2, S, RATE, C, NULL, 128, NF, 1));
    const size_t row = (size_t) NF * 1152 * C, stride = mp3mi_l12_batch_out_stride(b, NF);
    std::vector<int16_t> pcm(row * S);
    std::vector<uint8_t> out(stride * S);
    std::vector<uint32_t> len(S);
    for (int s = 0; s < S; s++) mp3mi_synth_pcm(pcm.data() + row * s, NF * 1152, C, RATE, (uint32_t) (100 + s), 0x6D70336Du);
    OK(mp3mi_l12_batch_encode(b, pcm.data(), NULL, NF, out.data(), stride, len.data())); // a whole-file call
    OK(mp3mi_l12_batch_sync(b));
    OK(mp3mi_l12_batch_encode_next(b, pcm.data(), NF, out.data(), stride, len.data())); // streaming
    OK(mp3mi_l12_batch_flush(b, out.data(), stride, len.data()));
    OK(mp3mi_l12_batch_sync(b));
    mp3mi_l12_batch_destroy(b);
    return 0;
}

int main(void)
{
    if (layer3() != 0 || layer2() != 0) return 1;
    printf("lifecycle ok: Layer III and Layer II batches created, driven and destroyed\n");
    return 0;
}
