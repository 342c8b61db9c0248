/* Layers I and II, host side: what a stream's bitrate means for the kernels (l12_stream_cfg, l12_dev.h) and for its output row --
 * set up here for the batch (l12_batch.cpp) and for the self-test hook that runs k12_alloc as the batch does (l12_alloc_debug.cpp).
 * Private to the library. */
#ifndef MP3MI_L12_HOST_H
#define MP3MI_L12_HOST_H

#include "host_util.h"
#include "l12_dev.h"

static inline int l12_samples_per_frame(int layer) { return layer == 1 ? 384 : 1152; }

// A stream of `layer` at kbps (rate_idx: rate_idx_of(rate_hz)): the header's bitrate index, the frame's size with slots never padded
// and, in Layer II, the allocation table with its subband limit.  False for a bitrate the layer does not have (src/common.c:122-123).
static inline bool l12_stream_cfg_of(int layer, int rate_hz, int rate_idx, int channels, int kbps, l12_stream_cfg *c)
{
    c->bitrate_index = bitrate_index_of(layer, kbps);
    if (!c->bitrate_index) return false;
    c->frame_bits = frame_bits(l12_samples_per_frame(layer), rate_idx, kbps, layer == 1 ? 32 : 8);
    c->table = 0;
    c->sblimit = 32;
    if (layer == 2) { // pick_table, src/common.c:291-318
        const int br_per_ch = kbps / channels, sfrq = rate_hz / 1000; // (int) s_freq: 44, 48, 32
        if ((sfrq == 48 && br_per_ch >= 56) || (br_per_ch >= 56 && br_per_ch <= 80)) c->table = 0;
        else if (sfrq != 48 && br_per_ch >= 96) c->table = 1;
        else if (sfrq != 32 && br_per_ch <= 48) c->table = 2;
        else c->table = 3;
        static const int SBL[4] = {27, 30, 8, 12};
        c->sblimit = SBL[c->table];
    }
    return true;
}

// Bytes a frame of frame_bits takes in an output row: two-channel Layer I below its fields' size has frames that outgrow their
// slots, as the reference's do (k_l12.hip)
static inline size_t l12_row_frame_bytes(int layer, int channels, int frame_bits)
{
    const size_t fb = (size_t) (frame_bits / 8);
    return (layer == 1 && channels == 2 && fb < 38) ? 38 : fb;
}

#endif
