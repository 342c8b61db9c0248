// The self-test hook mp3mi_debug_l12_alloc (include/mp3mi_l12.h): frames of GIVEN subband samples and signal-to-mask ratios through
// k12_alloc as the Layer I / II batch launches it (l12_batch.cpp): the samples repacked into k_filter's layout -- 18-slot granules,
// odd slots of odd subbands negated --, the ratios into k12_psy's records behind the lb warm-up passes, l12_geom and l12_stream_cfg
// built as the batch builds them, one launch for S streams x nf frames.  Host code only: k_l12.hip is untouched, the kernel is the
// one the encoder runs.
//
// What k12_alloc takes on trust from the stages before it is checked here first (input that breaks one of the rules is refused,
// nothing is launched):
//
//   every sample finite and |x| <= 2.0 = multiple[0].
//     The filterbank's output of 16-bit PCM scaled by 1 / 32768 stays below 2 (the window's absolute sum is below 2.1, the matrix's
//     rows are cosines; the reference's own table of scale factors starts there, src/common.c:127-150).  Above it the scale index is
//     0 and the quotient d = x / multiple[0] passes 1: d * a + b reaches 1.0, (unsigned) (d * 2^n) has bit n set on its own, and the
//     sign bit is ORed into a value that already has it -- the codeword no longer says what the sample was, and a grouped one passes
//     its field.  A NaN fails every comparison of the peak search and of l12_scale_index in its own way in each implementation.
//
//   every ratio finite.
//     The allocation orders the bands by a 64-bit key taken from the bits of mnr = snr[k] - ratio (l12_key): the order of the keys
//     is the order of the doubles only where there is no NaN, and a NaN fails `small > mnr` for ever in the reference where its key
//     here is just another number.  An infinite ratio makes every mnr of its band the same infinity, whatever the band was granted:
//     the rounds rest on a band's ratio RISING with its steps (k_l12.hip), so the hook keeps to the numbers that argument was made
//     for.  (-0.0 is harmless: 0.0 - (-0.0) = +0.0, and every other snr[k] is non-zero: no key is ever taken from a negative zero.)
//
//   a legal format: layer 1 or 2; 44100, 48000 or 32000 Hz; one channel with mode 3 (mono) or two with mode 0..2; a bitrate of the
//     layer's table per stream (src/common.c:122-123); crc 0 / 1; header flags 0..15; slot0 in 0..17 (the phase of the first
//     frame's first slot in its granule: the batch's chunks start at 16, 10 or 4 in Layer I and at 0 in Layer II); at most 4096
//     streams of at most 64 frames; out_stride >= n_frames * (bytes of the longest frame) + 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "l12_host.h"
#include "mp3mi_l12.h"

static const double LA_SAMPLE_MAX = 2.0; // multiple[0]

extern "C" int mp3mi_debug_l12_alloc(int layer, int rate_hz, int channels, int mode, int crc, int hdr_flags, int slot0, int n_streams,
                                     int n_frames, const int32_t *kbps, const double *sb, const float *ratio, uint8_t *out,
                                     size_t out_stride, uint32_t *out_len, void *seams)
{
    static_assert(sizeof(mp3mi_l12_frame_seams) == sizeof(l12_frame_dbg), "seam record of mp3mi_l12.h and l12_dev.h");
    if (!have_device()) return MP3MI_ERR_NO_DEVICE;
    const int ri = rate_idx_of(rate_hz);
    if ((layer != 1 && layer != 2) || ri < 0 || (channels != 1 && channels != 2) || mode < 0 || mode > 3 ||
        (channels == 1) != (mode == MP3MI_MODE_MONO) || (crc & ~1) || (hdr_flags & ~15) || slot0 < 0 || slot0 > 17 || n_streams <= 0 ||
        n_streams > 4096 || n_frames <= 0 || n_frames > 64 || !kbps || !sb || !ratio || !out || !out_len || !seams)
        return MP3MI_ERR_ARG;
    const size_t S = (size_t) n_streams, nf = (size_t) n_frames, C = (size_t) channels;
    const int parts = layer == 1 ? 1 : 3, nslot = 12 * parts, spf = l12_samples_per_frame(layer), lb = layer == 1 ? 3 : 2;
    const size_t n_sb = S * nf * C * (size_t) parts * 12 * 32, n_ratio = S * nf * (size_t) layer * C * 32;
    for (size_t i = 0; i < n_sb; i++)
        if (!(fabs(sb[i]) <= LA_SAMPLE_MAX)) return MP3MI_ERR_ARG; // (also catches NaN and the infinities)
    for (size_t i = 0; i < n_ratio; i++)
        if (!(fabsf(ratio[i]) <= 3.402823466e38f)) return MP3MI_ERR_ARG;
    host_mem<l12_stream_cfg> cfg_h(S);
    if (!cfg_h.p) return MP3MI_ERR_NOMEM;
    size_t max_frame_bytes = 0;
    for (size_t s = 0; s < S; s++) { // as mp3mi_l12_batch_create sets a stream up: the same two functions
        if (!l12_stream_cfg_of(layer, rate_hz, ri, channels, kbps[s], &cfg_h.p[s])) return MP3MI_ERR_ARG;
        const size_t fb = l12_row_frame_bytes(layer, channels, cfg_h.p[s].frame_bits);
        if (fb > max_frame_bytes) max_frame_bytes = fb;
    }
    if (out_stride < nf * max_frame_bytes + 1) return MP3MI_ERR_ARG;

    l12_geom g;
    memset(&g, 0, sizeof(g));
    g.n_streams = n_streams; g.channels = channels; g.layer = layer; g.rate_idx = ri;
    g.n_frames = n_frames; g.f0 = 0; g.nf = n_frames;
    g.lb = lb; g.np = n_frames * layer + lb;
    g.spf = spf; g.spp = layer == 1 ? 384 : 576; g.span = layer == 1 ? 1024 : 1056;
    const size_t G1 = ((size_t) slot0 + nf * (size_t) nslot + 17) / 18; // granules that hold the frames' slots
    g.g0 = 1; g.n_gran = (int) G1 - 1; g.slot0 = slot0;
    g.actual_mode = mode; g.crc = crc; g.hdr_flags = hdr_flags;
    g.whole_file = 1; // (the last frame's wavefront adds the file's last byte)

    const size_t n_sbs = S * G1 * C * 576, n_snr = S * (size_t) g.np * C * 32;
    host_mem<double> sbs_h(n_sbs);
    host_mem<float> snr_h(n_snr);
    host_mem<mp3mi_tables_l12> Th(1);
    if (!sbs_h.p || !snr_h.p || !Th.p) return MP3MI_ERR_NOMEM;
    int rc = tables_rc(mp3mi_build_tables_l12(Th.p, ri, layer));
    for (size_t s = 0; rc == MP3MI_OK && s < S; s++)
        if (layer == 2 && cfg_h.p[s].sblimit != Th.p->sblimit[cfg_h.p[s].table]) rc = MP3MI_ERR_TABLES;
    if (rc != MP3MI_OK) return rc;
    // k_filter's layout: [stream][granule][channel][slot of 18][subband], odd slots of odd subbands negated (src/mdct.c:57-60)
    for (size_t s = 0; s < S; s++)
        for (size_t f = 0; f < nf; f++)
            for (size_t ch = 0; ch < C; ch++)
                for (int u = 0; u < nslot; u++) {
                    const size_t sg = (size_t) slot0 + f * (size_t) nslot + (size_t) u, gi = sg / 18, qq = sg % 18;
                    const double *src = sb + ((((s * nf + f) * C + ch) * (size_t) parts + (size_t) (u / 12)) * 12 + (size_t) (u % 12)) * 32;
                    double *dst = sbs_h.p + ((s * G1 + gi) * C + ch) * 576 + qq * 32;
                    for (int i = 0; i < 32; i++) dst[i] = ((i & 1) && (qq & 1)) ? -src[i] : src[i];
                }
    // k12_psy's records: [stream][pass][channel][32], the chunk's passes behind the lb recomputed ones
    for (size_t s = 0; s < S; s++)
        for (size_t q = 0; q < nf * (size_t) layer; q++)
            memcpy(snr_h.p + ((s * (size_t) g.np + (size_t) lb + q) * C) * 32, ratio + ((s * nf * (size_t) layer + q) * C) * 32, C * 32 * sizeof(float));
    hook_bufs D;
    const mp3mi_tables_l12 *dT = D.copy_of(Th.p, 1);
    const l12_stream_cfg *dcfg = D.copy_of(cfg_h.p, S);
    const double *dsbs = D.copy_of(sbs_h.p, n_sbs);
    const float *dsnr = D.copy_of(snr_h.p, n_snr);
    uint8_t *dout = D.zeros<uint8_t>(S * out_stride);
    uint32_t *dlen = D.zeros<uint32_t>(S);
    l12_frame_dbg *ddbg = D.zeros<l12_frame_dbg>(S * nf);
    if (!D.ok) return D.rc();
    mp3mi_launch_l12_alloc(dT, g, dcfg, dsbs, dsnr, dout, out_stride, dlen, ddbg, 0);
    D.ok = hipGetLastError() == hipSuccess;
    D.sync();
    D.fetch(out, dout, S * out_stride);
    D.fetch(out_len, dlen, S);
    D.fetch((l12_frame_dbg *) seams, ddbg, S * nf);
    return D.rc();
}
