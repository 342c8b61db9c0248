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
#include "host_util.h"
#include "l12_dev.h"
#include "mp3mi_l12.h"

static const int LA_BITRATES[2][15] = { /* src/common.c:122-123 */
    {0, 32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 416, 448},
    {0, 32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384}};
static const double LA_SAMPLE_MAX = 2.0; // multiple[0]

extern "C" int mp3mi_debug_l12_alloc(int layer, int rate_hz, int channels, int mode, int crc, int hdr_flags, int slot0, int n_streams,
                                     int n_frames, const int32_t *kbps, const double *sb, const float *ratio, uint8_t *out,
                                     size_t out_stride, uint32_t *out_len, void *seams)
{
    static_assert(sizeof(mp3mi_l12_frame_seams) == sizeof(l12_frame_dbg), "seam record of mp3mi_l12.h and l12_dev.h");
    if (!have_device()) return MP3MI_ERR_NO_DEVICE;
    const int ri = rate_hz == 44100 ? 0 : (rate_hz == 48000 ? 1 : (rate_hz == 32000 ? 2 : -1));
    if ((layer != 1 && layer != 2) || ri < 0 || (channels != 1 && channels != 2) || mode < 0 || mode > 3 ||
        (channels == 1) != (mode == MP3MI_MODE_MONO) || (crc & ~1) || (hdr_flags & ~15) || slot0 < 0 || slot0 > 17 || n_streams <= 0 ||
        n_streams > 4096 || n_frames <= 0 || n_frames > 64 || !kbps || !sb || !ratio || !out || !out_len || !seams)
        return MP3MI_ERR_ARG;
    const size_t S = (size_t) n_streams, nf = (size_t) n_frames, C = (size_t) channels;
    const int parts = layer == 1 ? 1 : 3, nslot = 12 * parts, spf = 32 * nslot, lb = layer == 1 ? 3 : 2;
    const size_t n_sb = S * nf * C * (size_t) parts * 12 * 32, n_ratio = S * nf * (size_t) layer * C * 32;
    for (size_t i = 0; i < n_sb; i++)
        if (!(fabs(sb[i]) <= LA_SAMPLE_MAX)) return MP3MI_ERR_ARG; // (also catches NaN and the infinities)
    for (size_t i = 0; i < n_ratio; i++)
        if (!(fabsf(ratio[i]) <= 3.402823466e38f)) return MP3MI_ERR_ARG;
    l12_stream_cfg *cfg_h = (l12_stream_cfg *) calloc(S, sizeof(l12_stream_cfg));
    if (!cfg_h) return MP3MI_ERR_NOMEM;
    int max_frame_bytes = 0;
    for (size_t s = 0; s < S; s++) { // as mp3mi_l12_batch_create sets a stream up
        int bi = 1;
        while (bi < 15 && LA_BITRATES[layer - 1][bi] != kbps[s]) bi++;
        if (bi == 15) { free(cfg_h); return MP3MI_ERR_ARG; }
        l12_stream_cfg &c = cfg_h[s];
        c.bitrate_index = bi;
        c.frame_bits = frame_bits(spf, ri, kbps[s], layer == 1 ? 32 : 8);
        if (layer == 2) { // pick_table, src/common.c:291-318
            const int br_per_ch = kbps[s] / channels, sfrq = rate_hz / 1000;
            if ((sfrq == 48 && br_per_ch >= 56) || (br_per_ch >= 56 && br_per_ch <= 80)) c.table = 0;
            else if (sfrq != 48 && br_per_ch >= 96) c.table = 1;
            else if (sfrq != 32 && br_per_ch <= 48) c.table = 2;
            else c.table = 3;
            static const int SBL[4] = {27, 30, 8, 12};
            c.sblimit = SBL[c.table];
        } else { c.table = 0; c.sblimit = 32; }
        int fb = c.frame_bits / 8;
        if (layer == 1 && channels == 2 && fb < 38) fb = 38; // (the frame that outgrows its slot, k_l12.hip)
        if (fb > max_frame_bytes) max_frame_bytes = fb;
    }
    if (out_stride < nf * (size_t) max_frame_bytes + 1) { free(cfg_h); return MP3MI_ERR_ARG; }

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
    double *sbs_h = (double *) calloc(n_sbs, sizeof(double));
    float *snr_h = (float *) calloc(n_snr, sizeof(float));
    mp3mi_tables_l12 *Th = (mp3mi_tables_l12 *) malloc(sizeof(mp3mi_tables_l12));
    int rc = MP3MI_ERR_NOMEM;
    mp3mi_tables_l12 *dT = NULL;
    l12_stream_cfg *dcfg = NULL;
    double *dsbs = NULL;
    float *dsnr = NULL;
    uint8_t *dout = NULL;
    uint32_t *dlen = NULL;
    l12_frame_dbg *ddbg = NULL;
    if (sbs_h && snr_h && Th) {
        const int trc = mp3mi_build_tables_l12(Th, ri, layer);
        rc = trc == 0 ? MP3MI_OK : (trc == -8 ? MP3MI_ERR_TABLES : MP3MI_ERR_ARG);
        for (size_t s = 0; rc == MP3MI_OK && s < S; s++)
            if (layer == 2 && cfg_h[s].sblimit != Th->sblimit[cfg_h[s].table]) rc = MP3MI_ERR_TABLES;
    }
    if (rc == MP3MI_OK) {
        // k_filter's layout: [stream][granule][channel][slot of 18][subband], odd slots of odd subbands negated (src/mdct.c:57-60)
        for (size_t s = 0; s < S; s++)
            for (size_t f = 0; f < nf; f++)
                for (size_t ch = 0; ch < C; ch++)
                    for (int u = 0; u < nslot; u++) {
                        const size_t sg = (size_t) slot0 + f * (size_t) nslot + (size_t) u, gi = sg / 18, qq = sg % 18;
                        const double *src = sb + ((((s * nf + f) * C + ch) * (size_t) parts + (size_t) (u / 12)) * 12 + (size_t) (u % 12)) * 32;
                        double *dst = sbs_h + ((s * G1 + gi) * C + ch) * 576 + qq * 32;
                        for (int i = 0; i < 32; i++) dst[i] = ((i & 1) && (qq & 1)) ? -src[i] : src[i];
                    }
        // k12_psy's records: [stream][pass][channel][32], the chunk's passes behind the lb recomputed ones
        for (size_t s = 0; s < S; s++)
            for (size_t q = 0; q < nf * (size_t) layer; q++)
                memcpy(snr_h + ((s * (size_t) g.np + (size_t) lb + q) * C) * 32, ratio + ((s * nf * (size_t) layer + q) * C) * 32, C * 32 * sizeof(float));
        rc = MP3MI_ERR_HIP;
        if (hipMalloc((void **) &dT, sizeof(mp3mi_tables_l12)) == hipSuccess && hipMalloc((void **) &dcfg, S * sizeof(l12_stream_cfg)) == hipSuccess &&
            hipMalloc((void **) &dsbs, n_sbs * sizeof(double)) == hipSuccess && hipMalloc((void **) &dsnr, n_snr * sizeof(float)) == hipSuccess &&
            hipMalloc((void **) &dout, S * out_stride) == hipSuccess && hipMalloc((void **) &dlen, S * sizeof(uint32_t)) == hipSuccess &&
            hipMalloc((void **) &ddbg, S * nf * sizeof(l12_frame_dbg)) == hipSuccess &&
            hipMemcpy(dT, Th, sizeof(mp3mi_tables_l12), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dcfg, cfg_h, S * sizeof(l12_stream_cfg), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dsbs, sbs_h, n_sbs * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dsnr, snr_h, n_snr * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemset(dout, 0, S * out_stride) == hipSuccess && hipMemset(dlen, 0, S * sizeof(uint32_t)) == hipSuccess &&
            hipMemset(ddbg, 0, S * nf * sizeof(l12_frame_dbg)) == hipSuccess) {
            mp3mi_launch_l12_alloc(dT, g, dcfg, dsbs, dsnr, dout, out_stride, dlen, ddbg, 0);
            if (hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                hipMemcpy(out, dout, S * out_stride, hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(out_len, dlen, S * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(seams, ddbg, S * nf * sizeof(l12_frame_dbg), hipMemcpyDeviceToHost) == hipSuccess)
                rc = MP3MI_OK;
        }
    }
    if (dT) hipFree(dT);
    if (dcfg) hipFree(dcfg);
    if (dsbs) hipFree(dsbs);
    if (dsnr) hipFree(dsnr);
    if (dout) hipFree(dout);
    if (dlen) hipFree(dlen);
    if (ddbg) hipFree(ddbg);
    free(Th);
    free(snr_h);
    free(sbs_h);
    free(cfg_h);
    return rc;
}
