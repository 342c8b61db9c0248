/* TEST INFRASTRUCTURE -- not part of the product path.
 *
 * A second witness for tests/test_loop_edges.py: the UNMODIFIED reference's own iteration_loop (src/loop.c:232-362, with
 * src/reservoir.c below it), linked from its objects (oracle/Makefile target `ref`), on one chain of frames of GIVEN records read
 * from a file -- spectrum, perceptual entropy, masking ratios, block types -- as the frame loop hands them over (src/musicin.c:
 * 708-788).  The reference keeps its reservoir and calc_scfsi's memory in statics: a process per chain, and a chain starts fresh.
 * main_data_begin is what III_format_bitstream would have left for the next call: the reservoir's size in bytes, which this file
 * keeps track of from what each call returns (src/reservoir.c:141-145, 155-226).  Where an assertion of the reference's fails the
 * process dies with the assertion's words; what was written for the frames before stands (a flush per frame).
 *
 * usage: ref_harness_loop chain.bin out.bin
 *   chain.bin: int32 rate_hz, channels, kbps, crc, n_frames, 0, 0, 0; double xr[2 * n_frames][channels][576]; then
 *              [2 * n_frames][channels] mp3mi_psy_out records (csrc/mp3mi_dev.h: double pe, ratio_l[21], ratio_s[12][3], int32
 *              block_type, pad)
 *   out.bin  : per frame an mp3mi_frame_side record (226 int32) and int16 ix[2][channels][576], signed; then int32 ResvSize and
 *              address1..3 of [gr][ch] (12 int32, zeros for a channel that is not there)
 * Only compiled where the reference sources exist (its headers give the prototypes); nothing of the reference travels as source.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "encoder.h"
#include "l3side.h"
#include "loop.h"

/* globals the reference objects expect from their driver (src/musicin.c:148-156) */
FILE *musicin;
Bit_stream_struc bs;
char *programName = "ref_harness_loop";
int iswav = 0;
int littleData = 0;
int streaming_input = 0;
unsigned long frameNum = 0;

enum { GR_WORDS = 15 + 39, FRAME_WORDS = 10 + 4 * GR_WORDS, PSY_BYTES = 8 * (1 + 21 + 36) + 8 };

int main(int argc, char **argv)
{
    static double xr[2][2][576], xr_dec[2][2][576], pe[2][2];
    static int l3_enc[2][2][576];
    static III_psy_ratio ratio;
    static III_side_info_t l3_side;
    static III_scalefac_t scalefac;
    static frame_params fr_ps;
    static layer info;
    static const double s_freq[3] = {44.1, 48, 32};
    int hdr[8], n, C, ri, f, gr, ch, i, w, bitsPerFrame, mean_bits, resv = 0, tail[13];
    double *xr_in;
    unsigned char *psy;
    FILE *fi, *fo;
    if (argc != 3) { fprintf(stderr, "usage: %s chain.bin out.bin\n", argv[0]); return 2; }
    fi = fopen(argv[1], "rb");
    if (!fi || fread(hdr, 4, 8, fi) != 8) return 2;
    C = hdr[1];
    n = hdr[4];
    ri = hdr[0] == 44100 ? 0 : (hdr[0] == 48000 ? 1 : (hdr[0] == 32000 ? 2 : -1));
    if (n < 1 || ri < 0 || (C != 1 && C != 2)) return 2;
    xr_in = (double *) malloc((size_t) n * 2 * C * 576 * 8);
    psy = (unsigned char *) malloc((size_t) n * 2 * C * PSY_BYTES);
    if (!xr_in || !psy || fread(xr_in, 8, (size_t) n * 2 * C * 576, fi) != (size_t) n * 2 * C * 576 ||
        fread(psy, PSY_BYTES, (size_t) n * 2 * C, fi) != (size_t) n * 2 * C)
        return 3;
    fclose(fi);
    fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    memset(&info, 0, sizeof(info));
    info.version = 1; /* MPEG-1 */
    info.lay = 3;
    info.error_protection = hdr[3];
    for (i = 1; i < 15; i++)
        if (bitrate[info.version][info.lay - 1][i] == hdr[2]) info.bitrate_index = i;
    if (!info.bitrate_index) return 2;
    info.sampling_frequency = ri;
    info.mode = C == 1 ? MPG_MD_MONO : MPG_MD_STEREO;
    fr_ps.header = &info;
    fr_ps.tab_num = -1;
    fr_ps.alloc = NULL;
    hdr_to_frps(&fr_ps);
    bitsPerFrame = 8 * (int) (((double) 1152 / s_freq[ri]) * ((double) hdr[2] / 8.0));     /* src/musicin.c:561-567 */
    mean_bits = (bitsPerFrame - (32 + (C == 1 ? 136 : 256) + (hdr[3] ? 16 : 0))) / 2;       /* src/musicin.c:728-746 */
    for (f = 0; f < n; f++) {
        int out[FRAME_WORDS];
        static short ixs[2][2][576];
        frameNum++;
        for (gr = 0; gr < 2; gr++)
            for (ch = 0; ch < C; ch++) {
                const size_t rec = (size_t) (2 * f + gr) * C + ch;
                const unsigned char *r = psy + rec * PSY_BYTES;
                int bt;
                gr_info *g = &l3_side.gr[gr].ch[ch].tt;
                memcpy(xr[gr][ch], xr_in + rec * 576, sizeof(xr[0][0]));
                memcpy(&pe[gr][ch], r, 8);
                memcpy(ratio.l[gr][ch], r + 8, sizeof(ratio.l[0][0]));
                memcpy(ratio.s[gr][ch], r + 8 * 22, sizeof(ratio.s[0][0]));
                memcpy(&bt, r + 8 * 58, 4);
                g->block_type = (unsigned) bt;
                g->window_switching_flag = bt != 0;
                g->mixed_block_flag = 0;
            }
        l3_side.main_data_begin = resv / 8;
        iteration_loop(pe, xr, &ratio, &l3_side, l3_enc, mean_bits, C, xr_dec, &scalefac, &fr_ps, 0, bitsPerFrame);
        memset(out, 0, sizeof(out));
        out[0] = l3_side.main_data_begin;
        out[1] = l3_side.resvDrain;
        for (ch = 0; ch < C; ch++)
            for (i = 0; i < 4; i++) out[2 + 4 * ch + i] = (int) l3_side.scfsi[ch][i];
        /* the reservoir after the frame: every granule's mean_bits / stereo came in, the granules' bits and the drain went out,
           and an odd mean_bits gives a stereo frame one bit more (src/reservoir.c:141-145, 165-167) */
        resv += (C == 2 && (mean_bits & 1)) - l3_side.resvDrain;
        for (gr = 0; gr < 2; gr++)
            for (ch = 0; ch < C; ch++) {
                const gr_info *g = &l3_side.gr[gr].ch[ch].tt;
                int *q = out + 10 + (2 * gr + ch) * GR_WORDS;
                resv += mean_bits / C - (int) g->part2_3_length;
                q[0] = (int) g->part2_3_length; q[1] = (int) g->big_values; q[2] = (int) g->count1; q[3] = (int) g->global_gain;
                q[4] = (int) g->scalefac_compress; q[5] = (int) g->window_switching_flag; q[6] = (int) g->block_type;
                q[7] = (int) g->table_select[0]; q[8] = (int) g->table_select[1]; q[9] = (int) g->table_select[2];
                q[10] = (int) g->region0_count; q[11] = (int) g->region1_count; q[12] = (int) g->preflag;
                q[13] = (int) g->count1table_select; q[14] = (int) g->part2_length;
                if (g->window_switching_flag && g->block_type == 2) {
                    for (i = 0; i < 12; i++)
                        for (w = 0; w < 3; w++) q[15 + 3 * i + w] = scalefac.s[gr][ch][i][w];
                } else
                    for (i = 0; i < 21; i++) q[15 + i] = scalefac.l[gr][ch][i];
                for (i = 0; i < 576; i++) { /* the sign the formatter gives a value (src/l3bitstream.c:115-125) */
                    const int m = l3_enc[gr][ch][i];
                    ixs[gr][ch][i] = (short) ((xr[gr][ch][i] < 0 && m > 0) ? -m : m);
                }
            }
        fwrite(out, 4, FRAME_WORDS, fo);
        for (gr = 0; gr < 2; gr++)
            for (ch = 0; ch < C; ch++) fwrite(ixs[gr][ch], 2, 576, fo);
        fflush(fo);
    }
    memset(tail, 0, sizeof(tail));
    tail[0] = resv;
    for (gr = 0; gr < 2; gr++)
        for (ch = 0; ch < C; ch++) {
            const gr_info *g = &l3_side.gr[gr].ch[ch].tt;
            tail[1 + 3 * (2 * gr + ch)] = (int) g->address1;
            tail[2 + 3 * (2 * gr + ch)] = (int) g->address2;
            tail[3 + 3 * (2 * gr + ch)] = (int) g->address3;
        }
    fwrite(tail, 4, 13, fo);
    fclose(fo);
    return 0;
}
