/* TEST INFRASTRUCTURE -- not part of the product path.
 *
 * Formats chains of GIVEN frames (tests/format_edges.py): III_format_bitstream once per frame with the chain's quantised
 * values, side information and scalefactors, then III_FlushBitstream and the close.  Magnitudes go in through l3_enc, signs
 * through xr, as the frame loop hands them over (src/l3bitstream.c:115-125); the fields the loop would have set besides the
 * transmitted ones -- address1..3 (src/loop.c:1679-1700), sfb_lmax / sfb_smax (src/loop.c:2063-2081) -- are set here, and
 * main_data_begin is the one the call before left behind (src/l3bitstream.c:161).  Linked three ways (oracle/Makefile): against
 * the UNMODIFIED reference objects (_ref/fmt_probe_ref), over the library's drop-in symbols (_ref/fmt_probe) and over the
 * emulated test build (_ref/fmt_probe_emu); the files and the back pointers must be equal.
 *
 * usage: fmt_probe chain.bin out.mp3 mdb.bin
 *   chain.bin: int32 rate_hz, channels, kbps, mode, mode_ext, crc, copyright, original, emphasis, n_frames (>= 1), 0, 0;
 *              n_frames mp3mi_frame_side records (csrc/mp3mi_dev.h: 226 int32); int16 ix[2 * n_frames][channels][576], signed
 *   mdb.bin  : int32 main_data_begin after every call
 * usage: fmt_probe --dump-tables tables.bin      (reference link only)
 *   per Huffman table 0..33: int32 xlen, ylen, linbits, linmax, cells; then per cell uint32 code, int32 length
 * Only compiled where the reference sources exist (its headers give the prototypes); nothing of the reference travels as source.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "encoder.h"
#include "l3side.h"
#include "l3bitstream.h"
#include "huffman.h"

/* globals the reference objects expect from their driver (src/musicin.c:148-156) */
FILE *musicin;
Bit_stream_struc bs;
char *programName = "fmt_probe";
int iswav = 0;
int littleData = 0;
int streaming_input = 0;
unsigned long frameNum = 0;

extern void III_FlushBitstream(void);
extern struct huffcodetab ht[HTN] __attribute__((weak));

/* long-block scalefactor band edges, ISO 11172-3 table B.8 (44.1 / 48 / 32 kHz) */
static const int SFB_L[3][23] = {
    {0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 90, 110, 134, 162, 196, 238, 288, 342, 418, 576},
    {0, 4, 8, 12, 16, 20, 24, 30, 36, 42, 50, 60, 72, 88, 106, 128, 156, 190, 230, 276, 330, 384, 576},
    {0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 54, 66, 82, 102, 126, 156, 194, 240, 296, 364, 448, 550, 576}};

enum { GR_WORDS = 15 + 39, FRAME_WORDS = 10 + 4 * GR_WORDS };

static int dump_tables(const char *path)
{
    FILE *fo = fopen(path, "wb");
    int t, i;
    if (!fo || !ht) return 2;
    for (t = 0; t < HTN; t++) {
        int h[5];
        h[0] = (int) ht[t].xlen; h[1] = (int) ht[t].ylen; h[2] = (int) ht[t].linbits; h[3] = (int) ht[t].linmax;
        h[4] = ht[t].table ? h[0] * h[1] : 0;
        fwrite(h, 4, 5, fo);
        for (i = 0; i < h[4]; i++) {
            unsigned code = (unsigned) ht[t].table[i];
            int len = ht[t].hlen[i];
            fwrite(&code, 4, 1, fo);
            fwrite(&len, 4, 1, fo);
        }
    }
    return fclose(fo) ? 2 : 0;
}

int main(int argc, char **argv)
{
    static double xr[2][2][576];
    static int l3_enc[2][2][576];
    static III_side_info_t l3_side;
    static III_scalefac_t scalefac;
    static frame_params fr_ps;
    static layer info;
    static unsigned no_partition_table[4] = {0, 0, 0, 0};
    static const double s_freq[3] = {44.1, 48, 32};
    int hdr[12], *side, n, C, ri, f, gr, ch, i, w, bitsPerFrame;
    short *ix;
    FILE *fi, *fm;
    if (argc == 3 && !strcmp(argv[1], "--dump-tables")) return dump_tables(argv[2]);
    if (argc != 4) { fprintf(stderr, "usage: %s chain.bin out.mp3 mdb.bin | --dump-tables tables.bin\n", argv[0]); return 2; }
    fi = fopen(argv[1], "rb");
    if (!fi || fread(hdr, 4, 12, fi) != 12) return 2;
    n = hdr[9];
    C = hdr[1];
    ri = hdr[0] == 44100 ? 0 : (hdr[0] == 48000 ? 1 : (hdr[0] == 32000 ? 2 : -1));
    if (n < 1 || ri < 0 || (C != 1 && C != 2) || (C == 1) != (hdr[3] == MPG_MD_MONO)) return 2;
    side = (int *) malloc((size_t) n * FRAME_WORDS * 4);
    ix = (short *) malloc((size_t) n * 2 * C * 576 * 2);
    if (!side || !ix || fread(side, 4, (size_t) n * FRAME_WORDS, fi) != (size_t) n * FRAME_WORDS ||
        fread(ix, 2, (size_t) n * 2 * C * 576, fi) != (size_t) n * 2 * C * 576)
        return 3;
    fclose(fi);
    fm = fopen(argv[3], "wb");
    if (!fm) return 2;
    memset(&info, 0, sizeof(info));
    info.version = 1; /* MPEG-1 */
    info.lay = 3;
    info.error_protection = hdr[5];
    for (i = 1; i < 15; i++)
        if (bitrate[info.version][info.lay - 1][i] == hdr[2]) info.bitrate_index = i;
    if (!info.bitrate_index) return 2;
    info.sampling_frequency = ri;
    info.padding = 0;
    info.mode = hdr[3];
    info.mode_ext = hdr[4];
    info.copyright = hdr[6];
    info.original = hdr[7];
    info.emphasis = hdr[8];
    fr_ps.header = &info;
    fr_ps.tab_num = -1;
    fr_ps.alloc = NULL;
    hdr_to_frps(&fr_ps);
    bitsPerFrame = 8 * (int) (((double) 1152 / s_freq[ri]) * ((double) hdr[2] / 8.0)); /* src/musicin.c:561-567 */
    open_bit_stream_w(&bs, argv[2], BUFFER_SIZE);
    l3_side.main_data_begin = 0;
    for (f = 0; f < n; f++) {
        const int *fs = side + (size_t) f * FRAME_WORDS;
        frameNum++;
        l3_side.private_bits = 0;
        l3_side.resvDrain = fs[1];
        for (ch = 0; ch < 2; ch++)
            for (i = 0; i < 4; i++) l3_side.scfsi[ch][i] = (unsigned) fs[2 + 4 * ch + i];
        for (gr = 0; gr < 2; gr++)
            for (ch = 0; ch < C; ch++) {
                const int *q = fs + 10 + (2 * gr + ch) * GR_WORDS;
                const short *v = ix + ((size_t) (2 * f + gr) * C + ch) * 576;
                gr_info *g = &l3_side.gr[gr].ch[ch].tt;
                int shortb;
                memset(g, 0, sizeof(*g));
                g->part2_3_length = (unsigned) q[0]; g->big_values = (unsigned) q[1]; g->count1 = (unsigned) q[2];
                g->global_gain = (unsigned) q[3]; g->scalefac_compress = (unsigned) q[4]; g->window_switching_flag = (unsigned) q[5];
                g->block_type = (unsigned) q[6];
                g->table_select[0] = (unsigned) q[7]; g->table_select[1] = (unsigned) q[8]; g->table_select[2] = (unsigned) q[9];
                g->region0_count = (unsigned) q[10]; g->region1_count = (unsigned) q[11]; g->preflag = (unsigned) q[12];
                g->count1table_select = (unsigned) q[13]; g->part2_length = (unsigned) q[14];
                g->quantizerStepSize = (double) q[3] - 210.0;
                g->sfb_partition_table = no_partition_table;
                shortb = g->window_switching_flag && g->block_type == 2;
                g->sfb_lmax = shortb ? 0 : 21;
                g->sfb_smax = shortb ? 0 : 12;
                if (!g->window_switching_flag) {
                    g->address1 = (unsigned) SFB_L[ri][q[10] + 1];
                    g->address2 = (unsigned) SFB_L[ri][q[10] + q[11] + 2];
                    g->address3 = 2 * g->big_values;
                } else {
                    g->address1 = shortb ? 36 : (unsigned) SFB_L[ri][q[10] + 1];
                    g->address2 = 2 * g->big_values;
                    g->address3 = 0;
                }
                memset(scalefac.l[gr][ch], 0, sizeof(scalefac.l[gr][ch]));
                memset(scalefac.s[gr][ch], 0, sizeof(scalefac.s[gr][ch]));
                if (shortb) {
                    for (i = 0; i < 12; i++)
                        for (w = 0; w < 3; w++) scalefac.s[gr][ch][i][w] = q[15 + 3 * i + w];
                } else
                    for (i = 0; i < 21; i++) scalefac.l[gr][ch][i] = q[15 + i];
                for (i = 0; i < 576; i++) {
                    l3_enc[gr][ch][i] = v[i] < 0 ? -v[i] : v[i];
                    xr[gr][ch][i] = v[i] < 0 ? -1.0 : 1.0;
                }
            }
        III_format_bitstream(bitsPerFrame, &fr_ps, l3_enc, &l3_side, &scalefac, &bs, xr, NULL, 0);
        fwrite(&l3_side.main_data_begin, 4, 1, fm);
        fflush(fm);
    }
    III_FlushBitstream();
    close_bit_stream_w(&bs);
    fclose(fm);
    return 0;
}
