/* TEST INFRASTRUCTURE -- not part of the product path.
 *
 * A second witness for tests/test_quant_edges.py: the UNMODIFIED reference's own quantize() and count_bits()
 * (src/loop.c:1360-1428, 2099-2113), linked from its objects (oracle/Makefile target `ref`), on granules read from a file.
 * The band tables are selected as iteration_loop selects them (src/loop.c:267-268).
 *
 * usage: ref_harness_qc in.bin out.bin
 *   in.bin : int32 n, then n records of int32 rate_hz, block_type, quantizerStepSize, 0 and double xr[576]
 *   out.bin: n records of int32 ix[576] and int32 bits, big_values, count1, count1table_select, table_select[3],
 *            region0_count, region1_count, address1, address2, address3 (gr_info zeroed before every granule)
 *
 * Only compiled where the reference sources exist; nothing here travels as source of the reference.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "encoder.h"
#include "l3side.h"
#include "loop.h"

/* globals the reference objects expect from its driver (src/musicin.c:148-156) */
FILE *musicin;
Bit_stream_struc bs;
char *programName = "ref_harness_qc";
int iswav = 0;
int littleData = 0;
int streaming_input = 0;
unsigned long frameNum = 0;

extern int *scalefac_band_long, *scalefac_band_short;
void quantize(double xr[576], int ix[576], gr_info *cod_info);
int count_bits();

int main(int argc, char **argv)
{
    FILE *fi, *fo;
    int n, i;
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    fi = fopen(argv[1], "rb");
    fo = fopen(argv[2], "wb");
    if (!fi || !fo || fread(&n, 4, 1, fi) != 1) return 2;
    for (i = 0; i < n; i++) {
        int hdr[4], ix[576], f[12], sf;
        static double xr[576];
        gr_info g;
        if (fread(hdr, 4, 4, fi) != 4 || fread(xr, 8, 576, fi) != 576) return 3;
        sf = hdr[0] == 44100 ? 0 : (hdr[0] == 48000 ? 1 : (hdr[0] == 32000 ? 2 : -1));
        if (sf < 0) return 4;
        scalefac_band_long = &sfBandIndex[sf + 3].l[0]; /* version 1 (MPEG-1) */
        scalefac_band_short = &sfBandIndex[sf + 3].s[0];
        memset(&g, 0, sizeof(g));
        g.block_type = (unsigned) hdr[1];
        g.window_switching_flag = hdr[1] != 0;
        g.quantizerStepSize = (double) hdr[2];
        if (g.window_switching_flag && g.block_type == 2) { g.sfb_lmax = 0; g.sfb_smax = 0; } /* gr_deco, src/loop.c:2063 */
        else { g.sfb_lmax = 21; g.sfb_smax = 12; }
        quantize(xr, ix, &g);
        f[0] = count_bits(ix, &g);
        f[1] = (int) g.big_values; f[2] = (int) g.count1; f[3] = (int) g.count1table_select;
        f[4] = (int) g.table_select[0]; f[5] = (int) g.table_select[1]; f[6] = (int) g.table_select[2];
        f[7] = (int) g.region0_count; f[8] = (int) g.region1_count;
        f[9] = (int) g.address1; f[10] = (int) g.address2; f[11] = (int) g.address3;
        if (fwrite(ix, 4, 576, fo) != 576 || fwrite(f, 4, 12, fo) != 12) return 5;
    }
    fclose(fo);
    fclose(fi);
    return 0;
}
