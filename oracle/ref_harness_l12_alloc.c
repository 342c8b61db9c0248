/* TEST INFRASTRUCTURE -- not part of the product path.
 *
 * A second witness for tests/test_l12_alloc_edges.py: the UNMODIFIED reference's Layer I / II frame encoder behind the filterbank
 * and the model -- *_scale_factor_calc, *_combine_LR, II_transmission_pattern, *_main_bit_allocation, *_CRC_calc, encode_info,
 * encode_CRC, *_encode_bit_alloc, *_encode_scale, *_subband_quantization, *_sample_encoding and the padding bits, in the order of
 * src/musicin.c:627-658, 667-704 -- linked from its objects (oracle/Makefile target `ref`), on frames of GIVEN subband samples and
 * signal-to-mask ratios read from a file.  Every case is a first frame: nothing here carries state from frame to frame but what
 * the reference latches in statics at its first call -- `berr` and `init` of the *_a_bit_allocation functions (the error
 * protection's 16 bits), Layer I's rearranged snr[] and quantiser tables -- so a process takes ONE (layer, error protection), and
 * any bitrates.
 *
 * usage: ref_harness_l12_alloc cases.bin out.mpg out.bin
 *   cases.bin: int32 layer, rate_hz, channels, mode (0 stereo, 1 joint, 2 dual, 3 mono), flags (bit 0 -e, bit 1 -c, bit 2 -o),
 *              n_cases, 0, 0; then per case int32 kbps, 0; double sb[channels][parts][12][32] (parts 1 / 3); float
 *              ratio[passes][channels][32] (passes 1 / 2: Layer II keeps the larger of its two, src/psy.c:391-395)
 *   out.mpg  : the frames one behind the other (and the byte close_bit_stream_w adds)
 *   out.bin  : per case int32 bits written, 0; a stage_dump_l12_t
 * Only compiled where the reference sources exist (its headers give the prototypes); nothing of the reference travels as source.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "encoder.h"
#include "stage_dump_l12.h"

/* globals the reference objects expect from their driver (src/musicin.c:148-156) */
FILE *musicin;
Bit_stream_struc bs;
char *programName = "ref_harness_l12_alloc";
int iswav = 0;
int littleData = 0;
int streaming_input = 0;
unsigned long frameNum = 0;

int main(int argc, char **argv)
{
    typedef double SBS[2][3][SCALE_BLOCK][SBLIMIT];
    typedef double JSBS[3][SCALE_BLOCK][SBLIMIT];
    typedef unsigned int SUB[2][3][SCALE_BLOCK][SBLIMIT];
    static unsigned int bit_alloc[2][SBLIMIT], scfsi[2][SBLIMIT], scalar[2][3][SBLIMIT], j_scale[3][SBLIMIT];
    static double ltmin[2][SBLIMIT], max_sc[2][SBLIMIT];
    static stage_dump_l12_t d;
    static unsigned int crc;
    static float ratio[2][2][SBLIMIT];
    SBS *sb_sample;
    JSBS *j_sample;
    SUB *subband;
    frame_params fr_ps;
    layer info;
    FILE *fi, *fo;
    int hdr[8], head[2], lay, C, mode, flags, n, parts, passes, c, i, j, k, t, adb, whole_SpF, bitsPerSlot, samplesPerFrame, vers;
    unsigned long before;

    if (argc != 4) { fprintf(stderr, "usage: %s cases.bin out.mpg out.bin\n", argv[0]); return 2; }
    fi = fopen(argv[1], "rb");
    if (!fi || fread(hdr, 4, 8, fi) != 8) return 2;
    lay = hdr[0]; C = hdr[2]; mode = hdr[3]; flags = hdr[4]; n = hdr[5];
    if ((lay != 1 && lay != 2) || (C != 1 && C != 2) || mode < 0 || mode > 3 || (C == 1) != (mode == 3) || n < 0) return 2;
    parts = lay == 1 ? 1 : 3;
    passes = lay;
    sb_sample = (SBS *) mem_alloc(sizeof(SBS), "sb_sample");
    j_sample = (JSBS *) mem_alloc(sizeof(JSBS), "j_sample");
    subband = (SUB *) mem_alloc(sizeof(SUB), "subband");
    memset(&info, 0, sizeof(info));
    fr_ps.header = &info;
    fr_ps.tab_num = -1;
    fr_ps.alloc = NULL;
    info.lay = lay;
    info.error_protection = flags & 1;
    info.copyright = (flags >> 1) & 1;
    info.original = (flags >> 2) & 1;
    info.sampling_frequency = SmpFrqIndex((long) hdr[1], &info.version);
    if (info.sampling_frequency < 0 || info.version != 1) return 2;
    vers = info.version;
    if (lay == 1) { bitsPerSlot = 32; samplesPerFrame = 384; }
    else { bitsPerSlot = 8; samplesPerFrame = 1152; }
    open_bit_stream_w(&bs, argv[2], BUFFER_SIZE);
    fo = fopen(argv[3], "wb");
    if (!fo) return 2;

    for (c = 0; c < n; c++) {
        if (fread(head, 4, 2, fi) != 2) return 3;
        memset(*sb_sample, 0, sizeof(SBS));
        for (k = 0; k < C; k++)
            for (t = 0; t < parts; t++)
                if (fread((*sb_sample)[k][t], sizeof(double), SCALE_BLOCK * SBLIMIT, fi) != SCALE_BLOCK * SBLIMIT) return 3;
        for (t = 0; t < passes; t++)
            for (k = 0; k < C; k++)
                if (fread(ratio[t][k], sizeof(float), SBLIMIT, fi) != SBLIMIT) return 3;
        info.version = vers;
        info.bitrate_index = BitrateIndex(lay, head[0], info.version);
        if (info.bitrate_index < 0) return 2;
        info.mode = mode == 3 ? MPG_MD_MONO : mode == 2 ? MPG_MD_DUAL_CHANNEL : mode == 1 ? MPG_MD_JOINT_STEREO : MPG_MD_STEREO;
        info.mode_ext = 0;
        info.padding = 0; /* src/musicin.c:566-581: the fraction is dropped before it is looked at */
        hdr_to_frps(&fr_ps);
        whole_SpF = (int) (((double) samplesPerFrame / s_freq[info.version][info.sampling_frequency]) *
                           ((double) bitrate[info.version][lay - 1][info.bitrate_index] / (double) bitsPerSlot));
        adb = whole_SpF * bitsPerSlot;
        memset(ltmin, 0, sizeof(ltmin));
        for (k = 0; k < C; k++)
            for (i = 0; i < SBLIMIT; i++) {
                float v = ratio[0][k][i];
                if (lay == 2) v = (ratio[0][k][i] > ratio[1][k][i]) ? ratio[0][k][i] : ratio[1][k][i];
                ltmin[k][i] = (double) v;
            }
        memset(scalar, 0, sizeof(scalar)); memset(j_scale, 0, sizeof(j_scale)); memset(scfsi, 0, sizeof(scfsi));
        memset(bit_alloc, 0, sizeof(bit_alloc));
        crc = 0;
        before = sstell(&bs);
        frameNum++;
        if (lay == 1) { /* src/musicin.c:627-658 */
            I_scale_factor_calc(*sb_sample, scalar, C);
            if (fr_ps.actual_mode == MPG_MD_JOINT_STEREO) {
                I_combine_LR(*sb_sample, *j_sample);
                I_scale_factor_calc(j_sample, &j_scale, 1);
            }
            put_scale(scalar, &fr_ps, max_sc);
            I_main_bit_allocation(ltmin, bit_alloc, &adb, &fr_ps);
            if (info.error_protection) I_CRC_calc(&fr_ps, bit_alloc, &crc);
        } else { /* src/musicin.c:667-704 */
            II_scale_factor_calc(*sb_sample, scalar, C, fr_ps.sblimit);
            pick_scale(scalar, &fr_ps, max_sc);
            if (fr_ps.actual_mode == MPG_MD_JOINT_STEREO) {
                II_combine_LR(*sb_sample, *j_sample, fr_ps.sblimit);
                II_scale_factor_calc(j_sample, &j_scale, 1, fr_ps.sblimit);
            }
            II_transmission_pattern(scalar, scfsi, &fr_ps);
            II_main_bit_allocation(ltmin, scfsi, bit_alloc, &adb, &fr_ps);
            if (info.error_protection) II_CRC_calc(&fr_ps, bit_alloc, scfsi, &crc);
        }
        memset(&d, 0, sizeof(d));
        d.magic = STAGE_DUMP_L12_MAGIC;
        d.frame_index = 0;
        memcpy(d.sb_sample, *sb_sample, sizeof(d.sb_sample));
        memcpy(d.ltmin, ltmin, sizeof(ltmin));
        for (k = 0; k < 2; k++)
            for (i = 0; i < 32; i++) {
                for (j = 0; j < 3; j++) d.scalar[k][j][i] = (int32_t) scalar[k][j][i];
                d.scfsi[k][i] = (int32_t) scfsi[k][i];
                d.bit_alloc[k][i] = (int32_t) bit_alloc[k][i];
            }
        for (j = 0; j < 3; j++)
            for (i = 0; i < 32; i++) d.j_scale[j][i] = (int32_t) j_scale[j][i];
        d.mode = info.mode; d.mode_ext = info.mode_ext; d.jsbound = fr_ps.jsbound; d.sblimit = fr_ps.sblimit;
        d.adb_left = adb; d.crc = info.error_protection ? (int32_t) crc : 0;
        encode_info(&fr_ps, &bs);
        if (info.error_protection) encode_CRC(crc, &bs);
        if (lay == 1) {
            I_encode_bit_alloc(bit_alloc, &fr_ps, &bs);
            I_encode_scale(scalar, bit_alloc, &fr_ps, &bs);
            I_subband_quantization(scalar, *sb_sample, j_scale, *j_sample, bit_alloc, *subband, &fr_ps);
            I_sample_encoding(*subband, bit_alloc, &fr_ps, &bs);
        } else {
            II_encode_bit_alloc(bit_alloc, &fr_ps, &bs);
            II_encode_scale(bit_alloc, scfsi, scalar, &fr_ps, &bs);
            II_subband_quantization(scalar, *sb_sample, j_scale, *j_sample, bit_alloc, *subband, &fr_ps);
            II_sample_encoding(*subband, bit_alloc, &fr_ps, &bs);
        }
        for (i = 0; i < adb; i++) put1bit(&bs, 0);
        head[0] = (int) (sstell(&bs) - before);
        head[1] = 0;
        fwrite(head, 4, 2, fo);
        fwrite(&d, sizeof(d), 1, fo);
    }
    close_bit_stream_w(&bs);
    fclose(fo);
    fclose(fi);
    return 0;
}
