/* TEST INFRASTRUCTURE -- CPU restatement of the reference's Layer I / Layer II encoders with psychoacoustic
 * model 2 (SURVEY 8(f) row 4).  Included at the end of mp3_oracle.c: it shares that file's Hann window, real
 * split-radix FFT, polyphase filterbank and bit writer, which the reference shares too (src/subs.c, src/encode.c:287-409,
 * src/common.c:1134).  Same rules as mp3_oracle.h: only tests/, smoke() and bench.py's cpu_baseline leg may use it.
 *
 * Parity status: PINNED against the unmodified reference (oracle/_ref/ref_harness_l12: bytes and every
 * stage_dump_l12_t member; oracle/_ref/encode -l 1|2: bytes), tests/test_oracle_l12.py.
 *
 * Psychoacoustic model 1 (src/tonal.c) is not restated: the reference as shipped cannot run it -- it reads its
 * critical-band and threshold tables from files ("2cb0", "2th0", ...; src/tonal.c:86-150) that the repository does not
 * contain, and exits ("Please check 2cb0 boundary table").
 */
#include "stage_dump_l12.h"
#include "oracle_tables_l12_gen.h"

static const int L12_BITRATES[2][15] = { /* src/common.c:122-123 */
    {0, 32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 416, 448},
    {0, 32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384}};
static const double L12_SNR[18] = {0.00, 7.00, 11.00, 16.00, 20.84, 25.28, 31.59, 37.75, 43.84, /* src/encode.c:777-780 */
                                   49.89, 55.93, 61.96, 67.98, 74.01, 80.03, 86.05, 92.01, 98.01};
static const double L12_QA[17] = {0.750000000, 0.625000000, 0.875000000, 0.562500000, 0.937500000, /* src/encode.c:1195-1199 */
                                  0.968750000, 0.984375000, 0.992187500, 0.996093750, 0.998046875,
                                  0.999023438, 0.999511719, 0.999755859, 0.999877930, 0.999938965,
                                  0.999969482, 0.999984741};
static const double L12_QB[17] = {-0.250000000, -0.375000000, -0.125000000, -0.437500000, -0.062500000, /* :1201-1205 */
                                  -0.031250000, -0.015625000, -0.007812500, -0.003906250, -0.001953125,
                                  -0.000976563, -0.000488281, -0.000244141, -0.000122070, -0.000061035,
                                  -0.000030518, -0.000015259};
static const int L12_SFS_PER_SCFSI[4] = {3, 2, 1, 2}; /* src/encode.c:825 */

typedef struct {
    int layer, ri, kbps, bitrate_index, channels;
    int actual_mode, mode, mode_ext, crc_on, copyright, original, emphasis;
    int sblimit, jsbound, table, frame_bits;
    mp3o_stream *base; /* Hann window, FFT twiddles, filter matrix, filterbank ring, bit writer */
    /* psycho_anal's statics, src/psy.c:52-92 */
    int numlines[CBANDS], partition[HBLK];
    float cbval[CBANDS], rnorm[CBANDS], s[CBANDS][CBANDS];
    double tmn[CBANDS];
    float lthr[2][HBLK], r[2][2][HBLK], phi_sav[2][2][HBLK];
    int age_new, age_old, age_oldest;
    int flush, syncsize, sync_flush;
    short sam[2][1344];      /* the driver's sam[], src/musicin.c:480 */
    short buffer[2][1152];   /* the driver's buffer[], kept from frame to frame (Layer I reuses 64 samples) */
    double snr[18], qa[17], qb[17]; /* as the layer's first frame leaves them, src/encode.c:900-905, 1226-1231 */
    unsigned short alloc[32][16][4];
    double sb_sample[2][3][12][32], j_sample[1][3][12][32]; /* the driver's, zero-filled once (src/musicin.c:496-498) */
    unsigned sbband[2][3][12][32];
} l12_stream;

/* ---------------------------------------------------------------------------------------------------------------- */
/* psychoacoustic model 2 for Layers I and II, src/psy.c                                                            */
/* ---------------------------------------------------------------------------------------------------------------- */
static void l12_psy_init(l12_stream *L)
{ /* src/psy.c:107-237; every intermediate keeps the type the reference declares */
    static const float crit_band[27] = {0, 100, 200, 300, 400, 510, 630, 770, 920, 1080, 1270, 1480, 1720, 2000, 2320, 2700,
                                        3150, 3700, 4400, 5300, 6400, 7700, 9500, 12000, 15500, 25000, 30000};
    static const double rates[3] = {44100.0, 48000.0, 32000.0};
    float fthr[HBLK], freq_mult, bval_lo;
    double temp1, temp2, temp3;
    unsigned i, j;
    for (i = 0; i < HBLK; i++) {
        L->lthr[0][i] = 60802371420160.0;
        L->lthr[1][i] = 60802371420160.0;
    }
    freq_mult = rates[L->ri] / 1024; /* sfreq/BLKSIZE, a double rounded to FLOAT */
    for (i = 0; i < HBLK; i++) {
        temp1 = i * freq_mult; /* unsigned * FLOAT in float, then widened */
        j = 1;
        while (temp1 > crit_band[j]) j++;
        fthr[i] = j - 1 + (temp1 - crit_band[j - 1]) / (crit_band[j] - crit_band[j - 1]);
    }
    L->partition[0] = 0;
    temp2 = 1;
    L->cbval[0] = fthr[0];
    bval_lo = fthr[0];
    for (i = 1; i < HBLK; i++) {
        if ((fthr[i] - bval_lo) > 0.33) {
            L->partition[i] = L->partition[i - 1] + 1;
            L->cbval[L->partition[i - 1]] = L->cbval[L->partition[i - 1]] / temp2;
            L->cbval[L->partition[i]] = fthr[i];
            bval_lo = fthr[i];
            L->numlines[L->partition[i - 1]] = temp2;
            temp2 = 1;
        } else {
            L->partition[i] = L->partition[i - 1];
            L->cbval[L->partition[i]] += fthr[i];
            temp2++;
        }
    }
    L->numlines[L->partition[i - 1]] = temp2;
    L->cbval[L->partition[i - 1]] = L->cbval[L->partition[i - 1]] / temp2;
    assert(L->partition[HBLK - 1] < CBANDS);
    for (j = 0; j < CBANDS; j++)
        for (i = 0; i < CBANDS; i++) { /* :200-216 */
            temp1 = (L->cbval[i] - L->cbval[j]) * 1.05;
            if (temp1 >= 0.5 && temp1 <= 2.5) {
                temp2 = temp1 - 0.5;
                temp2 = 8.0 * (temp2 * temp2 - 2.0 * temp2);
            } else temp2 = 0;
            temp1 += 0.474;
            temp3 = 15.811389 + 7.5 * temp1 - 17.5 * sqrt((double) (1.0 + temp1 * temp1));
            if (temp3 <= -100) L->s[i][j] = 0;
            else {
                temp3 = (temp2 + temp3) * R_LN_TO_LOG10;
                L->s[i][j] = exp(temp3);
            }
        }
    for (j = 0; j < CBANDS; j++) { /* :219-228 */
        temp1 = 15.5 + L->cbval[j];
        L->tmn[j] = (temp1 > 24.5) ? temp1 : 24.5;
        L->rnorm[j] = 0;
        for (i = 0; i < CBANDS; i++) L->rnorm[j] += L->s[j][i];
    }
    if (L->layer == 1) { L->flush = 384; L->syncsize = 1024; L->sync_flush = 576; }
    else { L->flush = 576; L->syncsize = 1056; L->sync_flush = 480; }
    L->age_new = 0; L->age_old = 1; L->age_oldest = 0;
}

static void l12_psycho_anal(l12_stream *L, const short *buffer, int chn, float snr32[32])
{ /* src/psy.c:239-405 */
    static const float bmax[27] = {20.0, 20.0, 20.0, 20.0, 20.0, 17.0, 15.0, 10.0, 7.0, 4.4, 4.5, 4.5, 4.5, 4.5,
                                   4.5, 4.5, 4.5, 4.5, 4.5, 4.5, 4.5, 4.5, 4.5, 4.5, 3.5, 3.5, 3.5};
    const double nmt = 5.5;
    const tables_t *T = L->base->T;
    const float *absthr = T12_ABSTHR[L->ri];
    float wsamp[1024], energy[1024], phi[1024], c[HBLK], fthr[HBLK];
    float grouped_c[CBANDS], grouped_e[CBANDS], nb[CBANDS], cb[CBANDS], ecb[CBANDS], bc[CBANDS], snrtmp[2][32];
    float r_prime, phi_prime, minthres, sum_energy;
    double tb, temp1, temp2, temp3;
    short *savebuf = L->sam[chn];
    unsigned i, j, k;
    int nw, old, oldest;
    for (i = 0; i < (unsigned) L->layer; i++) {
        for (j = 0; j < (unsigned) L->syncsize; j++) { /* :258-266 */
            if (j < (unsigned) L->sync_flush) savebuf[j] = savebuf[j + L->flush];
            else savebuf[j] = *buffer++;
            if (j < 1024) wsamp[j] = T->window[j] * ((float) savebuf[j]);
        }
        fft_energy_phase(T, wsamp, energy, phi, 1024);
        if (L->layer == 2 || (L->layer == 1 && chn == 0)) { /* :277-281 */
            if (L->age_new == 0) { L->age_new = 1; L->age_oldest = 1; }
            else { L->age_new = 0; L->age_oldest = 0; }
            if (L->age_old == 0) L->age_old = 1; else L->age_old = 0;
        }
        nw = L->age_new; old = L->age_old; oldest = L->age_oldest;
        for (j = 0; j < HBLK; j++) { /* :282-292 */
            r_prime = 2.0 * L->r[chn][old][j] - L->r[chn][oldest][j];
            phi_prime = 2.0 * L->phi_sav[chn][old][j] - L->phi_sav[chn][oldest][j];
            L->r[chn][nw][j] = sqrt((double) energy[j]);
            L->phi_sav[chn][nw][j] = phi[j];
            temp1 = L->r[chn][nw][j] * cos((double) phi[j]) - r_prime * cos((double) phi_prime);
            temp2 = L->r[chn][nw][j] * sin((double) phi[j]) - r_prime * sin((double) phi_prime);
            temp3 = L->r[chn][nw][j] + fabs((double) r_prime);
            if (temp3 != 0) c[j] = sqrt(temp1 * temp1 + temp2 * temp2) / temp3;
            else c[j] = 0;
        }
        for (j = 1; j < CBANDS; j++) { grouped_e[j] = 0; grouped_c[j] = 0; } /* :297-306 */
        grouped_e[0] = energy[0];
        grouped_c[0] = energy[0] * c[0];
        for (j = 1; j < HBLK; j++) {
            grouped_e[L->partition[j]] += energy[j];
            grouped_c[L->partition[j]] += energy[j] * c[j];
        }
        for (j = 0; j < CBANDS; j++) { /* :312-323 */
            ecb[j] = 0;
            cb[j] = 0;
            for (k = 0; k < CBANDS; k++)
                if (L->s[j][k] != 0.0) {
                    ecb[j] += L->s[j][k] * grouped_e[k];
                    cb[j] += L->s[j][k] * grouped_c[k];
                }
            if (ecb[j] != 0) cb[j] = cb[j] / ecb[j];
            else cb[j] = 0;
        }
        for (j = 0; j < CBANDS; j++) { /* :329-338 */
            if (cb[j] < .05) cb[j] = 0.05;
            else if (cb[j] > .5) cb[j] = 0.5;
            tb = -0.434294482 * log((double) cb[j]) - 0.301029996;
            cb[j] = tb;
            bc[j] = L->tmn[j] * tb + nmt * (1.0 - tb);
            k = L->cbval[j] + 0.5;
            bc[j] = (bc[j] > bmax[k]) ? bc[j] : bmax[k];
            bc[j] = exp((double) -bc[j] * R_LN_TO_LOG10);
        }
        for (j = 0; j < CBANDS; j++) /* :345-348 */
            if (L->rnorm[j] && L->numlines[j]) nb[j] = ecb[j] * bc[j] / (L->rnorm[j] * L->numlines[j]);
            else nb[j] = 0;
        for (j = 0; j < HBLK; j++) { /* :349-362 */
            temp1 = nb[L->partition[j]];
            temp1 = (temp1 > absthr[j]) ? temp1 : absthr[j];
            if (L->layer == 1) {
                fthr[j] = (temp1 < L->lthr[chn][j]) ? temp1 : L->lthr[chn][j];
                temp2 = temp1 * 0.00316;
                fthr[j] = (temp2 > fthr[j]) ? temp2 : fthr[j];
            } else fthr[j] = temp1;
            L->lthr[chn][j] = 32.0 * temp1; /* LXMIN, src/encoder.h:96 */
        }
        for (j = 0; j < 193; j += 16) { /* :367-376 */
            minthres = 60802371420160.0;
            sum_energy = 0.0;
            for (k = 0; k < 17; k++) {
                if (minthres > fthr[j + k]) minthres = fthr[j + k];
                sum_energy += energy[j + k];
            }
            snrtmp[i][j / 16] = sum_energy / (minthres * 17.0);
            snrtmp[i][j / 16] = 4.342944819 * log((double) snrtmp[i][j / 16]);
        }
        for (j = 208; j < (HBLK - 1); j += 16) { /* :377-386 */
            minthres = 0.0;
            sum_energy = 0.0;
            for (k = 0; k < 17; k++) {
                minthres += fthr[j + k];
                sum_energy += energy[j + k];
            }
            snrtmp[i][j / 16] = sum_energy / minthres;
            snrtmp[i][j / 16] = 4.342944819 * log((double) snrtmp[i][j / 16]);
        }
    }
    for (i = 0; i < 32; i++) { /* :391-395 */
        if (L->layer == 2) snr32[i] = (snrtmp[0][i] > snrtmp[1][i]) ? snrtmp[0][i] : snrtmp[1][i];
        else snr32[i] = snrtmp[0][i];
    }
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* scale factors, src/encode.c:512-561, 638-691                                                                     */
/* ---------------------------------------------------------------------------------------------------------------- */
static void l12_scale_factor_calc(double sb[][3][12][32], unsigned scalar[][3][32], int nch, int nparts, int sblimit)
{ /* I_ / II_scale_factor_calc: nparts 1 / 3; the scalefactor just above the peak of 12 samples */
    int i, j, k, t;
    for (k = 0; k < nch; k++)
        for (t = 0; t < nparts; t++) {
            for (i = 0; i < sblimit; i++) {
                double sm = fabs(sb[k][t][0][i]);
                for (j = 1; j < 12; j++)
                    if (fabs(sb[k][t][j][i]) > sm) sm = fabs(sb[k][t][j][i]);
                scalar[k][t][i] = 0;
                for (j = 62; j >= 0; j--)
                    if (sm <= T12_MULTIPLE[j]) { scalar[k][t][i] = (unsigned) j; break; }
            }
            for (i = sblimit; i < 32; i++) scalar[k][t][i] = 63;
        }
}

static void l12_transmission_pattern(unsigned scalar[2][3][32], unsigned scfsi[2][32], int stereo, int sblimit)
{ /* II_transmission_pattern, src/encode.c:638-691 */
    static const int pattern[5][5] = {{0x123, 0x122, 0x122, 0x133, 0x123}, {0x113, 0x111, 0x111, 0x444, 0x113},
                                      {0x111, 0x111, 0x111, 0x333, 0x113}, {0x222, 0x222, 0x222, 0x333, 0x123},
                                      {0x123, 0x122, 0x122, 0x133, 0x123}};
    int dscf[2], cls[2], i, j, k;
    for (k = 0; k < stereo; k++)
        for (i = 0; i < sblimit; i++) {
            dscf[0] = (int) (scalar[k][0][i] - scalar[k][1][i]);
            dscf[1] = (int) (scalar[k][1][i] - scalar[k][2][i]);
            for (j = 0; j < 2; j++) {
                if (dscf[j] <= -3) cls[j] = 0;
                else if (dscf[j] > -3 && dscf[j] < 0) cls[j] = 1;
                else if (dscf[j] == 0) cls[j] = 2;
                else if (dscf[j] > 0 && dscf[j] < 3) cls[j] = 3;
                else cls[j] = 4;
            }
            switch (pattern[cls[0]][cls[1]]) {
            case 0x123: scfsi[k][i] = 0; break;
            case 0x122: scfsi[k][i] = 3; scalar[k][2][i] = scalar[k][1][i]; break;
            case 0x133: scfsi[k][i] = 3; scalar[k][1][i] = scalar[k][2][i]; break;
            case 0x113: scfsi[k][i] = 1; scalar[k][1][i] = scalar[k][0][i]; break;
            case 0x111: scfsi[k][i] = 2; scalar[k][1][i] = scalar[k][2][i] = scalar[k][0][i]; break;
            case 0x222: scfsi[k][i] = 2; scalar[k][0][i] = scalar[k][2][i] = scalar[k][1][i]; break;
            case 0x333: scfsi[k][i] = 2; scalar[k][0][i] = scalar[k][1][i] = scalar[k][2][i]; break;
            case 0x444:
                scfsi[k][i] = 2;
                if (scalar[k][0][i] > scalar[k][2][i]) scalar[k][0][i] = scalar[k][2][i];
                scalar[k][1][i] = scalar[k][2][i] = scalar[k][0][i];
            }
        }
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* bit allocation, src/encode.c:782-1172                                                                            */
/* ---------------------------------------------------------------------------------------------------------------- */
static mp3o_l12_alloc_trace_t *l12_trace; /* what the allocation reached, which no output shows (mp3o_l12_alloc_frames); NULL: none kept */

static void l12_trace_step(int ad, int needed)
{ /* one turn of *_a_bit_allocation's loop: the chosen band's step costs `needed` - what was spent before it of `ad` */
    mp3o_l12_alloc_trace_t *t = l12_trace;
    if (!t) return;
    if (ad >= needed) {
        t->steps++;
        if (t->closed_no_room) t->granted_after_close++;
        if (t->closed_no_room && ad == needed) t->exact_after_close++;
        if (ad - needed < t->min_slack) t->min_slack = ad - needed;
    } else {
        if (t->closed_no_room && needed - ad < t->min_short_after_close) t->min_short_after_close = needed - ad;
        t->closed_no_room++;
        if (needed - ad < t->min_short) t->min_short = needed - ad;
    }
}

static int l12_js_bound(int lay, int m_ext)
{ /* src/common.c:320-331 */
    static const int jsb_table[3][4] = {{4, 8, 12, 16}, {4, 8, 12, 16}, {0, 4, 8, 16}};
    return jsb_table[lay - 1][m_ext];
}

static int l1_bits_for_nonoise(const l12_stream *L, double perm_smr[2][32])
{ /* I_bits_for_nonoise, src/encode.c:782-806 */
    const int stereo = L->channels, jsbound = L->jsbound;
    int i, j, k, req_bits = 32 + 4 * ((jsbound * stereo) + (32 - jsbound));
    for (i = 0; i < 32; ++i)
        for (j = 0; j < ((i < jsbound) ? stereo : 1); ++j) {
            for (k = 0; k < 14; ++k)
                if ((-perm_smr[j][i] + L->snr[k]) >= 0.0) break;
            if (stereo == 2 && i >= jsbound)
                for (; k < 14; ++k)
                    if ((-perm_smr[1 - j][i] + L->snr[k]) >= 0.0) break;
            if (k > 0) req_bits += (k + 1) * 12 + 6 * ((i >= jsbound) ? stereo : 1);
        }
    return req_bits;
}

static int l2_bits_for_nonoise(const l12_stream *L, double perm_smr[2][32], unsigned scfsi[2][32])
{ /* II_bits_for_nonoise, src/encode.c:810-860 */
    const int stereo = L->channels, sblimit = L->sblimit, jsbound = L->jsbound;
    int sb, ch, ba, req_bits, bbal = 0, berr = L->crc_on ? 16 : 0, banc = 32, maxAlloc, sel_bits, sc_bits, smp_bits;
    for (sb = 0; sb < jsbound; ++sb) bbal += stereo * L->alloc[sb][0][1];
    for (sb = jsbound; sb < sblimit; ++sb) bbal += L->alloc[sb][0][1];
    req_bits = banc + bbal + berr;
    for (sb = 0; sb < sblimit; ++sb)
        for (ch = 0; ch < ((sb < jsbound) ? stereo : 1); ++ch) {
            maxAlloc = (1 << L->alloc[sb][0][1]) - 1;
            sel_bits = sc_bits = smp_bits = 0;
            for (ba = 0; ba < maxAlloc - 1; ++ba)
                if ((-perm_smr[ch][sb] + L->snr[L->alloc[sb][ba][3] + ((ba > 0) ? 1 : 0)]) >= 0.0) break;
            if (stereo == 2 && sb >= jsbound)
                for (; ba < maxAlloc - 1; ++ba)
                    if ((-perm_smr[1 - ch][sb] + L->snr[L->alloc[sb][ba][3] + ((ba > 0) ? 1 : 0)]) >= 0.0) break;
            if (ba > 0) {
                smp_bits = 12 * (L->alloc[sb][ba][2] * L->alloc[sb][ba][1]);
                sel_bits = 2;
                sc_bits = 6 * L12_SFS_PER_SCFSI[scfsi[ch][sb]];
                if (stereo == 2 && sb >= jsbound) {
                    sel_bits += 2;
                    sc_bits += 6 * L12_SFS_PER_SCFSI[scfsi[1 - ch][sb]];
                }
                req_bits += smp_bits + sel_bits + sc_bits;
            }
        }
    return req_bits;
}

static void l1_a_bit_allocation(l12_stream *L, double perm_smr[2][32], unsigned bit_alloc[2][32], int *adb)
{ /* I_a_bit_allocation, src/encode.c:974-1062 */
    const int stereo = L->channels, jsbound = L->jsbound;
    int i, k, smpl_bits, scale_bits, min_sb, min_ch, oth_ch, bspl, bscf, ad, bbal;
    const int banc = 32, berr = L->crc_on ? 16 : 0;
    double mnr[2][32], small;
    char used[2][32];
    bbal = 4 * ((jsbound * stereo) + (32 - jsbound));
    *adb -= bbal + berr + banc;
    ad = *adb;
    for (i = 0; i < 32; i++)
        for (k = 0; k < stereo; k++) {
            mnr[k][i] = L->snr[0] - perm_smr[k][i];
            bit_alloc[k][i] = 0;
            used[k][i] = 0;
        }
    bspl = bscf = 0;
    do {
        small = mnr[0][0] + 1; min_sb = -1; min_ch = -1;
        for (i = 0; i < 32; i++)
            for (k = 0; k < stereo; k++)
                if (used[k][i] != 2 && small > mnr[k][i]) { small = mnr[k][i]; min_sb = i; min_ch = k; }
        if (min_sb > -1) {
            if (used[min_ch][min_sb]) { smpl_bits = 12; scale_bits = 0; }
            else { smpl_bits = 24; scale_bits = 6; }
            if (min_sb >= jsbound) scale_bits *= stereo;
            l12_trace_step(ad, bspl + bscf + scale_bits + smpl_bits);
            if (ad >= bspl + bscf + scale_bits + smpl_bits) {
                bspl += smpl_bits;
                bscf += scale_bits;
                bit_alloc[min_ch][min_sb]++;
                used[min_ch][min_sb] = 1;
                mnr[min_ch][min_sb] = -perm_smr[min_ch][min_sb] + L->snr[bit_alloc[min_ch][min_sb]];
                if (bit_alloc[min_ch][min_sb] == 14) used[min_ch][min_sb] = 2;
            } else used[min_ch][min_sb] = 2;
            if (stereo == 2 && min_sb >= jsbound) {
                oth_ch = 1 - min_ch;
                bit_alloc[oth_ch][min_sb] = bit_alloc[min_ch][min_sb];
                used[oth_ch][min_sb] = used[min_ch][min_sb];
                mnr[oth_ch][min_sb] = -perm_smr[oth_ch][min_sb] + L->snr[bit_alloc[oth_ch][min_sb]];
            }
        }
    } while (min_sb > -1);
    ad -= bspl + bscf;
    *adb = ad;
}

static void l2_a_bit_allocation(l12_stream *L, double perm_smr[2][32], unsigned scfsi[2][32], unsigned bit_alloc[2][32], int *adb)
{ /* II_a_bit_allocation, src/encode.c:1066-1172 */
    const int stereo = L->channels, sblimit = L->sblimit, jsbound = L->jsbound;
    int i, min_ch, min_sb, oth_ch, k, increment, scale, seli, ba, bspl, bscf, bsel, ad, bbal = 0;
    const int banc = 32, berr = L->crc_on ? 16 : 0;
    double mnr[2][32], small;
    char used[2][32];
    for (i = 0; i < jsbound; ++i) bbal += stereo * L->alloc[i][0][1];
    for (i = jsbound; i < sblimit; ++i) bbal += L->alloc[i][0][1];
    *adb -= bbal + berr + banc;
    ad = *adb;
    for (i = 0; i < sblimit; i++)
        for (k = 0; k < stereo; k++) {
            mnr[k][i] = L->snr[0] - perm_smr[k][i];
            bit_alloc[k][i] = 0;
            used[k][i] = 0;
        }
    bspl = bscf = bsel = 0;
    do {
        small = 999999.0; min_sb = -1; min_ch = -1;
        for (i = 0; i < sblimit; i++)
            for (k = 0; k < stereo; ++k)
                if (used[k][i] != 2 && small > mnr[k][i]) { small = mnr[k][i]; min_sb = i; min_ch = k; }
        if (min_sb > -1) {
            const unsigned short (*al)[4] = L->alloc[min_sb];
            increment = 12 * (al[bit_alloc[min_ch][min_sb] + 1][2] * al[bit_alloc[min_ch][min_sb] + 1][1]);
            if (used[min_ch][min_sb]) increment -= 12 * (al[bit_alloc[min_ch][min_sb]][2] * al[bit_alloc[min_ch][min_sb]][1]);
            oth_ch = 1 - min_ch;
            if (used[min_ch][min_sb]) scale = seli = 0;
            else {
                seli = 2;
                scale = 6 * L12_SFS_PER_SCFSI[scfsi[min_ch][min_sb]];
                if (stereo == 2 && min_sb >= jsbound) {
                    seli += 2;
                    scale += 6 * L12_SFS_PER_SCFSI[scfsi[oth_ch][min_sb]];
                }
            }
            l12_trace_step(ad, bspl + bscf + bsel + seli + scale + increment);
            if (ad >= bspl + bscf + bsel + seli + scale + increment) {
                ba = (int) ++bit_alloc[min_ch][min_sb];
                bspl += increment;
                bscf += scale;
                bsel += seli;
                used[min_ch][min_sb] = 1;
                mnr[min_ch][min_sb] = -perm_smr[min_ch][min_sb] + L->snr[al[ba][3] + 1];
                if (ba >= (1 << al[0][1]) - 1) used[min_ch][min_sb] = 2;
            } else used[min_ch][min_sb] = 2;
            if (min_sb >= jsbound && stereo == 2) {
                ba = (int) (bit_alloc[oth_ch][min_sb] = bit_alloc[min_ch][min_sb]);
                used[oth_ch][min_sb] = used[min_ch][min_sb];
                mnr[oth_ch][min_sb] = -perm_smr[oth_ch][min_sb] + L->snr[al[ba][3] + 1];
            }
        }
    } while (min_sb > -1);
    ad -= bspl + bscf + bsel;
    *adb = ad;
    for (i = sblimit; i < 32; i++)
        for (k = 0; k < stereo; k++) bit_alloc[k][i] = 0;
}

static void l12_main_bit_allocation(l12_stream *L, double perm_smr[2][32], unsigned scfsi[2][32], unsigned bit_alloc[2][32], int *adb)
{ /* I_ / II_main_bit_allocation, src/encode.c:882-948: the joint stereo bound, then the allocation itself */
    if (L->actual_mode == 1) {
        int rq, mode_ext;
        L->mode = 0;
        L->mode_ext = 0;
        L->jsbound = L->sblimit;
        rq = (L->layer == 1) ? l1_bits_for_nonoise(L, perm_smr) : l2_bits_for_nonoise(L, perm_smr, scfsi);
        if (l12_trace) l12_trace->rq[l12_trace->n_rq++] = rq;
        if (rq > *adb) {
            L->mode = 1;
            mode_ext = 4;
            do {
                --mode_ext;
                L->jsbound = l12_js_bound(L->layer, mode_ext);
                rq = (L->layer == 1) ? l1_bits_for_nonoise(L, perm_smr) : l2_bits_for_nonoise(L, perm_smr, scfsi);
                if (l12_trace) l12_trace->rq[l12_trace->n_rq++] = rq;
            } while ((rq > *adb) && (mode_ext > 0));
            L->mode_ext = mode_ext;
        }
    }
    if (L->layer == 1) l1_a_bit_allocation(L, perm_smr, bit_alloc, adb);
    else l2_a_bit_allocation(L, perm_smr, scfsi, bit_alloc, adb);
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* CRC, src/common.c:1251-1327                                                                                      */
/* ---------------------------------------------------------------------------------------------------------------- */
static void l12_update_crc(unsigned data, unsigned length, unsigned *crc)
{
    unsigned masking = 1u << length, carry;
    while ((masking >>= 1)) {
        carry = *crc & 0x8000;
        *crc <<= 1;
        if (!carry ^ !(data & masking)) *crc ^= 0x8005;
    }
    *crc &= 0xffff;
}

static unsigned l12_crc_calc(const l12_stream *L, unsigned bit_alloc[2][32], unsigned scfsi[2][32])
{
    const int stereo = L->channels, sblimit = L->sblimit, jsbound = L->jsbound;
    unsigned crc = 0xffff;
    int i, k;
    l12_update_crc((unsigned) L->bitrate_index, 4, &crc);
    l12_update_crc((unsigned) L->ri, 2, &crc);
    l12_update_crc(0, 1, &crc); /* padding: never set, src/musicin.c:566-581 */
    l12_update_crc(0, 1, &crc); /* extension */
    l12_update_crc((unsigned) L->mode, 2, &crc);
    l12_update_crc((unsigned) L->mode_ext, 2, &crc);
    l12_update_crc((unsigned) L->copyright, 1, &crc);
    l12_update_crc((unsigned) L->original, 1, &crc);
    l12_update_crc((unsigned) L->emphasis, 2, &crc);
    if (L->layer == 1) {
        for (i = 0; i < 32; i++)
            for (k = 0; k < ((i < jsbound) ? stereo : 1); k++) l12_update_crc(bit_alloc[k][i], 4, &crc);
    } else {
        for (i = 0; i < sblimit; i++)
            for (k = 0; k < ((i < jsbound) ? stereo : 1); k++) l12_update_crc(bit_alloc[k][i], L->alloc[i][0][1], &crc);
        for (i = 0; i < sblimit; i++)
            for (k = 0; k < stereo; k++)
                if (bit_alloc[k][i]) l12_update_crc(scfsi[k][i], 2, &crc);
    }
    return crc;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* one frame, src/musicin.c:620-704                                                                                 */
/* ---------------------------------------------------------------------------------------------------------------- */
static void l12_encode_frame_tail(l12_stream *L, double ltmin[2][32], stage_dump_l12_t *d);

static void l12_encode_frame(l12_stream *L, stage_dump_l12_t *d)
{
    mp3o_stream *B = L->base;
    const int stereo = L->channels, nparts = (L->layer == 1) ? 1 : 3;
    double ltmin[2][32];
    float snr32[32];
    const short *win_buf[2];
    int i, j, k;
    memset(ltmin, 0, sizeof(ltmin));
    win_buf[0] = L->buffer[0]; win_buf[1] = L->buffer[1];
    for (i = 0; i < nparts; i++)
        for (j = 0; j < 12; j++)
            for (k = 0; k < stereo; k++) {
                filterbank_slot(B, win_buf[k], k, L->sb_sample[k][i][j]);
                win_buf[k] += 32;
            }
    for (k = 0; k < stereo; k++) {
        l12_psycho_anal(L, L->buffer[k], k, snr32);
        for (i = 0; i < 32; i++) ltmin[k][i] = (double) snr32[i];
    }
    l12_encode_frame_tail(L, ltmin, d);
}

/* everything behind the filterbank and the model: from L->sb_sample and the signal-to-mask ratios to the frame's bits.  (The
 * reference computes the scale factors before psycho_anal; neither reads what the other writes.) */
static void l12_encode_frame_tail(l12_stream *L, double ltmin[2][32], stage_dump_l12_t *d)
{
    double (*sb_sample)[3][12][32] = L->sb_sample, (*j_sample)[3][12][32] = L->j_sample;
    unsigned (*sbband)[3][12][32] = L->sbband;
    mp3o_stream *B = L->base;
    const int stereo = L->channels, nparts = (L->layer == 1) ? 1 : 3;
    unsigned scalar[2][3][32], j_scale[1][3][32], scfsi[2][32], bit_alloc[2][32], crc = 0;
    int adb = L->frame_bits, i, j, k, s, sblimit = L->sblimit, jsbound;
    memset(scalar, 0, sizeof(scalar)); memset(j_scale, 0, sizeof(j_scale)); memset(scfsi, 0, sizeof(scfsi));
    memset(bit_alloc, 0, sizeof(bit_alloc));
    l12_scale_factor_calc(sb_sample, scalar, stereo, nparts, sblimit);
    if (L->actual_mode == 1) { /* I_ / II_combine_LR, src/encode.c:469-494 */
        for (i = 0; i < sblimit; ++i)
            for (j = 0; j < 12; ++j)
                for (s = 0; s < nparts; ++s) j_sample[0][s][j][i] = .5 * (sb_sample[0][s][j][i] + sb_sample[1][s][j][i]);
        l12_scale_factor_calc(j_sample, j_scale, 1, nparts, sblimit);
    }
    if (L->layer == 2) l12_transmission_pattern(scalar, scfsi, stereo, sblimit);
    l12_main_bit_allocation(L, ltmin, scfsi, bit_alloc, &adb);
    jsbound = L->jsbound;
    if (L->crc_on) crc = l12_crc_calc(L, bit_alloc, scfsi);
    if (d) {
        memset(d, 0, sizeof(*d));
        memcpy(d->sb_sample, sb_sample, sizeof(L->sb_sample));
        memcpy(d->ltmin, ltmin, sizeof(d->ltmin));
        for (k = 0; k < 2; k++)
            for (i = 0; i < 32; i++) {
                for (s = 0; s < 3; s++) d->scalar[k][s][i] = (int32_t) scalar[k][s][i];
                d->scfsi[k][i] = (int32_t) scfsi[k][i];
                d->bit_alloc[k][i] = (int32_t) bit_alloc[k][i];
            }
        for (s = 0; s < 3; s++)
            for (i = 0; i < 32; i++) d->j_scale[s][i] = (int32_t) j_scale[0][s][i];
        d->mode = L->mode; d->mode_ext = L->mode_ext; d->jsbound = jsbound; d->sblimit = sblimit;
        d->adb_left = adb; d->crc = (int32_t) crc;
        d->magic = STAGE_DUMP_L12_MAGIC;
    }
    /* encode_info, src/encode.c:418-437 */
    put_bits(B, 0xfff, 12); put_bits(B, 1, 1); put_bits(B, (unsigned) (4 - L->layer), 2); put_bits(B, !L->crc_on, 1);
    put_bits(B, (unsigned) L->bitrate_index, 4); put_bits(B, (unsigned) L->ri, 2); put_bits(B, 0, 1); put_bits(B, 0, 1);
    put_bits(B, (unsigned) L->mode, 2); put_bits(B, (unsigned) L->mode_ext, 2); put_bits(B, (unsigned) L->copyright, 1);
    put_bits(B, (unsigned) L->original, 1); put_bits(B, (unsigned) L->emphasis, 2);
    if (L->crc_on) put_bits(B, crc, 16);
    if (L->layer == 1) {
        for (i = 0; i < 32; i++) /* I_encode_bit_alloc, src/encode.c:1328-1337 */
            for (k = 0; k < ((i < jsbound) ? stereo : 1); k++) put_bits(B, bit_alloc[k][i], 4);
        for (i = 0; i < 32; i++) /* I_encode_scale, src/encode.c:708-716 */
            for (j = 0; j < stereo; j++)
                if (bit_alloc[j][i]) put_bits(B, scalar[j][0][i], 6);
        for (j = 0; j < 12; j++) /* I_subband_quantization, src/encode.c:1233-1267 */
            for (i = 0; i < 32; i++)
                for (k = 0; k < ((i < jsbound) ? stereo : 1); k++)
                    if (bit_alloc[k][i]) {
                        double dd;
                        int n, sig;
                        if (stereo == 2 && i >= jsbound) dd = j_sample[0][0][j][i] / T12_MULTIPLE[j_scale[0][0][i]];
                        else dd = sb_sample[k][0][j][i] / T12_MULTIPLE[scalar[k][0][i]];
                        n = (int) bit_alloc[k][i];
                        dd = dd * L->qa[n - 1] + L->qb[n - 1];
                        if (dd >= 0) sig = 1;
                        else { sig = 0; dd += 1.0; }
                        sbband[k][0][j][i] = (unsigned) (dd * (double) (1L << n));
                        if (sig) sbband[k][0][j][i] |= 1u << n;
                    }
        for (j = 0; j < 12; j++) /* I_sample_encoding, src/encode.c:1373-1378 */
            for (i = 0; i < 32; i++)
                for (k = 0; k < ((i < jsbound) ? stereo : 1); k++)
                    if (bit_alloc[k][i]) put_bits(B, sbband[k][0][j][i], (int) bit_alloc[k][i] + 1);
    } else {
        for (i = 0; i < sblimit; i++) /* II_encode_bit_alloc, src/encode.c:1341-1354 */
            for (k = 0; k < ((i < jsbound) ? stereo : 1); k++) put_bits(B, bit_alloc[k][i], L->alloc[i][0][1]);
        for (i = 0; i < sblimit; i++) /* II_encode_scale, src/encode.c:720-748 */
            for (k = 0; k < stereo; k++)
                if (bit_alloc[k][i]) put_bits(B, scfsi[k][i], 2);
        for (i = 0; i < sblimit; i++)
            for (k = 0; k < stereo; k++)
                if (bit_alloc[k][i]) switch (scfsi[k][i]) {
                    case 0: for (j = 0; j < 3; j++) put_bits(B, scalar[k][j][i], 6); break;
                    case 1:
                    case 3: put_bits(B, scalar[k][0][i], 6); put_bits(B, scalar[k][2][i], 6); break;
                    case 2: put_bits(B, scalar[k][0][i], 6);
                    }
        for (s = 0; s < 3; s++) /* II_subband_quantization, src/encode.c:1271-1325 */
            for (j = 0; j < 12; j++)
                for (i = 0; i < sblimit; i++)
                    for (k = 0; k < ((i < jsbound) ? stereo : 1); k++)
                        if (bit_alloc[k][i]) {
                            double dd;
                            int n, sig, qnt;
                            unsigned stps;
                            if (stereo == 2 && i >= jsbound) dd = j_sample[0][s][j][i] / T12_MULTIPLE[j_scale[0][s][i]];
                            else dd = sb_sample[k][s][j][i] / T12_MULTIPLE[scalar[k][s][i]];
                            qnt = L->alloc[i][bit_alloc[k][i]][3];
                            dd = dd * L->qa[qnt] + L->qb[qnt];
                            if (dd >= 0) sig = 1;
                            else { sig = 0; dd += 1.0; }
                            n = 0;
                            stps = L->alloc[i][bit_alloc[k][i]][0];
                            while ((1L << n) < (long) stps) n++;
                            n--;
                            sbband[k][s][j][i] = (unsigned) (dd * (double) (1L << n));
                            if (sig) sbband[k][s][j][i] |= 1u << n;
                        }
        for (s = 0; s < 3; s++) /* II_sample_encoding, src/encode.c:1382-1416 */
            for (j = 0; j < 12; j += 3)
                for (i = 0; i < sblimit; i++)
                    for (k = 0; k < ((i < jsbound) ? stereo : 1); k++)
                        if (bit_alloc[k][i]) {
                            const unsigned short *e = L->alloc[i][bit_alloc[k][i]];
                            if (e[2] == 3) {
                                int x;
                                for (x = 0; x < 3; x++) put_bits(B, sbband[k][s][j + x][i], e[1]);
                            } else {
                                unsigned y = e[0];
                                unsigned temp = sbband[k][s][j][i] + sbband[k][s][j + 1][i] * y + sbband[k][s][j + 2][i] * y * y;
                                put_bits(B, temp, e[1]);
                            }
                        }
    }
    for (i = 0; i < adb; i++) put_bits(B, 0, 1); /* src/musicin.c:657, 703 */
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* a whole stream                                                                                                   */
/* ---------------------------------------------------------------------------------------------------------------- */
/* a fresh stream as the driver sets it up (src/musicin.c:528-581, src/common.c:291-347); with_tables: the window, the FFT and the
 * filterbank's matrix too (what is in front of the scale factors) */
static l12_stream *l12_stream_new(int layer, int ri, int kbps, int bi, int channels, int m, const char *mode, int with_tables)
{
    static const double s_freq[3] = {44.1, 48, 32};
    l12_stream *L;
    mp3o_stream *B;
    int i, whole_SpF, spf, br_per_ch, sfrq;
    L = (l12_stream *) calloc(1, sizeof(*L));
    B = (mp3o_stream *) calloc(1, sizeof(*B));
    B->T = with_tables ? make_tables(ri) : NULL;
    L->base = B;
    L->layer = layer; L->ri = ri; L->kbps = kbps; L->bitrate_index = bi; L->channels = channels;
    L->actual_mode = L->mode = m; L->mode_ext = 0;
    if (mode && mode[0]) {
        L->crc_on = strchr(mode + 1, 'e') != NULL;
        L->copyright = strchr(mode + 1, 'c') != NULL;
        L->original = strchr(mode + 1, 'o') != NULL;
    }
    spf = (layer == 1) ? 384 : 1152;
    /* src/musicin.c:562-569: the fraction is thrown away, so no frame is ever padded */
    whole_SpF = (int) (((double) spf / s_freq[ri]) * ((double) kbps / (double) (layer == 1 ? 32 : 8)));
    L->frame_bits = whole_SpF * (layer == 1 ? 32 : 8);
    memcpy(L->snr, L12_SNR, sizeof(L->snr)); memcpy(L->qa, L12_QA, sizeof(L->qa)); memcpy(L->qb, L12_QB, sizeof(L->qb));
    if (layer == 1) {
        L->sblimit = 32;
        L->snr[2] = L->snr[3]; /* src/encode.c:900-905 */
        for (i = 3; i < 16; i++) L->snr[i] = L->snr[i + 2];
        L->qa[1] = L->qa[2]; L->qb[1] = L->qb[2]; /* src/encode.c:1226-1231 */
        for (i = 2; i < 15; i++) { L->qa[i] = L->qa[i + 2]; L->qb[i] = L->qb[i + 2]; }
    } else { /* pick_table, src/common.c:291-318 */
        br_per_ch = kbps / channels;
        sfrq = (int) s_freq[ri];
        if ((sfrq == 48 && br_per_ch >= 56) || (br_per_ch >= 56 && br_per_ch <= 80)) L->table = 0;
        else if (sfrq != 48 && br_per_ch >= 96) L->table = 1;
        else if (sfrq != 32 && br_per_ch <= 48) L->table = 2;
        else L->table = 3;
        L->sblimit = T12_ALLOC_SBLIMIT[L->table];
        memcpy(L->alloc, T12_ALLOC[L->table], sizeof(L->alloc));
    }
    L->jsbound = (m == 1) ? l12_js_bound(layer, 0) : L->sblimit; /* hdr_to_frps, src/common.c:333-347 */
    if (with_tables) l12_psy_init(L);
    return L;
}

size_t mp3o_encode_pcm_l12(int layer, int rate_hz, int kbps, int channels, const char *mode, const int16_t *pcm,
                           size_t n_total, uint8_t **out, stage_dump_l12_t *dumps, int max_dumps)
{ /* mode: NULL, or the driver's -m letter (s / d / j / m) followed by e / c / o for -e / -c / -o.
     Returns 0 and *out = NULL for what the reference refuses. */
    l12_stream *L;
    mp3o_stream *B;
    size_t pos = 0, len, per_frame;
    int ri, bi, i, j, frame = 0, m, spf;
    *out = NULL;
    if (layer != 1 && layer != 2) return 0;
    if (rate_hz == 44100) ri = 0; else if (rate_hz == 48000) ri = 1; else if (rate_hz == 32000) ri = 2; else return 0;
    for (bi = 1; bi < 15; bi++)
        if (L12_BITRATES[layer - 1][bi] == kbps) break;
    if (bi == 15 || (channels != 1 && channels != 2)) return 0;
    m = (channels == 1) ? 3 : 0;
    if (mode && mode[0]) m = mode[0] == 'm' ? 3 : mode[0] == 'd' ? 2 : mode[0] == 'j' ? 1 : 0;
    if ((channels == 1) != (m == 3)) return 0;
    L = l12_stream_new(layer, ri, kbps, bi, channels, m, mode, 1);
    B = L->base;
    spf = (layer == 1) ? 384 : 1152;
    per_frame = (size_t) spf * (size_t) channels;
    while (pos < n_total) { /* get_audio / read_samples, src/encode.c:123-256 */
        size_t n = n_total - pos < per_frame ? n_total - pos : per_frame;
        if (layer == 1) {
            for (j = 0; j < 448; j++)
                for (i = 0; i < 2; i++) {
                    if (j < 64) L->buffer[i][j] = (i < channels) ? L->buffer[i][j + 384] : 0;
                    else {
                        size_t q = (size_t) (j - 64) * (size_t) channels + (size_t) i;
                        L->buffer[i][j] = (i < channels && q < n) ? pcm[pos + q] : 0;
                    }
                }
        } else {
            for (j = 0; j < 1152; j++)
                for (i = 0; i < 2; i++) {
                    size_t q = (size_t) j * (size_t) channels + (size_t) i;
                    L->buffer[i][j] = (i < channels && q < n) ? pcm[pos + q] : 0;
                }
        }
        pos += n;
        l12_encode_frame(L, (dumps && frame < max_dumps) ? &dumps[frame] : NULL);
        if (dumps && frame < max_dumps) dumps[frame].frame_index = frame;
        frame++;
    }
    /* close_bit_stream_w: empty_buffer(bs, buf_byte_idx) also writes the byte under construction (src/common.c:843-868) */
    put_bits(B, 0, 0);
    len = (B->out_bits >> 3) + 1;
    *out = (uint8_t *) malloc(len);
    memcpy(*out, B->out, len);
    free_tables(B->T);
    free(B->out);
    free(B);
    free(L);
    return len;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* the frame encoder alone, on given subband samples and ratios (mp3_oracle.h)                                      */
/* ---------------------------------------------------------------------------------------------------------------- */
void mp3o_l12_tables(double multiple[64], uint16_t alloc[4][32][16][4], int32_t sblimit[4], double snr[18], double qa[17], double qb[17])
{
    int i;
    memcpy(multiple, T12_MULTIPLE, sizeof(T12_MULTIPLE));
    memcpy(alloc, T12_ALLOC, sizeof(T12_ALLOC));
    for (i = 0; i < 4; i++) sblimit[i] = T12_ALLOC_SBLIMIT[i];
    memcpy(snr, L12_SNR, sizeof(L12_SNR));
    memcpy(qa, L12_QA, sizeof(L12_QA));
    memcpy(qb, L12_QB, sizeof(L12_QB));
}

int mp3o_l12_alloc_frames(int layer, int rate_hz, int channels, const char *mode, int n, const int32_t *kbps, const double *sb,
                          const float *ratio, uint8_t *out, size_t out_stride, uint32_t *out_len, stage_dump_l12_t *dumps,
                          mp3o_l12_alloc_trace_t *trace)
{
    const int nparts = layer == 1 ? 1 : 3, passes = layer == 1 ? 1 : 2;
    int ri, m, c, k, i, t;
    if ((layer != 1 && layer != 2) || (channels != 1 && channels != 2) || n < 0 || !kbps || !sb || !ratio || !out || !out_len) return -1;
    if (rate_hz == 44100) ri = 0; else if (rate_hz == 48000) ri = 1; else if (rate_hz == 32000) ri = 2; else return -1;
    m = (channels == 1) ? 3 : 0;
    if (mode && mode[0]) m = mode[0] == 'm' ? 3 : mode[0] == 'd' ? 2 : mode[0] == 'j' ? 1 : 0;
    if ((channels == 1) != (m == 3)) return -1;
    for (c = 0; c < n; c++) {
        int bi;
        for (bi = 1; bi < 15; bi++)
            if (L12_BITRATES[layer - 1][bi] == kbps[c]) break;
        if (bi == 15) return -1;
    }
    for (c = 0; c < n; c++) {
        l12_stream *L;
        double ltmin[2][32];
        const double *x = sb + (size_t) c * channels * nparts * 12 * 32;
        const float *r = ratio + (size_t) c * passes * channels * 32;
        size_t len;
        int bi;
        for (bi = 1; bi < 15; bi++)
            if (L12_BITRATES[layer - 1][bi] == kbps[c]) break;
        L = l12_stream_new(layer, ri, kbps[c], bi, channels, m, mode, 0);
        memset(ltmin, 0, sizeof(ltmin));
        for (k = 0; k < channels; k++) {
            for (t = 0; t < nparts; t++) memcpy(L->sb_sample[k][t], x + ((size_t) k * nparts + t) * 12 * 32, sizeof(double) * 12 * 32);
            for (i = 0; i < 32; i++) { /* src/psy.c:391-395: Layer II keeps the larger of its two passes */
                const float a = r[(size_t) k * 32 + i], b = passes == 2 ? r[((size_t) channels + k) * 32 + i] : a;
                ltmin[k][i] = (double) ((passes == 2 && !(a > b)) ? b : a);
            }
        }
        if (trace) {
            memset(&trace[c], 0, sizeof(trace[c]));
            trace[c].min_slack = trace[c].min_short = trace[c].min_short_after_close = 0x7fffffff;
            trace[c].frame_bits = L->frame_bits;
        }
        l12_trace = trace ? &trace[c] : NULL;
        l12_encode_frame_tail(L, ltmin, dumps ? &dumps[c] : NULL);
        l12_trace = NULL;
        put_bits(L->base, 0, 0);
        len = L->base->out_bits >> 3;
        if (len > out_stride) { free(L->base->out); free(L->base); free(L); return -1; }
        memcpy(out + (size_t) c * out_stride, L->base->out, len);
        out_len[c] = (uint32_t) len;
        free(L->base->out);
        free(L->base);
        free(L);
    }
    return 0;
}
