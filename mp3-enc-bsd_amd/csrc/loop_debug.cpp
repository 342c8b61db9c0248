// The self-test hook mp3mi_debug_iteration_loop (include/mp3mi.h): chains of given records -- spectrum, perceptual entropy, masking
// ratios, block type -- through the iteration loop as the drop-in iteration_loop launches it (dropin.cpp, frame_chain_launch):
// k_prep_tail, k_prep on the list it leaves, k_loop with no placement and no gate, for S streams x nf frames in one launch.  Host
// code only: k_loop.hip and loop_pass.h are untouched, the kernels are the ones the encoder runs.
//
// What the three kernels take on trust from the stages before them is checked here first (a chain that breaks one of the rules is
// refused, nothing is launched).  The two bounds that are not a matter of type:
//
//   |xr| <= 2^64 (LD_XR_MAX), a non-zero |xr| >= 2^-500 (LD_XR_MIN).
//     Above: k_loop keeps |xr|^(3/4) as float, computed as sqrt(a * sqrt(a)) from the float a = |xr| (loop_power34): a * sqrt(a)
//     leaves the float range at a = 2^85.3, from where every line would quantise to the table's end at every step.  The search
//     multiplies a band by at most sqrt(2)^3 (pre-emphasis) * sqrt(2)^16 (a scalefactor reaches 16 and scale_bitcount ends the
//     search) = 2^9.5, and the quantiser's table begins at 0.5946^(4/3) > 0.49: at a step q with q / 4 > log2 max|xr| + 9.5 + 1.05
//     every line of every pass quantises to 0, a pass counts 0 bits and inner_loop stops.  For 2^85 that is q = 383; 2^64 leaves
//     room to spare (q <= 299) and is 2^44 times what a 16-bit signal's MDCT can hold.
//     Below: xr^2 stays a normal double, so that quantanf_init's log(xr^2) is finite (k_prep's and k_mdct's tails leave a
//     subnormal square to the reference's walk; an underflow to 0 gives log(0), and nint(-inf) is undefined in C).
//
//   The start step.  k_loop reads mp3mi_tables::step[q - MP3MI_STEP_MIN] (2^(q/4), q = -400 .. 400) at every step q it visits.
//     quantanf_init (src/loop.c:369-402) starts at q0 = max(nint(8 ln sfm), -100) - 70 >= -170.  bin_search_StepSize probes
//     (top + bot) / 2 between q0 and 200, inner_loop raises the step from the last probe until the bits fit, at the latest when
//     everything is 0.  So every step lies in [min(q0, 200), max(q0, 200, q_zero)], q_zero as above.  The low end is never below
//     -170.  The high end: 8 ln sfm has NO upper bound -- sfm is the geometric mean over the non-zero lines, raised to (their
//     number / 576), over the arithmetic mean of all 576: one line of 2^-40 gives 8 ln sfm = 493, q0 = 423 -- so it is computed
//     here, in plain double the reference's way (sequential sums, libm), with a margin of 1e-6 max(1, |v|) on v = 8 ln sfm (the
//     kernels' own value is within 1e-9 of the reference's, k_prep.hip; libm's within 1e-12), and a granule is refused unless
//     max(nint(v + margin) - 70, 200, q_zero) <= 400.  (k_prep and k_mdct's tail also clamp what they write to 400 -- a caller of
//     the drop-in iteration_loop is not checked --, which changes nothing a stream shows: k_prep.hip.  The hook still refuses
//     such a granule: with the clamp the search visits other steps than the reference's, and only the status word is the same.)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "host_util.h"
#include "mp3mi.h"

void mp3mi_launch_prep_tail(const mp3mi_tables *T, const mp3mi_geom &g, const double *xr, const mp3mi_psy_out *psy, mp3mi_loop_prep *prep,
                            mp3mi_prep_fixlist *fix, hipStream_t st);

static const double LD_XR_MAX = 0x1p64, LD_XR_MIN = 0x1p-500;
static const double LD_PE_MAX = 1e8;     // (int) (pe * 3.1 - mean_bits) stays an int (src/reservoir.c:117)
static const double LD_RATIO_MAX = 1e30; // xmin = ratio * energy / width, doubled 16 times and pre-emphasised (* 8), stays finite: 2^100 * 2^138 * 2^19

static inline int ld_nint(double in) { return (in < 0) ? (int) (in - 0.5) : (int) (in + 0.5); } // src/loop.c:2020

// one granule's 576 lines: 1 where every step the search can visit has its entry in the step table (see the head of the file)
static int ld_granule_ok(const double *xr)
{
    double sum1 = 0.0, sum2 = 0.0, amax = 0.0;
    for (int i = 0; i < 576; i++) {
        const double a = fabs(xr[i]);
        if (!(a <= LD_XR_MAX) || (a != 0.0 && a < LD_XR_MIN)) return 0; // (also catches NaN and the infinities)
        if (a != 0.0) {
            const double t = xr[i] * xr[i];
            sum1 += log(t);
            sum2 += t;
        }
        amax = a > amax ? a : amax;
    }
#if !defined(MP3MI_LOOP_DEBUG_NO_STEP_RULE) // (csrc never defines it: the stand-alone bounds check of tests/hipemu/loop_steps_main.cpp does)
    if (amax != 0.0) {
        const double v = 8.0 * log(exp(sum1 / 576.0) / (sum2 / 576.0));
        if (!(fabs(v) < 1e6)) return 0;
        const int q0_hi = ld_nint(v + 1e-6 * (fabs(v) > 1.0 ? fabs(v) : 1.0)) - 70;
        const int q_zero = (int) ceil(4.0 * (log2(amax) + 9.5 + 1.05));
        const int reach = q0_hi > q_zero ? q0_hi : q_zero;
        if (reach > MP3MI_STEP_MIN + MP3MI_STEP_N - 1) return 0;
    }
#endif
    return 1;
}

extern "C" int mp3mi_debug_iteration_loop(int rate_hz, int channels, int crc, int n_streams, int n_frames, const int32_t *kbps,
                                          const double *xr, const void *psy_v, const void *state_in, int16_t *ix, void *side,
                                          void *state_out, int32_t *n_listed)
{
    if (!have_device()) return MP3MI_ERR_NO_DEVICE;
    const mp3mi_psy_out *psy = (const mp3mi_psy_out *) psy_v;
    const mp3mi_loop_state *st_in = (const mp3mi_loop_state *) state_in;
    const int ri = rate_idx_of(rate_hz);
    if (ri < 0 || (channels != 1 && channels != 2) || (crc & ~1) || n_streams <= 0 || n_streams > 4096 || n_frames <= 0 || n_frames > 64 ||
        !kbps || !xr || !psy || !ix || !side || !state_out || !n_listed)
        return MP3MI_ERR_ARG;
    const size_t S = (size_t) n_streams, nf = (size_t) n_frames, C = (size_t) channels, n_rec = S * 2 * nf * C;
    host_mem<int32_t> bits_h(S);
    int32_t *bits = bits_h.p;
    if (!bits) return MP3MI_ERR_NOMEM;
    bool legal = true;
    for (size_t s = 0; legal && s < S; s++) {
        if (!bitrate_index_of(3, kbps[s])) { legal = false; break; }
        bits[s] = frame_bits(1152, ri, kbps[s], 8);
        legal = (bits[s] - (32 + 16 * crc + (channels == 1 ? 136 : 256))) / 2 / channels > 0;
        if (st_in) { // src/reservoir.c:45-93: the reservoir's size is the back pointer's bytes, within what the frame length leaves
            const mp3mi_loop_state &t = st_in[s];
            int ResvMax = bits[s] > 7680 ? 0 : 7680 - bits[s];
            if (ResvMax > 4088) ResvMax = 4088;
            legal = legal && t.ResvSize >= 0 && t.ResvSize <= ResvMax && t.ResvSize % 8 == 0 && t.ref_abort == 0;
            for (int i = 0; legal && i < 12; i++) legal = (&t.addr[0][0][0])[i] >= 0 && (&t.addr[0][0][0])[i] <= 576;
            // (calc_scfsi adds up to 21 differences of the stored integer logarithms.  sc_xrmax is only ever compared with 0 and
            // may hold anything: it is (int) max |xr|, a cast that is out of range for a legal spectrum above 2^31 -- the device
            // saturates, x86 gives INT_MIN -- so a state_out may carry either)
            for (int i = 0; legal && i < 4 + 84 + 84; i++) legal = abs((&t.sc_en_tot[0][0])[i]) <= (1 << 20);
        }
    }
    for (size_t r = 0; legal && r < n_rec; r++) {
        const mp3mi_psy_out &p = psy[r];
        legal = p.pe >= 0.0 && p.pe <= LD_PE_MAX && p.block_type >= 0 && p.block_type <= 3; // (a NaN fails both comparisons)
        for (int b = 0; legal && b < 21; b++) legal = p.ratio_l[b] >= 0.0 && p.ratio_l[b] <= LD_RATIO_MAX;
        for (int b = 0; legal && b < 36; b++) legal = (&p.ratio_s[0][0])[b] >= 0.0 && (&p.ratio_s[0][0])[b] <= LD_RATIO_MAX;
        legal = legal && ld_granule_ok(xr + r * 576);
    }
    if (!legal) return MP3MI_ERR_ARG;
    host_mem<mp3mi_tables> Th(1);
    const int trc = tables_into(Th, ri);
    if (trc != MP3MI_OK) return trc;
    hook_bufs D;
    const mp3mi_tables *dT = D.copy_of(Th.p, 1);
    // (a record more than the launch has behind the spectrum, the records and the quantised values, as format_debug.cpp leaves one)
    const double *dxr = D.copy_of(xr, n_rec * 576, 576);
    const mp3mi_psy_out *dpsy = D.copy_of(psy, n_rec, 1);
    mp3mi_loop_prep *dprep = D.zeros<mp3mi_loop_prep>(n_rec + 1);
    mp3mi_prep_fixlist *dfix = (mp3mi_prep_fixlist *) D.zeros<uint8_t>(mp3mi_prep_fixlist_bytes(n_rec + 1));
    const int32_t *dbits = D.copy_of(bits, S);
    mp3mi_loop_state *dstate = st_in ? D.copy_of(st_in, S) : D.zeros<mp3mi_loop_state>(S);
    int16_t *dix = D.zeros<int16_t>((n_rec + 1) * 576);
    mp3mi_frame_side *dside = D.zeros<mp3mi_frame_side>(S * nf + 1);
    if (!D.ok) return D.rc();
    // the three launches of the drop-in iteration_loop (dropin.cpp, frame_chain_launch), for all streams and frames at once
    mp3mi_geom g = mp3mi_make_geom(n_streams, channels, ri, n_frames, 0, n_frames);
    g.crc = crc;
    mp3mi_launch_prep_tail(dT, g, dxr, dpsy, dprep, dfix, 0);
    mp3mi_launch_prep(dT, g, dxr, dpsy, dprep, dfix, 0, 0);
    mp3mi_launch_loop(dT, g, dxr, dpsy, dprep, dbits, (void *) dstate, dix, dside, NULL, mp3mi_loop_place{NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0}, 0);
    unsigned listed = 0;
    D.sync();
    D.fetch(ix, dix, n_rec * 576);
    D.fetch((mp3mi_frame_side *) side, dside, S * nf);
    D.fetch((mp3mi_loop_state *) state_out, dstate, S);
    if (D.fetch(&listed, &dfix->count, 1)) *n_listed = (int32_t) listed;
    return D.rc();
}
