// The quantise+count pass of the iteration loop -- the quantiser, the Huffman table choice and the bit count -- with the
// structures it works on: what k_loop.hip (the search) and k_loop_qc.hip (the self-test hooks) share.  Device code only;
// each of the two translation units includes it once.
#ifndef MP3MI_LOOP_PASS_H
#define MP3MI_LOOP_PASS_H
#include "mp3mi_host.h"
#include "dmath.h"
#include "mp3mi.h"
#include <stdlib.h>

struct loop_gr { // wave-uniform working copy of gr_info (src/l3side.h:60-87)
    int part2_3_length, big_values, count1, scalefac_compress;
    int wsf, block_type, table_select[3], region0_count, region1_count;
    int preflag, count1table_select, part2_length;
    int sfb_lmax, sfb_smax, address1, address2, address3, q;
};

// 7.7 KB per wavefront plus one 1.9 KB copy of the code-length tables per workgroup of LOOP_W = 4 wavefronts: the 16
// wavefronts per CU that 4096 streams on 256 CUs need take 131 KB of its 160 KB of LDS (k_filter's three workgroups of 8.7 KB fit beside them), and at 80 VGPRs 320 of a SIMD's
// 512 registers -- the feed-forward kernels of the next chunk find room beside them (batch.cpp).
struct loop_lds {
    double xr[576 + 2] __attribute__((aligned(16))); // the granule's spectrum (amplified in place; [576] = [577] = 0: the pair a finished noise job
                      // reads on, ix[576] = ix[577] = 0 too): kept here, not in registers, because the
                      // quantise/count passes only need |xr|^(3/4) (registers) and the 18 VGPRs decide
                      // between 4 wavefronts per SIMD with and without scratch spills
    int16_t ix[576 + 128] __attribute__((aligned(4))); // padded: the region walks read whole 64-pair steps and mask what lies past the end; pair p as one word
    int sf_gr0[2][21];
    // per-band state of the distortion loop, lane b = band b (long) / sfb * 3 + window (short): it is touched once per
    // iteration, between two runs of quantise+count passes, and lives here -- not in registers -- across them
    double band_xmin[36]; // allowed distortion (calc_xmin, doubled / pre-emphasised along the way)
    int band_sf[36];      // scalefactors of the iteration in progress
    int band_sfsave[36];  // and of the last iteration whose result stands (src/loop.c:505-519)
    mp3mi_loop_state st;
    // long / start / stop blocks, lane < 32: the peak line of cell `lane` -- the line of the cell whose quantised value is the cell's largest
    // in every pass (mp3mi_dev.h, peak cells; loop_count_bits); lanes 32..63: 1024 | lane & 1 (loop_stream sets them once)
    uint16_t peak[64];
    // of the frame's side information only what a later granule or the end of the frame reads back; the records
    // themselves go straight to memory
    int p23[2][2];      // part2_3_length (ResvFrameEnd adds the stuffing bits, src/reservoir.c:190-224)
    int preflag0[2];    // granule 0's preflag (src/loop.c:1172-1176)
};

// The reference DIES on some inputs (an assert fails: tests/golden/coverage_notes.json, "reference_aborts").  A batch cannot
// die for one stream: the first such event is recorded in the stream's state (code | frame index << 8; wave-uniform, so
// it lives in a scalar register until the state goes back to memory), the search goes on with something harmless, and
// k_format / k_stream_tail void the stream's output (mp3mi.h, mp3mi_batch_stream_status).
#define LOOP_REF_ABORT(code, frame) do { if (ref_abort == 0) ref_abort = MP3MI_DEV_STATUS(code, frame); } while (0)

// Wavefronts (streams) per workgroup.  They share nothing but the code-length tables in LDS (1.9 KB that every stream
// would otherwise hold a copy of) and synchronise only per wavefront.
#define LOOP_W 4

// one entry per lane, read with wave_readlane_i32(reg, uniform index)
struct loop_regs {
    int desc_a;  // lane < 27: Huffman group descriptor of region maximum class `lane` (see loop_desc_index)
    int desc_b;  // lane < 27: offset of that group's cells in glut
};

__device__ static const int LOOP_PRETAB[21] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 3, 2};
// slen1 / slen2 of scalefac_compress k (src/loop.c:746-747: {0,0,0,0,3,1,1,1,2,2,2,3,3,3,4,4} and
// {0,1,2,3,0,1,2,3,1,2,3,1,2,3,2,3}) as nibble k of an immediate: a table in memory would be a dependent scalar
// load on the path between two passes
MP3MI_DEVFN int loop_slen1(int k) { return (int) ((0x4433322211130000ull >> (4 * k)) & 15ull); }
MP3MI_DEVFN int loop_slen2(int k) { return (int) ((0x3232132132103210ull >> (4 * k)) & 15ull); }

// Diagnostic build only (-DMP3MI_LOOP_PROFILE): cycles per phase, summed over all waves.
#if defined(MP3MI_LOOP_PROFILE) && !defined(MP3MI_EMU)
__device__ unsigned long long g_loop_prof[8];
__device__ unsigned long long g_loop_wave[2 * 65536];
__device__ unsigned long long g_loop_start[65536];
__device__ unsigned long long g_loop_work[65536]; // per stream: cycles from first to last instruction, HW_ID
__device__ unsigned long long g_cb_prof[8]; // phases inside loop_count_bits
#define CBPROF_ARG , unsigned long long *cbp
#define CBPROF_PASS , cb_acc
#define CBPROF_START unsigned long long cb_t = __builtin_amdgcn_s_memtime()
#define CBPROF(i) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); cbp[i] += n_ - cb_t; cb_t = n_; } while (0)
#define PROF_DECL unsigned long long cb_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long prof_t = __builtin_amdgcn_s_memtime(), prof_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; if (wave_lane() == 0 && block < 65536) g_loop_start[block] = __builtin_amdgcn_s_memrealtime()
#define PROF(i) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); prof_acc[i] += n_ - prof_t; prof_t = n_; } while (0)
#define PROF_END do { if (lane == 0) { for (int i_ = 0; i_ < 8; i_++) { atomicAdd(&g_loop_prof[i_], prof_acc[i_]); atomicAdd(&g_cb_prof[i_], cb_acc[i_]); } \
    if (s < 65536) { unsigned long long tot_ = 0; for (int i_ = 0; i_ < 8; i_++) tot_ += prof_acc[i_]; g_loop_wave[2 * s] = tot_; \
    g_loop_wave[2 * s + 1] = (unsigned long long) __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) | ((unsigned long long) __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) << 32); } } } while (0)
#else
#define PROF_DECL
#define PROF(i)
#define PROF_END
#define CBPROF_ARG
#define CBPROF_PASS
#define CBPROF_START
#define CBPROF(i)
#endif

MP3MI_DEVFN int loop_nint(double in) { return (in < 0) ? (int) (in - 0.5) : (int) (in + 0.5); } // src/loop.c:2020

// ---- quantiser: ix = max{p in [0,2047] : tab[p] <= x}  (src/pow_nint.h:15-49, src/loop.c:1360-1428) ----
// A float estimate of x^(3/4)+0.4054 settles every line that is not within 2^-9 of a table
// boundary; the others are settled against the exact table.  The result never depends on the
// quality of the estimate.  Leaves the values in p[] and in L.ix (followed by a barrier).
// y34[j] = |xr[j]|^(3/4) in float (loop_power34), so that x^(3/4) = y34 * 2^(-3q/16) costs one multiply per pass.
// Only an estimate (the quantiser settles borderline lines exactly), so the raw 1-ulp hardware
// square root is enough; the correctly rounded expansion costs ~20 instructions per root.
// (LOOP_FAST_SQRTF / LOOP_FAST_EXP2F: mp3mi_dev.h; their error on the device is measured by k_debug.hip,
// mp3mi_debug_fastmath_bounds, and asserted by tests/test_gpu_tiers.py)
// Returns the largest y34 of the granule (wave-uniform): a step size that quantises it to zero
// quantises everything to zero.
// ---- which lines a lane owns ----
// Lane l holds pairs l, l + 64, .. l + 256 (LOOP_SLOTS slots; the pairs from 288 on -- slot 4 of lanes 32..63 -- do not exist:
// their y34 is 0, they quantise to 0, and what is stored for them lands in L.ix's padding).  Value j of a lane is line
// 2 * (l + 64 * (j / 2)) + j % 2.
#define LOOP_SLOTS 5
#define LOOP_NV (2 * LOOP_SLOTS)
MP3MI_DEVFN int loop_pair_of(int lane, int k) { return lane + 64 * k; }

MP3MI_DEVFN float loop_power34(const double xr[LOOP_NV], float y34[LOOP_NV])
{
    float m = 0.0f;
#pragma unroll
    for (int j = 0; j < LOOP_NV; j++) {
        const float a = (float) __builtin_fabs(xr[j]);
        y34[j] = LOOP_FAST_SQRTF(a * LOOP_FAST_SQRTF(a));
        m = y34[j] > m ? y34[j] : m;
    }
    return __builtin_bit_cast(float, wave_max_i32(__builtin_bit_cast(int, m))); // non-negative floats order like their bits
}

// |xr * sqrt(2)^n|^(3/4) = y34 * 2^(3n/8): when a band is amplified (n = 1) or pre-emphasised (n = pretab)
// the cached power is rescaled instead of taking two roots again.  One float rounding of the
// constant and one of the product per call: < 1.2e-7 relative (the quantiser's guard band budgets it).
MP3MI_DEVFN float loop_rescale34(float y34, int n)
{
    const float c = n == 1 ? 1.2968395546510096f : (n == 2 ? 1.681792830507429f : (n == 3 ? 2.1810154653305154f : 1.0f));
    return y34 * c;
}
// upper bound of the largest y34 after such a rescaling (the all-zero shortcut of the bisection reads it, which runs
// before the first amplification, and the quantiser, to know that no line reaches the table's end: loop_quantize)
#define LOOP_Y34MAX_GROW 2.1810157f
#define LOOP_Y34MAX_AMP 1.29684f /* one amplification (n = 1) */

// Pre-emphasis of the lane's lines (src/loop.c:1161-1214, what it does to the spectrum): the pairs of band b < sfb_lmax are
// multiplied by sqrt(2)^pretab[b] in L.xr, and their cached powers with them.  Long blocks only: a pair is of one band, six
// bits per slot in bandpack's low word.  The caller grows y34max (LOOP_Y34MAX_GROW) and synchronises the wavefront.
MP3MI_DEVFN void loop_preemph_lines(const mp3mi_tables *T, loop_lds &L, float y34[LOOP_NV], unsigned long long bandpack, int lane, int sfb_lmax)
{
#pragma unroll
    for (int k = 0; k < LOOP_SLOTS; k++) {
        const int b = (int) (((unsigned) bandpack >> (6 * k)) & 63u); // (63: a pair that does not exist)
        const int line = 2 * loop_pair_of(lane, k);
        if (b < sfb_lmax) {
            const double f = T->pretab_xr[LOOP_PRETAB[b]];
            L.xr[line] = L.xr[line] * f;
            L.xr[line + 1] = L.xr[line + 1] * f;
            y34[2 * k] = loop_rescale34(y34[2 * k], LOOP_PRETAB[b]);
            y34[2 * k + 1] = loop_rescale34(y34[2 * k + 1], LOOP_PRETAB[b]);
        }
    }
}

// Amplification of the lane's lines in long / start / stop blocks (amp_scalefac_bands, src/loop.c:1225-1350, what it does to the
// spectrum): the pairs of the bands whose bit is set in amp32 are multiplied by ifqstep = sqrt(2) in L.xr.  A pair is of one
// band, six bits per slot in bandlo, and the 21 band lanes' mask is one word.  The caller grows y34max (LOOP_Y34MAX_AMP) and
// synchronises the wavefront.  (Short blocks, whose two lines of a pair may lie in different bands, are written out where they
// are needed: loop_stream, and a copy of it in k_loop_qc.hip.)
MP3MI_DEVFN void loop_amp_pairs(loop_lds &L, float y34[LOOP_NV], unsigned bandlo, unsigned amp32, double ifqstep, int lane)
{
#pragma unroll
    for (int k = 0; k < LOOP_SLOTS; k++) {
        const unsigned b = (bandlo >> (6 * k)) & 63u;
        const int line = 2 * loop_pair_of(lane, k);
        if (b < 32u && ((amp32 >> b) & 1u)) { // (a slot none of whose pairs is amplified: the branch over an empty execution mask)
            L.xr[line] = L.xr[line] * ifqstep;
            L.xr[line + 1] = L.xr[line + 1] * ifqstep;
            y34[2 * k] = y34[2 * k] * 1.2968395546510096f; // loop_rescale34(y34, 1)
            y34[2 * k + 1] = y34[2 * k + 1] * 1.2968395546510096f;
        }
    }
}

MP3MI_DEVFN float loop_estimate(float y34, float cq) { return __builtin_fmaf(y34, cq, 0.4054f); } // of x^(3/4) + 0.4054

// true: every line quantises to 0 at this step (wave-uniform).  loop_estimate is monotone in y34 and lies above the upper
// estimate the quantiser rounds (see loop_quantize: (1 + 3.5e-6) y34 cq + 0.4054 + 2e-6 < 0.999 + 3.5e-6 + 2e-6 < 1 <=> below 0.5 after
// the quantiser's - 0.5), so the quantiser would leave every line at 0 unflagged.
MP3MI_DEVFN bool loop_all_zero(float y34max, int q)
{
    return loop_estimate(y34max, LOOP_FAST_EXP2F(-0.1875f * (float) q)) < 0.999f;
}

// What a pass needs to know about the quantised values besides the values themselves (which go to L.ix): the run
// lengths of calc_runlen for long blocks, the two region maxima of short blocks.  Taken while every value is still
// in a register, so that the values of a lane are never alive across the counting.
struct loop_qinfo {
    int n_nz, n_big; // lines up to the last non-zero PAIR / the last pair with a value above 1 (2 * pairs: even; 0 = none)
    int m1, m2;      // short blocks: this lane's maximum over lines [0, 36) / [36, 576)
};

// The quantiser's first tier, two lines -- a pair -- at a time.  With t = x^(3/4) + 0.4054 the answer is floor(t) (clamped to the
// table's end).  u = y34 * cq + 0.4054 - 0.5 estimates t - 0.5 with an error below 2.8e-6 y34 cq relative (the two 1-ulp roots,
// exp2, the roundings, at most 17 rescalings of y34 by loop_rescale34: 16 amplifications, one pre-emphasis) plus the roundings of
// what is computed here (the constants' products and the multiply-add: 2e-7 relative).  An UPPER and a LOWER estimate
//     u_hi = y34 * cq (1 + 3.5e-6) + (0.4054 - 0.5 + 2e-6),   u_lo = y34 * cq (1 - 3.5e-6) + (0.4054 - 0.5 - 2e-6)
// bracket t - 0.5, and v_cvt_pknorm_u16_f32 -- on a / 65535 it returns a rounded to the NEAREST integer, computed from the exact
// product and clamped to [0, 65535] (every float of the range against double arithmetic: mp3mi_debug_pknorm_bound, k_debug.hip;
// tests/test_gpu_tiers.py) -- rounds both, a pair per instruction, straight into the halves of the pair word x | y << 16:
//     n_hi >= u_hi - 0.5 > t - 1  =>  n_hi >= floor(t);     n_lo <= u_lo + 0.5 < t  =>  n_lo <= floor(t)
// (n_lo < t gives n_lo <= floor(t) also for an integer t).  So a line whose two roundings agree is settled, whatever the quality
// of the estimate; the others -- those within the band of a table boundary: small values, the common case, almost never --
// are settled against the exact table.  Five instructions per pair: two packed multiply-adds, two conversions, one compare-accumulate.
// scale = 1 / 65535: the conversion's; the constants are rounded ONCE, here, by the compiler.
#define LOOP_Q_HI ((1.0 + 3.5e-6) / 65535.0)
#define LOOP_Q_LO ((1.0 - 3.5e-6) / 65535.0)
#define LOOP_Q_CHI ((0.4054 - 0.5 + 2e-6) / 65535.0)
#define LOOP_Q_CLO ((0.4054 - 0.5 - 2e-6) / 65535.0)
struct loop_qscale { float a_hi, a_lo; };
MP3MI_DEVFN loop_qscale loop_quant_scale(int q)
{
    const float cq = LOOP_FAST_EXP2F(-0.1875f * (float) q);
    loop_qscale s = {cq * (float) LOOP_Q_HI, cq * (float) LOOP_Q_LO};
    return s;
}
MP3MI_DEVFN unsigned loop_quant_pair(float y0, float y1, float a, float c)
{
#if defined(MP3MI_EMU)
    return LOOP_PKNORM_U16(__builtin_fmaf(y0, a, c), __builtin_fmaf(y1, a, c));
#else
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 y = {y0, y1}, av = {a, a}, cv = {c, c};
    const f32x2 u = __builtin_elementwise_fma(y, av, cv); // v_pk_fma_f32: both lines in one instruction
    return LOOP_PKNORM_U16(u.x, u.y);
#endif
}

// ix = max{p in [0,2047] : tab[p] <= x}  (src/pow_nint.h:15-49, src/loop.c:1360-1428) for the lane's ten lines: the pair
// words go to L.ix (followed by a barrier).  y34[j] = |xr[j]|^(3/4) in float (loop_power34), so that x^(3/4) = y34 * 2^(-3q/16)
// costs one multiply per pass.  Only an estimate (the quantiser settles borderline lines exactly), so the raw 1-ulp hardware
// square root is enough; the correctly rounded expansion costs ~20 instructions per root.
// (LOOP_FAST_SQRTF / LOOP_FAST_EXP2F: mp3mi_dev.h; their error on the device is measured by k_debug.hip,
// mp3mi_debug_fastmath_bounds, and asserted by tests/test_gpu_tiers.py)
// force_exact (MP3MI_QUANT_EXACT=1, tests): every line is settled against the exact table, whatever the estimate says.
MP3MI_DEVFN loop_qinfo loop_quantize(const mp3mi_tables *T, loop_lds &L, const float y34[LOOP_NV], float y34max, int q, bool all_zero, bool force_exact, bool shortb)
{
    const int lane = wave_lane_here();
    unsigned *ixw = (unsigned *) L.ix; // pair p as one word: x | y << 16
    loop_qinfo qi = {0, 0, 0, 0};
    if (all_zero && !force_exact) {
#pragma unroll
        for (int k = 0; k < LOOP_SLOTS; k++) ixw[loop_pair_of(lane, k)] = 0u;
        wave_sync();
        return qi;
    }
    unsigned pw[LOOP_SLOTS];
    const loop_qscale qs = loop_quant_scale(q);
    unsigned differ = 0u; // some line's upper and lower estimate round to different integers
#pragma unroll
    for (int k = 0; k < LOOP_SLOTS; k++) {
        pw[k] = loop_quant_pair(y34[2 * k], y34[2 * k + 1], qs.a_hi, (float) LOOP_Q_CHI);
        const unsigned lo = loop_quant_pair(y34[2 * k], y34[2 * k + 1], qs.a_lo, (float) LOOP_Q_CLO);
        differ += pw[k] ^ lo; // (five terms below 2^28: no overflow; v_xad_u32)
    }
    // The rare tier.  From 2047.5 on the answer is the table's last entry; whether any line gets there is known from the granule's
    // largest y34 (an upper bound, wave-uniform): almost never -- so the clamps are not in the pass but in here, where the
    // lines whose two estimates differ are settled against the exact table.
    const bool over = !(loop_estimate(y34max, qs.a_hi * 65535.0f) < 2047.0f);
    if (force_exact || over || wave_any(differ != 0u)) {
        const double ostep = 1.0 / T->step[q - MP3MI_STEP_MIN];
#pragma unroll
        for (int j = 0; j < LOOP_NV; j++) {
            const int k = j >> 1, sh = 16 * (j & 1);
            // (the lower estimate again, here: nothing of it lives through the common path)
            unsigned lo = (loop_quant_pair(y34[2 * k], y34[2 * k + 1], qs.a_lo, (float) LOOP_Q_CLO) >> sh) & 0xffffu;
            int pp = (int) ((pw[k] >> sh) & 0xffffu);
            lo = lo < 2047u ? lo : 2047u;
            pp = pp < 2047 ? pp : 2047;
            const int line = 2 * loop_pair_of(lane, k) + (j & 1);
            if ((force_exact || lo != (unsigned) pp) && line < 576) {
                const double x = __builtin_fabs(L.xr[line]) * ostep;
                while (pp > 0 && x < T->pow_nint_tab[pp]) pp--;
                while (pp < 2047 && x >= T->pow_nint_tab[pp + 1]) pp++;
            }
            pw[k] = (pw[k] & ~(0xffffu << sh)) | ((unsigned) pp << sh);
        }
    }
#pragma unroll
    for (int k = 0; k < LOOP_SLOTS; k++) ixw[loop_pair_of(lane, k)] = pw[k];
    // Run lengths (calc_runlen, src/loop.c:1488-1520), by pairs: big_values and count1 only ask for the last PAIR that holds a
    // non-zero value / a value above 1 (loop_count_bits).  And the short-block maxima.
    if (shortb) { // (a short block's big_values is 288 whatever the values: no run lengths)
#pragma unroll
        for (int k = 0; k < LOOP_SLOTS; k++) {
            const int x = (int) (pw[k] & 0xffffu), y = (int) (pw[k] >> 16);
            const int v = x > y ? x : y;
            const bool low = loop_pair_of(lane, k) < 18; // lines [0, 36)
            qi.m1 = (low && v > qi.m1) ? v : qi.m1;
            qi.m2 = (!low && v > qi.m2) ? v : qi.m2;
        }
    } else {
        // min(x, 2) | min(y, 2) of the lane's five pairs as 2-bit fields of one word, slot k in bits 2k, 2k + 1: its highest set bit
        // names the lane's last non-zero pair, the highest set ODD bit its last pair with a value above 1.
        // (both halves of a pair word clamped to 2 by ONE packed instruction, the five words shifted together while x and y are
        // still apart -- the x codes in bits 0..9, the y codes in bits 16..25 --, then one OR of the halves: a field reads 0, 1, 2 or 3,
        // 3 = one value 1 beside one above 1, which the two questions below answer as they answer 2)
        const mp3mi_u16x2 two2 = {2, 2};
        unsigned wp = __builtin_bit_cast(unsigned, LOOP_PK_MIN_U16(__builtin_bit_cast(mp3mi_u16x2, pw[0]), two2));
#pragma unroll
        for (int k = 1; k < LOOP_SLOTS; k++)
            wp |= __builtin_bit_cast(unsigned, LOOP_PK_MIN_U16(__builtin_bit_cast(mp3mi_u16x2, pw[k]), two2)) << (2 * k);
        const unsigned w = (wp & 0xffffu) | (wp >> 16);
        // ONE reduction -- the OR of the words names the last slot that holds a non-zero pair / a pair with a value above 1 -- and a
        // lane mask per run length for the last lane of that slot.
        const unsigned wo = wave_or_u32(w);
        const int t_nz = 31 - __clz((int) wo), t_big = 31 - __clz((int) (wo & 0x2AAu)); // -1 for an empty word
        const int k_nz = t_nz >> 1, k_big = t_big >> 1;
        const unsigned long long m_nz = __ballot((w & (3u << ((2 * k_nz) & 31))) != 0u), m_big = __ballot((w & (2u << ((2 * k_big) & 31))) != 0u);
        qi.n_nz = t_nz < 0 ? 0 : 2 * (64 * k_nz + 64 - __clzll((long long) m_nz));
        qi.n_big = t_big < 0 ? 0 : 2 * (64 * k_big + 64 - __clzll((long long) m_big));
    }
    wave_sync();
    return qi;
}

// ---- Huffman table choice and code-length look-up, grouped ----
// new_choose_table (src/loop.c:1793-1897) only ever compares tables of one "group": {1},
// {2,3}, {5,6}, {7,8,9}, {10,11,12}, {13,15}, {15,24+}, {16+,24+}; within a group all tables have
// the same geometry.  The group is a function of the region maximum alone:
//   max < 16        -> entry max        of the descriptor table
//   max >= 16       -> entry 15 + bit length of (max - 15)   (the ht[].linmax thresholds of
//                      src/loop.c:1872-1888 are all of the form 2^k - 1)
// R.desc_a / R.desc_b hold that table one entry per lane (built in tables_host.cpp):
//   desc_a = c0 | c1 << 5 | c2 << 10 | ylen << 15 | linbits(c0) << 20 | linbits(c1) << 24
//   desc_b = offset of the group's cells in T->glut
// T->glut holds, per group and (x,y) cell, the code lengths of all its tables packed 5 bits
// each, so ONE LDS read prices a pair for every candidate.
#define GL_C1 897 /* count1 tables A | B << 5 */

MP3MI_DEVFN int loop_desc_index(int max)
{
    return max < 16 ? max : 15 + (32 - __clz(max - 15));
}

// descriptor of class `cls` (run once per wave, lane = cls): the candidate searches over ht[].xlen
// and ht[].linmax of src/loop.c:1812-1817, 1872-1888, 1919-1939 written as comparisons
MP3MI_DEVFN void loop_desc_init(const mp3mi_tables *T, int cls, int *desc_a, int *desc_b)
{
    *desc_a = 0;
    *desc_b = 0;
    if (cls == 0 || cls > 26) return;
    const int max = cls < 16 ? cls : 15 + (1 << (cls - 16));
    int c0, c1 = 0, c2 = 0, off, ylen;
    if (max < 15) {
        if (max <= 1) { c0 = 1; off = 0; ylen = 2; }
        else if (max == 2) { c0 = 2; c1 = 3; off = 4; ylen = 3; }
        else if (max == 3) { c0 = 5; c1 = 6; off = 13; ylen = 4; }
        else if (max <= 5) { c0 = 7; c1 = 8; c2 = 9; off = 29; ylen = 6; }
        else if (max <= 7) { c0 = 10; c1 = 11; c2 = 12; off = 65; ylen = 8; }
        else { c0 = 13; c1 = 15; off = 129; ylen = 16; }
    } else {
        const int m = max - 15;
        c0 = m <= 0 ? 15 : (m <= 1 ? 16 : (m <= 3 ? 17 : (m <= 7 ? 18 : (m <= 15 ? 19 : (m <= 63 ? 20 : (m <= 255 ? 21 : (m <= 1023 ? 22 : 23)))))));
        c1 = m <= 15 ? 24 : (m <= 31 ? 25 : (m <= 63 ? 26 : (m <= 127 ? 27 : (m <= 255 ? 28 : (m <= 511 ? 29 : (m <= 2047 ? 30 : 31))))));
        off = c0 == 15 ? 385 : 641;
        ylen = 16;
    }
    *desc_a = c0 | (c1 << 5) | (c2 << 10) | (ylen << 15) | ((int) T->ht_linbits[c0] << 20) | ((int) T->ht_linbits[c1] << 24);
    *desc_b = off;
}

// code lengths of pair (x, y), sign bits included (glut) and the linbits of src/loop.c:172-225 added,
// for the (up to) three tables of a group, spread to 10-bit fields.
// da/db: the group's descriptor words (may differ per lane).
MP3MI_DEVFN int loop_pair_cost3(const uint16_t *GL, int da, int db, int x, int y)
{
    const int xc = x > 15 ? 15 : x, yc = y > 15 ? 15 : y;
    const int nesc = (x > 14) + (y > 14);
    const int ylen = (da >> 15) & 31, lb = ((da >> 20) & 15) | (((da >> 24) & 15) << 10);
    const int e = GL[db + xc * ylen + yc];
    const int spread = (e & 31) | (((e >> 5) & 31) << 10) | (((e >> 10) & 31) << 20);
    return spread + nesc * lb;
}

// new_choose_table's decision from the candidates' bit sums (src/loop.c:1819-1897): '<=' moves to the later table among
// tables without linbits, '<' among the linbits pair -- taken on values that live in ONE LANE of vector registers (the sums as the reduction leaves them): the
// descriptor is taken into a vector register too, so that every instruction of the decision is a vector one.
// s01 = candidate 0's sum | candidate 1's << 16.  NC3: some region of the pass has a third candidate.
template <bool NC3>
MP3MI_DEVFN int loop_pick_v(int da, int s01, int s2, int *sum)
{
    int dav = da;
#if !defined(MP3MI_EMU)
    asm volatile("" : "+v"(dav));
#endif
    const int c0 = dav & 31, c1 = (dav >> 5) & 31;
    const int s0 = s01 & 0xffff, s1 = (int) ((unsigned) s01 >> 16);
    // the linbits pair compares with '<' (s1 + 1 <= s0), the others with '<='; no second candidate: never
    const int t1 = c1 ? s1 + (c0 >= 15 ? 1 : 0) : 0x7fffffff;
    const bool take1 = t1 <= s0;
    int best = take1 ? s1 : s0, choice = take1 ? c1 : c0;
    if (NC3) {
        const int c2 = (dav >> 10) & 31;
        const int t2 = c2 ? s2 : 0x7fffffff;
        const bool take2 = t2 <= best;
        best = take2 ? s2 : best;
        choice = take2 ? c2 : choice;
    }
    *sum = best;
    return choice;
}

// Cost of the pairs of lines [lo, hi) under the candidate tables of one group (descriptor dA/dB), per lane:
// *a01 = candidate 0 | candidate 1 << 16, *a2 = third candidate.  Walks 64 pairs per step straight out of
// L.ix.  ESC: the group's tables have linbits (x or y > 14 then costs them); NC3: it has a third candidate.
// (k15: the constant 15 in a scalar register -- loop_walk_consts --: compiled without the machine-level hoisting of loop
// invariants, a step would otherwise set it up again, in a vector register)
struct loop_walk_k { int k15; unsigned m1f; };
MP3MI_DEVFN loop_walk_k loop_walk_consts(void)
{
    loop_walk_k k = {15, 0x1f001fu};
#if !defined(MP3MI_EMU)
    asm volatile("" : "+s"(k.k15), "+s"(k.m1f));
#endif
    return k;
}
// byte address of the cell of pair word xy = x | y << 16 in a group whose values stay below 16: x * ylen2 + 2 y + dB2, as two
// multiply-adds that read the halves of the word where they lie (no unpacking, no clamp)
MP3MI_DEVFN unsigned loop_cell_of_word(unsigned xy, int ylen2, int dB2)
{
#if defined(MP3MI_EMU)
    return (xy & 0xffffu) * (unsigned) ylen2 + 2u * (xy >> 16) + (unsigned) dB2;
#else
    unsigned idx; // (one statement: between two the compiler puts a wait state it cannot know to be unnecessary)
    asm("v_mad_u32_u16 %0, %1, 2, %2 op_sel:[1,0,0,0]\n\tv_mad_u32_u16 %0, %1, %3, %0" : "=&v"(idx) : "v"(xy), "s"(dB2), "s"(ylen2));
    return idx;
#endif
}
// A step of a walk: the 64 pairs [w, w + 64) of a region, a pair word xy per lane, in the two halves that each follow an LDS read -- the
// cell's address from the pair word, the sums from the cell.  LAST: the region's last step, which can reach past its end -- `inside`
// says whether this lane's pair still belongs to it; the others are priced as some cell all the same and masked out of the sums (a
// conditional load costs three scalar instructions and two branches per step).
template <bool ESC, bool LAST>
MP3MI_DEVFN unsigned loop_walk_cell(unsigned xy, bool inside, int ylen2, int dB2, const loop_walk_k &K)
{
    unsigned at;
    if (ESC) { // values above 15 occur: clamped (which also keeps a pair past the end inside the table, whatever the padding holds)
        const int x = (int) (xy & 0xffffu), y = (int) (xy >> 16);
        const int xc = x > K.k15 ? K.k15 : x, yc = y > K.k15 ? K.k15 : y;
        unsigned cell = 2u * (unsigned) yc + (unsigned) dB2; // (kept apart: re-associated, the sum takes three instructions instead of two)
#if !defined(MP3MI_EMU)
        asm volatile("" : "+v"(cell));
        at = (unsigned) __umul24((unsigned) xc, (unsigned) ylen2) + cell; // (xc <= 15: a 24-bit multiply-add)
#else
        at = (unsigned) (xc * ylen2) + cell;
#endif
    } else { // the region's maximum is below 16: so is every value in it -- only a pair PAST its end can be larger, and counts as (0, 0)
        if (LAST) xy = inside ? xy : 0u;
        at = loop_cell_of_word(xy, ylen2, dB2);
    }
    return at;
}
template <bool ESC, bool NC3, bool LAST>
MP3MI_DEVFN void loop_walk_add(unsigned e, bool inside, int lb01, const loop_walk_k &K, int &s01, int &s2)
{
    if (LAST) e = inside ? e : 0u;
    int c = (int) (((e << 11) | e) & K.m1f); // candidate 0's length | candidate 1's << 16: a shift-or and a mask
    if (ESC) c += (int) ((e >> 10) & 3u) * lb01; // (how many of x, y are escapes: in the cell, tables_host.cpp)
    s01 += c;
    if (NC3) s2 += (int) (e >> 10); // (a cell's bit 15 is clear: the third length needs no mask)
}
template <bool ESC, bool NC3, bool LAST>
MP3MI_DEVFN void loop_walk_step(const uint16_t *GL, unsigned xy, bool inside, int ylen2, int dB2, int lb01, const loop_walk_k &K, int &s01, int &s2)
{
    const unsigned at = loop_walk_cell<ESC, LAST>(xy, inside, ylen2, dB2, K);
    loop_walk_add<ESC, NC3, LAST>(*(const uint16_t *) ((const char *) GL + at), inside, lb01, K, s01, s2);
}

// A region of N steps, the last one masked, as TWO trips to LDS and not two per step: every pair word is asked for before the first
// cell address is formed, every cell before the first sum.  The instructions are the steps' own, in another order, less the tests
// between the steps; the compiler joins pair reads and the steps' sums.  What the step gains by is those fewer instructions -- the
// waits it saves pass under the other wavefronts' instructions either way (profiles/r13_experiments.txt, K2-K5).
template <bool ESC, bool NC3, int N>
MP3MI_DEVFN void loop_walk_n(const uint16_t *GL, const unsigned *p, int lane, int rest, int ylen2, int dB2, int lb01, const loop_walk_k &K, int &s01, int &s2)
{
    unsigned xy[N], at[N], e[N];
#pragma unroll
    for (int k = 0; k < N; k++) xy[k] = p[64 * k];
    const bool inside = lane < rest; // of the last step: 1 .. 64 pairs
#pragma unroll
    for (int k = 0; k < N - 1; k++) at[k] = loop_walk_cell<ESC, false>(xy[k], true, ylen2, dB2, K);
    at[N - 1] = loop_walk_cell<ESC, true>(xy[N - 1], inside, ylen2, dB2, K);
#pragma unroll
    for (int k = 0; k < N; k++) e[k] = *(const uint16_t *) ((const char *) GL + at[k]);
#pragma unroll
    for (int k = 0; k < N - 1; k++) loop_walk_add<ESC, NC3, false>(e[k], true, lb01, K, s01, s2);
    loop_walk_add<ESC, NC3, true>(e[N - 1], inside, lb01, K, s01, s2);
}

MP3MI_DEVFN int loop_opaque_s(int v) // a wave-uniform value the compiler knows nothing about
{
#if !defined(MP3MI_EMU)
    asm volatile("" : "+s"(v));
#endif
    return v;
}

template <bool ESC, bool NC3>
MP3MI_DEVFN void loop_region_walk(const uint16_t *GL, const unsigned *ixw, int lane, int lo, int hi, int dA, int dB, const loop_walk_k &K, int *a01, int *a2)
{
    const int ylen2 = 2 * ((dA >> 15) & 31), dB2 = 2 * dB, lb01 = ((dA >> 20) & 15) | (((dA >> 24) & 15) << 16);
    int s01 = 0, s2 = 0;
    const unsigned *p = ixw + (lo >> 1) + lane; // this lane's pair of the first step
    // Steps of 64 pairs, every step at a constant offset from the lane's first pair; the last one is masked -- pairs past the end of
    // the region are read all the same (L.ix is padded) and left out of the sums.  One to four steps (a long block's regions: at most
    // 221 pairs) are written out by their number, reads first (loop_walk_n); the fifth that region 1 of a start / stop block can
    // take follows step by step.  The number of steps is never formed: the region's pairs are compared with the step boundaries,
    // one step -- regions 0 and 1 of every long block -- first, and what is left of them for the last step is its mask.
    // (the count behind an optimisation barrier after the first test: the chain of tests stays a chain of scalar branches, where the
    // compiler would build a switch and then flags to leave it by)
    int np = hi > lo ? (hi - lo) >> 1 : 0; // (lo, hi even; a walk only runs on a region that holds a value: lo < hi)
    if (__builtin_expect(np <= 64, 1)) loop_walk_n<ESC, NC3, 1>(GL, p, lane, np, ylen2, dB2, lb01, K, s01, s2);
    else {
        np = loop_opaque_s(np);
        if (np <= 128) loop_walk_n<ESC, NC3, 2>(GL, p, lane, np - 64, ylen2, dB2, lb01, K, s01, s2);
        else {
            if (np <= 192) loop_walk_n<ESC, NC3, 3>(GL, p, lane, np - 128, ylen2, dB2, lb01, K, s01, s2);
            else { // (a fifth step: the fourth is whole)
                loop_walk_n<ESC, NC3, 4>(GL, p, lane, np - 192, ylen2, dB2, lb01, K, s01, s2);
                if (np > 256) loop_walk_step<ESC, NC3, true>(GL, p[256], lane < np - 256, ylen2, dB2, lb01, K, s01, s2);
            }
        }
    }
    *a01 = s01;
    *a2 = s2;
}

MP3MI_DEVFN void loop_region_cost(const uint16_t *GL, const unsigned *ixw, int lane, int lo, int hi, int m, int dA, int dB, const loop_walk_k &K, int *a01, int *a2)
{
    *a01 = 0;
    *a2 = 0;
    if (m == 0) return; // no table, no bits (src/loop.c:1771-1777)
    const bool esc = (dA >> 20) != 0, nc3 = ((dA >> 10) & 31) != 0; // tables with linbits never come in threes
    if (esc) loop_region_walk<true, false>(GL, ixw, lane, lo, hi, dA, dB, K, a01, a2);
    else if (nc3) loop_region_walk<false, true>(GL, ixw, lane, lo, hi, dA, dB, K, a01, a2);
    else loop_region_walk<false, false>(GL, ixw, lane, lo, hi, dA, dB, K, a01, a2);
}

// calc_runlen + count1_bitcount + subdivide + bigv_tab_select + bigv_bitcount
// (src/loop.c:1488-2014) on the freshly quantised values (pair words in registers, L.ix in LDS).
// Returns the Huffman bit count and fills g.  Written branch-free over the lanes: region
// membership is a predicate, never a divergent branch.
MP3MI_DEVFN int loop_count_bits(const mp3mi_tables *T, const loop_regs &R, loop_lds &L, const uint16_t *GL, loop_gr &g, const loop_qinfo &qi, bool all_zero CBPROF_ARG)
{
    CBPROF_START;
    const int lane = wave_lane_here();
#if defined(LOOP_EXP_SALU) && !defined(MP3MI_EMU) // experiment (profiles/r06_experiments.txt, F6): what does a pass pay for N more scalar / vector instructions?
    { int t_ = 0;
#pragma unroll
      for (int i_ = 0; i_ < LOOP_EXP_SALU; i_++) asm volatile("s_add_u32 %0, %0, 1" : "+s"(t_) : : "scc"); }
#endif
#if defined(LOOP_EXP_VALU) && !defined(MP3MI_EMU)
    { int t_ = lane;
#pragma unroll
      for (int i_ = 0; i_ < LOOP_EXP_VALU; i_++) asm volatile("v_add_u32_e32 %0, 1, %0" : "+v"(t_)); }
#endif
#if defined(LOOP_EXP_VALU3) && !defined(MP3MI_EMU)
    { int t_ = lane;
#pragma unroll
      for (int i_ = 0; i_ < LOOP_EXP_VALU3; i_++) asm volatile("v_add3_u32 %0, %0, %0, 1" : "+v"(t_)); }
#endif
    const bool shortb = g.wsf && g.block_type == 2;
    const unsigned *ixw = (const unsigned *) L.ix; // (x, y) of pair pr as one word: x | y << 16
    int bits = 0, nslot = 9; // nslot: slots (of 64 lines) that can hold a non-zero value
    int c1part = 0;          // this lane's part of the count1 region's bits: table A | table B << 16
    if (shortb) {
        g.count1 = 0;
        g.big_values = 288;
        g.count1table_select = 1; // count1_bitcount with no quadruples: sum0 == sum1 -> table B
    } else if (all_zero) {
        g.count1 = 0;
        g.big_values = 0;
        g.count1table_select = 1;
        nslot = 0;
    } else {
        const int hh[2] = {qi.n_nz, qi.n_big}; // from the quantiser, taken while the values were in registers
        // hh[0] = n: lines up to the last non-zero one, hh[1] = b <= n: lines up to the last one above 1.  The
        // reference's i = 2 * (top / 2 + 1) is n rounded up to even (0 for n = 0); everything is non-negative,
        // so the divisions are shifts (src/loop.c:1488-1520)
        const unsigned n_nz = (unsigned) hh[0], n_big = (unsigned) hh[1];
        nslot = (int) ((n_nz + 63u) >> 6);
        const unsigned i0 = (n_nz + 1u) & ~1u;
        const unsigned c1 = (i0 - n_big) >> 2;
        g.count1 = (int) c1;
        g.big_values = (int) ((i0 - 4u * c1) >> 1);
        // count1 region: table A vs table B (values are 0/1, so v+2w+4x+8y comes from two words)
        int s01 = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) { // at most 144 quadruples
            if (64 * k >= g.count1) break;
            const int qd = lane + 64 * k;
            const bool in = qd < g.count1;
            // (quadruples past the end are read all the same -- still inside this wavefront's LDS -- and masked out of the sum)
            const int w0 = g.big_values + 2 * qd;
            const unsigned a = ixw[w0], b = ixw[w0 + 1];
            // values 0 / 1 in the four halves of two words: v | w << 16 and x | y << 16 -> v + 2 w + 4 x + 8 y in three instructions
            const unsigned t = a | (b << 2);
            const int pp = (int) ((t | (t >> 15)) & 15u);
            const int e = GL[GL_C1 + pp]; // code length + sign bits: table A | table B << 5
            const int c = (e & 31) | ((e >> 5) << 16);
            s01 += in ? c : 0;
        }
        c1part = s01; // reduced further down, together with the region maxima
    }
    CBPROF(0); // run lengths + count1 region
    // subdivide (src/loop.c:1638-1706); address1..3 keep their old values when big_values == 0.
    // (Results go through plain locals and are assigned once: stores to the fields from several branches
    // made the compiler keep them in scratch memory.)
    {
        int r0c = 0, r1c = 0, ad1 = g.address1, ad2 = g.address2, ad3 = g.address3;
        if (g.big_values != 0) {
            const int bvr = 2 * g.big_values;
            if (g.wsf == 0) {
                // scfb_anz = number of band edges below bvr picks the counts from subdv_table, both lowered until
                // the regions end at or below bvr: a function of big_values alone, tabulated at table build
                const unsigned sd = T->subdiv_lut[g.big_values];
                r0c = (int) (sd & 15u);
                r1c = (int) ((sd >> 4) & 15u);
                ad1 = (int) ((sd >> 8) & 1023u);
                ad2 = (int) (sd >> 18);
                ad3 = bvr;
            } else {
                const bool sb = g.block_type == 2;
                r0c = sb ? 8 : 7;
                r1c = sb ? 36 : 13;
                ad1 = sb ? 36 : T->sfb_l[8]; // (36 at every MPEG-1 rate; start / stop blocks are rare)
                ad2 = bvr;
                ad3 = 0;
            }
        }
        g.region0_count = r0c; g.region1_count = r1c;
        g.address1 = ad1; g.address2 = ad2; g.address3 = ad3;
    }
    g.table_select[0] = g.table_select[1] = g.table_select[2] = 0;
    CBPROF(1); // subdivide
    if (nslot == 0) { // nothing but zeros: every region maximum is 0, no table, no bits
        g.count1table_select = 1; // count1_bitcount without quadruples: sum0 == sum1 -> table B
        return bits;
    }
    if (shortb) {
        // region maxima over lines [0,36) and [36,576); pair (6m+w, 6m+3+w), m<96, w<3
        int m1 = qi.m1, m2 = qi.m2; // this lane's part, from the quantiser
        {
            int mv[2] = {m1, m2};
            wave_reduce_i32<0, 2>(mv);
            m1 = mv[0]; m2 = mv[1];
        }
        // choose_table (src/loop.c:1908-1947): the first table that can hold the maximum
        const int da0 = wave_readlane_i32(R.desc_a, loop_desc_index(m1)), db0 = wave_readlane_i32(R.desc_b, loop_desc_index(m1));
        const int da1 = wave_readlane_i32(R.desc_a, loop_desc_index(m2)), db1 = wave_readlane_i32(R.desc_b, loop_desc_index(m2));
        const int t0 = m1 ? (da0 & 31) : 0, t1 = m2 ? (da1 & 31) : 0;
        g.table_select[0] = t0;
        g.table_select[1] = t1;
        int sum = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int pr = lane + 64 * k;
            const bool in = pr < 288;
            const int m = in ? pr / 3 : 0, w = in ? pr - 3 * m : 0;
            const int x = L.ix[6 * m + w], y = L.ix[6 * m + 3 + w];
            const bool first = m < 6;
            const int c = loop_pair_cost3(GL, first ? da0 : da1, first ? db0 : db1, x, y) & 0x3ff;
            sum += (in && (first ? t0 : t1)) ? c : 0;
        }
        return wave_sum_i32(sum);
    }
    // long / start / stop blocks: regions [0,a1), [a1,a2), [a2,e2) (src/loop.c:1771-1777).  The
    // reference's enable tests (a1 > 0, a2 > a1, e2 > a2) are exactly "the range is not empty",
    // and region 2 is non-empty only right after subdivide set a1 <= a2 <= e2, so the three
    // ranges never overlap.  Lines from slot nslot on are zero, so the maxima may skip them; but a
    // region can reach past big_values (stale or clamped addresses) and a pair of zeros still has a
    // code length, so the pricing loop runs to the end of the last region.
    // (the addresses may come out of LDS: make their uniformity explicit, they bound the loops below)
    const int a1 = __builtin_amdgcn_readfirstlane(g.address1), a2 = __builtin_amdgcn_readfirstlane(g.address2);
    const int e2 = __builtin_amdgcn_readfirstlane(2 * g.big_values);
    // Region 0 = lines [0, a1), 1 = [a1, a2), 2 = [a2, e2).
    int red[4]; // the count1 region's two bit sums and the three region maxima: four reductions in lock-step
    red[0] = c1part;
    // The maxima.  subdivide has just set the addresses (big_values > 0) to band edges with a1 <= a2 <= e2 -- or to [0, sfb_l[8]) and
    // [sfb_l[8], e2) for a start / stop block --: every region is then a run of whole peak cells, but for the cell that e2 cuts, and a
    // cell's largest value is the one at its peak line, in every pass (mp3mi_dev.h): ONE read per lane, and the peak line itself says
    // which region the cell is of (a1 and a2 are cell edges).  The cut cell: if it starts below n_big it holds a value above 1, so does
    // its peak line, which therefore lies below n_big <= e2 -- inside the region.  If it starts at n_big or later, it starts AT n_big
    // and e2 = n_big + 2 (both even, e2 - n_big is 0 or 2): its part of the region is the one pair in front of e2, values 0 / 1, while
    // its peak may lie past e2 (it then counts for no region) and read 1 where the pair holds zeros.  So the two lines of the pair in
    // front of e2 are read as well, by lanes 32 and up -- which have no cell --, as cells of one line: always right, since they ARE in
    // the region the test puts them in.
    // Anything else -- stale addresses (big_values == 0), an address past e2 (a band edge above a small big_values) -- walks the regions.
    if (e2 > 0 && a1 <= a2 && a2 <= e2) {
        const int w = (int) L.peak[lane];
        const int p = w < 1024 ? w : e2 - 1026 + w; // (lanes 32..63 hold 1024 | lane & 1: lines e2 - 2, e2 - 1)
        const int v = (int) ((const uint16_t *) L.ix)[p];
        red[1] = p < a1 ? v : 0;
        red[2] = (p >= a1 && p < a2) ? v : 0;
        red[3] = (p >= a2 && p < e2) ? v : 0;
    } else {
        // Each region is walked on its own, 64 pairs (one word each) per step straight out of L.ix; lines from slot nslot on are
        // zero, so the maxima may skip them.  (Written out per region: arrays indexed by the region would live in scratch memory.)
        const int nzend = 64 * nslot;
        auto region_max = [&](int lo, int hi) {
            hi = hi < nzend ? hi : nzend; // both even
            mp3mi_u16x2 m = {0, 0}; // the maxima of the x and of the y of this lane's pairs: one packed instruction a step
            const unsigned *p = ixw + (lo >> 1) + lane;
            const int span = hi > lo ? hi - lo : 0, nfull = span >> 7, rest = (span & 127) >> 1; // whole steps of 64 pairs (nothing to mask), and a last one
            if (nfull > 0) {
                m = LOOP_PK_MAX_U16(m, __builtin_bit_cast(mp3mi_u16x2, p[0]));
                if (nfull > 1) {
                    m = LOOP_PK_MAX_U16(m, __builtin_bit_cast(mp3mi_u16x2, p[64]));
                    if (nfull > 2) {
                        m = LOOP_PK_MAX_U16(m, __builtin_bit_cast(mp3mi_u16x2, p[128]));
                        if (nfull > 3) m = LOOP_PK_MAX_U16(m, __builtin_bit_cast(mp3mi_u16x2, p[192]));
                    }
                }
            }
            if (rest) {
                // read unconditionally (L.ix is padded: pairs past the end exist) and mask: a conditional load costs
                // three scalar instructions and two branches per step
                const unsigned xy = lane < rest ? p[64 * nfull] : 0u;
                m = LOOP_PK_MAX_U16(m, __builtin_bit_cast(mp3mi_u16x2, xy));
            }
            return (int) (m.x > m.y ? m.x : m.y); // this lane's part
        };
        red[1] = region_max(0, a1);
        red[2] = region_max(a1, a2);
        red[3] = region_max(a2, e2);
    }
    wave_reduce_i32<1, 3>(red);
    CBPROF(2); // region maxima + reduction
    {
        const int sum0 = red[0] & 0xffff, sum1 = (red[0] >> 16) & 0xffff; // table A vs table B (src/loop.c:1531-1580)
        if (sum0 < sum1) { g.count1table_select = 0; bits = sum0; }
        else { g.count1table_select = 1; bits = sum1; }
    }
    const int m0 = red[1], m1 = red[2], m2 = red[3];
    const int mx[3] = {m0, m1, m2};
    int da[3], db[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const int idx = loop_desc_index(mx[r]);
        da[r] = wave_readlane_i32(R.desc_a, idx);
        db[r] = wave_readlane_i32(R.desc_b, idx);
    }
    // cost of every candidate over its region: per lane three 10-bit partial sums per region.  A region can
    // reach past big_values (stale or clamped addresses) and a pair of zeros still has a code length, so the
    // pricing walks to the end of the region, not only over the non-zero slots.
    // Per region two partial sums per lane: candidates 0 and 1 in the halves of one word (the layout the
    // reduction wants), the third candidate -- only the groups {7,8,9} and {10,11,12} have one -- in another.
    int s01p[3], s2p[3];
    const loop_walk_k K = loop_walk_consts(); // (once a pass, not once a region)
    loop_region_cost(GL, ixw, lane, 0, a1, m0, da[0], db[0], K, &s01p[0], &s2p[0]);
    loop_region_cost(GL, ixw, lane, a1, a2, m1, da[1], db[1], K, &s01p[1], &s2p[1]);
    loop_region_cost(GL, ixw, lane, a2, e2, m2, da[2], db[2], K, &s01p[2], &s2p[2]);
    CBPROF(3); // descriptors + region walks
    const bool third = (((da[0] | da[1] | da[2]) >> 10) & 31) != 0; // (descriptors of empty regions are zero)
    // The sums stay where the reduction leaves them -- lane 63 of a vector register -- and new_choose_table's decision
    // is taken THERE, by vector instructions on values no other lane holds; four lane reads bring back the bit count and
    // the three tables.  As scalar code (until round 4) the decision cost ~20 scalar instructions per
    // region, and a scalar instruction costs this kernel more than a vector one.  An empty
    // region's descriptor and sums are zero: table 0, no bits, as src/loop.c:1771-1777 leaves it.
    {
        // ... and for the three regions AT ONCE: the sums of regions 0, 1, 2 are moved to lanes 61, 62, 63 of one register (the
        // reductions leave each in lane 63 of its own), their descriptors to the same lanes of another, and one run of the
        // decision serves all three; a sum over the three lanes is the bit count, three lane reads are the tables.
        int dav = wave_put_lane<63>(wave_put_lane<62>(wave_put_lane<61>(0, da[0]), da[1]), da[2]);
        int best, choice;
        if (third) { // five reductions in lock-step
            int fs[5] = {s01p[0], s01p[1], s01p[2], s2p[0] | (s2p[1] << 16), s2p[2]};
            wave_reduce_keep_i32<5, 0>(fs);
            const int x01 = wave_tail_place(wave_tail_place(fs[2], fs[1], 1), fs[0], 2);
            const int x2 = wave_tail_place(wave_tail_place(fs[4], (int) ((unsigned) fs[3] >> 16), 1), fs[3] & 0xffff, 2);
            choice = loop_pick_v<true>(dav, x01, x2, &best);
        } else {
            wave_reduce_keep_i32<3, 0>(s01p);
            const int x01 = wave_tail_place(wave_tail_place(s01p[2], s01p[1], 1), s01p[0], 2);
            choice = loop_pick_v<false>(dav, x01, 0, &best);
        }
        bits += wave_tail_sum3(best);
#pragma unroll
        for (int r = 0; r < 3; r++) g.table_select[r] = wave_readlane_i32(choice, 61 + r);
    }
    CBPROF(4); // cost reductions + picks
    return bits;
}

#endif
