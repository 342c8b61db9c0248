// The self-test hooks of the iteration loop (include/mp3mi.h): mp3mi_debug_quantize_count, one quantise+count pass of
// k_loop on given granules, and mp3mi_debug_peak_lines.  They live in a translation unit of their own and not in
// k_loop.hip, so that k_loop is compiled exactly as without them; the note k_loop.hip carried while they were there:
// "a second kernel in this translation unit that calls the pass functions changes how the compiler allocates k_loop's
// registers".  Nothing here is reached by k_loop.
#undef MP3MI_LOOP_PROFILE
#include "loop_pass.h"
#include "host_util.h"

// ---- self-test hook: one quantise+count pass of k_loop on given granules (include/mp3mi.h, mp3mi_debug_quantize_count) ----
// A wavefront per granule runs what a pass of loop_stream runs, with these functions, in this order: loop_power34, a rescale
// plan, loop_all_zero, loop_quantize (first tier and rare tier as in the product) and loop_count_bits.  The rescale plan marks
// every band; pre-emphasis (loop_preemph_lines) and the amplification of long / start / stop blocks (loop_amp_pairs) are the
// functions loop_stream calls.  Two blocks are still COPIES of loop_stream's statements, written inline there: the granule
// load around loop_power34 and the amplification of short blocks.  As functions shared with loop_stream -- the load taking
// (xr_all, rec), whole or as its two loops; the short-block loop, alone or in one function with the long-block one -- they
// compile, but change k_loop's instruction stream (profiles/r12_experiments.txt, E2), which this file exists to leave alone.
struct loop_qc_gran { int32_t q, block_type, n_amp, pre; };
__global__ void __launch_bounds__(64) k_debug_quantize_count(const mp3mi_tables *__restrict__ T, const double *__restrict__ xr_in,
                                                             const loop_qc_gran *__restrict__ gin, int16_t *__restrict__ ix_out,
                                                             double *__restrict__ xr_out, int32_t *__restrict__ f_out)
{
    __shared__ loop_lds L;
    __shared__ uint16_t GL[928];
    __shared__ double zeros[8];
    for (int i = (int) threadIdx.x; i < 928; i += 64) GL[i] = T->glut[i];
    if (threadIdx.x < 8) zeros[threadIdx.x] = 0.0;
    __syncthreads();
    const size_t gi = blockIdx.x;
    const int lane = wave_lane();
    const loop_qc_gran in = gin[gi];
    loop_regs R;
    loop_desc_init(T, lane, &R.desc_a, &R.desc_b);
    L.ix[576 + lane] = 0; L.ix[640 + lane] = 0; // (the padding, as loop_stream sets it)
    if (lane < 2) L.xr[576 + lane] = 0.0;
    loop_gr g = {};
    g.block_type = in.block_type;
    g.wsf = g.block_type != 0;
    const bool shortb = g.wsf && g.block_type == 2;
    g.sfb_lmax = shortb ? 0 : 21;
    g.sfb_smax = shortb ? 0 : 12;
    g.q = in.q;
    const int nband = shortb ? 36 : 21;
    float y34[LOOP_NV], y34max;
    {
        double xr[LOOP_NV];
#pragma unroll
        for (int k = 0; k < LOOP_SLOTS; k++) {
            const int pr = loop_pair_of(lane, k);
            const bool there = k < 4 || pr < 288;
            xr[2 * k] = there ? xr_in[gi * 576 + 2 * pr] : 0.0;
            xr[2 * k + 1] = there ? xr_in[gi * 576 + 2 * pr + 1] : 0.0;
        }
        y34max = loop_power34(xr, y34);
#pragma unroll
        for (int k = 0; k < LOOP_SLOTS; k++) {
            const int pr = loop_pair_of(lane, k);
            if (k < 4 || pr < 288) { L.xr[2 * pr] = xr[2 * k]; L.xr[2 * pr + 1] = xr[2 * k + 1]; }
        }
    }
    wave_sync();
    if (!shortb) { // the peak lines of xr_in, by the walk that takes them in the pipeline (k_mdct's tail: mp3mi_cell_peak over mp3mi_peak_cell)
        int first, lines;
        mp3mi_peak_cell(T->sfb_l, lane & (MP3MI_PEAK_CELLS - 1), &first, &lines);
        const int at = mp3mi_cell_peak((const double *) &L.xr[first], (const double *) zeros, lines, wave_max_i32(lines));
        L.peak[lane] = lane < MP3MI_PEAK_CELLS ? (uint16_t) (first + at) : (uint16_t) (1024 | (lane & 1)); // (as loop_stream fills it)
        wave_sync();
    }
    const unsigned long long bandpack = T->lane_bands[shortb][lane];
    if (in.pre && !shortb) { // preemphasis with every one of sfb 17..20 violating (loop_stream)
        loop_preemph_lines(T, L, y34, bandpack, lane, g.sfb_lmax);
        y34max = y34max * LOOP_Y34MAX_GROW;
    }
    wave_sync();
    const double ifqstep = T->sqrt2;
    const unsigned long long ampmask = (1ull << nband) - 1ull; // amp_scalefac_bands with every band amplified (loop_stream)
    for (int a = 0; a < in.n_amp; a++) {
        if (!shortb) {
            loop_amp_pairs(L, y34, (unsigned) bandpack, (unsigned) ampmask, ifqstep, lane);
        } else { // (loop_stream's short-block statements, restated)
#pragma unroll
            for (int j = 0; j < LOOP_NV; j++) {
                const unsigned b = (unsigned) ((bandpack >> (6 * j)) & 63ull);
                const bool f = ((ampmask >> b) & 1ull) != 0;
                const int line = 2 * loop_pair_of(lane, j >> 1) + (j & 1);
                if (f) {
                    L.xr[line] = L.xr[line] * ifqstep;
                    y34[j] = y34[j] * 1.2968395546510096f;
                }
            }
        }
        y34max = y34max * LOOP_Y34MAX_AMP;
        wave_sync();
    }
    // diagnostics, from the same estimates the quantiser forms (never part of the result)
    const bool az = loop_all_zero(y34max, g.q);
    const loop_qscale qs = loop_quant_scale(g.q);
    unsigned differ = 0u;
    int n_differ = 0;
#pragma unroll
    for (int k = 0; k < LOOP_SLOTS; k++) {
        const unsigned hi = loop_quant_pair(y34[2 * k], y34[2 * k + 1], qs.a_hi, (float) LOOP_Q_CHI);
        const unsigned lo = loop_quant_pair(y34[2 * k], y34[2 * k + 1], qs.a_lo, (float) LOOP_Q_CLO);
        differ |= hi ^ lo;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            unsigned a = (hi >> (16 * h)) & 0xffffu, b = (lo >> (16 * h)) & 0xffffu;
            a = a < 2047u ? a : 2047u;
            b = b < 2047u ? b : 2047u;
            n_differ += (a != b && 2 * loop_pair_of(lane, k) + h < 576) ? 1 : 0;
        }
    }
    const bool over = !(loop_estimate(y34max, qs.a_hi * 65535.0f) < 2047.0f);
    const bool rare = !az && (over || wave_any(differ != 0u));
    n_differ = wave_sum_i32(n_differ);
    // the pass
    const loop_qinfo qi = loop_quantize(T, L, y34, y34max, g.q, az, false, shortb);
    const int bits = loop_count_bits(T, R, L, GL, g, qi, az CBPROF_PASS);
    wave_sync();
    for (int i = lane; i < 576; i += 64) {
        ix_out[gi * 576 + i] = L.ix[i];
        xr_out[gi * 576 + i] = L.xr[i];
    }
    const int m1 = wave_max_i32(qi.m1), m2 = wave_max_i32(qi.m2);
    if (lane == 0) {
        int32_t *f = f_out + gi * MP3MI_QC_FIELDS;
        f[MP3MI_QC_N_NZ] = qi.n_nz; f[MP3MI_QC_N_BIG] = qi.n_big; f[MP3MI_QC_M1] = m1; f[MP3MI_QC_M2] = m2;
        f[MP3MI_QC_BITS] = bits; f[MP3MI_QC_BIG_VALUES] = g.big_values; f[MP3MI_QC_COUNT1] = g.count1;
        f[MP3MI_QC_COUNT1TABLE_SELECT] = g.count1table_select;
        f[MP3MI_QC_TABLE_SELECT0] = g.table_select[0]; f[MP3MI_QC_TABLE_SELECT1] = g.table_select[1]; f[MP3MI_QC_TABLE_SELECT2] = g.table_select[2];
        f[MP3MI_QC_REGION0_COUNT] = g.region0_count; f[MP3MI_QC_REGION1_COUNT] = g.region1_count;
        f[MP3MI_QC_ADDRESS1] = g.address1; f[MP3MI_QC_ADDRESS2] = g.address2; f[MP3MI_QC_ADDRESS3] = g.address3;
        f[MP3MI_QC_ALL_ZERO] = az; f[MP3MI_QC_RARE_TIER] = rare; f[MP3MI_QC_N_DIFFER] = n_differ; f[MP3MI_QC_OVER] = !az && over;
    }
}

extern "C" int mp3mi_debug_quantize_count(int rate_hz, int n_gran, const double *xr, const int32_t *gran, int16_t *ix,
                                          double *xr_out, int32_t *fields)
{
    if (!have_device()) return MP3MI_ERR_NO_DEVICE;
    const int ri = rate_idx_of(rate_hz);
    if (ri < 0 || n_gran < 0 || (n_gran > 0 && (!xr || !gran || !ix || !xr_out || !fields))) return MP3MI_ERR_ARG;
    for (int i = 0; i < n_gran; i++) {
        const int32_t *p = gran + 4 * i;
        if (p[0] < MP3MI_STEP_MIN || p[0] >= MP3MI_STEP_MIN + MP3MI_STEP_N || p[1] < 0 || p[1] > 3 || p[2] < 0 || p[2] > 16 ||
            p[3] < 0 || p[3] > 1 || (p[3] && p[1] == 2))
            return MP3MI_ERR_ARG;
    }
    if (n_gran == 0) return MP3MI_OK;
    host_mem<mp3mi_tables> Th(1);
    const int trc = tables_into(Th, ri);
    if (trc != MP3MI_OK) return trc;
    const size_t n = (size_t) n_gran;
    hook_bufs D;
    const mp3mi_tables *dT = D.copy_of(Th.p, 1);
    const double *dxr = D.copy_of(xr, n * 576);
    double *dxo = D.raw<double>(n * 576);
    const loop_qc_gran *dg = D.copy_of((const loop_qc_gran *) gran, n);
    int16_t *dix = D.raw<int16_t>(n * 576);
    int32_t *df = D.raw<int32_t>(n * MP3MI_QC_FIELDS);
    if (!D.ok) return D.rc();
    hipLaunchKernelGGL(k_debug_quantize_count, dim3((unsigned) n), dim3(64), 0, 0, dT, dxr, dg, dix, dxo, df);
    D.sync();
    D.fetch(ix, dix, n * 576);
    D.fetch(xr_out, dxo, n * 576);
    D.fetch(fields, df, n * MP3MI_QC_FIELDS);
    return D.rc();
}

// ---- self-test hook: the peak lines k_mdct's tail would record for given granules, and the cells they are the peaks of ----
__global__ void __launch_bounds__(64) k_debug_peak_lines(const mp3mi_tables *__restrict__ T, const double *__restrict__ xr_in, uint16_t *__restrict__ peak_out)
{
    __shared__ double xr[576 + 8]; // (eight zeros behind the spectrum: what a lane past its cell's end reads)
    const int lane = wave_lane();
    for (int i = lane; i < 576 + 8; i += 64) xr[i] = i < 576 ? xr_in[(size_t) blockIdx.x * 576 + i] : 0.0;
    __syncthreads();
    int first, lines;
    mp3mi_peak_cell(T->sfb_l, lane & (MP3MI_PEAK_CELLS - 1), &first, &lines);
    const int at = mp3mi_cell_peak((const double *) &xr[first], (const double *) &xr[576], lines, wave_max_i32(lines));
    if (lane < MP3MI_PEAK_CELLS) peak_out[(size_t) blockIdx.x * MP3MI_PEAK_CELLS + lane] = (uint16_t) (first + at);
}

extern "C" int mp3mi_debug_peak_lines(int rate_hz, int n_gran, const double *xr, uint16_t *peak, int32_t *cell_first)
{
    if (!have_device()) return MP3MI_ERR_NO_DEVICE;
    const int ri = rate_idx_of(rate_hz);
    if (ri < 0 || n_gran < 0 || !cell_first || (n_gran > 0 && (!xr || !peak))) return MP3MI_ERR_ARG;
    host_mem<mp3mi_tables> Th_h(1);
    const int trc = tables_into(Th_h, ri);
    if (trc != MP3MI_OK) return trc;
    const mp3mi_tables *Th = Th_h.p;
    for (int c = 0; c <= MP3MI_PEAK_CELLS; c++) { // (the cells as the kernels cut them; entry MP3MI_PEAK_CELLS closes the last cell)
        int first = 576, lines = 0, cells = 0;
        for (int b = 0; b < 22; b++) {
            const int nb = (Th->sfb_l[b + 1] - Th->sfb_l[b] + MP3MI_PEAK_CELL_LINES - 1) / MP3MI_PEAK_CELL_LINES;
            if (c >= cells && c < cells + nb) first = Th->sfb_l[b] + (c - cells) * MP3MI_PEAK_CELL_LINES;
            cells += nb;
        }
        cell_first[c] = first;
    }
    const size_t n = (size_t) n_gran;
    if (n == 0) return MP3MI_OK;
    hook_bufs D;
    const mp3mi_tables *dT = D.copy_of(Th, 1);
    const double *dxr = D.copy_of(xr, n * 576);
    uint16_t *dpk = D.raw<uint16_t>(n * MP3MI_PEAK_CELLS);
    if (!D.ok) return D.rc();
    hipLaunchKernelGGL(k_debug_peak_lines, dim3((unsigned) n), dim3(64), 0, 0, dT, dxr, dpk);
    D.sync();
    D.fetch(peak, dpk, n * MP3MI_PEAK_CELLS);
    return D.rc();
}
