// Iteration loop: allowed distortion, scfsi, bit reservoir, quantiser step search, Huffman
// table selection and bit counting, noise calculation and scalefactor amplification.
//
// Replaces iteration_loop (src/loop.c:232-362) with everything below it (src/loop.c:369-2140,
// src/pow_nint.h, src/reservoir.c) for a whole batch.  The search is serial per stream (the
// reservoir size threads through every granule), so ONE WAVEFRONT OWNS ONE STREAM and walks its
// frames in order; the 64 lanes share each granule's 288 PAIRS of lines (pair p = lines 2p, 2p + 1 -- what the
// Huffman tables code together -- belongs to lane p%64, slot p/64; slot 4 is half empty), all loop
// decisions are wave-uniform, bit counts are wave-reduced (DPP, several reductions in lock-step).
// The spectrum and the quantised values live in LDS; what stays in registers between passes is
// |xr|^(3/4) of the lane's ten lines and the per-band state.
//
// The stateless head of the loop (calc_xmin, quantanf_init, the values calc_scfsi stores) comes
// from k_mdct's tail (k_fbmdct.hip; k_prep.hip).  Band noise -- only ever compared with the allowed distortion -- is summed in
// ~10-line parts by all lanes, with the reference's sequential order as the fallback when a band
// lands within 1e-12 of its threshold.  Integer work is order-free.
//
// The kernel is instruction-issue-bound: what matters is the total instruction count of
// a pass and keeping memory operations out of its dependent chain (no scratch access inside the
// pass loops: lane-derived addresses are recomputed where used, see wave_lane_here).
//
// Small tables the search consults with wave-uniform indices (scalefactor band edges, Huffman
// table geometry, the region subdivision table) live one entry per lane in registers and are
// read with v_readlane; per-line Huffman code lengths sit in LDS; the quantiser boundary table
// and i^(4/3) are read through L1/L2.
//
// HBM per (granule, channel): 4608 B xr in, 472 B psy record and 536 B prep record in, 1152 B ix out,
// ~54 words of side information out.
#include "loop_pass.h"

// scfsi_m: bit b = scfsi[ch][b] of this frame when gr == 1, 0 for gr == 0 (whose scalefactors are always sent)
MP3MI_DEVFN int loop_part2_length(const loop_gr &g, int scfsi_m)
{ // src/loop.c:731-780
    const int slen1 = loop_slen1(g.scalefac_compress), slen2 = loop_slen2(g.scalefac_compress);
    if (g.wsf == 1 && g.block_type == 2) return 18 * slen1 + 18 * slen2;
    int bits = 0;
    if ((scfsi_m & 1) == 0) bits += 6 * slen1;
    if ((scfsi_m & 2) == 0) bits += 5 * slen1;
    if ((scfsi_m & 4) == 0) bits += 5 * slen2;
    if ((scfsi_m & 8) == 0) bits += 5 * slen2;
    return bits;
}

// Sequential sum of the noise terms (|xr| - ix^(4/3) step)^2 of lines first + k*stride, k < count, in index
// order (src/loop.c:1030-1060); xr and ix come from LDS, i^(4/3) from the table.  Every lane runs the
// same loop with its own range (a partial-sum job, or a whole band for the exact tier).
MP3MI_DEVFN double loop_noise_sum(const mp3mi_tables *T, const loop_lds &L, double step, int first, int count, int stride)
{
    // (addresses as in loop_noise_jobs: 32-bit byte offsets, all shifts of the one line index)
    const char *lds = (const char *) &L.xr[0];
    const unsigned ix_off = (unsigned) ((const char *) &L.ix[0] - (const char *) &L.xr[0]);
    const char *tab = (const char *) &T->pow43[0];
    double sum = 0.0;
    unsigned line = (unsigned) first;
    int k = 0;
    for (; k + 2 <= count; k += 2) { // two terms in flight, added in order (the rare tier: it must not be what sets the kernel's register count)
        double t[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const unsigned ln = line + (unsigned) (u * stride);
            const unsigned q = *(const uint16_t *) (lds + ix_off + 2u * ln);
            t[u] = __builtin_fabs(*(const double *) (lds + 8u * ln)) - *(const double *) (tab + (size_t) (8u * q)) * step;
        }
        line += (unsigned) (2 * stride);
#pragma unroll
        for (int u = 0; u < 2; u++) sum = sum + t[u] * t[u];
    }
    for (; k < count; k++) {
        const unsigned q = *(const uint16_t *) (lds + ix_off + 2u * line);
        const double t = __builtin_fabs(*(const double *) (lds + 8u * line)) - *(const double *) (tab + (size_t) (8u * q)) * step;
        line += (unsigned) stride;
        sum = sum + t * t;
    }
    return sum;
}

// The partial-sum jobs of the first tier: all lanes take the same number of steps (kmax, the longest job,
// a multiple of 4) and a job that is through reads pair 288 -- xr = 0, ix = 0, terms of exactly +0 -- instead
// of dropping out: no divergent loop, no remainder loop.
// LONG blocks: a job is a run of whole PAIRS of lines (tables_host.cpp: first and count are even), two pairs a step: per pair ONE
// 16-byte read of the spectrum, ONE word of quantised values, two table reads -- four terms in flight on half the address
// arithmetic and half the LDS reads of a line-by-line walk.
typedef double loop_f64x2 __attribute__((ext_vector_type(2)));
MP3MI_DEVFN double loop_noise_jobs_long(const mp3mi_tables *T, const loop_lds &L, double step, int first, int count, int kmax)
{
    // Addresses as 32-bit byte offsets from three bases, all shifts of the one pair index: as `L.ix[line]` and
    // `T->pow43[L.ix[line]]` the compiler derived the second LDS address from the first by a 64-bit multiply-add (a quarter-rate
    // instruction) and sign-extended the table index to 64 bits (L.ix holds magnitudes).
    const char *lds = (const char *) &L.xr[0];
    const unsigned ix_off = (unsigned) ((const char *) &L.ix[0] - (const char *) &L.xr[0]);
    const char *tab = (const char *) &T->pow43[0];
    double sum = 0.0;
    unsigned pr = (unsigned) first >> 1;
    const unsigned npairs = (unsigned) count >> 1;
#if !defined(LOOP_NOISE_PAIRS)
#define LOOP_NOISE_PAIRS 4 /* pairs in flight per step: the jobs of all three rates are at most four pairs long -- one step, no loop */
#endif
    for (int k = 0; 2 * k < kmax; k += LOOP_NOISE_PAIRS) {
        // the quantised values first, then the table entries they select -- the long latency --, the spectrum two pairs at a time behind
        // them: what is in flight at once decides the kernel's register count
        unsigned p[LOOP_NOISE_PAIRS], w[LOOP_NOISE_PAIRS];
        double q43[2 * LOOP_NOISE_PAIRS];
#pragma unroll
        for (int u = 0; u < LOOP_NOISE_PAIRS; u++) {
            p[u] = (unsigned) (k + u) < npairs ? pr + (unsigned) u : 288u;
            w[u] = *(const unsigned *) (lds + ix_off + 4u * p[u]);
        }
#pragma unroll
        for (int u = 0; u < LOOP_NOISE_PAIRS; u++) {
            q43[2 * u] = *(const double *) (tab + (size_t) ((w[u] << 3) & 0x7fff8u));
            q43[2 * u + 1] = *(const double *) (tab + (size_t) ((w[u] >> 13) & 0x7fff8u));
        }
        pr += (unsigned) LOOP_NOISE_PAIRS;
#pragma unroll
        for (int u = 0; u < LOOP_NOISE_PAIRS; u++) {
#if !defined(MP3MI_EMU)
            if ((u & 1) == 0) asm volatile("" ::: "memory"); // (the spectrum's reads stay here, two pairs at a time, behind the table reads)
#endif
#if defined(MP3MI_EMU)
            const double x0 = *(const double *) (lds + 16u * p[u]), x1 = *(const double *) (lds + 16u * p[u] + 8u);
#else
            const loop_f64x2 xx = *(const loop_f64x2 *) (lds + 16u * p[u]);
            const double x0 = xx.x, x1 = xx.y;
#endif
            const double t0 = __builtin_fabs(x0) - q43[2 * u] * step, t1 = __builtin_fabs(x1) - q43[2 * u + 1] * step;
            // (this is the FIRST tier: its sum only has to lie within 1e-12 of the reference's -- loop_noise_close -- and a fused
            // square-and-add differs from the reference's two roundings by an ulp of the running sum per term, < 2.2e-14 over the
            // 192 terms of the widest band; the difference itself stays two roundings: fused, a value of 8000 could move a term by 1.6e-12)
            sum = __builtin_fma(t0, t0, sum);
            sum = __builtin_fma(t1, t1, sum);
        }
    }
    return sum;
}
// SHORT blocks (one granule in twenty): a job's lines are three apart; line by line, two terms a step (what is in flight here, not the
// kernel's common path, would otherwise set its register count).
MP3MI_DEVFN double loop_noise_jobs_short(const mp3mi_tables *T, const loop_lds &L, double step, int first, int count, int kmax)
{
    const char *lds = (const char *) &L.xr[0];
    const unsigned ix_off = (unsigned) ((const char *) &L.ix[0] - (const char *) &L.xr[0]);
    const char *tab = (const char *) &T->pow43[0];
    double sum = 0.0;
    unsigned line = (unsigned) first;
    for (int k = 0; k < kmax; k += 2) {
        double t[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const unsigned ln = (unsigned) (k + u) < (unsigned) count ? line + (unsigned) (3 * u) : 576u;
            const double x = *(const double *) (lds + 8u * ln);
            const unsigned q = *(const uint16_t *) (lds + ix_off + 2u * ln);
            t[u] = __builtin_fabs(x) - *(const double *) (tab + (size_t) (8u * q)) * step;
        }
        line += 6u;
#pragma unroll
        for (int u = 0; u < 2; u++) sum = __builtin_fma(t[u], t[u], sum); // (first tier: see loop_noise_jobs_long)
    }
    return sum;
}

// the reference's sequential band sums (src/loop.c:1030-1060)
MP3MI_DEVFN double loop_noise_exact(const mp3mi_tables *T, const loop_lds &L, double step, bool bandlane, int sfirst, int scount, int sstride)
{
    const double sum = loop_noise_sum(T, L, step, sfirst, bandlane ? scount : 0, sstride);
    return bandlane ? sum / (double) scount : 0.0;
}

// is the partial-sum noise of this band lane too close to its threshold to decide `noise > xmin`?
MP3MI_DEVFN bool loop_noise_close(bool bandlane, double xfsf, double xmin)
{
    return bandlane && xmin > 0.0 && __builtin_fabs(xfsf - xmin) <= 1e-12 * xmin;
}

// The kernel's arguments as ONE record.  The search needs a dozen pointers and launch constants a few times per granule,
// per frame or per stream -- and every scalar register matters in between: held in registers across the whole kernel they were
// what the compiler spilled (131 scalar registers into the lanes of three vector registers, written and read back by vector
// instructions in the granule's set-up and in every iteration of the distortion loop).  Now the record stays where the launch
// put it -- the kernel argument segment -- and a value is fetched by a scalar load WHERE IT IS USED (LOOP_ARG: the pointer
// behind an optimisation barrier, so that the loads are not hoisted to the kernel's top again).
struct loop_kargs { // (the table block is a kernel argument of its own: a read-only, no-alias pointer, whose loads are scalar loads)
    mp3mi_geom geo;
    const double *xr_all;
    const mp3mi_psy_out *psy;
    const mp3mi_loop_prep *prep;
    const int32_t *bits_per_frame;
    mp3mi_loop_state *state;
    int16_t *ix_out;
    mp3mi_frame_side *side_out;
    unsigned *gate_count;
    mp3mi_loop_place place;
};
#if defined(MP3MI_EMU)
typedef const loop_kargs *loop_kargs_p;
#define LOOP_ARG(field) (ka->field)
#define loop_kargs_ptr(ka) (ka)
#else
typedef const __attribute__((address_space(4))) loop_kargs *loop_kargs_p;
MP3MI_DEVFN loop_kargs_p loop_kargs_here(loop_kargs_p p)
{
    int z = 0;
    asm volatile("" : "+s"(z));
    return (loop_kargs_p) ((const __attribute__((address_space(4))) char *) p + z);
}
#define LOOP_ARG(field) (loop_kargs_here(ka)->field)
#define loop_kargs_ptr(ka) loop_kargs_here(ka)
#endif

// frames of the chunk [f0, f0 + nf) that a stream with n valid samples per channel still has
MP3MI_DEVFN int loop_frames_here(int f0, int nf, int n)
{
    const int total = (n + 1151) / 1152, left = total - f0;
    return left < 0 ? 0 : (left < nf ? left : nf);
}

// ---- placement: which stream does this wavefront take? ----
// The kernel ends when its most loaded SIMD ends.  The hardware decides where a workgroup runs,
// so instead of stream = blockIdx a wavefront looks at where it landed (HW_ID / XCC_ID) and takes a
// stream from the list sorted by the previous chunk's cost such that every SIMD gets a heavy, a
// light and two middle streams: the r-th wavefront to arrive on the SIMD with arrival ticket i
// takes sorted position r*NS + i (r even) or (r+1)*NS - 1 - i (r odd), NS = place.n_simd.
// Any wavefront that finds its position missing or taken (more streams than slots, an uneven
// spread) takes the next free one from a scan counter, so every stream is taken exactly once.
MP3MI_DEVFN int loop_place_stream(loop_kargs_p ka, int n_streams, int block)
{
#if defined(MP3MI_EMU)
    return ka->place.order ? ka->place.order[block] : block;
#else
    mp3mi_loop_place pl; // (field by field: the record lives in the kernel argument segment)
    pl.order = LOOP_ARG(place.order);
    if (!pl.order) return block;
    pl.taken = LOOP_ARG(place.taken); pl.simd_slots = LOOP_ARG(place.simd_slots); pl.simd_idx = LOOP_ARG(place.simd_idx);
    pl.ticket = LOOP_ARG(place.ticket); pl.scan = LOOP_ARG(place.scan); pl.n_simd = LOOP_ARG(place.n_simd);
    int pos = -1;
    if (wave_lane() == 0) {
        const unsigned hw = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));   // HW_ID
        const unsigned xcc = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11));  // XCC_ID
        // simd_id[5:4] cu_id[11:8] sh_id[12] se_id[15:13]
        const unsigned key = ((xcc & 7u) << 10) | (((hw >> 13) & 7u) << 7) | (((hw >> 12) & 1u) << 6) | (((hw >> 8) & 15u) << 2) | ((hw >> 4) & 3u);
        const unsigned r = atomicAdd(&pl.simd_slots[key], 1u);
        unsigned idx = 0xffffffffu;
        if (r == 0) {
            idx = atomicAdd(pl.ticket, 1u);
            __hip_atomic_store(&pl.simd_idx[key], idx + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        } else if (r < 4) {
            for (int spin = 0; spin < 20000; spin++) { // the first arrival on this SIMD publishes within microseconds
                const unsigned v = __hip_atomic_load(&pl.simd_idx[key], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                if (v) { idx = v - 1u; break; }
                __builtin_amdgcn_s_sleep(2);
            }
        }
        if (r < 4 && idx < (unsigned) pl.n_simd) {
            const int p = (r & 1u) ? (int) ((r + 1u) * pl.n_simd - 1u - idx) : (int) (r * pl.n_simd + idx);
            if (p < n_streams && atomicExch(&pl.taken[p], 1u) == 0u) pos = p;
        }
        while (pos < 0) { // n_streams wavefronts claim n_streams positions: this always finds one
            const unsigned p = atomicAdd(pl.scan, 1u);
            if (p >= (unsigned) n_streams) { pos = block; break; } // cannot happen; never spin forever
            if (atomicExch(&pl.taken[p], 1u) == 0u) pos = (int) p;
        }
        pos = pl.order[pos];
    }
    return __builtin_amdgcn_readfirstlane(pos);
#endif
}

// order[rank] = stream, streams ranked by cost (descending, ties by index): one thread per stream.
__global__ void __launch_bounds__(256) k_rank(const int *__restrict__ cost, int *__restrict__ order, int n)
{
    const int i = (int) (blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int ci = cost[i];
    int rank = 0;
    for (int j = 0; j < n; j++) {
        const int cj = cost[j];
        rank += (cj > ci || (cj == ci && j < i)) ? 1 : 0;
    }
    order[rank] = i;
}

void mp3mi_launch_rank(const int *cost, int *order, int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_rank, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, cost, order, n);
}

// 80 VGPRs: four resident wavefronts per SIMD leave 192 of its 512 registers to the kernels of the next chunk.
// One stream, start to end, by one wavefront (k_loop below).
MP3MI_DEVFN void loop_stream(const mp3mi_tables *__restrict__ T, loop_kargs_p ka, loop_lds &L, const uint16_t *GL, int block)
{
    const int lane = wave_lane();
    const int C = LOOP_ARG(geo.channels), G = 2 * LOOP_ARG(geo.nf);
    const int s = loop_place_stream(ka, LOOP_ARG(geo.n_streams), block);
    int work = 0; // cost of this stream in this launch: 4 per quantise+count pass, 5 per distortion-loop iteration
    const int bitsPerFrame = LOOP_ARG(bits_per_frame)[s];
    const int mean_bits = (bitsPerFrame - (32 + (C == 1 ? 136 : 256) + (LOOP_ARG(geo.crc) ? 16 : 0))) / 2; // src/musicin.c:729-746
    PROF_DECL;
    // Residency census (batch.cpp, k_gate): every wavefront counts itself in when it starts.  The
    // counter only ever grows; nothing in this kernel waits on it.
    {
        unsigned *gate_count = LOOP_ARG(gate_count);
        if (gate_count && lane == 0) atomicAdd(gate_count, 1u);
    }
#if !defined(MP3MI_EMU)
    // this wavefront is on the critical path of the whole batch: let it issue ahead of the
    // feed-forward kernels of the next chunk that run beside it (batch.cpp); adjusted
    // per frame by the pacing below
    __builtin_amdgcn_s_setprio(2);
#endif

    loop_regs R;
    loop_desc_init(T, lane, &R.desc_a, &R.desc_b);

    for (int i = lane; i < (int) (sizeof(mp3mi_loop_state) / 4); i += 64) ((int *) &L.st)[i] = ((const int *) &LOOP_ARG(state)[s])[i];
    L.ix[576 + lane] = 0; L.ix[640 + lane] = 0; // (the padding: pairs that do not exist)
    if (lane < 2) L.xr[576 + lane] = 0.0;
    if (lane >= MP3MI_PEAK_CELLS) L.peak[lane] = (uint16_t) (1024 | (lane & 1)); // (loop_count_bits: the lanes without a peak cell)
    wave_sync();
    int ref_abort = __builtin_amdgcn_readfirstlane(L.st.ref_abort); // (sticky: the first event of the stream stands)

    // ragged batch: frames of this stream beyond its last (zero-filled) one are not encoded
    const int nf_s = LOOP_ARG(geo.n_samples) ? loop_frames_here(LOOP_ARG(geo.f0), LOOP_ARG(geo.nf), LOOP_ARG(geo.n_samples)[s]) : LOOP_ARG(geo.nf);
    for (int fl = 0; fl < nf_s; fl++) {
        // ResvFrameBegin (src/reservoir.c:45-93); main_data_begin*8 == ResvSize by construction
        int ResvSize = L.st.ResvSize;
        int ResvMax = (bitsPerFrame > 7680) ? 0 : 7680 - bitsPerFrame;
        if (ResvMax > 4088) ResvMax = 4088;
        const int main_data_begin = ResvSize / 8;
        int resvDrain = 0;
        wave_sync();

        for (int gr = 0; gr < 2; gr++)
            for (int ch = 0; ch < C; ch++) {
                const int lane = wave_lane_here(); // nothing derived from the lane index outlives this granule
                const int gl = 2 * fl + gr;
                const size_t rec = ((size_t) s * G + gl) * C + ch;
                // (the granule's pointers in one go: one laundered base, the scalar loads behind it issue together)
                loop_kargs_p kg = loop_kargs_ptr(ka);
                const mp3mi_psy_out *po = &kg->psy[rec];
                loop_gr g;
                g.block_type = po->block_type;
                g.wsf = g.block_type != 0;
                const bool shortb = g.wsf && g.block_type == 2;
                g.sfb_lmax = shortb ? 0 : 21; // gr_deco, src/loop.c:2063
                g.sfb_smax = shortb ? 0 : 12;
                g.address1 = L.st.addr[gr][ch][0];
                g.address2 = L.st.addr[gr][ch][1];
                g.address3 = L.st.addr[gr][ch][2];
                const int nband = shortb ? 36 : 21;   // band lanes
                float y34[LOOP_NV], y34max;
                {
                    double xr[LOOP_NV];
                    const double *xr_all = kg->xr_all;
#pragma unroll
                    for (int k = 0; k < LOOP_SLOTS; k++) { // a pair = 16 bytes per lane
                        const int pr = loop_pair_of(lane, k);
                        const bool there = k < 4 || pr < 288;
                        xr[2 * k] = there ? xr_all[rec * 576 + 2 * pr] : 0.0;
                        xr[2 * k + 1] = there ? xr_all[rec * 576 + 2 * pr + 1] : 0.0;
                    }
                    y34max = loop_power34(xr, y34);
#pragma unroll
                    for (int k = 0; k < LOOP_SLOTS; k++) {
                        const int pr = loop_pair_of(lane, k);
                        if (k < 4 || pr < 288) { L.xr[2 * pr] = xr[2 * k]; L.xr[2 * pr + 1] = xr[2 * k + 1]; }
                    }
                }

                // ---- calc_xmin (src/loop.c:1085-1118) and the values calc_scfsi stores (src/loop.c:631-667)
                //      were computed by k_mdct's tail (k_prep); only the stateful decision of calc_scfsi happens here ----
                PROF(0);
                const mp3mi_loop_prep *pp = &kg->prep[rec];
                // per-band state (allowed distortion, scalefactors): L.band_*
                if (lane < 36) {
                    L.band_xmin[lane] = lane < nband ? pp->xmin[lane] : 0.0;
                    L.band_sf[lane] = 0;
                    L.band_sfsave[lane] = 0;
                }
                if (lane == 0) {
                    L.st.sc_xrmax[gr][ch] = pp->sc_xrmax;
                    L.st.sc_en_tot[gr][ch] = pp->sc_en_tot;
                }
                if (!shortb && lane < 21) {
                    L.st.sc_en[gr][ch][lane] = pp->sc_en[lane];
                    L.st.sc_xm[gr][ch][lane] = pp->sc_xm[lane];
                }
                if (!shortb && lane < MP3MI_PEAK_CELLS) L.peak[lane] = pp->peak[lane]; // (read from the first pass on: barriers enough in between)
                const int nonzero = pp->nonzero;
                int scfsi_m = 0; // this granule's scfsi bits (wave-uniform): what the search asks for between passes
                wave_sync();
                if (gr == 1) {
                    int condition = 0;
                    for (int gr2 = 0; gr2 < 2; gr2++) {
                        if (L.st.sc_xrmax[ch][gr2] != 0) condition++; // [ch][gr2], sic
                        if (!shortb) condition++;
                    }
                    condition++; // abs(en_tot[0]-en_tot[1]) is a pointer difference in the reference
                    int d = 0, dx = 0;
                    if (lane < 21) {
                        d = abs(L.st.sc_en[ch][0][lane] - L.st.sc_en[ch][1][lane]);
                        dx = abs(L.st.sc_xm[ch][0][lane] - L.st.sc_xm[ch][1][lane]);
                    }
                    if (wave_sum_i32(d) < 100) condition++;
                    if (condition == 6) {
                        for (int band = 0; band < 4; band++) {
                            const int lo = (band == 0) ? 0 : (band == 1 ? 6 : (band == 2 ? 11 : 16));
                            const int hi = (band == 0) ? 6 : (band == 1 ? 11 : (band == 2 ? 16 : 21));
                            const bool in = lane >= lo && lane < hi;
                            const int s0 = wave_sum_i32(in ? d : 0), s1 = wave_sum_i32(in ? dx : 0);
                            const int v = (s0 < 10 && s1 < 10) ? 1 : 0;
                            scfsi_m |= v << band;
                        }
                    }
                    if (lane < 4) LOOP_ARG(side_out)[(size_t) s * LOOP_ARG(geo.nf) + fl].scfsi[ch][lane] = (scfsi_m >> lane) & 1; // (always decided in granule 1)
                }
                wave_sync();

                // ---- ResvMaxBits (src/reservoir.c:101-134) ----
                int max_bits;
                {
                    const int mb = mean_bits / C;
                    max_bits = mb > 4095 ? 4095 : mb;
                    if (ResvMax != 0) {
                        const int more_bits = (int) (po->pe * 3.1 - (double) mb);
#if defined(MP3MI_ULP_CENSUS) && !defined(MP3MI_EMU)
                        if (lane == 0) { // site 3b: (int)(pe * 3.1 - mean_bits); pe within 1.8e-12 of the reference's (k_psy.hip)
                            const double t = po->pe * 3.1 - (double) mb, fr = __builtin_fabs(t - __builtin_rint(t));
                            ULP_CENSUS(UC_PE_RESV, fr <= 6e-12, fr <= 6e-12 * 1048576.0);
                        }
#endif
                        int add_bits = 0;
                        if (more_bits > 100) {
                            const int frac = (ResvSize * 6) / 10;
                            add_bits = frac < more_bits ? frac : more_bits;
                        }
                        const int over_bits = ResvSize - ((ResvMax * 8) / 10) - add_bits;
                        if (over_bits > 0) add_bits += over_bits;
                        max_bits += add_bits;
                        if (max_bits > 4095) max_bits = 4095;
                    }
                }

                // ---- reset of iteration variables (src/loop.c:318-344) ----
                g.part2_3_length = 0; g.big_values = 0; g.count1 = 0; g.scalefac_compress = 0;
                g.table_select[0] = g.table_select[1] = g.table_select[2] = 0;
                g.region0_count = 0; g.region1_count = 0; g.part2_length = 0; g.preflag = 0;
                g.count1table_select = 0; g.q = 0;
#pragma unroll
                for (int k = 0; k < LOOP_SLOTS; k++) ((unsigned *) L.ix)[loop_pair_of(lane, k)] = 0u;
                wave_sync();

                if (nonzero) {
                    g.q = pp->q0; // quantanf_init (src/loop.c:369-402), from k_prep
                    const int test_flags = LOOP_ARG(geo.test_flags); // (tests: an exact tier only)

                    // ---- outer_loop (src/loop.c:415-558) ----
                    int iteration = 0, bits = 0, over, status, save_preflag, save_compress;
                    do {
                        const int lane = wave_lane_here(); // ... nor an iteration of the distortion loop
                        iteration++;
                        work += 5;
                        g.part2_length = loop_part2_length(g, scfsi_m);
                        int huff_bits = max_bits - g.part2_length;
                        if (huff_bits < 0) {
                            // assert( max_bits >= 0 ) of inner_loop (src/loop.c:579): the scalefactors alone exceed the
                            // granule's budget and the reference dies.  Without the assert its loop -- and the one below --
                            // would raise the step for ever: no count is <= a negative budget.  The stream is void from
                            // here on; any budget lets the search run out.
                            LOOP_REF_ABORT(MP3MI_DEV_ABORT_HUFF_BITS, LOOP_ARG(geo.fabs0) + LOOP_ARG(geo.f0) + fl);
                            huff_bits = max_bits;
                        }
                        // bin_search_StepSize (src/loop.c:2119-2140, first iteration only) and inner_loop (src/loop.c:569-606)
                        // as ONE loop around ONE copy of the quantise+count pass (the pass is ~3 k instructions; a second
                        // inlined copy is instruction-cache pressure for nothing).  The bisection probes (top + bot) / 2
                        // until the count equals max_bits or the probes are one step apart; inner_loop then raises the step
                        // until the bits fit -- and its first pass repeats the bisection's last probe (same step, same xr),
                        // which is taken over instead of recomputed.
                        {
                            bool bisect = iteration == 1;
                            int top = g.q, bot = 200, next = g.q, last = g.q;
                            for (;;) {
                                if (bisect) {
                                    last = next;
                                    next = (top + bot) / 2;
                                    g.q = next;
                                }
                                PROF(1);
                                const bool quant_exact = (test_flags & 8) != 0; // MP3MI_QUANT_EXACT=1: the quantiser's exact tier only (tests)
                                const bool az = !quant_exact && loop_all_zero(y34max, g.q);
                                work += 4;
                                const loop_qinfo qi = loop_quantize(T, L, y34, y34max, g.q, az, quant_exact, shortb);
                                PROF(2);
                                bits = loop_count_bits(T, R, L, GL, g, qi, az CBPROF_PASS);
                                PROF(3);
                                wave_sync();
                                if (bisect) {
                                    if (bits > max_bits) top = next; else bot = next;
                                    if (bits != max_bits && abs(last - next) > 1) continue;
                                    bisect = false; // this probe is inner_loop's first pass
                                }
                                if (!(bits > huff_bits)) break;
                                g.q += 1;
                            }
                        }

                        PROF(1);
                        // ---- the distortion side of the iteration.  What it knows about "its" bands and noise jobs a
                        //      lane fetches HERE (two 8-byte loads of packed constants, mp3mi_tables::lane_bands / lane_jobs),
                        //      and the per-band state comes from / goes back to L.band_*: nothing of it is alive during
                        //      the quantise+count passes above ----
                        const bool bandlane = lane < nband;
                        // (registers: the partial sums below are where the kernel's register count is set -- ten y34, four terms in
                        // flight --, so nothing that is only needed behind them is fetched or unpacked in front of them)
                        unsigned long long jobs = T->lane_jobs[shortb][lane];
                        const int jfirst = (int) (jobs & 1023ull), jcount = (int) ((jobs >> 10) & 255ull);
                        const int sstride = shortb ? 3 : 1;
                        const int jmax4 = (T->nj_max[shortb] + 3) & ~3; // the longest job, in steps of four terms
                        double xfsf_r = 0.0;
                        // calc_noise (src/loop.c:1007-1067).  The noise of a band is only ever COMPARED with the
                        // allowed distortion, and it is a sum of non-negative terms, so any summation order
                        // agrees with the reference's sequential one to within 2(n-1) ulp (n <= 102 lines:
                        // < 2.3e-14 relative; the fused square-and-add of the partial sums adds an ulp per term, the
                        // multiplication by 1 / n in place of the division 1.5).  First tier: every band is cut into parts of ~10 lines summed by
                        // different lanes.  Only if a band lands within 1e-12 of its threshold is the
                        // reference's order used (loop_noise_exact) -- at both places that compare.
                        bool xfsf_exact = (test_flags & 1) != 0;
                        const double noise_step = T->step[g.q - MP3MI_STEP_MIN];
                        double vjob = 0.0;
                        if (!xfsf_exact) vjob = shortb ? loop_noise_jobs_short(T, L, noise_step, jfirst, jcount, jmax4) : loop_noise_jobs_long(T, L, noise_step, jfirst, jcount, jmax4);
                        // band of each of this lane's five PAIRS (a band's edges are even: both lines of a pair are of one band), 6 bits
                        // each; short blocks: the lines of a pair belong to two windows, i.e. two band lanes: 10 fields of a 64-bit word
                        // (asked for here: its latency passes under the band sums' reduction)
                        const unsigned long long bandpack = T->lane_bands[shortb][wave_lane_here()];
                        const double inv_lines = T->lane_inv_lines[shortb][wave_lane_here()]; // 1 / (lines of this band lane's band)
                        // the band lane's state (fetched behind the partial sums, see above)
                        const int bl = wave_lane_here();
                        double xmin_r = bandlane ? L.band_xmin[bl] : 0.0;
                        int sf_r = bandlane ? L.band_sf[bl] : 0;
                        {
                            if (!xfsf_exact) {
                                // The jobs of a band sit in consecutive lanes: a segmented sum by doubling (lane l takes
                                // over the sum of lane l + d where that is a job of the same band: bit of jseg) leaves
                                // the band's sum in its first job's lane, where the band lane fetches it.  Any order
                                // of these non-negative terms is as good as another here (see above).
                                double v = vjob;
                                jobs = wave_opaque_u64(jobs);
                                const int jseg = (int) ((jobs >> 18) & 31ull), pj0 = (int) ((jobs >> 23) & 63ull), scount = (int) ((jobs >> 35) & 255ull);
                                // (a band has at most 16 jobs -- tables_host.cpp refuses a table with more -- so four doublings do)
                                const int lane4 = 4 * lane;
                                { const double o = wave_down_f64<1>(v, lane4); v = v + ((jseg & 1) ? o : 0.0); }
                                { const double o = wave_down_f64<2>(v, lane4); v = v + ((jseg & 2) ? o : 0.0); }
                                { const double o = wave_down_f64<4>(v, lane4); v = v + ((jseg & 4) ? o : 0.0); }
                                { const double o = wave_down_f64<8>(v, lane4); v = v + ((jseg & 8) ? o : 0.0); }
                                const double sum = __shfl(v, pj0);
                                (void) scount;
                                xfsf_r = bandlane ? sum * inv_lines : 0.0; // (first tier: within 1.5 ulp of the reference's quotient; the exact tier divides)
                                if (wave_any(loop_noise_close(bandlane, xfsf_r, xmin_r))) xfsf_exact = true;
                            }
                            if (xfsf_exact) xfsf_r = loop_noise_exact(T, L, noise_step, bandlane, (int) ((jobs >> 43) & 1023ull), (int) ((jobs >> 35) & 255ull), sstride);
                        }
                        if (bandlane) L.band_sfsave[lane] = sf_r; // the result of this iteration stands (src/loop.c:505-519)
                        save_preflag = g.preflag;
                        save_compress = g.scalefac_compress;
                        // bands whose noise exceeds the allowed distortion (bit b = band lane b)
                        const unsigned long long viol = __ballot(bandlane && xfsf_r > xmin_r);

                        PROF(4);
                        // preemphasis (src/loop.c:1161-1214)
                        {
                            bool skip = false;
                            if (scfsi_m) {
                                g.preflag = L.preflag0[ch];
                                skip = true;
                            }
                            if (!skip && g.block_type != 2 && g.preflag == 0) {
                                if ((viol & 0x1E0000ull) == 0x1E0000ull) { // sfb 17..20 all violate
                                    g.preflag = 1;
                                    if (lane < g.sfb_lmax) xmin_r = xmin_r * T->pretab_xmin[LOOP_PRETAB[lane]];
                                    // the thresholds moved: amp_scalefac_bands compares against the new ones
                                    if (!xfsf_exact && wave_any(loop_noise_close(bandlane, xfsf_r, xmin_r))) {
                                        xfsf_exact = true;
                                        xfsf_r = loop_noise_exact(T, L, noise_step, bandlane, (int) ((jobs >> 43) & 1023ull), (int) ((jobs >> 35) & 255ull), sstride);
                                    }
                                    loop_preemph_lines(T, L, y34, bandpack, lane, g.sfb_lmax);
                                    y34max = y34max * LOOP_Y34MAX_GROW;
                                }
                            }
                        }
                        wave_sync();

                        // amp_scalefac_bands (src/loop.c:1225-1350)
                        {
                            int copySF = 0, preventSF = 0;
                            if (scfsi_m) {
                                if (iteration == 1) copySF = 1; else preventSF = 1;
                            }
                            const double ifqstep = T->sqrt2, ifqstep2 = ifqstep * ifqstep;
                            bool amp = false;
                            if (bandlane) {
                                bool skipband = false;
                                if (!shortb && (copySF || preventSF)) {
                                    const int sb4 = (lane < 6) ? 0 : (lane < 11 ? 1 : (lane < 16 ? 2 : 3));
                                    if ((scfsi_m >> sb4) & 1) {
                                        if (copySF) sf_r = L.sf_gr0[ch][lane];
                                        skipband = true;
                                    }
                                }
                                if (!skipband && xfsf_r > xmin_r) {
                                    amp = true;
                                    xmin_r = xmin_r * ifqstep2;
                                    sf_r = sf_r + 1;
                                }
                                L.band_xmin[lane] = xmin_r; // (pre-emphasised and / or doubled, or as it was)
                                L.band_sf[lane] = sf_r;
                            }
                            const unsigned long long ampmask = __ballot(amp); // bit b = band lane b amplified
                            over = __popcll(ampmask);
                            if (over) {
                                // The amplified bands are a few runs of consecutive lines, so most of the five slots of 64
                                // pairs hold none of them: a slot's lines are skipped as a whole,
                                // and inside a slot only the amplified lines touch the LDS.  ampmask only has bits of
                                // band lanes, so lines above the last band (b >= nband) find a zero bit.
                                if (!shortb) { // a pair is of one band; 21 band lanes: the mask is one word
                                    loop_amp_pairs(L, y34, (unsigned) bandpack, (unsigned) ampmask, ifqstep, lane);
                                } else {
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
                            }
                        }
                        wave_sync(); // amplified lines in L.xr are read by other lanes' noise sums

                        PROF(5);
                        // loop_break (src/loop.c:1131-1152) then scale_bitcount (src/loop.c:792-860)
                        {
                            status = !wave_any(bandlane && sf_r == 0);
                            if (status == 0) {
                                int m1, m2;
                                if (shortb) {
                                    m1 = (lane < 18) ? sf_r : 0;
                                    m2 = (lane >= 18 && lane < 36) ? sf_r : 0;
                                } else {
                                    m1 = (lane < 11) ? sf_r : 0;
                                    m2 = (lane >= 11 && lane < 21) ? sf_r : 0;
                                }
                                int mmv[2] = {m1, m2};
                                wave_reduce_i32<0, 2>(mmv); // in lock-step: each fills the other's DPP wait states
                                const int mm1 = mmv[0], mm2 = mmv[1];
                                // the first k with mm1 < 2^slen1[k] and mm2 < 2^slen2[k] only depends on the bit lengths
                                // of the two maxima: tabulated, a nibble per (length of mm1 <= 4, length of mm2 <= 3)
                                const int bl1 = 32 - __clz(mm1), bl2 = 32 - __clz(mm2);
                                int ep = 2;
                                if (bl1 <= 4 && bl2 <= 3) {
                                    const unsigned long long w = bl1 < 4 ? (0xdcb4a98476543210ull >> (16 * bl1)) : 0xfeeeull;
                                    g.scalefac_compress = (int) ((w >> (4 * bl2)) & 15ull);
                                    ep = 0;
                                }
                                status = ep;
                            }
                        }
                    } while (status == 0 && over > 0);
                    g.preflag = save_preflag;
                    g.scalefac_compress = save_compress;
                    g.part2_length = loop_part2_length(g, scfsi_m);
                    g.part2_3_length = g.part2_length + bits;
                }

                // ResvAdjust (src/reservoir.c:141-145), global_gain (src/loop.c:357)
                ResvSize += (mean_bits / C) - g.part2_3_length;
                const int global_gain = loop_nint((double) g.q + 210.0);
                if (global_gain >= 256) LOOP_REF_ABORT(MP3MI_DEV_ABORT_GLOBAL_GAIN, LOOP_ARG(geo.fabs0) + LOOP_ARG(geo.f0) + fl); // assert, src/loop.c:358

                PROF(6);
                // ---- hand the granule over: signed ix (src/l3bitstream.c:115-125) and side info ----
                loop_kargs_p ko = loop_kargs_ptr(ka);
                unsigned *ix_out = (unsigned *) ko->ix_out;
#pragma unroll
                for (int k = 0; k < LOOP_SLOTS; k++) {
                    const int pr = loop_pair_of(lane, k);
                    if (k < 4 || pr < 288) {
                        const unsigned w = ((const unsigned *) L.ix)[pr]; // what the last pass (or the reset) left
                        int x = (int) (w & 0xffffu), y = (int) (w >> 16);
                        if (L.xr[2 * pr] < 0 && x > 0) x = -x;
                        if (L.xr[2 * pr + 1] < 0 && y > 0) y = -y;
                        ix_out[rec * 288 + pr] = ((unsigned) x & 0xffffu) | ((unsigned) y << 16);
                    }
                }
                {
                    mp3mi_gr_side *o = &ko->side_out[(size_t) s * ko->geo.nf + fl].gr[gr][ch]; // straight to memory
                    if (lane == 0) {
                        o->part2_3_length = g.part2_3_length; o->big_values = g.big_values; o->count1 = g.count1;
                        o->global_gain = global_gain; o->scalefac_compress = g.scalefac_compress;
                        o->window_switching_flag = g.wsf; o->block_type = g.block_type;
                        o->table_select[0] = g.table_select[0]; o->table_select[1] = g.table_select[1];
                        o->table_select[2] = g.table_select[2];
                        o->region0_count = g.region0_count; o->region1_count = g.region1_count;
                        o->preflag = g.preflag; o->count1table_select = g.count1table_select;
                        o->part2_length = g.part2_length;
                        L.p23[gr][ch] = g.part2_3_length;
                        if (gr == 0) L.preflag0[ch] = g.preflag;
                        L.st.addr[gr][ch][0] = g.address1; L.st.addr[gr][ch][1] = g.address2; L.st.addr[gr][ch][2] = g.address3;
                    }
                    if (lane < 39) { // the scalefactors of the last iteration whose result stands (all 0 without a search)
                        const int sfv = lane < nband ? L.band_sfsave[lane] : 0;
                        o->scalefac[lane] = sfv;
                        if (gr == 0 && lane < 21) L.sf_gr0[ch][lane] = shortb ? 0 : sfv;
                    }
                }
                wave_sync();
            }

        // ---- ResvFrameEnd (src/reservoir.c:155-226) ----
        if (C == 2 && (mean_bits & 1)) ResvSize += 1;
        {
            int over_bits = ResvSize - ResvMax;
            if (over_bits < 0) over_bits = 0;
            ResvSize -= over_bits;
            int stuffingBits = over_bits;
            if ((over_bits = ResvSize % 8)) { stuffingBits += over_bits; ResvSize -= over_bits; }
            if (lane == 0) {
                bool moved = false; // some part2_3_length took stuffing bits: the records in memory follow
                if (stuffingBits) {
                    moved = true;
                    if (L.p23[0][0] + stuffingBits < 4095)
                        L.p23[0][0] += stuffingBits;
                    else {
                        for (int gr = 0; gr < 2; gr++)
                            for (int ch = 0; ch < C; ch++) {
                                if (stuffingBits == 0) break;
                                const int extra = 4095 - L.p23[gr][ch];
                                const int now = extra < stuffingBits ? extra : stuffingBits;
                                L.p23[gr][ch] += now;
                                stuffingBits -= now;
                            }
                        resvDrain = stuffingBits;
                    }
                }
                mp3mi_frame_side *o = &LOOP_ARG(side_out)[(size_t) s * LOOP_ARG(geo.nf) + fl];
                if (moved)
                    for (int gr = 0; gr < 2; gr++)
                        for (int ch = 0; ch < C; ch++) o->gr[gr][ch].part2_3_length = L.p23[gr][ch];
                o->main_data_begin = main_data_begin;
                o->resvDrain = resvDrain;
                L.st.ResvSize = ResvSize;
            }
        }
        wave_sync();
#if !defined(MP3MI_EMU)
        // Pacing: the kernel ends when its slowest stream ends, and streams differ by up to 1.5x in
        // work.  gate_count[1] counts the frames finished by all streams of this launch; a stream
        // behind the average raises its wave priority (it then issues ahead of the three other
        // wavefronts of its SIMD), a stream ahead of it lowers it.  Purely a scheduling hint.
        unsigned *gate_count = LOOP_ARG(gate_count);
        if (gate_count) {
            const unsigned done_all = __builtin_amdgcn_readfirstlane((int) (lane == 0 ? atomicAdd(gate_count + 1, 1u) + 1u : 0u));
            // (frames per wavefront so far against the average over the wavefronts of the launch: a wavefront on its
            // second stream has that stream's frames on top of the first one's)
            const int n_act = LOOP_ARG(geo.n_streams); // (fetched and converted here, once per frame)
            const float lead = (float) (fl + 1) - (float) done_all / (float) n_act;
            if (lead < -1.0f) __builtin_amdgcn_s_setprio(3);
            else if (lead < 0.0f) __builtin_amdgcn_s_setprio(2);
            else if (lead < 1.0f) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
#endif
    }
    {
        const int ln = wave_lane_here(); // (not the address the state was loaded through, kept alive across the whole kernel)
        if (ln == 0) L.st.ref_abort = ref_abort;
        wave_sync();
        for (int i = ln; i < (int) (sizeof(mp3mi_loop_state) / 4); i += 64) ((int *) &LOOP_ARG(state)[s])[i] = ((const int *) &L.st)[i];
    }
    {
        int *cost = LOOP_ARG(place.cost);
        if (cost && lane == 0) cost[s] = work;
    }
#if defined(MP3MI_LOOP_PROFILE) && !defined(MP3MI_EMU)
    if (lane == 0 && s < 65536) g_loop_work[s] = (unsigned long long) work | ((unsigned long long) __builtin_amdgcn_s_memrealtime() << 20);
#endif
    PROF(7);
    PROF_END;
}

// what every wavefront of a workgroup does first: its share of the code-length tables (the workgroup's only barrier;
// from there on every wavefront is on its own)
#define LOOP_KERNEL_PROLOGUE                                                                                         \
    __shared__ loop_lds LL[LOOP_W];                                                                                  \
    __shared__ uint16_t GL[928]; /* code lengths grouped as new_choose_table compares them (mp3mi_tables::glut) */    \
    const int wv = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);                                           \
    loop_lds &L = LL[wv];                                                                                            \
    for (int i = (int) threadIdx.x; i < 928; i += 64 * LOOP_W) GL[i] = T->glut[i];                                   \
    __syncthreads()

// As many wavefronts as streams, each takes one.
__global__ void __attribute__((amdgpu_num_vgpr(80))) __launch_bounds__(64 * LOOP_W) k_loop(const mp3mi_tables *__restrict__ T, loop_kargs A)
{
    LOOP_KERNEL_PROLOGUE;
    const int block = (int) blockIdx.x * LOOP_W + wv;
#if defined(MP3MI_EMU)
    loop_kargs_p ka = &A;
#else
    // (the record follows the table pointer in the kernel argument segment)
    loop_kargs_p ka = (loop_kargs_p) ((const __attribute__((address_space(4))) char *) __builtin_amdgcn_kernarg_segment_ptr() + sizeof(void *));
    static_assert(alignof(loop_kargs) == 8, "loop_kargs follows an 8-byte argument");
#endif
    if (block < A.geo.n_streams) loop_stream(T, ka, L, GL, block);
}

#if defined(MP3MI_LOOP_PROFILE) && !defined(MP3MI_EMU)
extern "C" void mp3mi_debug_loop_profile(unsigned long long *out)
{
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out, HIP_SYMBOL(g_loop_prof), sizeof(z));
    hipMemcpyToSymbol(HIP_SYMBOL(g_loop_prof), z, sizeof(z));
}
extern "C" void mp3mi_debug_cb_profile(unsigned long long *out)
{
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cb_prof), sizeof(z));
    hipMemcpyToSymbol(HIP_SYMBOL(g_cb_prof), z, sizeof(z));
}
extern "C" void mp3mi_debug_loop_work(unsigned long long *out, int n_streams)
{
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out, HIP_SYMBOL(g_loop_work), sizeof(unsigned long long) * (size_t) n_streams);
}
extern "C" void mp3mi_debug_loop_starts(unsigned long long *out, int n_streams)
{
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out, HIP_SYMBOL(g_loop_start), sizeof(unsigned long long) * (size_t) n_streams);
}
extern "C" void mp3mi_debug_loop_waves(unsigned long long *out, int n_streams)
{
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out, HIP_SYMBOL(g_loop_wave), sizeof(unsigned long long) * 2 * (size_t) n_streams);
}
#endif

// workgroups that are resident together: four of LOOP_W = 4 wavefronts per CU (four wavefronts per SIMD: what stays
// resident beside the feed-forward kernels, batch.cpp)
static int loop_wg_cap(void) { return mp3mi_current_cu_count() * 4; }

// streams one launch of k_loop holds resident, a wavefront each
int mp3mi_loop_resident(void) { return loop_wg_cap() * LOOP_W; }

// A wavefront per stream.  batch.cpp cuts a batch into parts of at most mp3mi_loop_resident() streams, so that a launch is
// resident at once; a larger launch (the emulator's parts of 64 streams) is valid all the same: the hardware starts the
// workgroups beyond the resident ones as others end.
void mp3mi_launch_loop(const mp3mi_tables *T, const mp3mi_geom &g, const double *xr, const mp3mi_psy_out *psy,
                       const mp3mi_loop_prep *prep, const int32_t *bits_per_frame, void *loop_state, int16_t *ix,
                       mp3mi_frame_side *side, unsigned *gate_count, mp3mi_loop_place place, hipStream_t st)
{
    const int want = (g.n_streams + LOOP_W - 1) / LOOP_W;
    loop_kargs A;
    A.geo = g; A.xr_all = xr; A.psy = psy; A.prep = prep; A.bits_per_frame = bits_per_frame;
    A.state = (mp3mi_loop_state *) loop_state; A.ix_out = ix; A.side_out = side; A.gate_count = gate_count; A.place = place;
    hipLaunchKernelGGL(k_loop, dim3((unsigned) want), dim3(64 * LOOP_W), 0, st, T, A);
}

// Holds the front stream back until the k_loop launch whose census target is `target` has (all but
// a few of) its wavefronts running, so that the feed-forward kernels queued behind this one fill the
// chip BEHIND k_loop instead of taking its wave slots.  One wavefront, a BOUNDED wait (max_ticks of
// the 100 MHz real-time counter): k_loop fills every register file, so the slot this wavefront
// occupies keeps one k_loop wavefront out until it leaves -- hence "all but a few", and hence short.
__global__ void __launch_bounds__(64) k_gate(const unsigned *__restrict__ count, unsigned target, unsigned max_ticks)
{
#if !defined(MP3MI_EMU)
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while ((int) (__hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {
        if (__builtin_amdgcn_s_memrealtime() - t0 > (unsigned long long) max_ticks) break;
        __builtin_amdgcn_s_sleep(32);
    }
#endif
}

void mp3mi_launch_gate(const unsigned *count, unsigned target, unsigned max_ticks, hipStream_t st)
{
    hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, st, count, target, max_ticks);
}

// Holds the loop stream back in front of the LAST k_loop of a call until the call AFTER it has had its first transforms
// (k_fft takes whole CUs' LDS: run behind that k_loop's start they would wait for its end, and everything of the next
// call's first chunk with them -- 20 ms of an otherwise idle chip per call), or until the host lets go (a call that waits
// for results: batch.cpp, hold_release), or until max_ticks of the 100 MHz counter have passed: the hold only ever
// changes WHEN the kernel behind it starts, never what it computes, so running out is harmless.  flag[] is host memory
// mapped into the device's address space; tickets only ever grow.  flag[0]: the highest ticket a NEXT CALL has let go
// (k_hold_release, on the device, behind that call's first transforms); flag[1 + ticket % 8]: the ticket the HOST lets go -- that
// one and no other: the host runs far ahead of the device, and when it waits for the last call it must not let go the holds of
// the calls before it, which the device has not reached yet and whose successors are already queued.  (A ring of eight words:
// a release the device has not looked at yet survives the next seven.)
__global__ void __launch_bounds__(64) k_hold(const unsigned *flag, unsigned ticket, unsigned max_ticks)
{
#if !defined(MP3MI_EMU)
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while ((int) (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - ticket) < 0 &&
           __hip_atomic_load(flag + 1 + (ticket & 7u), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != ticket) {
        if (__builtin_amdgcn_s_memrealtime() - t0 > (unsigned long long) max_ticks) break;
        __builtin_amdgcn_s_sleep(64);
    }
#endif
}
__global__ void __launch_bounds__(64) k_hold_release(unsigned *flag, unsigned ticket)
{
#if defined(MP3MI_EMU)
    if (threadIdx.x == 0 && (int) (*flag - ticket) < 0) *flag = ticket;
#else
    if (threadIdx.x == 0) __hip_atomic_fetch_max(flag, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
#endif
}
void mp3mi_launch_hold(const unsigned *flag, unsigned ticket, unsigned max_ticks, hipStream_t st)
{
    hipLaunchKernelGGL(k_hold, dim3(1), dim3(64), 0, st, flag, ticket, max_ticks);
}
void mp3mi_launch_hold_release(unsigned *flag, unsigned ticket, hipStream_t st)
{
    hipLaunchKernelGGL(k_hold_release, dim3(1), dim3(64), 0, st, flag, ticket);
}

ULP_CENSUS_ACCESSOR(mp3mi_debug_ulp_census_loop)
