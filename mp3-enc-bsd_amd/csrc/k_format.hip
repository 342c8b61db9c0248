// Layer III bitstream formatting: header + side information, scalefactors, Huffman code
// words, count1 quadruples, stuffing, and placement of each frame's main data behind its
// back pointer.
//
// Replaces III_format_bitstream / encodeSideInfo / encodeMainData / Huffmancodebits
// (src/l3bitstream.c:67-767), HuffmanCode (src/huffcode.h:16-139), BF_BitstreamFrame /
// WriteMainDataBits (src/formatBitstream.c:52-270) and putbits (src/common.c:1134-1161).
//
// The reference interleaves main data and headers through a queue; because the stream is
// CBR without padding (src/musicin.c:566-581) the result has a closed form: header n sits at
// byte n*frame_bytes, and byte k of the concatenated main data sits in slot k / slot_bytes at
// offset k % slot_bytes behind that slot's header + side info.  Frame n's main data starts at
// main-data offset n*slot_bytes - main_data_begin[n].  Hence every frame formats independently:
// one wavefront per (stream, frame); lanes own code words, a wave prefix sum of the code
// lengths gives each word its bit position, words are OR-ed into an LDS image and the image
// is scattered to the frame's byte positions.
#include "mp3mi_host.h"

struct fmt_lds {
    unsigned words[640];  // main data image, big-endian bit order inside each word
    unsigned si[12];      // header + side info image (<= 36 bytes)
    int sfb_l[23], sfb_s[14];
    unsigned ht_meta[34]; // Huffman table t: first cell | ylen << 16 | linbits << 24 (a code word's cell then is ONE round trip away)
    mp3mi_frame_side side; // the frame's side information: one coalesced read, then every field from here (the kernel reads some
                           // sixty of them, one by one and in dependent steps: from memory that was a round trip each)
};

__device__ static const int FMT_SLEN1[16] = {0, 0, 0, 0, 3, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4};
__device__ static const int FMT_SLEN2[16] = {0, 1, 2, 3, 0, 1, 2, 3, 1, 2, 3, 1, 2, 3, 2, 3};

MP3MI_DEVFN void fmt_or(unsigned *w, unsigned v)
{
#if defined(MP3MI_EMU)
    *w |= v;
#else
    atomicOr(w, v);
#endif
}

// put the low n bits of val at bit position pos (MSB first) of a word image
MP3MI_DEVFN void fmt_put(unsigned *img, int pos, unsigned val, int n)
{
    if (n <= 0) return;
    if (n < 32) val &= (1u << n) - 1u;
    const int wi = pos >> 5, off = pos & 31;
    if (off + n <= 32)
        fmt_or(&img[wi], val << (32 - off - n));
    else {
        const int n2 = off + n - 32;
        fmt_or(&img[wi], val >> n2);
        fmt_or(&img[wi + 1], val << (32 - n2));
    }
}

// exclusive prefix sum over the wave; *total receives the wave sum
MP3MI_DEVFN int fmt_scan(int v, int *total)
{
#if !defined(MP3MI_EMU)
    // inclusive scan inside every row of 16 lanes by four shifts (a lane without a source adds 0), then the totals of row 0
    // into row 1 and of row 2 into row 3 (row_bcast15), then lane 31's -- rows 0 + 1 -- into rows 2 and 3 (row_bcast31): six
    // vector instructions, where six __shfl_up cost an LDS-pipe instruction, an address and a select each
    int incl = v;
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, false); // row_shr:1
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, false); // row_shr:2
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, false); // row_shr:4
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, false); // row_shr:8
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xa, 0xf, false); // row_bcast15 into rows 1 and 3
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xc, 0xf, false); // row_bcast31 into rows 2 and 3
    *total = __builtin_amdgcn_readlane(incl, 63);
    return incl - v;
#else
    const int lane = wave_lane();
    int incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, (unsigned) d);
        if (lane >= d) incl += o;
    }
    *total = __shfl(incl, 63);
    return incl - v;
#endif
}

// code word(s) of one big-value pair (src/huffcode.h:16-139): code/cbits then ext/xbits
MP3MI_DEVFN void fmt_pair(const mp3mi_tables *T, const unsigned *ht_meta, int t, int x, int y, unsigned *code, int *cbits,
                          unsigned *ext, int *xbits)
{
    *code = 0; *cbits = 0; *ext = 0; *xbits = 0;
    if (t == 0) return;
    unsigned signx = 0, signy = 0;
    if (x < 0) { x = -x; signx = 1; }
    if (y < 0) { y = -y; signy = 1; }
    const unsigned meta = ht_meta[t];
    const int ylen = (int) ((meta >> 16) & 255u), linbits = (int) (meta >> 24), toff = (int) (meta & 0xffffu);
    if (t > 15) {
        unsigned lx = 0, ly = 0, e = 0;
        int xb = 0;
        const int x0 = x, y0 = y;
        if (x > 14) { lx = (unsigned) (x - 15); x = 15; }
        if (y > 14) { ly = (unsigned) (y - 15); y = 15; }
        const int idx = toff + x * ylen + y;
        *code = T->ht_code[idx];
        *cbits = T->ht_len[idx];
        if (x0 > 14) { e |= lx; xb += linbits; }
        if (x0 != 0) { e <<= 1; e |= signx; xb += 1; }
        if (y0 > 14) { e <<= linbits; e |= ly; xb += linbits; }
        if (y0 != 0) { e <<= 1; e |= signy; xb += 1; }
        *ext = e;
        *xbits = xb;
    } else {
        const int idx = toff + x * ylen + y;
        unsigned c = T->ht_code[idx];
        int cb = T->ht_len[idx];
        if (x != 0) { c = (c << 1) | signx; cb += 1; }
        if (y != 0) { c = (c << 1) | signy; cb += 1; }
        *code = c;
        *cbits = cb;
    }
}

// BF_FlushBitstream (src/formatBitstream.c:87-105) writes sum(frameLength - SILength) zero bits over the queued headers in
// words of 32 and ends with WriteMainDataBits(0, bits % 32).  When the main data written so far ends exactly on a slot
// boundary (nothing left in the current slot) with k >= 1 headers still queued and k * slot bits are a multiple of 32, that
// last call has nothing to write but finds BitCount == ThisFrameSize, asks for another header and get_side_info's
// assert( l ) fails (src/formatBitstream.c:225-230, 381-390): the reference dies in its flush.  n_done frames encoded,
// m_end bytes of main data written, slot = main-data bytes per frame.
MP3MI_DEVFN bool fmt_flush_dies(long n_done, long m_end, int slot)
{
    if (n_done <= 0) return false;
    const long written = (m_end + slot - 1) / slot; // headers written so far: one per slot the main data has entered
    const long queued = n_done - written;
    return queued >= 1 && written * slot == m_end && ((queued * (long) slot * 8) % 32) == 0;
}

// Length of the file of a stream that ends after n_done frames with m_end bytes of main data written
// (src/formatBitstream.c:87-120 + src/common.c:843-868, 968): the flush stops short of the last slot by what the current
// slot still has free, and close writes the byte under construction as well.  No frames: no file body.
MP3MI_DEVFN long fmt_file_end(long n_done, long m_end, int slot, int frame_bytes)
{
    if (n_done <= 0) return 0;
    const long rem = ((m_end + slot - 1) / slot) * slot - m_end;
    return n_done * frame_bytes - rem + 1;
}

#define FMT_KERNEL_ARGS const mp3mi_tables *__restrict__ T, mp3mi_geom geo, const int16_t *__restrict__ ix_all,                          \
                        const mp3mi_frame_side *__restrict__ side_all, const int32_t *__restrict__ bits_per_frame,                 \
                        const int32_t *__restrict__ bitrate_index, uint8_t *__restrict__ out, size_t out_stride,                   \
                        uint32_t *__restrict__ out_len, int32_t *__restrict__ loop_state, int loop_state_words,                    \
                        unsigned *__restrict__ voided

// one frame of one stream, by one wavefront (the body of k_format and of k_format_marked)
MP3MI_DEVFN void fmt_frame(fmt_lds &L, FMT_KERNEL_ARGS)
{
    const int lane = wave_lane();
    const int C = geo.channels, G = geo.n_gran;
    const int fl = (int) blockIdx.x % geo.nf, s = (int) blockIdx.x / geo.nf;
    const long n_call = (long) geo.f0 + fl;     // frame index within this call
    const long n_abs = (geo.fabs_s ? (long) geo.fabs_s[s] : geo.fabs0) + n_call; // and within the stream: what places the frame in the file
    // ragged batch: this stream's frame count; frames beyond it were not encoded and emit nothing
    const long n_frames_s = geo.n_samples ? ((long) geo.n_samples[s] + 1151) / 1152 : (long) geo.n_frames;
    if (n_call >= n_frames_s) {
        if (n_frames_s == 0 && n_call == 0 && geo.whole_file && wave_lane() == 0) out_len[s] = 0; // no samples, no file body
        return;
    }
    {
        const int32_t *src = (const int32_t *) &side_all[(size_t) s * geo.nf + fl];
        for (int i = lane; i < (int) (sizeof(mp3mi_frame_side) / 4); i += 64) ((int32_t *) &L.side)[i] = src[i];
    }
    const mp3mi_frame_side *sd = &L.side; // (valid behind the barrier below)
    // ... and the frame's quantised values as pairs, a word a lane and step, for all four (granule, channel) records at once:
    // where they are does not depend on the side information, so they travel together with it (pair e = lines 2 e, 2 e + 1)
    unsigned pw[4][5];
#pragma unroll
    for (int gc = 0; gc < 4; gc++) {
        const size_t rec = ((size_t) s * G + (2 * fl + (gc >= C ? 1 : 0))) * C + (gc >= C ? gc - C : gc);
        const unsigned *ixw = (const unsigned *) (ix_all + rec * 576);
#pragma unroll
        for (int j = 0; j < 5; j++) pw[gc][j] = (gc < 2 * C && 64 * j + lane < 288) ? ixw[64 * j + lane] : 0u;
    }
    const int frame_bytes = bits_per_frame[s] / 8;
    const int crc_bits = geo.crc ? 16 : 0; // the reference's CRC word for Layer III is always 0 (src/l3bitstream.c:312, 338-342)
    const int si_bytes = (32 + crc_bits + (C == 2 ? 256 : 136)) / 8;
    const int slot = frame_bytes - si_bytes;
    // byte 0 of the stream's output row is file position out_base[s] (streaming: what earlier calls delivered)
    uint8_t *dst = out + (size_t) s * out_stride - (geo.out_base ? (size_t) geo.out_base[s] : (size_t) 0);

    for (int i = lane; i < 640; i += 64) L.words[i] = 0;
    if (lane < 12) L.si[lane] = 0;
    if (lane < 23) L.sfb_l[lane] = T->sfb_l[lane];
    if (lane < 14) L.sfb_s[lane] = T->sfb_s[lane];
    if (lane < 34) L.ht_meta[lane] = (unsigned) T->ht_off[lane] | ((unsigned) T->ht_ylen[lane] << 16) | ((unsigned) T->ht_linbits[lane] << 24);
    __syncthreads();

    // ---- header and side information (src/l3bitstream.c:314-458) ----
    if (lane == 4) {
        int pos = 0;
        fmt_put(L.si, pos, 0xfff, 12); pos += 12;
        fmt_put(L.si, pos, 1, 1); pos += 1;                       // MPEG-1
        fmt_put(L.si, pos, 1, 2); pos += 2;                       // 4 - layer
        fmt_put(L.si, pos, geo.crc ? 0u : 1u, 1); pos += 1;       // protection bit: set = no CRC
        fmt_put(L.si, pos, (unsigned) bitrate_index[s], 4); pos += 4;
        fmt_put(L.si, pos, (unsigned) T->rate_idx, 2); pos += 2;
        pos += 2;                                                 // padding 0, extension 0
        fmt_put(L.si, pos, (unsigned) geo.hdr_mode, 2); pos += 2; // mode
        fmt_put(L.si, pos, (unsigned) geo.hdr_flags, 6); pos += 6; // mode_ext, copyright, original, emphasis
        pos += crc_bits;                                          // CRC word: zeros
        fmt_put(L.si, pos, (unsigned) sd->main_data_begin, 9); pos += 9;
        pos += (C == 2) ? 3 : 5;                                  // private_bits 0
        for (int ch = 0; ch < C; ch++)
            for (int b = 0; b < 4; b++) { fmt_put(L.si, pos, (unsigned) sd->scfsi[ch][b], 1); pos += 1; }
    }
    if (lane < 2 * C) {
        const int gr = lane / C, ch = lane % C;
        const mp3mi_gr_side *g = &sd->gr[gr][ch];
        int pos = 32 + crc_bits + 9 + ((C == 2) ? 3 : 5) + 4 * C + 59 * lane;
        fmt_put(L.si, pos, (unsigned) g->part2_3_length, 12); pos += 12;
        fmt_put(L.si, pos, (unsigned) g->big_values, 9); pos += 9;
        fmt_put(L.si, pos, (unsigned) g->global_gain, 8); pos += 8;
        fmt_put(L.si, pos, (unsigned) g->scalefac_compress, 4); pos += 4;
        fmt_put(L.si, pos, (unsigned) g->window_switching_flag, 1); pos += 1;
        if (g->window_switching_flag) {
            fmt_put(L.si, pos, (unsigned) g->block_type, 2); pos += 2;
            pos += 1; // mixed_block_flag 0
            fmt_put(L.si, pos, (unsigned) g->table_select[0], 5); pos += 5;
            fmt_put(L.si, pos, (unsigned) g->table_select[1], 5); pos += 5;
            pos += 9; // subblock_gain 0
        } else {
            for (int r = 0; r < 3; r++) { fmt_put(L.si, pos, (unsigned) g->table_select[r], 5); pos += 5; }
            fmt_put(L.si, pos, (unsigned) g->region0_count, 4); pos += 4;
            fmt_put(L.si, pos, (unsigned) g->region1_count, 3); pos += 3;
        }
        fmt_put(L.si, pos, (unsigned) g->preflag, 1); pos += 1;
        pos += 1; // scalefac_scale 0
        fmt_put(L.si, pos, (unsigned) g->count1table_select, 1);
    }

    // ---- main data (src/l3bitstream.c:174-310, 516-716) ----
    int gpos = 0; // bit position of the current granule-channel in the image
#pragma unroll
    for (int gc = 0; gc < 4; gc++) {
        if (gc < 2 * C) {
            const int gr = gc >= C ? 1 : 0, ch = gc >= C ? gc - C : gc;
            const mp3mi_gr_side *g = &sd->gr[gr][ch];
            const size_t rec = ((size_t) s * G + (2 * fl + gr)) * C + ch;
            const int16_t *ix = ix_all + rec * 576;
            const bool shortb = g->window_switching_flag && g->block_type == 2;
            const int slen1 = FMT_SLEN1[g->scalefac_compress], slen2 = FMT_SLEN2[g->scalefac_compress];
            int pos = gpos, total;
            { // scalefactors
                int n = 0;
                if (shortb) { if (lane < 36) n = (lane < 18) ? slen1 : slen2; }
                else if (lane < 21) {
                    const int band = (lane < 6) ? 0 : (lane < 11 ? 1 : (lane < 16 ? 2 : 3));
                    if (gr == 0 || sd->scfsi[ch][band] == 0) n = (lane < 11) ? slen1 : slen2;
                }
                const int ofs = fmt_scan(n, &total);
                if (n) fmt_put(L.words, pos + ofs, (unsigned) g->scalefac[lane], n);
                pos += total;
            }
            // Code words: EVERYTHING THAT COMES OUT OF MEMORY FIRST -- the pairs and quadruples of every step of the granule and the
            // table entries they select (two dependent round trips a step) are independent of the bit positions, so all of the
            // granule's (at most five + three) steps are asked for together; the positions -- a scan per step -- and the puts follow.
            // (One step at a time, load - look up - scan - put, the kernel spent 77 % of its wavefronts' time waiting, and its
            // 315 000 one-wavefront workgroups kept the transforms' and k_mdct's out of the CUs for 3.4 ms between two k_loop launches.)
            const int bigvalues = g->big_values * 2;
            const int r1s = (shortb || !bigvalues) ? 0 : L.sfb_l[g->region0_count + 1];
            const int r2s = (shortb || !bigvalues) ? 0 : L.sfb_l[g->region0_count + g->region1_count + 2];
            // (a granule has 576 lines: at most 288 pairs -- five steps of 64 -- and 144 quadruples -- three)
            const int npairs = bigvalues ? (shortb ? 288 : (bigvalues / 2 < 288 ? bigvalues / 2 : 288)) : 0;
            const int nquad = g->count1 < 144 ? g->count1 : 144;
            const int ts0 = g->table_select[0], ts1 = g->table_select[1], ts2 = g->table_select[2];
            const int toff = (int) (L.ht_meta[32 + g->count1table_select] & 0xffffu);
            unsigned code[5], ext[5], qval[3];
            int cb[5], xb[5], qnb[3];
#pragma unroll
            for (int j = 0; j < 5; j++) {
                code[j] = 0; ext[j] = 0; cb[j] = 0; xb[j] = 0;
                if (64 * j < npairs) {
                    const int e = 64 * j + lane;
                    if (e < npairs) {
                        int x, y, t;
                        if (shortb) { // sfb -> window -> line order (src/l3bitstream.c:556-579)
                            int sfb = 0;
                            while (3 * L.sfb_s[sfb + 1] / 2 <= e) sfb++;
                            const int start = L.sfb_s[sfb], half = (L.sfb_s[sfb + 1] - start) / 2;
                            const int r = e - 3 * start / 2, w = r / half, line = start + 2 * (r - w * half);
                            x = ix[line * 3 + w];
                            y = ix[(line + 1) * 3 + w];
                            t = (start < 12) ? ts0 : ts1;
                        } else {
                            const int i = 2 * e;
                            x = (int) (int16_t) (pw[gc][j] & 0xffffu);
                            y = (int) (int16_t) (pw[gc][j] >> 16);
                            t = (i < r1s) ? ts0 : (i < r2s ? ts1 : ts2);
                        }
                        fmt_pair(T, L.ht_meta, t, x, y, &code[j], &cb[j], &ext[j], &xb[j]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 3; j++) { // count1 quadruples (src/l3bitstream.c:727-767): at most 144
                qval[j] = 0; qnb[j] = 0;
                if (64 * j < nquad) {
                    const int qd = 64 * j + lane;
                    if (qd < nquad) {
                        const int i = bigvalues + 4 * qd;
                        int q[4];
                        unsigned sg[4];
                        for (int k = 0; k < 4; k++) {
                            q[k] = ix[i + k];
                            if (q[k] > 0) sg[k] = 0; else { q[k] = -q[k]; sg[k] = 1; }
                        }
                        const int p = q[0] + (q[1] << 1) + (q[2] << 2) + (q[3] << 3);
                        unsigned val = T->ht_code[toff + p];
                        int nb = T->ht_len[toff + p];
                        for (int k = 0; k < 4; k++)
                            if (q[k]) { val = (val << 1) | sg[k]; nb += 1; }
                        qval[j] = val;
                        qnb[j] = nb;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 5; j++) {
                if (64 * j < npairs) {
                    const int ofs = fmt_scan(cb[j] + xb[j], &total);
                    if (cb[j]) fmt_put(L.words, pos + ofs, code[j], cb[j]);
                    if (xb[j]) fmt_put(L.words, pos + ofs + cb[j], ext[j], xb[j]);
                    pos += total;
                }
            }
#pragma unroll
            for (int j = 0; j < 3; j++) {
                if (64 * j < nquad) {
                    const int ofs = fmt_scan(qnb[j], &total);
                    if (qnb[j]) fmt_put(L.words, pos + ofs, qval[j], qnb[j]);
                    pos += total;
                }
            }
            { // stuffing with ones up to part2_3_length (src/l3bitstream.c:695-710)
                const int endpos = gpos + g->part2_3_length;
                for (int p = pos + lane * 32; p < endpos; p += 64 * 32) {
                    const int n = (endpos - p < 32) ? endpos - p : 32;
                    fmt_put(L.words, p, 0xffffffffu, n);
                }
                gpos = endpos;
            }
        }
    }
    gpos += sd->resvDrain; // zeros (src/l3bitstream.c:492-509)
    __syncthreads();

    // ---- scatter: header + side info at n*frame_bytes, main data behind the back pointer ----
    const size_t hdr = (size_t) n_abs * (size_t) frame_bytes;
    if (lane < si_bytes) dst[hdr + lane] = (uint8_t) (L.si[lane >> 2] >> (24 - 8 * (lane & 3)));
    // main-data byte m = n_abs * slot - main_data_begin + k lives in frame m / slot at offset m % slot behind that
    // frame's side info.  main_data_begin < 512, so the quotient and remainder of the first byte come from small
    // 32-bit numbers, and every further byte needs one 32-bit division instead of two 64-bit ones.
    const unsigned mdb = (unsigned) sd->main_data_begin, uslot = (unsigned) slot;
    const unsigned back = (mdb + uslot - 1u) / uslot;          // frames the data reaches back
    const long q0 = (long) n_abs - (long) back;                // frame of the first byte (>= 0: the reservoir starts empty)
    const unsigned r0 = back * uslot - mdb;                    // its offset
    const int nbytes = gpos / 8;
    for (int k = lane; k < nbytes; k += 64) {
        const unsigned r = r0 + (unsigned) k, dq = r / uslot, rem = r - dq * uslot;
        const size_t phys = (size_t) (q0 + (long) dq) * (size_t) frame_bytes + (size_t) si_bytes + (size_t) rem;
        dst[phys] = (uint8_t) (L.words[k >> 2] >> (24 - 8 * (k & 3)));
    }
    if (geo.whole_file && n_call == n_frames_s - 1 && lane == 0) {
        // file length (fmt_file_end)
        const long mend = (long) n_abs * (long) slot - (long) mdb + nbytes; // once per stream
        uint32_t len = (uint32_t) fmt_file_end(n_frames_s, mend, slot, frame_bytes);
        if (loop_state) {
            int32_t *st = &loop_state[(size_t) s * loop_state_words + (loop_state_words - 1)];
            if (*st == 0 && fmt_flush_dies(n_frames_s, mend, slot)) *st = MP3MI_DEV_STATUS(MP3MI_DEV_ABORT_FLUSH_SLOT, n_frames_s);
            if (*st != 0) { // the reference died on this stream: there is no file
                len = 0;
                if (voided) atomicAdd(voided, 1u);
            }
        }
        out_len[s] = len;
    }
}


__global__ void __launch_bounds__(64) k_format(FMT_KERNEL_ARGS)
{
    __shared__ fmt_lds L;
    fmt_frame(L, T, geo, ix_all, side_all, bits_per_frame, bitrate_index, out, out_stride, out_len, loop_state, loop_state_words, voided);
}

// The drop-in symbols' formatter (dropin.cpp: one frame, one workgroup): it tells the spinning host that the kernel BEFORE it on
// the stream has finished (k_loop: a kernel starts when the one before it has ended and its stores are visible) and, at its own
// end, that the frame's bytes are in place -- two stores to host-mapped memory instead of two one-thread kernels between and behind
// the two (4-5 us of dispatch latency each).
__global__ void __launch_bounds__(64) k_format_marked(FMT_KERNEL_ARGS, volatile unsigned *flag, unsigned seq_before, unsigned seq_done,
                                                      unsigned *__restrict__ ix_host, unsigned *__restrict__ side_host)
{
    __shared__ fmt_lds L;
    // k_loop left the frame's values and side information in device memory (this kernel reads them many times over, in dependent
    // steps: from host-mapped memory that was most of its time); the host's copies are written here, before the host is told
    for (int i = (int) threadIdx.x; i < geo.channels * 2 * 576 / 2; i += 64) ix_host[i] = ((const unsigned *) ix_all)[i];
    for (int i = (int) threadIdx.x; i < (int) (sizeof(mp3mi_frame_side) / 4); i += 64) side_host[i] = ((const unsigned *) side_all)[i];
    __threadfence_system();
    if (threadIdx.x == 0) *flag = seq_before;
    fmt_frame(L, T, geo, ix_all, side_all, bits_per_frame, bitrate_index, out, out_stride, out_len, loop_state, loop_state_words, voided);
    __threadfence_system(); // (every lane: its stores to the host's window first)
    if (threadIdx.x == 0) *flag = seq_done;
}

// ---- streaming (mp3mi_batch_encode_next / mp3mi_batch_flush) ----
// The file bytes of a stream become final in order: once m bytes of main data have been written, everything up
// to the physical position of main-data byte m - 1 is final (the reference emits exactly these, src/formatBitstream.c
// :218-247); the rest of that slot and the headers behind it still wait for later frames' main data.  A call
// therefore delivers the bytes [final_before, final_after) of every stream's file and keeps [final_after, end of
// the call's last frame) in the stream's carry buffer; the next call starts its output row with them.
MP3MI_DEVFN long fmt_final_upto(long m, int slot, int frame_bytes, int si_bytes)
{
    if (m == 0) return 0;
    return ((m - 1) / slot) * (long) frame_bytes + si_bytes + ((m - 1) % slot) + 1;
}

__global__ void __launch_bounds__(64) k_carry_in(const uint8_t *__restrict__ carry, const int32_t *__restrict__ carry_len,
                                                 uint8_t *__restrict__ out, size_t out_stride)
{
    const int s = (int) blockIdx.x, n = carry_len[s];
    for (int i = (int) threadIdx.x; i < n; i += 64) out[(size_t) s * out_stride + i] = carry[(size_t) s * MP3MI_CARRY_BYTES + i];
}

// After the call's frames are formatted (flush = 0): how much of the row is final, what stays in the carry.
// flush = 1 (III_FlushBitstream + close_bit_stream_w, src/formatBitstream.c:87-120, src/common.c:843-868, 968):
// the carry goes out up to where the last main data ends, plus the byte under construction.
// Per-slot calls (geo.slot_ctl, mp3mi_batch_encode_slots): a slot in which no stream is open delivers nothing and keeps its
// state; a stream that ENDs with the call (flush = 0) has its carry and this call's frames in the row already, so only the
// file's end is settled there -- where the whole-file call's last frame settles it (fmt_file_end).
__global__ void __launch_bounds__(64) k_stream_tail(mp3mi_geom geo, int flush, int32_t *__restrict__ loop_state, int loop_state_words,
                                                    const int32_t *__restrict__ bits_per_frame, uint8_t *__restrict__ out, size_t out_stride,
                                                    int64_t *__restrict__ out_base, uint8_t *__restrict__ carry,
                                                    int32_t *__restrict__ carry_len, uint32_t *__restrict__ out_len,
                                                    unsigned *__restrict__ voided)
{
    const int s = (int) blockIdx.x, lane = (int) threadIdx.x;
    const int C = geo.channels;
    const int ctl = geo.slot_ctl ? (int) geo.slot_ctl[s] : MP3MI_SLOT_DEV_ACTIVE;
    if (!(ctl & MP3MI_SLOT_DEV_ACTIVE)) { // nothing open in the slot
        if (lane == 0) out_len[s] = 0;
        return;
    }
    int32_t *st = &loop_state[(size_t) s * loop_state_words + (loop_state_words - 1)];
    const long f_first = geo.fabs_s ? (long) geo.fabs_s[s] : geo.fabs0;
    if (geo.fabs_s && lane == 0 && *st != 0 && !(*st & MP3MI_DEV_ABORT_REPORTED)) {
        // k_loop of a per-slot call counts the frame of its status from the call's first (its geo.fabs0 is 0): place it in the stream
        const long fr = (long) ((*st >> 8) & MP3MI_DEV_STATUS_FRAME_MAX) + f_first;
        *st = MP3MI_DEV_STATUS(*st & 255, fr);
    }
    const bool ends = !flush && (ctl & MP3MI_SLOT_DEV_END);
    const int frame_bytes = bits_per_frame[s] / 8, si_bytes = (32 + (geo.crc ? 16 : 0) + (C == 2 ? 256 : 136)) / 8, slot = frame_bytes - si_bytes;
    // frames of the stream encoded so far
    const long n_done = f_first + (flush ? 0 : (ends ? ((long) geo.n_samples[s] + 1151) / 1152 : (long) geo.n_frames));
    const long resv_bytes = loop_state[(size_t) s * loop_state_words] / 8; // ResvSize / 8 = the next frame's main_data_begin
    const long m_end = n_done * slot - resv_bytes;                 // main data written so far
    const long base = out_base[s];
    uint8_t *row = out + (size_t) s * out_stride;
    uint8_t *cr = carry + (size_t) s * MP3MI_CARRY_BYTES;
    if (!flush && !ends) {
        const long fin = fmt_final_upto(m_end, slot, frame_bytes, si_bytes), end = n_done * frame_bytes;
        const int keep = (int) (end - fin); // <= 511 bytes of open slots plus the headers in between
        for (int i = lane; i < keep && i < MP3MI_CARRY_BYTES; i += 64) cr[i] = row[fin - base + i];
        if (lane == 0) {
            // (a stream the reference died on delivers nothing more; mp3mi_batch_stream_status says why.  The sync after
            // the call in which it happened reports it -- once: MP3MI_DEV_ABORT_REPORTED marks the word)
            if (*st != 0 && !(*st & MP3MI_DEV_ABORT_REPORTED)) {
                *st |= MP3MI_DEV_ABORT_REPORTED;
                if (voided) atomicAdd(voided, 1u);
            }
            out_len[s] = *st ? 0u : (uint32_t) (fin - base);
            carry_len[s] = keep < MP3MI_CARRY_BYTES ? keep : MP3MI_CARRY_BYTES;
            out_base[s] = fin;
        }
    } else {
        const long total = fmt_file_end(n_done, m_end, slot, frame_bytes);
        const int n = (int) (total - base), have = carry_len[s];
        if (flush)
            for (int i = lane; i < n; i += 64) row[i] = i < have ? cr[i] : (uint8_t) 0;
        if (lane == 0) {
            if (*st == 0 && fmt_flush_dies(n_done, m_end, slot)) *st = MP3MI_DEV_STATUS(MP3MI_DEV_ABORT_FLUSH_SLOT, n_done);
            if (*st != 0 && !(*st & MP3MI_DEV_ABORT_REPORTED)) { // (an earlier call of the stream may have reported it already)
                *st |= MP3MI_DEV_ABORT_REPORTED;
                if (voided) atomicAdd(voided, 1u);
            }
            out_len[s] = *st ? 0u : (uint32_t) (n > 0 ? n : 0);
            carry_len[s] = 0;
            out_base[s] = total;
        }
    }
}

__global__ void __launch_bounds__(256) k_status_gather(int n_streams, const int32_t *__restrict__ loop_state, int loop_state_words, int32_t *__restrict__ status)
{
    const int s = (int) (blockIdx.x * 256 + threadIdx.x);
    if (s < n_streams) status[s] = loop_state[(size_t) s * loop_state_words + (loop_state_words - 1)] & ~MP3MI_DEV_ABORT_REPORTED;
}

void mp3mi_launch_status_gather(int n_streams, const int32_t *loop_state, int loop_state_words, int32_t *status, hipStream_t st)
{
    hipLaunchKernelGGL(k_status_gather, dim3((unsigned) ((n_streams + 255) / 256)), dim3(256), 0, st, n_streams, loop_state, loop_state_words, status);
}

__global__ void __launch_bounds__(256) k_status_scatter(int n_streams, int32_t *__restrict__ loop_state, int loop_state_words, const int32_t *__restrict__ status)
{
    const int s = (int) (blockIdx.x * 256 + threadIdx.x);
    if (s < n_streams && status[s] != 0) loop_state[(size_t) s * loop_state_words + (loop_state_words - 1)] = status[s] | MP3MI_DEV_ABORT_REPORTED;
}

void mp3mi_launch_status_scatter(int n_streams, int32_t *loop_state, int loop_state_words, const int32_t *status, hipStream_t st)
{
    hipLaunchKernelGGL(k_status_scatter, dim3((unsigned) ((n_streams + 255) / 256)), dim3(256), 0, st, n_streams, loop_state, loop_state_words, status);
}

// ---- per-slot streaming (mp3mi_batch_encode_slots) ----
// Fresh state for the slots a call STARTs: what reset_impl gives every stream, for the listed slots only -- one workgroup per
// listed slot zeroes that slot's record of each region with plain word stores.  batch.cpp launches it twice, once per HIP stream,
// each time with the regions that stream owns (the psy state and the PCM history on the front stream; the loop state, the file
// position and the carry length on the loop stream).
__global__ void __launch_bounds__(256) k_slot_begin(const int32_t *__restrict__ list, mp3mi_slot_region r0, mp3mi_slot_region r1,
                                                    mp3mi_slot_region r2)
{
    const size_t s = (size_t) list[blockIdx.x];
    const mp3mi_slot_region r[3] = {r0, r1, r2};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (!r[k].base) continue;
        const size_t words = r[k].bytes / 4;
        uint32_t *p = (uint32_t *) ((char *) r[k].base + s * r[k].bytes);
        for (size_t i = threadIdx.x; i < words; i += 256) p[i] = 0u;
    }
}

void mp3mi_launch_slot_begin(const int32_t *list, int n_list, mp3mi_slot_region r0, mp3mi_slot_region r1, mp3mi_slot_region r2,
                             hipStream_t st)
{
    if (n_list <= 0) return;
    hipLaunchKernelGGL(k_slot_begin, dim3((unsigned) n_list), dim3(256), 0, st, list, r0, r1, r2);
}

// The bitrate of the streams a call STARTs (mp3mi_batch_encode_slots_kbps): lane i puts the frame size in bits and the header's
// bitrate index of the i-th listed slot -- computed on the host, in the call's control block -- into the live arrays that k_loop,
// k_format and k_stream_tail read per stream.  On the loop stream only, where every reader runs (batch.cpp).
__global__ void __launch_bounds__(64) k_slot_rate(const int32_t *__restrict__ list, int n_list, const int32_t *__restrict__ bits,
                                                  const int32_t *__restrict__ index, int32_t *__restrict__ bits_per_frame,
                                                  int32_t *__restrict__ bitrate_index)
{
    const int i = (int) (blockIdx.x * 64 + threadIdx.x);
    if (i >= n_list) return;
    const int s = list[i];
    bits_per_frame[s] = bits[i];
    bitrate_index[s] = index[i];
}

void mp3mi_launch_slot_rate(const int32_t *list, int n_list, const int32_t *bits, const int32_t *index, int32_t *bits_per_frame,
                            int32_t *bitrate_index, hipStream_t st)
{
    if (n_list <= 0) return;
    hipLaunchKernelGGL(k_slot_rate, dim3((unsigned) ((n_list + 63) / 64)), dim3(64), 0, st, list, n_list, bits, index, bits_per_frame, bitrate_index);
}

// ---- parking and resuming the streams of slots (mp3mi_batch_slots_export / mp3mi_batch_slots_import) ----
// Everything a stream carries from call to call is a record per slot in a handful of regions (batch.cpp).  k_slot_park moves
// the listed slots' records between those regions and the caller's state records (one per listed slot, `stride` bytes apart;
// region k at offset t.r[k].off, a multiple of 16): to_state != 0 gathers (export), 0 scatters (import).  Workgroup (i, y):
// the i-th listed slot -- one load of the list, uniform -- and every gridDim.y-th access of each region.  A region whose
// record size is a multiple of 16 moves 16 bytes per lane and access (its base comes from hipMalloc, the state records are
// 16-byte aligned with a stride of a multiple of 16: batch.cpp checks); the others -- the file position, the carry length, the
// two bitrate words -- move words.  Nothing is reused: no LDS.  batch.cpp launches it twice per direction, once per HIP stream
// with the regions that stream owns, exactly as k_slot_begin.
__global__ void __launch_bounds__(256) k_slot_park(const int32_t *__restrict__ list, mp3mi_park_table t, uint8_t *__restrict__ state,
                                                   size_t stride, int to_state)
{
    const size_t i = blockIdx.x, s = (size_t) list[i];
    const size_t lane = (size_t) blockIdx.y * 256 + threadIdx.x, step = (size_t) 256 * gridDim.y;
#pragma unroll
    for (int k = 0; k < MP3MI_PARK_REGIONS; k++) {
        if (k >= t.n) break;
        const size_t bytes = t.r[k].bytes;
        uint8_t *live = (uint8_t *) t.r[k].base + s * bytes, *rec = state + i * stride + t.r[k].off;
        const uint8_t *src = to_state ? live : rec;
        uint8_t *dst = to_state ? rec : live;
        if (bytes % 16 == 0) {
            const size_t n = bytes / 16;
            for (size_t j = lane; j < n; j += step) ((uint4 *) dst)[j] = ((const uint4 *) src)[j];
        } else {
            const size_t n = bytes / 4;
            for (size_t j = lane; j < n; j += step) ((uint32_t *) dst)[j] = ((const uint32_t *) src)[j];
        }
    }
}

void mp3mi_launch_slot_park(const int32_t *list, int n_list, const mp3mi_park_table &t, void *state, size_t stride, int to_state, hipStream_t st)
{
    if (n_list <= 0 || t.n <= 0) return;
    size_t most = 0;
    for (int k = 0; k < t.n; k++) most = t.r[k].bytes > most ? t.r[k].bytes : most;
    size_t ny = (most + 256 * 16 - 1) / (256 * 16); // an access per lane of the largest region, at most four workgroups a slot
    if (ny > 4) ny = 4;
    hipLaunchKernelGGL(k_slot_park, dim3((unsigned) n_list, (unsigned) ny), dim3(256), 0, st, list, t, (uint8_t *) state, stride, to_state);
}

// ---- per-slot streaming on host buffers (mp3mi_batch_encode_slots_host_async) ----
// The caller's buffers hold one ROW per live slot, dense; the encoder's kernels read and write one row per SLOT.  Two bandwidth
// kernels sit between the copies and the encoder: both move 16 bytes per lane and access (one wavefront-instruction = 1 KiB,
// contiguous), the row of a workgroup -- and with it the slot, one load of the map -- is uniform, and no LDS is involved:
// nothing is reused, so registers are the whole staging.
//
// k_rows_in: the columns [col0, col0 + width) -- a chunk's frames -- of the dense rows into the slot rows of the device PCM
// copy.  Bytes throughout; pitch, col0 and width are multiples of 16 (a frame of one channel is 2304 bytes), both bases come
// from hipMalloc.  gridDim.y workgroups share a row; four accesses are in flight per lane.
__global__ void __launch_bounds__(256) k_rows_in(const int32_t *__restrict__ row_slot, const uint8_t *__restrict__ dense,
                                                 uint8_t *__restrict__ pcm, size_t pitch, size_t col0, size_t width)
{
    const size_t r = blockIdx.x, s = (size_t) row_slot[r];
    const uint4 *src = (const uint4 *) (dense + r * pitch + col0);
    uint4 *dst = (uint4 *) (pcm + s * pitch + col0);
    const size_t n = width / 16, step = (size_t) 256 * gridDim.y;
    size_t i = (size_t) blockIdx.y * 256 + threadIdx.x;
    for (; i + 3 * step < n; i += 4 * step) {
        const uint4 a = src[i], b = src[i + step], c = src[i + 2 * step], d = src[i + 3 * step];
        dst[i] = a; dst[i + step] = b; dst[i + 2 * step] = c; dst[i + 3 * step] = d;
    }
    for (; i < n; i += step) dst[i] = src[i];
}

void mp3mi_launch_rows_in(const int32_t *row_slot, int n_rows, const int16_t *dense, int16_t *pcm, size_t pitch_bytes, size_t col0_bytes,
                          size_t width_bytes, hipStream_t st)
{
    if (n_rows <= 0 || width_bytes == 0) return;
    const size_t per_wg = (size_t) 256 * 16 * 4; // four accesses per lane
    size_t ny = (width_bytes + per_wg - 1) / per_wg;
    if (ny > 8) ny = 8;
    hipLaunchKernelGGL(k_rows_in, dim3((unsigned) n_rows, (unsigned) ny), dim3(256), 0, st, row_slot, (const uint8_t *) dense, (uint8_t *) pcm,
                       pitch_bytes, col0_bytes, width_bytes);
}

// k_rows_out: behind the call's k_stream_tail, the out_len bytes of every listed slot's row, and the length, into dense rows of
// the caller's stride (the rest of a dense row is zeroed: the download is one plain copy of whole rows).  The slot rows' stride
// is a multiple of 256; the dense stride is the caller's: 16 bytes per lane when it is a multiple of 16, bytes otherwise.
__global__ void __launch_bounds__(256) k_rows_out(const int32_t *__restrict__ row_slot, const uint8_t *__restrict__ out, size_t out_stride,
                                                  const uint32_t *__restrict__ out_len, uint8_t *__restrict__ dense, size_t dense_stride,
                                                  uint32_t *__restrict__ dense_len)
{
    const size_t r = blockIdx.x, s = (size_t) row_slot[r];
    const size_t lim = out_stride < dense_stride ? out_stride : dense_stride;
    size_t len = out_len[s];
    if (len > lim) len = lim; // (a row never holds more: out_len <= out_stride, and the caller's stride is checked on the host)
    const uint8_t *src = out + s * out_stride;
    uint8_t *dst = dense + r * dense_stride;
    if (threadIdx.x == 0) dense_len[r] = (uint32_t) len;
    if (dense_stride % 16 == 0) {
        const size_t n = dense_stride / 16, n_src = (len + 15) / 16; // (16 n_src <= out_stride: a multiple of 256)
        for (size_t i = threadIdx.x; i < n; i += 256) {
            uint4 v;
            v.x = v.y = v.z = v.w = 0u;
            if (i < n_src) {
                v = ((const uint4 *) src)[i];
                const size_t keep = len - 16 * i; // bytes of this vector that belong to the file (>= 16: all)
                if (keep < 16) { // the file's last vector: word j keeps its first keep - 4 j bytes
                    auto mask = [&](int j) { const long k = (long) keep - 4 * j; return k >= 4 ? 0xFFFFFFFFu : (k <= 0 ? 0u : 0xFFFFFFFFu >> (8 * (4 - k))); };
                    v.x &= mask(0); v.y &= mask(1); v.z &= mask(2); v.w &= mask(3);
                }
            }
            ((uint4 *) dst)[i] = v;
        }
    } else {
        for (size_t i = threadIdx.x; i < dense_stride; i += 256) dst[i] = i < len ? src[i] : (uint8_t) 0;
    }
}

void mp3mi_launch_rows_out(const int32_t *row_slot, int n_rows, const uint8_t *out, size_t out_stride, const uint32_t *out_len, uint8_t *dense,
                           size_t dense_stride, uint32_t *dense_len, hipStream_t st)
{
    if (n_rows <= 0) return;
    hipLaunchKernelGGL(k_rows_out, dim3((unsigned) n_rows), dim3(256), 0, st, row_slot, out, out_stride, out_len, dense, dense_stride, dense_len);
}

// ---- the feeder (mp3mi_feed_tick): a device FIFO per lane in front of the per-slot call ----
// A lane's logical stream is ring[head .. head + pending), wrapping at cap, followed by push[0 .. n_push).  k_feed moves its
// first `take` samples into the lane's row of the dense rows the per-slot call reads, and appends what the rows do not take of
// the push to the ring at (head + pending + the pushed samples the row took) % cap -- the position those samples have in the
// logical stream, so the host's new head is (head + take) % cap whatever the case.  pending + n_push <= cap (the host checks),
// so the span that is written and the span that is read never meet: nothing is moved within the ring, and no workgroup reads
// what another writes.  That makes at most five plain copies per lane -- ring -> row (two: the wrap), push -> row, push -> ring
// (two: the wrap) -- of spans whose source and destination are misaligned against each other by any multiple of a sample.
//
// feed_copy: n bytes, both ends aligned to 2.  The destination's naturally aligned 16-byte vectors are dealt to the lanes of the
// lane's workgroups (lane of gridDim.y * 256, one store of 16 bytes each: a wavefront's store is 1 KiB, contiguous).  A vector
// that lies wholly inside the span is put together from the ALIGNED 16-byte source vectors that hold its bytes -- one when the two
// sides agree mod 16, else two and a funnel shift by the difference (even, 2 .. 14 bytes; uniform over the span) -- provided
// these lie inside the source span too: nothing is loaded from outside [src, src + n).  The others, at most two at either
// end, go sample by sample.  A wavefront's loads are contiguous as well; the second vector of a lane is the first of its
// neighbour, so the cache serves it.
MP3MI_DEVFN void feed_copy(uint8_t *dst, const uint8_t *src, size_t n, size_t lane, size_t step)
{
    if (n == 0) return;
    const uintptr_t d0 = (uintptr_t) dst, s0 = (uintptr_t) src, dv0 = d0 & ~(uintptr_t) 15;
    const size_t n_vec = (size_t) ((d0 + n + 15 - dv0) / 16);
    const unsigned k = (unsigned) ((s0 - d0) & 15u); // where a destination vector's first byte lies in its first source vector
    const unsigned ws = k >> 2, bs = (k & 2u) * 8u;
    for (size_t v = lane; v < n_vec; v += step) {
        const uintptr_t dv = dv0 + 16 * v;     // the destination vector
        const uintptr_t sv = dv + (s0 - d0);   // its first byte in the source
        const uintptr_t sa = sv - k;           // the aligned source vector that holds it
        const bool whole = dv >= d0 && dv + 16 <= d0 + n;
        if (whole && sa >= s0 && sa + (k ? 32 : 16) <= s0 + n) {
            uint4 o = *(const uint4 *) sa;
            if (k) {
                const uint4 a = o, b = *(const uint4 *) (sa + 16);
                const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                unsigned t[5];
#pragma unroll
                for (int j = 0; j < 5; j++) t[j] = ws == 0 ? w[j] : ws == 1 ? w[j + 1] : ws == 2 ? w[j + 2] : w[j + 3];
                if (bs) {
                    o.x = (t[0] >> 16) | (t[1] << 16); o.y = (t[1] >> 16) | (t[2] << 16);
                    o.z = (t[2] >> 16) | (t[3] << 16); o.w = (t[3] >> 16) | (t[4] << 16);
                } else {
                    o.x = t[0]; o.y = t[1]; o.z = t[2]; o.w = t[3];
                }
            }
            *(uint4 *) dv = o;
        } else {
            const uintptr_t lo = dv > d0 ? dv : d0, hi = dv + 16 < d0 + n ? dv + 16 : d0 + n;
            for (uintptr_t p = lo; p < hi; p += 2) *(uint16_t *) p = *(const uint16_t *) (p + (s0 - d0));
        }
    }
}

// The five copies of one lane (above): its ring rg of cap samples, its row and its push row ps.
MP3MI_DEVFN void feed_move(uint8_t *rg, uint8_t *row, const uint8_t *ps, size_t head, size_t pending, size_t n_push, size_t take, size_t cap,
                           size_t esz, size_t lane, size_t step)
{
    const size_t from_ring = take < pending ? take : pending; // the row's samples that come out of the ring
    const size_t from_push = take - from_ring;                // ... and out of the push
    const size_t r1 = from_ring < cap - head ? from_ring : cap - head;
    feed_copy(row, rg + head * esz, r1 * esz, lane, step);
    feed_copy(row + r1 * esz, rg, (from_ring - r1) * esz, lane, step);
    feed_copy(row + from_ring * esz, ps, from_push * esz, lane, step);
    const size_t n_app = n_push - from_push, at = (head + pending + from_push) % cap;
    const size_t a1 = n_app < cap - at ? n_app : cap - at;
    feed_copy(rg + at * esz, ps + from_push * esz, a1 * esz, lane, step);
    feed_copy(rg, ps + (from_push + a1) * esz, (n_app - a1) * esz, lane, step);
}

// Workgroup (s, y): lane s -- its descriptor {head, pending, n_push, take} is one uniform 16-byte load -- and every
// gridDim.y-th vector of each of its copies.  esz: bytes of a sample of all channels; cap: the ring's samples; the three pitches
// in bytes (rows and rings: multiples of 16 from 16-byte aligned bases; the push rows: the caller's).  No LDS: nothing is reused.
__global__ void __launch_bounds__(256) k_feed(const uint4 *__restrict__ desc, uint8_t *ring, size_t ring_pitch, unsigned cap, unsigned esz,
                                              const uint8_t *__restrict__ push, size_t push_pitch, uint8_t *__restrict__ rows, size_t row_pitch)
{
    const size_t s = blockIdx.x;
    const uint4 d = desc[s];
    const size_t head = d.x, pending = d.y, n_push = d.z, take = d.w;
    if (n_push == 0 && take == 0) return;
    const size_t lane = (size_t) blockIdx.y * 256 + threadIdx.x, step = (size_t) 256 * gridDim.y;
    feed_move(ring + s * ring_pitch, rows + s * row_pitch, push + s * push_pitch, head, pending, n_push, take, cap, esz, lane, step);
}

static size_t feed_grid_y(size_t most_bytes)
{
    const size_t per_wg = (size_t) 256 * 16 * 4; // four stores per lane of the longest copy
    const size_t ny = (most_bytes + per_wg - 1) / per_wg;
    return ny < 1 ? 1 : ny > 8 ? 8 : ny;
}

void mp3mi_launch_feed(const void *desc, int n_lanes, int16_t *ring, size_t ring_pitch_bytes, int cap, int channels, const int16_t *push,
                       size_t push_pitch_bytes, int16_t *rows, size_t row_pitch_bytes, size_t most_bytes, hipStream_t st)
{
    if (n_lanes <= 0) return;
    hipLaunchKernelGGL(k_feed, dim3((unsigned) n_lanes, (unsigned) feed_grid_y(most_bytes)), dim3(256), 0, st, (const uint4 *) desc, (uint8_t *) ring,
                       ring_pitch_bytes, (unsigned) cap, (unsigned) (2 * channels), (const uint8_t *) push, push_pitch_bytes, (uint8_t *) rows,
                       row_pitch_bytes);
}

// ---- more lanes than slots (mp3mi_feed_tick_lanes) ----
// k_feed_lanes is k_feed over a LIST: workgroup (i, y) works on the i-th lane that moves in the tick -- one that pushes, takes or
// both -- and nothing is launched for the lanes that do neither, however many there are.  Its descriptor is 32 bytes, one uniform
// load: {head, pending, n_push, take | lane, push_row, slot, 0}.  The ring is the lane's; the push is row push_row of the caller's
// buffer (the caller brings a row per pushing lane, not per lane); the row that is cut is the SLOT's in which the lane encodes
// this tick (unused when take is 0: a lane that only pushes, or waits for a slot, has none).  Two descriptors of a launch never
// name the same lane, slot (with take > 0) or push row (with n_push > 0) -- the host's scheduler guarantees it -- so with the
// ring's rule (above) no workgroup writes what another reads or writes.  The same five copies: feed_move.  No LDS.
__global__ void __launch_bounds__(256) k_feed_lanes(const uint4 *__restrict__ desc, uint8_t *ring, size_t ring_pitch, unsigned cap, unsigned esz,
                                                    const uint8_t *__restrict__ push, size_t push_pitch, uint8_t *__restrict__ rows, size_t row_pitch)
{
    const uint4 d = desc[2 * (size_t) blockIdx.x], w = desc[2 * (size_t) blockIdx.x + 1];
    const size_t head = d.x, pending = d.y, n_push = d.z, take = d.w;
    if (n_push == 0 && take == 0) return;
    const size_t lane = (size_t) blockIdx.y * 256 + threadIdx.x, step = (size_t) 256 * gridDim.y;
    feed_move(ring + (size_t) w.x * ring_pitch, rows + (size_t) w.z * row_pitch, push + (size_t) w.y * push_pitch, head, pending, n_push, take, cap,
              esz, lane, step);
}

void mp3mi_launch_feed_lanes(const void *desc, int n_active, int16_t *ring, size_t ring_pitch_bytes, int cap, int channels, const int16_t *push,
                             size_t push_pitch_bytes, int16_t *rows, size_t row_pitch_bytes, size_t most_bytes, hipStream_t st)
{
    if (n_active <= 0) return;
    hipLaunchKernelGGL(k_feed_lanes, dim3((unsigned) n_active, (unsigned) feed_grid_y(most_bytes)), dim3(256), 0, st, (const uint4 *) desc,
                       (uint8_t *) ring, ring_pitch_bytes, (unsigned) cap, (unsigned) (2 * channels), (const uint8_t *) push, push_pitch_bytes,
                       (uint8_t *) rows, row_pitch_bytes);
}

// ---- ticks on host buffers (mp3mi_feed_tick_lanes_host_async) ----
// k_feed_packed is k_feed_lanes with two differences.  The pushes of a tick lie back to back in one staging buffer, so word 5 of a
// descriptor is the push's first SAMPLE there and a push begins at any even byte: feed_copy takes that as it takes any other
// misalignment -- it loads aligned source vectors that lie wholly inside [src, src + n) and goes sample by sample at the ends, so
// it never reads a neighbouring packet, let alone past the buffer.  And the grid is 1-D over a work list the host built
// (mp3mi_feed_work_list): item {descriptor, part | parts << 16}, one uniform 8-byte load; the workgroup is part `part` of the
// `parts` among which the descriptor's vectors are dealt.  A packet of a few KB beside rows of 147 KB then costs one workgroup,
// not the eight the longest copy of the launch asks for.  No LDS.
__global__ void __launch_bounds__(256) k_feed_packed(const uint4 *__restrict__ desc, const uint2 *__restrict__ work, uint8_t *ring, size_t ring_pitch,
                                                     unsigned cap, unsigned esz, const uint8_t *__restrict__ packed, uint8_t *__restrict__ rows,
                                                     size_t row_pitch)
{
    const uint2 it = work[blockIdx.x];
    const uint4 d = desc[2 * (size_t) it.x], w = desc[2 * (size_t) it.x + 1];
    const size_t head = d.x, pending = d.y, n_push = d.z, take = d.w;
    if (n_push == 0 && take == 0) return;
    const size_t part = it.y & 0xFFFFu, parts = it.y >> 16;
    const size_t lane = part * 256 + threadIdx.x, step = 256 * parts;
    feed_move(ring + (size_t) w.x * ring_pitch, rows + (size_t) w.z * row_pitch, packed + (size_t) w.y * esz, head, pending, n_push, take, cap, esz,
              lane, step);
}

void mp3mi_launch_feed_packed(const void *desc, const void *work, int n_items, int16_t *ring, size_t ring_pitch_bytes, int cap, int channels,
                              const int16_t *packed, int16_t *rows, size_t row_pitch_bytes, hipStream_t st)
{
    if (n_items <= 0) return;
    hipLaunchKernelGGL(k_feed_packed, dim3((unsigned) n_items), dim3(256), 0, st, (const uint4 *) desc, (const uint2 *) work, (uint8_t *) ring,
                       ring_pitch_bytes, (unsigned) cap, (unsigned) (2 * channels), (const uint8_t *) packed, (uint8_t *) rows, row_pitch_bytes);
}

// ---- the feeder of Layers I and II (mp3mi_l12_feed_tick, csrc/l12_feed.h) ----
// k12_feed is k_feed_lanes with two differences.  The ring KEEPS HISTORY: a stream of these layers carries nothing from call to call
// but the samples before the call's first, so the samples behind `head` stay where they are -- the host keeps keep + pending +
// n_push <= cap for every descriptor, keep being the longer history row -- and ALL n_push samples are appended at (head + pending)
// % cap, those the row takes straight from the push included: they are the history of a later tick.  The row's samples come from
// ring[head ..) and then from the push, as in feed_move; the host's new head is (head + take) % cap.  And RESUME is part of the
// cut: word 7 of a descriptor is 0, or bit 31 with n_hist below it, and then the slot's two live history rows are written too --
// hist_a[slot] ([len_a][C]) the n_hist samples before head with zeros in front, hist_b[slot] ([len_b][C], len_b <= len_a) the last
// len_b of the same samples -- what a state record of the parked stream would hold.  The spans that are read (history, pending:
// behind head + pending) and the span that is written (the append: from there on, short of the history) never meet, the rows by
// slot and the history rows by slot belong to one descriptor each: nothing a workgroup writes is read by another in the launch.
// At most nine plain copies per lane and two runs of zeros; no LDS.
MP3MI_DEVFN void feed_zero(uint8_t *dst, size_t n, size_t lane, size_t step) // n bytes of zeros, both ends aligned to 2; as feed_copy deals them
{
    if (n == 0) return;
    const uintptr_t d0 = (uintptr_t) dst, dv0 = d0 & ~(uintptr_t) 15;
    const size_t n_vec = (size_t) ((d0 + n + 15 - dv0) / 16);
    const uint4 zero = {0u, 0u, 0u, 0u};
    for (size_t v = lane; v < n_vec; v += step) {
        const uintptr_t dv = dv0 + 16 * v;
        if (dv >= d0 && dv + 16 <= d0 + n) *(uint4 *) dv = zero;
        else {
            const uintptr_t lo = dv > d0 ? dv : d0, hi = dv + 16 < d0 + n ? dv + 16 : d0 + n;
            for (uintptr_t p = lo; p < hi; p += 2) *(uint16_t *) p = 0;
        }
    }
}

// One history row of len samples: the last min(n_hist, len) samples before head, zeros in front of them
MP3MI_DEVFN void feed_hist(uint8_t *dst, size_t len, const uint8_t *rg, size_t head, size_t n_hist, size_t cap, size_t esz, size_t lane, size_t step)
{
    const size_t n = n_hist < len ? n_hist : len, z = len - n;
    feed_zero(dst, z * esz, lane, step);
    const size_t from = (head + cap - n) % cap; // (n <= len <= cap)
    const size_t h1 = n < cap - from ? n : cap - from;
    feed_copy(dst + z * esz, rg + from * esz, h1 * esz, lane, step);
    feed_copy(dst + (z + h1) * esz, rg, (n - h1) * esz, lane, step);
}

// Workgroup (i, y): the i-th lane that moves in the tick -- descriptor {head, pending, n_push, take | lane, push_row, slot, resume},
// one uniform 32-byte load -- and every gridDim.y-th vector of each of its copies
__global__ void __launch_bounds__(256) k12_feed(const uint4 *__restrict__ desc, uint8_t *ring, size_t ring_pitch, unsigned cap, unsigned esz,
                                                const uint8_t *__restrict__ push, size_t push_pitch, uint8_t *__restrict__ rows, size_t row_pitch,
                                                uint8_t *__restrict__ hist_a, unsigned len_a, uint8_t *__restrict__ hist_b, unsigned len_b)
{
    const uint4 d = desc[2 * (size_t) blockIdx.x], w = desc[2 * (size_t) blockIdx.x + 1];
    const size_t head = d.x, pending = d.y, n_push = d.z, take = d.w, e = esz, n_cap = cap;
    const bool resume = w.w >> 31;
    if (n_push == 0 && take == 0 && !resume) return;
    const size_t lane = (size_t) blockIdx.y * 256 + threadIdx.x, step = (size_t) 256 * gridDim.y;
    uint8_t *rg = ring + (size_t) w.x * ring_pitch, *row = rows + (size_t) w.z * row_pitch;
    const uint8_t *ps = push + (size_t) w.y * push_pitch;
    const size_t from_ring = take < pending ? take : pending, from_push = take - from_ring;
    const size_t r1 = from_ring < n_cap - head ? from_ring : n_cap - head;
    feed_copy(row, rg + head * e, r1 * e, lane, step);
    feed_copy(row + r1 * e, rg, (from_ring - r1) * e, lane, step);
    feed_copy(row + from_ring * e, ps, from_push * e, lane, step);
    const size_t at = (head + pending) % n_cap, a1 = n_push < n_cap - at ? n_push : n_cap - at;
    feed_copy(rg + at * e, ps, a1 * e, lane, step);
    feed_copy(rg, ps + a1 * e, (n_push - a1) * e, lane, step);
    if (resume) {
        const size_t n_hist = w.w & 0x7FFFFFFFu, slot = w.z;
        feed_hist(hist_a + slot * len_a * e, len_a, rg, head, n_hist, n_cap, e, lane, step);
        feed_hist(hist_b + slot * len_b * e, len_b, rg, head, n_hist, n_cap, e, lane, step);
    }
}

void mp3mi_launch_l12_feed(const void *desc, int n_active, int16_t *ring, size_t ring_pitch_bytes, int cap, int channels, const int16_t *push,
                           size_t push_pitch_bytes, int16_t *rows, size_t row_pitch_bytes, int16_t *hist_a, int len_a, int16_t *hist_b, int len_b,
                           size_t most_bytes, hipStream_t st)
{
    if (n_active <= 0) return;
    hipLaunchKernelGGL(k12_feed, dim3((unsigned) n_active, (unsigned) feed_grid_y(most_bytes)), dim3(256), 0, st, (const uint4 *) desc, (uint8_t *) ring,
                       ring_pitch_bytes, (unsigned) cap, (unsigned) (2 * channels), (const uint8_t *) push, push_pitch_bytes, (uint8_t *) rows,
                       row_pitch_bytes, (uint8_t *) hist_a, (unsigned) len_a, (uint8_t *) hist_b, (unsigned) len_b);
}

// the last MP3MI_PCM_HIST samples of the call (a frame has 1152 > MP3MI_PCM_HIST) are the next call's history
__global__ void __launch_bounds__(256) k_hist_save(mp3mi_geom geo, const int16_t *__restrict__ pcm, int16_t *__restrict__ hist)
{
    const int s = (int) blockIdx.x, C = geo.channels;
    const size_t n_call = (size_t) geo.n_frames * 1152;
    const int16_t *src = pcm + ((size_t) s * n_call + (n_call - MP3MI_PCM_HIST)) * C;
    int16_t *dst = hist + (size_t) s * MP3MI_PCM_HIST * C;
    for (int i = (int) threadIdx.x; i < MP3MI_PCM_HIST * C; i += 256) dst[i] = src[i];
}

void mp3mi_launch_carry_in(int n_streams, const uint8_t *carry, const int32_t *carry_len, uint8_t *out, size_t out_stride, hipStream_t st)
{
    hipLaunchKernelGGL(k_carry_in, dim3((unsigned) n_streams), dim3(64), 0, st, carry, carry_len, out, out_stride);
}

void mp3mi_launch_stream_tail(const mp3mi_geom &g, int flush, int32_t *loop_state, int loop_state_words, const int32_t *bits_per_frame,
                              uint8_t *out, size_t out_stride, int64_t *out_base, uint8_t *carry, int32_t *carry_len, uint32_t *out_len,
                              unsigned *voided, hipStream_t st)
{
    hipLaunchKernelGGL(k_stream_tail, dim3((unsigned) g.n_streams), dim3(64), 0, st, g, flush, loop_state, loop_state_words, bits_per_frame,
                       out, out_stride, out_base, carry, carry_len, out_len, voided);
}

void mp3mi_launch_hist_save(const mp3mi_geom &g, const int16_t *pcm, int16_t *hist, hipStream_t st)
{
    hipLaunchKernelGGL(k_hist_save, dim3((unsigned) g.n_streams), dim3(256), 0, st, g, pcm, hist);
}

void mp3mi_launch_format(const mp3mi_tables *T, const mp3mi_geom &g, const int16_t *ix, const mp3mi_frame_side *side,
                         const int32_t *bits_per_frame, const int32_t *bitrate_index, uint8_t *out,
                         size_t out_stride, uint32_t *out_len, int32_t *loop_state, int loop_state_words, unsigned *voided, hipStream_t st)
{
    const unsigned grid = (unsigned) (g.n_streams * g.nf);
    hipLaunchKernelGGL(k_format, dim3(grid), dim3(64), 0, st, T, g, ix, side, bits_per_frame, bitrate_index, out,
                       out_stride, out_len, loop_state, loop_state_words, voided);
}

void mp3mi_launch_format_marked(const mp3mi_tables *T, const mp3mi_geom &g, const int16_t *ix, const mp3mi_frame_side *side,
                                const int32_t *bits_per_frame, const int32_t *bitrate_index, uint8_t *out, size_t out_stride, uint32_t *out_len,
                                unsigned *flag, unsigned seq_before, unsigned seq_done, int16_t *ix_host, mp3mi_frame_side *side_host, hipStream_t st)
{
    hipLaunchKernelGGL(k_format_marked, dim3(1), dim3(64), 0, st, T, g, ix, side, bits_per_frame, bitrate_index, out, out_stride, out_len,
                       (int32_t *) NULL, 0, (unsigned *) NULL, (volatile unsigned *) flag, seq_before, seq_done, (unsigned *) ix_host, (unsigned *) side_host);
}
