// The self-test hook mp3mi_debug_format_frames (include/mp3mi.h): chains of given frames -- quantised values, side information,
// scalefactors -- through k_format as the batch launches it for a whole file.  Host code only: k_format.hip is untouched, the
// kernel is the one the encoder runs.
//
// What k_format takes on trust from k_loop is checked here first (a chain that breaks one of the rules is refused, nothing is
// launched): the rules are those under which the reference's III_format_bitstream (src/l3bitstream.c:67-162) runs through all
// of its asserts and its bit counts stay inside the frame image (fmt_lds.words) and the output row.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <utility>
#include <vector>
#include "host_util.h"
#include "l12_dev.h"
#include "mp3mi.h"
#include "mp3mi_l12.h"

static const int FD_SLEN1[16] = {0, 0, 0, 0, 3, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4};                      // src/l3bitstream.c:171-172
static const int FD_SLEN2[16] = {0, 1, 2, 3, 0, 1, 2, 3, 1, 2, 3, 1, 2, 3, 2, 3};
static const int FD_IMAGE_BITS = 640 * 32; // fmt_lds.words (k_format.hip)

static inline int fd_abs(int v) { return v < 0 ? -v : v; }

// table t may code the pair (x, y) of magnitudes: 0 for an all-zero region only; no escape below table 16
static bool fd_table_takes(const mp3mi_tables *T, int t, int x, int y)
{
    const int m = x > y ? x : y;
    if (t == 0) return m == 0;
    if (t < 0 || t > 31 || T->ht_xlen[t] == 0) return false; // (4 and 14 do not exist)
    if (t < 16) return m < (int) T->ht_xlen[t];
    return m - 15 <= (int) T->ht_linmax[t];
}

// bits of the pair in table t (src/huffcode.h:16-139)
static int fd_pair_bits(const mp3mi_tables *T, int t, int x, int y)
{
    if (t == 0) return 0;
    const int lin = T->ht_linbits[t], ylen = T->ht_ylen[t];
    int bits = (x != 0) + (y != 0);
    if (t > 15) {
        if (x > 14) { x = 15; bits += lin; }
        if (y > 14) { y = 15; bits += lin; }
    }
    return bits + T->ht_len[T->ht_off[t] + x * ylen + y];
}

// one (granule, channel): 1 where it keeps every rule, scalefactor + code bits <= part2_3_length among them
static int fd_check_granule(const mp3mi_tables *T, const mp3mi_gr_side *g, const int32_t scfsi[4], int gr, const int16_t *ix)
{
    if (g->part2_3_length < 0 || g->part2_3_length > 4095 || g->big_values < 0 || g->count1 < 0 ||
        2 * g->big_values + 4 * g->count1 > 576 || g->global_gain < 0 || g->global_gain > 255 || g->scalefac_compress < 0 ||
        g->scalefac_compress > 15 || (g->window_switching_flag & ~1) || (g->preflag & ~1) || (g->count1table_select & ~1))
        return 0;
    if (g->window_switching_flag ? (g->block_type < 1 || g->block_type > 3) : g->block_type != 0) return 0;
    const bool shortb = g->window_switching_flag && g->block_type == 2;
    const int slen1 = FD_SLEN1[g->scalefac_compress], slen2 = FD_SLEN2[g->scalefac_compress];
    int part2 = 0;
    if (shortb) {
        for (int i = 0; i < 36; i++)
            if (g->scalefac[i] < 0 || g->scalefac[i] >= (1 << (i < 18 ? slen1 : slen2))) return 0;
        part2 = 18 * (slen1 + slen2);
    } else {
        for (int i = 0; i < 21; i++)
            if (g->scalefac[i] < 0 || g->scalefac[i] >= (1 << (i < 11 ? slen1 : slen2))) return 0;
        static const int n_band[4] = {6, 5, 5, 5};
        for (int b = 0; b < 4; b++)
            if (gr == 0 || scfsi[b] == 0) part2 += n_band[b] * (b < 2 ? slen1 : slen2);
    }
    if (g->part2_length != part2) return 0;
    int bits = part2;
    const int bigvalues = 2 * g->big_values;
    if (shortb) { // src/loop.c:1493-1497 leaves (288, 0), or nothing at all
        if (!((g->big_values == 288 || g->big_values == 0) && g->count1 == 0)) return 0;
        if (g->big_values)
            for (int sfb = 0; sfb < 13; sfb++) {
                const int start = T->sfb_s[sfb], end = T->sfb_s[sfb + 1], t = start < 12 ? g->table_select[0] : g->table_select[1];
                for (int w = 0; w < 3; w++)
                    for (int line = start; line < end; line += 2) {
                        const int x = fd_abs(ix[line * 3 + w]), y = fd_abs(ix[(line + 1) * 3 + w]);
                        if (!fd_table_takes(T, t, x, y)) return 0;
                        bits += fd_pair_bits(T, t, x, y);
                    }
            }
    } else {
        if (g->window_switching_flag ? (g->region0_count != 7 || g->region1_count != 13)
                                     : (g->region0_count < 0 || g->region0_count > 15 || g->region1_count < 0 || g->region1_count > 7 ||
                                        g->region0_count + g->region1_count + 2 > 22))
            return 0;
        const int r1s = T->sfb_l[g->region0_count + 1], r2s = T->sfb_l[g->region0_count + g->region1_count + 2];
        for (int i = 0; i < bigvalues; i += 2) {
            const int t = i < r1s ? g->table_select[0] : (i < r2s ? g->table_select[1] : g->table_select[2]);
            const int x = fd_abs(ix[i]), y = fd_abs(ix[i + 1]);
            if (!fd_table_takes(T, t, x, y)) return 0;
            bits += fd_pair_bits(T, t, x, y);
        }
    }
    const int c1end = bigvalues + 4 * g->count1, toff = T->ht_off[32 + g->count1table_select];
    for (int i = bigvalues; i < c1end; i += 4) {
        int p = 0;
        for (int k = 0; k < 4; k++) {
            const int q = fd_abs(ix[i + k]);
            if (q > 1) return 0;
            p |= q << k;
            bits += q;
        }
        bits += T->ht_len[toff + p];
    }
    for (int i = c1end; i < 576; i++)
        if (ix[i] != 0) return 0;
    return bits <= g->part2_3_length; // the rest is stuffing
}

extern "C" int mp3mi_debug_format_frames(int rate_hz, int channels, int kbps, int hdr_mode, int hdr_flags, int crc, int n_streams,
                                         int n_frames, const int32_t *n_frames_s, const int16_t *ix, const void *side_v,
                                         uint8_t *out, size_t out_stride, uint32_t *out_len, int32_t *status)
{
    if (!have_device()) return MP3MI_ERR_NO_DEVICE;
    const mp3mi_frame_side *side = (const mp3mi_frame_side *) side_v;
    const int ri = rate_idx_of(rate_hz), bi = bitrate_index_of(3, kbps);
    if (ri < 0 || bi == 0 || (channels != 1 && channels != 2) || hdr_mode < 0 || hdr_mode > 3 || (channels == 1) != (hdr_mode == 3) ||
        (hdr_flags & ~63) || (crc & ~1) || n_streams <= 0 || n_frames < 0 || !n_frames_s || !out_len || !status ||
        (n_frames > 0 && (!ix || !side || !out)))
        return MP3MI_ERR_ARG;
    const int frame_bytes = frame_bits(1152, ri, kbps, 8) / 8;
    const int si_bytes = 4 + 2 * crc + (channels == 2 ? 32 : 17), slot = frame_bytes - si_bytes;
    if (slot <= 0 || out_stride < (size_t) n_frames * frame_bytes + 1) return MP3MI_ERR_ARG;
    host_mem<mp3mi_tables> Th(1);
    const int trc = tables_into(Th, ri);
    if (trc != MP3MI_OK) return trc;
    const int C = channels;
    bool legal = true;
    for (int s = 0; legal && s < n_streams; s++) {
        if (n_frames_s[s] < 0 || n_frames_s[s] > n_frames) { legal = false; break; }
        long mdb = 0; // the reservoir starts empty
        for (int f = 0; legal && f < n_frames_s[s]; f++) {
            const mp3mi_frame_side *sd = &side[(size_t) s * n_frames + f];
            long bits = sd->resvDrain;
            legal = sd->resvDrain >= 0 && sd->main_data_begin == mdb && mdb <= 511;
            for (int gr = 0; legal && gr < 2; gr++)
                for (int ch = 0; legal && ch < C; ch++) {
                    for (int b = 0; b < 4; b++) legal = legal && !(sd->scfsi[ch][b] & ~1);
                    const int16_t *q = ix + (((size_t) s * 2 * n_frames + (2 * f + gr)) * C + ch) * 576;
                    legal = legal && fd_check_granule(Th.p, &sd->gr[gr][ch], sd->scfsi[ch], gr, q);
                    bits += sd->gr[gr][ch].part2_3_length;
                }
            legal = legal && bits % 8 == 0 && bits <= FD_IMAGE_BITS && bits / 8 <= mdb + slot; // (data never passes its own slot's end)
            mdb += slot - bits / 8;
        }
    }
    if (!legal) return MP3MI_ERR_ARG;
    const size_t S = (size_t) n_streams, nf = (size_t) n_frames, n_ix = S * nf * 2 * C * 576;
    host_mem<int32_t> par(4 * S); // bits_per_frame, bitrate_index, n_samples, status: [4][S]
    if (!par.p) return MP3MI_ERR_NOMEM;
    for (size_t s = 0; s < S; s++) {
        par.p[s] = 8 * frame_bytes;
        par.p[S + s] = bi;
        par.p[2 * S + s] = n_frames_s[s] * 1152;
    }
    hook_bufs D;
    const mp3mi_tables *dT = D.copy_of(Th.p, 1);
    int32_t *dpar = D.copy_of(par.p, 4 * S);
    uint8_t *dout = D.zeros<uint8_t>(S * out_stride);
    uint32_t *dlen = D.zeros<uint32_t>(S);
    // (a sample and a record more than the frames hold, not initialised; a chain of no frames uploads nothing)
    int16_t *dix = D.raw<int16_t>(n_ix + 1);
    mp3mi_frame_side *dside = D.raw<mp3mi_frame_side>(S * nf + 1);
    if (nf) {
        D.put(dix, ix, n_ix);
        D.put(dside, side, S * nf);
    }
    if (!D.ok) return D.rc();
    // the whole-file geometry of a batch call (batch.cpp); a stream of no frames has no file body
    mp3mi_geom g = mp3mi_make_geom(n_streams, C, ri, n_frames, 0, n_frames > 0 ? n_frames : 1);
    g.hdr_mode = hdr_mode;
    g.hdr_flags = hdr_flags;
    g.crc = crc;
    g.n_samples = dpar + 2 * S;
    mp3mi_launch_format(dT, g, dix, dside, dpar, dpar + S, dout, out_stride, dlen, dpar + 3 * S, 1, (unsigned *) NULL, 0);
    D.sync();
    D.fetch(out_len, dlen, S);
    D.fetch(status, dpar + 3 * S, S);
    if (nf) D.fetch(out, dout, S * out_stride);
    return D.rc();
}

// The self-test hook mp3mi_debug_feed (include/mp3mi.h): k_feed alone, through the launcher the feeder uses, on given rings, push rows
// and dense rows.  The three arrays go to the device whole -- the caller's pitches leave room between the lanes' records, which it
// fills with a canary -- and come back whole.  Every descriptor is checked against the rules the feeder's tick keeps
// (csrc/mp3mi_host.h, mp3mi_launch_feed): a descriptor that breaks one launches nothing.
extern "C" int mp3mi_debug_feed(int channels, int n_lanes, int cap, int row_samples, const uint32_t *desc, int16_t *ring, size_t ring_pitch,
                                int16_t *push, size_t push_pitch, int16_t *rows, size_t row_pitch)
{
    if (!have_device()) return MP3MI_ERR_NO_DEVICE;
    if ((channels != 1 && channels != 2) || n_lanes <= 0 || cap <= 0 || row_samples <= 0 || !desc || !ring || !push || !rows) return MP3MI_ERR_ARG;
    const size_t C = (size_t) channels, esz = 2 * C, S = (size_t) n_lanes;
    if (ring_pitch < (size_t) cap || row_pitch < (size_t) row_samples || push_pitch == 0 || ring_pitch * esz % 16 != 0 || row_pitch * esz % 16 != 0)
        return MP3MI_ERR_ARG;
    size_t most = 0;
    for (size_t s = 0; s < S; s++) {
        const uint64_t head = desc[4 * s], pending = desc[4 * s + 1], n_push = desc[4 * s + 2], take = desc[4 * s + 3];
        if (head >= (uint64_t) cap || pending + n_push > (uint64_t) cap || take > pending + n_push || take > (uint64_t) row_samples || n_push > push_pitch)
            return MP3MI_ERR_ARG;
        const size_t longest = (size_t) (take > n_push ? take : n_push) * esz;
        most = longest > most ? longest : most;
    }
    hook_bufs D;
    const uint32_t *ddesc = D.copy_of(desc, 4 * S);
    int16_t *dring = D.copy_of(ring, S * ring_pitch * C), *dpush = D.copy_of(push, S * push_pitch * C), *drows = D.copy_of(rows, S * row_pitch * C);
    if (!D.ok) return D.rc();
    mp3mi_launch_feed(ddesc, n_lanes, dring, ring_pitch * esz, cap, channels, dpush, push_pitch * esz, drows, row_pitch * esz, most, 0);
    D.sync();
    D.fetch(ring, dring, S * ring_pitch * C);
    D.fetch(push, dpush, S * push_pitch * C);
    D.fetch(rows, drows, S * row_pitch * C);
    return D.rc();
}

// The self-test hook mp3mi_debug_feed_lanes (include/mp3mi.h): k_feed_lanes alone, through the launcher mp3mi_feed_tick_lanes uses, on
// given rings (one per lane), push rows and dense rows (one per slot), whole up and whole back like the hook above.  The rules the
// feeder's scheduler keeps are checked here: a descriptor set that breaks one launches nothing.
extern "C" int mp3mi_debug_feed_lanes(int channels, int n_active, int n_lanes, int n_push_rows, int n_slots, int cap, int row_samples,
                                      const uint32_t *desc, int16_t *ring, size_t ring_pitch, int16_t *push, size_t push_pitch, int16_t *rows,
                                      size_t row_pitch)
{
    if (!have_device()) return MP3MI_ERR_NO_DEVICE;
    if ((channels != 1 && channels != 2) || n_active <= 0 || n_lanes <= 0 || n_push_rows <= 0 || n_slots <= 0 || n_active > n_lanes || cap <= 0 ||
        row_samples <= 0 || !desc || !ring || !push || !rows)
        return MP3MI_ERR_ARG;
    const size_t C = (size_t) channels, esz = 2 * C, A = (size_t) n_active;
    if (ring_pitch < (size_t) cap || row_pitch < (size_t) row_samples || push_pitch == 0 || ring_pitch * esz % 16 != 0 || row_pitch * esz % 16 != 0)
        return MP3MI_ERR_ARG;
    std::vector<char> lane_seen((size_t) n_lanes, 0), row_seen((size_t) n_push_rows, 0), slot_seen((size_t) n_slots, 0);
    size_t most = 0;
    for (size_t i = 0; i < A; i++) {
        const uint32_t *d = desc + 8 * i;
        const uint64_t head = d[0], pending = d[1], n_push = d[2], take = d[3];
        if (head >= (uint64_t) cap || pending + n_push > (uint64_t) cap || take > pending + n_push || take > (uint64_t) row_samples || n_push > push_pitch)
            return MP3MI_ERR_ARG;
        if (d[4] >= (uint32_t) n_lanes || d[5] >= (uint32_t) n_push_rows || d[6] >= (uint32_t) n_slots || d[7] != 0) return MP3MI_ERR_ARG;
        if (lane_seen[d[4]] || (n_push && row_seen[d[5]]) || (take && slot_seen[d[6]])) return MP3MI_ERR_ARG;
        lane_seen[d[4]] = 1;
        if (n_push) row_seen[d[5]] = 1;
        if (take) slot_seen[d[6]] = 1;
        const size_t longest = (size_t) (take > n_push ? take : n_push) * esz;
        most = longest > most ? longest : most;
    }
    const size_t n_ring = (size_t) n_lanes * ring_pitch * C, n_pushed = (size_t) n_push_rows * push_pitch * C, n_rows = (size_t) n_slots * row_pitch * C;
    hook_bufs D;
    const uint32_t *ddesc = D.copy_of(desc, 8 * A);
    int16_t *dring = D.copy_of(ring, n_ring), *dpush = D.copy_of(push, n_pushed), *drows = D.copy_of(rows, n_rows);
    if (!D.ok) return D.rc();
    mp3mi_launch_feed_lanes(ddesc, n_active, dring, ring_pitch * esz, cap, channels, dpush, push_pitch * esz, drows, row_pitch * esz, most, 0);
    D.sync();
    D.fetch(ring, dring, n_ring);
    D.fetch(push, dpush, n_pushed);
    D.fetch(rows, drows, n_rows);
    return D.rc();
}

// The self-test hook mp3mi_debug_feed_packed (include/mp3mi.h): k_feed_packed alone, through the launcher and the work list
// mp3mi_feed_tick_lanes_host_async uses, on given rings (one per lane), a packed push buffer of n_packed samples and dense rows (one
// per slot), whole up and whole back like the hooks above.  wg_bytes: what a workgroup moves, for the work list (the product's is
// MP3MI_FEED_WG_BYTES; a small one deals every descriptor to several workgroups).  A descriptor set outside the rules launches nothing.
extern "C" int mp3mi_debug_feed_packed(int channels, int n_active, int n_lanes, int n_packed, int n_slots, int cap, int row_samples, size_t wg_bytes,
                                       const uint32_t *desc, int16_t *ring, size_t ring_pitch, int16_t *packed, int16_t *rows, size_t row_pitch)
{
    if (!have_device()) return MP3MI_ERR_NO_DEVICE;
    if ((channels != 1 && channels != 2) || n_active <= 0 || n_lanes <= 0 || n_packed <= 0 || n_slots <= 0 || n_active > n_lanes || cap <= 0 ||
        row_samples <= 0 || wg_bytes == 0 || !desc || !ring || !packed || !rows)
        return MP3MI_ERR_ARG;
    const size_t C = (size_t) channels, esz = 2 * C, A = (size_t) n_active;
    if (ring_pitch < (size_t) cap || row_pitch < (size_t) row_samples || ring_pitch * esz % 16 != 0 || row_pitch * esz % 16 != 0) return MP3MI_ERR_ARG;
    std::vector<char> lane_seen((size_t) n_lanes, 0), slot_seen((size_t) n_slots, 0);
    std::vector<std::pair<uint64_t, uint64_t> > spans; // the pushes' samples in the packed buffer: inside it, and no two share a sample
    for (size_t i = 0; i < A; i++) {
        const uint32_t *d = desc + 8 * i;
        const uint64_t head = d[0], pending = d[1], n_push = d[2], take = d[3];
        if (head >= (uint64_t) cap || pending + n_push > (uint64_t) cap || take > pending + n_push || take > (uint64_t) row_samples) return MP3MI_ERR_ARG;
        if (d[4] >= (uint32_t) n_lanes || (uint64_t) d[5] + n_push > (uint64_t) n_packed || d[6] >= (uint32_t) n_slots || d[7] != 0) return MP3MI_ERR_ARG;
        if (lane_seen[d[4]] || (take && slot_seen[d[6]])) return MP3MI_ERR_ARG;
        lane_seen[d[4]] = 1;
        if (take) slot_seen[d[6]] = 1;
        if (n_push) spans.push_back(std::make_pair((uint64_t) d[5], (uint64_t) d[5] + n_push));
    }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); i++)
        if (spans[i].first < spans[i - 1].second) return MP3MI_ERR_ARG;
    std::vector<uint32_t> work(2 * MP3MI_FEED_MAX_PARTS * A);
    const size_t n_items = mp3mi_feed_work_list(desc, A, esz, wg_bytes, work.data());
    const size_t n_ring = (size_t) n_lanes * ring_pitch * C, n_pushed = (size_t) n_packed * C, n_rows = (size_t) n_slots * row_pitch * C;
    hook_bufs D;
    const uint32_t *ddesc = D.copy_of(desc, 8 * A), *dwork = D.copy_of(work.data(), 2 * n_items);
    int16_t *dring = D.copy_of(ring, n_ring), *dpush = D.copy_of(packed, n_pushed), *drows = D.copy_of(rows, n_rows);
    if (!D.ok) return D.rc();
    mp3mi_launch_feed_packed(ddesc, dwork, (int) n_items, dring, ring_pitch * esz, cap, channels, dpush, drows, row_pitch * esz, 0);
    D.sync();
    D.fetch(ring, dring, n_ring);
    D.fetch(packed, dpush, n_pushed);
    D.fetch(rows, drows, n_rows);
    return D.rc();
}

// The self-test hook mp3mi_debug_l12_feed (include/mp3mi_l12.h): k12_feed alone, through the launcher mp3mi_l12_feed_tick uses, on
// given rings (one per lane), push rows, dense rows and the two history rows per slot ([n_slots][1792][C] and [n_slots][1056][C],
// dense), whole up and whole back like the hooks above.  The rules the feeder's tick keeps are checked here: a descriptor set that
// breaks one launches nothing.
extern "C" int mp3mi_debug_l12_feed(int channels, int n_active, int n_lanes, int n_push_rows, int n_slots, int cap, int row_samples,
                                    const uint32_t *desc, int16_t *ring, size_t ring_pitch, int16_t *push, size_t push_pitch, int16_t *rows,
                                    size_t row_pitch, int16_t *hist, int16_t *fb_hist)
{
    if (!have_device()) return MP3MI_ERR_NO_DEVICE;
    if ((channels != 1 && channels != 2) || n_active <= 0 || n_lanes <= 0 || n_push_rows <= 0 || n_slots <= 0 || n_active > n_lanes || cap <= 0 ||
        row_samples <= 0 || !desc || !ring || !push || !rows || !hist || !fb_hist)
        return MP3MI_ERR_ARG;
    const size_t C = (size_t) channels, esz = 2 * C, A = (size_t) n_active;
    const uint64_t keep = L12_PCM_HIST;
    if (ring_pitch < (size_t) cap || row_pitch < (size_t) row_samples || push_pitch == 0 || ring_pitch * esz % 16 != 0 || row_pitch * esz % 16 != 0)
        return MP3MI_ERR_ARG;
    std::vector<char> lane_seen((size_t) n_lanes, 0), row_seen((size_t) n_push_rows, 0), slot_seen((size_t) n_slots, 0);
    size_t most = 0;
    for (size_t i = 0; i < A; i++) {
        const uint32_t *d = desc + 8 * i;
        const uint64_t head = d[0], pending = d[1], n_push = d[2], take = d[3];
        const bool resume = d[7] & MP3MI_L12_FEED_RESUME;
        if (head >= (uint64_t) cap || keep + pending + n_push > (uint64_t) cap || take > pending + n_push || take > (uint64_t) row_samples ||
            n_push > push_pitch)
            return MP3MI_ERR_ARG;
        if (d[4] >= (uint32_t) n_lanes || d[5] >= (uint32_t) n_push_rows || d[6] >= (uint32_t) n_slots) return MP3MI_ERR_ARG;
        if (resume ? (d[7] & ~MP3MI_L12_FEED_RESUME) > keep : d[7] != 0) return MP3MI_ERR_ARG;
        if (lane_seen[d[4]] || (n_push && row_seen[d[5]]) || ((take || resume) && slot_seen[d[6]])) return MP3MI_ERR_ARG;
        lane_seen[d[4]] = 1;
        if (n_push) row_seen[d[5]] = 1;
        if (take || resume) slot_seen[d[6]] = 1;
        size_t longest = (size_t) (take > n_push ? take : n_push);
        if (resume && longest < (size_t) keep) longest = (size_t) keep;
        most = longest * esz > most ? longest * esz : most;
    }
    const size_t n_ring = (size_t) n_lanes * ring_pitch * C, n_pushed = (size_t) n_push_rows * push_pitch * C, n_rows = (size_t) n_slots * row_pitch * C;
    const size_t n_hist = (size_t) n_slots * L12_PCM_HIST * C, n_fb = (size_t) n_slots * MP3MI_PCM_HIST * C;
    hook_bufs D;
    const uint32_t *ddesc = D.copy_of(desc, 8 * A);
    int16_t *dring = D.copy_of(ring, n_ring), *dpush = D.copy_of(push, n_pushed), *drows = D.copy_of(rows, n_rows);
    int16_t *dhist = D.copy_of(hist, n_hist), *dfb = D.copy_of(fb_hist, n_fb);
    if (!D.ok) return D.rc();
    mp3mi_launch_l12_feed(ddesc, n_active, dring, ring_pitch * esz, cap, channels, dpush, push_pitch * esz, drows, row_pitch * esz, dhist, L12_PCM_HIST,
                          dfb, MP3MI_PCM_HIST, most, 0);
    D.sync();
    D.fetch(ring, dring, n_ring);
    D.fetch(push, dpush, n_pushed);
    D.fetch(rows, drows, n_rows);
    D.fetch(hist, dhist, n_hist);
    D.fetch(fb_hist, dfb, n_fb);
    return D.rc();
}
