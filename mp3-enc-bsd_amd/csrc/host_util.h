/* Small host-side helpers shared by the translation units that drive HIP (batch.cpp, l12_batch.cpp, the self-test hooks):
 * error check, device scope, fences, a ring of upload blocks; what a sampling rate and a bitrate mean for a stream; the per-slot
 * bookkeeping of a streaming batch (slot_book); the buffers of a self-test hook (hook_bufs).  Private to the library. */
#ifndef MP3MI_HOST_UTIL_H
#define MP3MI_HOST_UTIL_H

#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "mp3mi_host.h"
#include "mp3mi.h"

/* returns MP3MI_ERR_HIP (mp3mi.h) from the calling function when a HIP call fails */
#define CHK(call)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "mp3mi: %s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return MP3MI_ERR_HIP;                                                              \
        }                                                                                      \
    } while (0)

// Every entry point runs on the batch's own device whatever the calling thread's current device is, and leaves
// the caller's current device as it found it.
struct device_scope {
    int prev;
    bool ok;
    explicit device_scope(int dev) : prev(-1), ok(true)
    {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; prev = -1; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~device_scope() { if (prev >= 0) (void) hipSetDevice(prev); }
};
#define ON_DEVICE(b)                                                                                     \
    device_scope dev_scope_((b)->device);                                                                \
    if (!dev_scope_.ok) { fprintf(stderr, "mp3mi: cannot select device %d\n", (b)->device); return MP3MI_ERR_HIP; }

static inline int have_device(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

// Bits of a frame of samples_per_frame samples at kbps, slots of slot_bits (32 for Layer I, 8 for II and III) per frame never
// padded: src/musicin.c:562-569, the fraction of a slot dropped -- and with it every padding decision.  The arithmetic is the
// reference's, in double, as written there: frame sizes depend on it.  rate_idx: 0 = 44.1 kHz, 1 = 48, 2 = 32 (src/common.c:113).
static inline int frame_bits(int samples_per_frame, int rate_idx, int kbps, int slot_bits)
{
    static const double s_freq[3] = {44.1, 48, 32};
    const int whole_SpF = (int) (((double) samples_per_frame / s_freq[rate_idx]) * ((double) kbps / (double) slot_bits));
    return whole_SpF * slot_bits;
}

// ---- stream set-up: the one place that knows the sampling rates, the bitrates and what mp3mi_build_tables answers ----
// The header's sampling-frequency code, -1 for anything but the three MPEG-1 rates (the MPEG-2 LSF ones: src/l3psy.c:170-176 and
// src/psy.c:131-136 exit on them)
static inline int rate_idx_of(int rate_hz) { return rate_hz == 44100 ? 0 : rate_hz == 48000 ? 1 : rate_hz == 32000 ? 2 : -1; }

static const int L3_BITRATES[15] = {0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320}; // src/common.c:124
static const int L12_BITRATES[2][15] = { /* src/common.c:122-123 */
    {0, 32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 416, 448},
    {0, 32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384}};
// The header's bitrate index of kbps in Layer `layer` (1, 2 or 3), 0 where the layer has no such bitrate (src/common.c:460-481)
static inline int bitrate_index_of(int layer, int kbps)
{
    const int *row = layer == 3 ? L3_BITRATES : L12_BITRATES[layer - 1];
    for (int bi = 1; bi < 15; bi++)
        if (row[bi] == kbps) return bi;
    return 0;
}

// What mp3mi_build_tables / mp3mi_build_tables_l12 return, as an error of mp3mi.h: -8 is "the host's libm does not reproduce the
// pinned tables" (tables_host.cpp), anything else but 0 an argument they refuse
static inline int tables_rc(int trc) { return trc == 0 ? MP3MI_OK : trc == -8 ? MP3MI_ERR_TABLES : MP3MI_ERR_ARG; }

// An event and whether it has ever been recorded: the last reader (or writer) of something that is used again and again.
// Whoever uses it next waits -- a stream (wait_on) or the host (sync) -- and waits for nothing when there was no use before.
// WHEN to wait, and what to let go before, is the caller's business.  Created where its owner is; zero-initialised before that.
struct fence {
    hipEvent_t ev;
    bool recorded;
    hipError_t create(void) { return hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
    hipError_t record(hipStream_t st)
    {
        const hipError_t e = hipEventRecord(ev, st);
        if (e == hipSuccess) recorded = true;
        return e;
    }
    hipError_t wait_on(hipStream_t st) const { return recorded ? hipStreamWaitEvent(st, ev, 0) : hipSuccess; }
    hipError_t sync(void) const { return recorded ? hipEventSynchronize(ev) : hipSuccess; }
    bool done(void) const // everything ahead of the last record is through (never recorded: nothing was)
    {
#if defined(MP3MI_EMU)
        return true; // (the emulator runs every launch where it is issued)
#else
        return !recorded || hipEventQuery(ev) == hipSuccess;
#endif
    }
    void destroy(void) { if (ev) (void) hipEventDestroy(ev); ev = 0; recorded = false; }
};

// N blocks that go up to the device call by call: pinned staging, the device copy, and a fence behind the last reader of either.
// take() is the block of this call's turn; the host waits for its fence before it writes the staging again -- the call N before --
// and next() ends the turn of a call that was issued.  The owner allocates the entries (eagerly or with their first turn).
template <typename T, int N> struct upload_ring {
    struct entry {
        T *stage, *dev;
        fence free;
    } e[N];
    unsigned calls;
    entry &take(void) { return e[calls % (unsigned) N]; }
    void next(void) { calls++; }
};

// v grows to n events (flags 0: with timing)
static inline hipError_t grow_events(std::vector<hipEvent_t> &v, size_t n, unsigned flags)
{
    while (v.size() < n) {
        hipEvent_t e;
        const hipError_t rc = flags ? hipEventCreateWithFlags(&e, flags) : hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        v.push_back(e);
    }
    return hipSuccess;
}

// ---- per-slot streaming: the bookkeeping (include/mp3mi.h, mp3mi_batch_encode_slots; the same rules for all three layers) ----
// A stream index of a streaming batch is a SLOT through which one stream after another passes.  While `on` is false the slots are
// as frames_all says -- all open at frames_all when it is > 0, else all closed -- and every call runs the whole-batch path it always
// ran; a per-slot call (or a park) sets `on`, and the slots are as `frames` says, until settle() hands back.  A call takes now() into
// a vector f of its own, checks rules_ok(f) before anything changes state, writes its control block with fill(f), and once it is
// issued advance(f) and settle(f) say where the slots are behind it.
struct slot_book {
    bool on;
    long frames_all;             // frames every stream has been given since the last close(), by calls on the whole batch
    std::vector<int64_t> frames; // frames encoded by the stream open in each slot, -1: no stream open there

    void init(int n_slots) { on = false; frames_all = 0; frames.assign((size_t) n_slots, -1); }
    int n_slots(void) const { return (int) frames.size(); }
    // What slot s holds: the frames of the stream open in it, -1 for none
    int64_t at(int s) const { return on ? frames[(size_t) s] : (frames_all > 0 ? (int64_t) frames_all : -1); }
    void now(int64_t *f) const { for (int s = 0; s < n_slots(); s++) f[s] = at(s); }
    int count_open(void) const
    {
        int n = 0;
        for (int s = 0; s < n_slots(); s++) n += at(s) >= 0;
        return n;
    }
    bool any_open(void) const { return count_open() > 0; }

    // The rules of a per-slot call of n_frames frames of samples_per_frame samples, slot by slot (f: now()): no bit but START and
    // END; END only of a stream that is open or starts; and n_samples_host (NULL: whole frames for every stream in the call) 0 for
    // a slot with no stream, the whole call for a stream that goes on, at most that for one that ends
    bool rules_ok(const int64_t *f, int n_frames, int samples_per_frame, const uint8_t *ctl_host, const int32_t *n_samples_host) const
    {
        const int32_t full = (int32_t) n_frames * samples_per_frame;
        for (int s = 0; s < n_slots(); s++) {
            const int c = ctl_host[s];
            if (c & ~(MP3MI_SLOT_START | MP3MI_SLOT_END)) return false;
            const bool open = f[s] >= 0, start = c & MP3MI_SLOT_START, end = c & MP3MI_SLOT_END, part = open || start;
            if (end && !part) return false;
            const int32_t n = n_samples_host ? n_samples_host[s] : (part ? full : 0);
            if (!part ? n != 0 : (!end ? n != full : (n < 0 || n > full))) return false;
        }
        return true;
    }
    // The four arrays the control blocks of both batches share (staging, one entry per slot each; checked: rules_ok): where the
    // call's first frame lies in the slot's stream, the valid samples per channel, MP3MI_SLOT_DEV_*, and the START slots in
    // ascending order at the head of `list` (zeros behind them).  Returns how many START.
    int fill(const int64_t *f, int n_frames, int samples_per_frame, const uint8_t *ctl_host, const int32_t *n_samples_host,
             int64_t *fabs, int32_t *n_samples, uint8_t *ctl, int32_t *list) const
    {
        const int32_t full = (int32_t) n_frames * samples_per_frame;
        int n_start = 0;
        for (int s = 0; s < n_slots(); s++) {
            const int c = ctl_host[s];
            const bool open = f[s] >= 0, start = c & MP3MI_SLOT_START, part = open || start;
            fabs[s] = (start || !open) ? 0 : f[s];
            n_samples[s] = n_samples_host ? n_samples_host[s] : (part ? full : 0);
            ctl[s] = (uint8_t) ((start ? MP3MI_SLOT_DEV_START : 0) | (c & MP3MI_SLOT_END ? MP3MI_SLOT_DEV_END : 0) | (part ? MP3MI_SLOT_DEV_ACTIVE : 0));
            list[s] = 0;
            if (start) list[n_start++] = s;
        }
        return n_start;
    }
    // f behind a per-slot call that was issued: a stream that STARTs is at 0, one that ENDs leaves its slot closed, the others
    // have n_frames more
    void advance(int64_t *f, const uint8_t *ctl_host, int n_frames) const
    {
        for (int s = 0; s < n_slots(); s++) {
            const int c = ctl_host[s];
            if (c & MP3MI_SLOT_START) f[s] = 0;
            if (c & MP3MI_SLOT_END) f[s] = -1;
            else if (f[s] >= 0) f[s] += n_frames;
        }
    }
    // The per-slot bookkeeping is in force, with the slots as f says -- unless every slot is open at the same frame: then it hands
    // over to the whole-batch counter, and the next call runs exactly as if there had never been a per-slot call (a batch whose
    // streams all began together)
    void settle(const int64_t *f)
    {
        frames.assign(f, f + n_slots());
        on = true;
        for (int s = 1; s < n_slots(); s++)
            if (f[s] != f[0]) return;
        if (f[0] > 0) {
            on = false;
            frames_all = (long) f[0];
        }
    }
    // Every stream is over: the whole-batch counter again, at the start of new streams
    void close(void) { on = false; frames_all = 0; }
};

// ---- the self-test hooks (mp3mi_debug_*): host memory and device buffers that go with the call ----
template <typename T> struct host_mem { // n zeroed T's, or NULL
    T *p;
    explicit host_mem(size_t n) : p((T *) calloc(n, sizeof(T))) {}
    ~host_mem() { free(p); }
    host_mem(const host_mem &) = delete;
    host_mem &operator=(const host_mem &) = delete;
};
// The host copy of the Layer III tables of sampling-frequency code ri in Th; the outcome as an error of mp3mi.h
static inline int tables_into(host_mem<mp3mi_tables> &Th, int ri) { return Th.p ? tables_rc(mp3mi_build_tables(Th.p, ri)) : MP3MI_ERR_NOMEM; }

// The device buffers of one hook call, freed when it returns.  A hook reads: check the arguments -- a refused input allocates and
// launches nothing --, allocate and fill, launch, sync, fetch, return rc().  The first HIP call that fails sticks: every later call
// of the object does nothing, and rc() is MP3MI_ERR_HIP.
struct hook_bufs {
    std::vector<void *> owned;
    bool ok;
    hook_bufs() : ok(true) {}
    ~hook_bufs() { for (void *p : owned) (void) hipFree(p); }
    hook_bufs(const hook_bufs &) = delete;
    hook_bufs &operator=(const hook_bufs &) = delete;
    template <typename T> T *raw(size_t n) // n T's, as hipMalloc leaves them
    {
        void *p = NULL;
        if (ok && (ok = hipMalloc(&p, n * sizeof(T)) == hipSuccess)) owned.push_back(p);
        return (T *) p;
    }
    template <typename T> T *zeros(size_t n)
    {
        T *p = raw<T>(n);
        ok = ok && hipMemset(p, 0, n * sizeof(T)) == hipSuccess;
        return p;
    }
    // n T's from the host; with extra_zeroed, that many more behind them, the whole buffer zeroed first
    template <typename T> T *copy_of(const T *host, size_t n, size_t extra_zeroed = 0)
    {
        T *p = extra_zeroed ? zeros<T>(n + extra_zeroed) : raw<T>(n);
        put(p, host, n);
        return p;
    }
    template <typename T> bool put(T *dev, const T *host, size_t n)
    {
        return ok = ok && hipMemcpy(dev, host, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
    }
    bool sync(void) { return ok = ok && hipDeviceSynchronize() == hipSuccess; }
    template <typename T> bool fetch(T *host_dst, const T *dev, size_t n)
    {
        return ok = ok && hipMemcpy(host_dst, dev, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
    }
    int rc(void) const { return ok ? MP3MI_OK : MP3MI_ERR_HIP; }
};

#endif
