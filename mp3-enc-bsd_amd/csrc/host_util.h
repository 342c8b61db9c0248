/* Small host-side helpers shared by the translation units that drive HIP (batch.cpp, l12_batch.cpp, format_debug.cpp):
 * error check, device scope, fences, a ring of upload blocks, the frame size of a bitrate.  Private to the library. */
#ifndef MP3MI_HOST_UTIL_H
#define MP3MI_HOST_UTIL_H

#include <stdio.h>
#include <vector>
#include "mp3mi_host.h"

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

#endif
