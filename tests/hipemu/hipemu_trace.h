// TEST INFRASTRUCTURE -- the enqueue trace of the CPU emulator (hipemu.h): what the host side enqueues, on which stream, in which
// order.  A translation unit compiled with `-include hipemu_trace.h` (enqueue_trace.mk: the product sources once more, into objects
// of their own) reaches the emulator's host shims through the wrappers below, which write one line each while a trace is on
// (hipemu_trace; NULL = off, the state at start) and then do what the shim does:
//   kernel launches: the kernel's name, grid and block dimensions, the stream;  hipMemcpyAsync / hipMemcpy2DAsync: bytes or width x
//   height, the kind, the stream;  hipMemsetAsync: bytes, the stream;  hipEventRecord, hipStreamWaitEvent: the event and the stream;
//   hipEventSynchronize, hipStreamSynchronize, hipEventCreate*, hipStreamCreate*.
// Streams and events are named by small numbers in order of creation, never by pointers, which differ from run to run: here a
// stream's handle IS its number (the shims give every stream the handle 0; no emulated code dereferences one), and an event's
// number is kept by its address until it is destroyed.
//
// Why wrappers and a makefile of their own, not some thirty lines inside the shims: hipemu.h is what the test build, every emulated
// test and every sanitizer program (feed.mk, l12_park.mk, ...) is made of, and its objects are shared between them.  A trace inside
// it changes the text, and with it the build, of everything the `-m "not gpu"` suite rests on, for the sake of one program that no test
// runs; kept apart, hipemu.h, hipemu.cpp, the Makefile and every object of the test build stay byte for byte what they were, and a
// version of this tree's tests can be run on another version's build (a parent's tests on a change's, say) whatever either does to the
// trace.  The price is the list below: a shim added to hipemu.h that enqueues something needs its wrapper and its #define here, or
// it goes untraced -- enqueue_trace_main.cpp would then show a call with no line, not a wrong line.
#ifndef HIPEMU_TRACE_H
#define HIPEMU_TRACE_H

#include "hipemu.h"

void hipemu_trace(FILE *to);
namespace hipemu_tr {
extern FILE *to;
hipStream_t new_stream(const char *how);
void new_event(const char *how, hipEvent_t e);
void drop_event(hipEvent_t e);
int event_no(hipEvent_t e);
static inline int stream_no(hipStream_t s) { return (int) (uintptr_t) s; }
static inline const char *kind_name(hipMemcpyKind k) { return k == hipMemcpyHostToDevice ? "H2D" : k == hipMemcpyDeviceToHost ? "D2H" : k == hipMemcpyDeviceToDevice ? "D2D" : "default"; }
}
#define HIPEMU_TRACE(...) do { if (hipemu_tr::to) fprintf(hipemu_tr::to, __VA_ARGS__); } while (0)

static inline hipError_t tr_hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t st = 0)
{
    HIPEMU_TRACE("memcpy    %zu bytes %s  stream %d\n", n, hipemu_tr::kind_name(k), hipemu_tr::stream_no(st));
    return hipMemcpyAsync(d, s, n, k, st);
}
static inline hipError_t tr_hipMemcpy2DAsync(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind k, hipStream_t st = 0)
{
    HIPEMU_TRACE("memcpy2d  %zu x %zu bytes %s  stream %d\n", w, h, hipemu_tr::kind_name(k), hipemu_tr::stream_no(st));
    return hipMemcpy2DAsync(d, dp, s, sp, w, h, k, st);
}
static inline hipError_t tr_hipMemsetAsync(void *d, int v, size_t n, hipStream_t st = 0)
{
    HIPEMU_TRACE("memset    %zu bytes  stream %d\n", n, hipemu_tr::stream_no(st));
    return hipMemsetAsync(d, v, n, st);
}
static inline hipError_t tr_hipStreamSynchronize(hipStream_t st) { HIPEMU_TRACE("sync      stream %d\n", hipemu_tr::stream_no(st)); return hipStreamSynchronize(st); }
// (the shim runs, then its handle -- 0 for every stream -- is replaced by the stream's number)
static inline hipError_t tr_hipStreamCreate(hipStream_t *s)
{
    const hipError_t rc = hipStreamCreate(s);
    *s = hipemu_tr::new_stream("hipStreamCreate");
    return rc;
}
static inline hipError_t tr_hipStreamCreateWithFlags(hipStream_t *s, unsigned flags)
{
    const hipError_t rc = hipStreamCreateWithFlags(s, flags);
    *s = hipemu_tr::new_stream("hipStreamCreateWithFlags");
    return rc;
}
static inline hipError_t tr_hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int priority)
{
    const hipError_t rc = hipStreamCreateWithPriority(s, flags, priority);
    *s = hipemu_tr::new_stream("hipStreamCreateWithPriority");
    return rc;
}
static inline hipError_t tr_hipEventCreate(hipEvent_t *e)
{
    const hipError_t rc = hipEventCreate(e);
    hipemu_tr::new_event("hipEventCreate", *e);
    return rc;
}
static inline hipError_t tr_hipEventCreateWithFlags(hipEvent_t *e, unsigned flags)
{
    const hipError_t rc = hipEventCreateWithFlags(e, flags);
    hipemu_tr::new_event("hipEventCreateWithFlags", *e);
    return rc;
}
static inline hipError_t tr_hipEventDestroy(hipEvent_t e) { hipemu_tr::drop_event(e); return hipEventDestroy(e); }
static inline hipError_t tr_hipEventRecord(hipEvent_t e, hipStream_t st = 0)
{
    HIPEMU_TRACE("record    event %d  stream %d\n", hipemu_tr::event_no(e), hipemu_tr::stream_no(st));
    return hipEventRecord(e, st);
}
static inline hipError_t tr_hipStreamWaitEvent(hipStream_t st, hipEvent_t e, unsigned flags)
{
    HIPEMU_TRACE("wait      stream %d  event %d\n", hipemu_tr::stream_no(st), hipemu_tr::event_no(e));
    return hipStreamWaitEvent(st, e, flags);
}
static inline hipError_t tr_hipEventSynchronize(hipEvent_t e) { HIPEMU_TRACE("sync      event %d\n", hipemu_tr::event_no(e)); return hipEventSynchronize(e); }
static inline void tr_launch(const char *kernel, dim3 grid, dim3 block, hipStream_t st)
{
    HIPEMU_TRACE("launch    %s  grid %u %u %u  block %u %u %u  stream %d\n", kernel, grid.x, grid.y, grid.z, block.x, block.y, block.z, hipemu_tr::stream_no(st));
}

// from here on the names of the shims mean the wrappers
#define hipMemcpyAsync tr_hipMemcpyAsync
#define hipMemcpy2DAsync tr_hipMemcpy2DAsync
#define hipMemsetAsync tr_hipMemsetAsync
#define hipStreamSynchronize tr_hipStreamSynchronize
#define hipStreamCreate tr_hipStreamCreate
#define hipStreamCreateWithFlags tr_hipStreamCreateWithFlags
#define hipStreamCreateWithPriority tr_hipStreamCreateWithPriority
#define hipEventCreate tr_hipEventCreate
#define hipEventCreateWithFlags tr_hipEventCreateWithFlags
#define hipEventDestroy tr_hipEventDestroy
#define hipEventRecord tr_hipEventRecord
#define hipStreamWaitEvent tr_hipStreamWaitEvent
#define hipEventSynchronize tr_hipEventSynchronize
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) \
    (tr_launch(#kernel, (grid), (block), (stream)), hipemu::launch((grid), (block), [&]() { kernel(__VA_ARGS__); }))

#endif
