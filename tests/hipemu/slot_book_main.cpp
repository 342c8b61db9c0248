// TEST INFRASTRUCTURE (CPU only): the per-slot bookkeeping of both batches (csrc/host_util.h: slot_book) under a host sanitizer, for
// its BOUNDS -- what it means is the business of tests/test_slot_book.py.  Books of 1, 2 and 3 slots go through every ctl vector
// over {0, START, END, START | END, an illegal bit} with every n_samples_host vector over {0, 1, full - 1, full, full + 1} and with
// none, to a depth of three calls (a refused call leaves the book where it was and ends its branch; a book already seen at the same
// depth is not walked again); every array a call hands to the book, and every array fill() writes, is a heap block of exactly S
// entries, so that one step past an end is a report.
// Build and run: make -C tests/hipemu slot_book
#include <stdint.h>
#include <stdio.h>
#include <memory>
#include <set>
#include <tuple>
#include "host_util.h"

static const int SPF = 1152, DEPTH = 3;
static const uint8_t CTL[5] = {0, MP3MI_SLOT_START, MP3MI_SLOT_END, MP3MI_SLOT_START | MP3MI_SLOT_END, 4};
static long n_calls, n_refused;
static std::set<std::tuple<int, bool, long, std::vector<int64_t>>> seen; // (depth, the book)

template <typename T> static std::unique_ptr<T[]> exactly(int n) { return std::unique_ptr<T[]>(new T[(size_t) n]); }

// one call on a copy of `book`: rules, fill, advance, settle as slots_impl (batch.cpp) and l12_slots_impl (l12_batch.cpp) run them
static int call(slot_book book, int n_frames, const uint8_t *ctl, const int32_t *ns, int depth);

static int calls_from(const slot_book &book, int depth)
{
    const int S = book.n_slots();
    if (depth == DEPTH || !seen.insert(std::make_tuple(depth, book.on, book.frames_all, book.frames)).second) return 0;
    if (book.any_open() != (book.count_open() > 0) || book.count_open() > S) return 1;
    int n_ctl = 1, n_ns = 1;
    for (int s = 0; s < S; s++) { n_ctl *= 5; n_ns *= 5; }
    auto ctl = exactly<uint8_t>(S);
    auto ns = exactly<int32_t>(S);
    for (int n_frames = 1; n_frames <= 2; n_frames++) {
        const int32_t full = n_frames * SPF, N[5] = {0, 1, full - 1, full, full + 1};
        for (int ci = 0; ci < n_ctl; ci++) {
            for (int s = 0, v = ci; s < S; s++, v /= 5) ctl[s] = CTL[v % 5];
            if (call(book, n_frames, ctl.get(), NULL, depth)) return 1;
            for (int ni = 0; ni < n_ns; ni++) {
                for (int s = 0, v = ni; s < S; s++, v /= 5) ns[s] = N[v % 5];
                if (call(book, n_frames, ctl.get(), ns.get(), depth)) return 1;
            }
        }
    }
    return 0;
}

static int call(slot_book book, int n_frames, const uint8_t *ctl_host, const int32_t *ns_host, int depth)
{
    const int S = book.n_slots();
    auto f = exactly<int64_t>(S);
    book.now(f.get());
    n_calls++;
    if (!book.rules_ok(f.get(), n_frames, SPF, ctl_host, ns_host)) { n_refused++; return 0; }
    auto fabs = exactly<int64_t>(S);
    auto n_samples = exactly<int32_t>(S);
    auto ctl = exactly<uint8_t>(S);
    auto list = exactly<int32_t>(S);
    const int n_start = book.fill(f.get(), n_frames, SPF, ctl_host, ns_host, fabs.get(), n_samples.get(), ctl.get(), list.get());
    if (n_start < 0 || n_start > S) { fprintf(stderr, "slot_book: %d STARTs in %d slots\n", n_start, S); return 1; }
    for (int i = 0; i < S; i++) // (reads every entry fill() is to have written: an unwritten one is the sanitizer's to report)
        if (list[i] < 0 || list[i] >= S || fabs[i] < 0 || n_samples[i] < 0 || n_samples[i] > n_frames * SPF || (ctl[i] & ~7)) {
            fprintf(stderr, "slot_book: fill() wrote list %d, fabs %lld, n_samples %d, ctl %d for slot %d of %d\n", list[i], (long long) fabs[i],
                    n_samples[i], ctl[i], i, S);
            return 1;
        }
    book.advance(f.get(), ctl_host, n_frames);
    book.settle(f.get());
    return calls_from(book, depth + 1);
}

int main(void)
{
    for (int S = 1; S <= 3; S++) {
        seen.clear();
        slot_book book;
        book.init(S);
        if (calls_from(book, 0)) return 1;
        book.close();
        book.frames_all = 2; // (every slot open, by the whole-batch counter)
        if (calls_from(book, DEPTH - 1)) return 1;
    }
    printf("slot_book: %ld calls, %ld refused\n", n_calls, n_refused);
    return 0;
}
