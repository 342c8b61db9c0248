# TEST INFRASTRUCTURE (CPU only): the `feed_host` target, on top of feed.mk (and through it of the Makefile beside it):
#     make -C tests/hipemu -f feed_host.mk feed_host
# A feeder's ticks on host buffers (mp3mi_feed_tick_lanes_host_async, mp3mi_feed_host_wait, mp3mi_feed_host_io_stats) under the host
# sanitizers of `feed` (feed_host_main.cpp; nothing preloaded): batch.cpp (with feed.h), the emulator, the program and k_format.hip --
# k_feed_packed, k_rows_out, k_slot_park and the other plumbing kernels of a tick -- instrumented, the other objects of _build/ as
# they are.  Passes when it exits 0 with no sanitizer or leak report.
include feed.mk
_build/feed_host: $(addprefix _build/san_,$(addsuffix .o,$(FEED_SAN) batch hipemu feed_host_main)) $(filter-out $(addprefix _build/,$(addsuffix .o,$(FEED_SAN) batch hipemu)),$(OBJS))
	$(CXX) $(SAN) -o $@ $^ -lm -ldl
feed_host: _build/feed_host
	ASAN_OPTIONS=detect_leaks=1 _build/feed_host
.PHONY: feed_host
