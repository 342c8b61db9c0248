# TEST INFRASTRUCTURE (CPU only): the `feed_lanes` target, on top of feed.mk (and through it of the Makefile beside it):
#     make -C tests/hipemu -f feed_lanes.mk feed_lanes
# A feeder with more lanes than slots (mp3mi_feed_create_lanes, mp3mi_feed_tick_lanes) under the host sanitizers of `feed`
# (feed_lanes_main.cpp; nothing preloaded): batch.cpp (with feed.h), the emulator, the program and k_format.hip -- k_feed_lanes,
# k_slot_park and the other plumbing kernels of a tick -- instrumented, the other objects of _build/ as they are.  Passes when it
# exits 0 with no sanitizer or leak report.
include feed.mk
_build/feed_lanes: $(addprefix _build/san_,$(addsuffix .o,$(FEED_SAN) batch hipemu feed_lanes_main)) $(filter-out $(addprefix _build/,$(addsuffix .o,$(FEED_SAN) batch hipemu)),$(OBJS))
	$(CXX) $(SAN) -o $@ $^ -lm -ldl
feed_lanes: _build/feed_lanes
	ASAN_OPTIONS=detect_leaks=1 _build/feed_lanes
.PHONY: feed_lanes
