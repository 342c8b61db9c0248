# TEST INFRASTRUCTURE (CPU only): the `feed` target, on top of the rules and variables of the Makefile beside it:
#     make -C tests/hipemu -f feed.mk feed
# The feeder of a Layer III slot batch (mp3mi_feed_*) under the host sanitizers of `lifecycle` (feed_main.cpp; nothing preloaded):
# batch.cpp (with feed.h), the emulator, the program and k_format.hip -- k_feed, k_slot_park and the other plumbing kernels of a
# tick -- instrumented, the other objects of _build/ as they are.  Passes when it exits 0 with no sanitizer or leak report.
include Makefile
FEED_SAN = k_format
_build/san_%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.h) $(wildcard ../../include/*.h) hipemu.h | _build
	$(CXX) $(CXXFLAGS) $(SAN) -x c++ -c $< -o $@
_build/feed: $(addprefix _build/san_,$(addsuffix .o,$(FEED_SAN) batch hipemu feed_main)) $(filter-out $(addprefix _build/,$(addsuffix .o,$(FEED_SAN) batch hipemu)),$(OBJS))
	$(CXX) $(SAN) -o $@ $^ -lm -ldl
feed: _build/feed
	ASAN_OPTIONS=detect_leaks=1 _build/feed
.PHONY: feed
