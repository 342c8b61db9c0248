# TEST INFRASTRUCTURE (CPU only): the `l12_feed` target, on top of the rules and variables of the Makefile beside it:
#     make -C tests/hipemu -f l12_feed.mk l12_feed
# The feeder of the Layer I / II batch under the host sanitizers of `lifecycle` (l12_feed_main.cpp; nothing preloaded): l12_batch.cpp
# with l12_feed.h, the emulator, the program and the kernel files a tick runs -- k_format among them, for k12_feed -- instrumented, the
# other objects of _build/ as they are.  Passes when it exits 0 with no sanitizer or leak report.
include Makefile
L12_FEED_SAN = k_l12 k_fft k_fbmdct k_format
_build/san_%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.h) $(wildcard ../../include/*.h) hipemu.h | _build
	$(CXX) $(CXXFLAGS) $(SAN) -x c++ -c $< -o $@
_build/l12_feed: $(addprefix _build/san_,$(addsuffix .o,$(L12_FEED_SAN) l12_batch hipemu l12_feed_main)) $(filter-out $(addprefix _build/,$(addsuffix .o,$(L12_FEED_SAN) l12_batch hipemu)),$(OBJS))
	$(CXX) $(SAN) -o $@ $^ -lm -ldl
l12_feed: _build/l12_feed
	ASAN_OPTIONS=detect_leaks=1 _build/l12_feed
.PHONY: l12_feed
