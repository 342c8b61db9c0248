# TEST INFRASTRUCTURE (CPU only): the `l12_slots` target, on top of the rules and variables of the Makefile beside it:
#     make -C tests/hipemu -f l12_slots.mk l12_slots
# Per-slot calls of the Layer I / II batch under the host sanitizers of `lifecycle` (l12_slots_main.cpp; nothing preloaded):
# l12_batch.cpp, the emulator, the program and the kernel files a per-slot call runs instrumented, the other objects of _build/ as
# they are.  Passes when it exits 0 with no sanitizer or leak report.
include Makefile
L12_SAN = k_l12 k_fft k_fbmdct
_build/san_%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.h) $(wildcard ../../include/*.h) hipemu.h | _build
	$(CXX) $(CXXFLAGS) $(SAN) -x c++ -c $< -o $@
_build/l12_slots: $(addprefix _build/san_,$(addsuffix .o,$(L12_SAN) l12_batch hipemu l12_slots_main)) $(filter-out $(addprefix _build/,$(addsuffix .o,$(L12_SAN) l12_batch hipemu)),$(OBJS))
	$(CXX) $(SAN) -o $@ $^ -lm -ldl
l12_slots: _build/l12_slots
	ASAN_OPTIONS=detect_leaks=1 _build/l12_slots
.PHONY: l12_slots
