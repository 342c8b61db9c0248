# TEST INFRASTRUCTURE (CPU only): the `l12_park` target, on top of the rules and variables of the Makefile beside it:
#     make -C tests/hipemu -f l12_park.mk l12_park
# A bitrate per stream, export and import of the Layer I / II batch under the host sanitizers of `lifecycle` (l12_park_main.cpp; nothing
# preloaded): l12_batch.cpp, the emulator, the program and the kernel files such calls run instrumented, the other objects of _build/ as
# they are.  Passes when it exits 0 with no sanitizer or leak report.
include Makefile
L12_SAN = k_l12 k_fft k_fbmdct
_build/san_%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.h) $(wildcard ../../include/*.h) hipemu.h | _build
	$(CXX) $(CXXFLAGS) $(SAN) -x c++ -c $< -o $@
_build/l12_park: $(addprefix _build/san_,$(addsuffix .o,$(L12_SAN) l12_batch hipemu l12_park_main)) $(filter-out $(addprefix _build/,$(addsuffix .o,$(L12_SAN) l12_batch hipemu)),$(OBJS))
	$(CXX) $(SAN) -o $@ $^ -lm -ldl
l12_park: _build/l12_park
	ASAN_OPTIONS=detect_leaks=1 _build/l12_park
.PHONY: l12_park
