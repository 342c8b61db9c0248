# TEST INFRASTRUCTURE (CPU only): the `enqueue_trace` target, on top of the Makefile beside it:
#     make -C tests/hipemu -f enqueue_trace.mk enqueue_trace
# The enqueue trace of a fixed script of calls (enqueue_trace_main.cpp): what the host side enqueues, on which stream, in which order,
# to stdout.  Every source that launches, copies or records is compiled once more, with hipemu_trace.h in front of it, into
# _build/tr_*.o; the test build's own objects, its library and hipemu.h stay as they are.  No sanitizer and no expected output: build
# the program against two versions of the sources (CSRC=...) and diff the two outputs.
include Makefile
TRACED = $(KERNELS) batch l12_batch dropin format_debug loop_debug l12_alloc_debug
_build/tr_%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.h) $(wildcard ../../include/*.h) hipemu.h hipemu_trace.h | _build
	$(CXX) $(CXXFLAGS) -include hipemu_trace.h -x c++ -c $< -o $@
_build/tr_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(wildcard ../../include/*.h) hipemu.h hipemu_trace.h | _build
	$(CXX) $(CXXFLAGS) -include hipemu_trace.h -c $< -o $@
_build/enqueue_trace: enqueue_trace_main.cpp hipemu_trace.h $(addprefix _build/tr_,$(addsuffix .o,$(TRACED))) $(filter-out $(addprefix _build/,$(addsuffix .o,$(TRACED))),$(OBJS))
	$(CXX) $(CXXFLAGS) -o $@ $(filter %.cpp %.o,$^) -lm -ldl
enqueue_trace: _build/enqueue_trace
	_build/enqueue_trace
.PHONY: enqueue_trace
