// The self-test hook mp3mi_debug_quantize_count (include/mp3mi.h): k_loop.hip's quantise+count pass in a translation unit of its
// own, so that k_loop is compiled exactly as without it (see the end of k_loop.hip).
#undef MP3MI_LOOP_PROFILE
#define MP3MI_LOOP_PASS_ONLY
#include "k_loop.hip"
