// TEST INFRASTRUCTURE: does k_loop's search stay inside its table of step sizes (mp3mi_tables::step, q = -400 .. 400)?
// `make loop_steps` builds this program over the emulated library's objects with k_loop, k_prep, k_fbmdct, the hook and the emulator
// compiled under -fsanitize=address,undefined (the bounds check is what matters: step[] lies inside the table block, so only the
// array-index check sees an index past its end) and runs it: it passes when it exits 0 with no sanitizer report.
//
// The hook mp3mi_debug_iteration_loop refuses a granule whose start step lies above the table; here it is compiled with that rule
// out of the way (MP3MI_LOOP_DEBUG_NO_STEP_RULE), and the granules are the ones it refuses: a few tiny lines behind silence, whose
// quantanf_init start value 8 ln sfm - 70 has no upper bound (423 for one line of 2^-40, 1087 for one of 2^-100).  The kernels
// clamp what they hand to the search to 400 (k_prep.hip); every such stream ends with global_gain >= 256, the reference's
// assertion, whatever the search does on the way: each stream's status word is compared with the ORACLE's (mp3o_iteration_loop,
// oracle/mp3_oracle.h, whose search starts from the unclamped step and has no table to leave) -- the check that nothing a stream
// shows changes with the clamp -- and with the word written down here.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mp3mi.h"
#include "mp3mi_dev.h"
#include "../../oracle/mp3_oracle.h"

int main(void)
{
    enum { S = 5, NF = 2, STATE_WORDS = 190 };
    static double xr[S][2 * NF][576];
    static mp3mi_psy_out psy[S][2 * NF];
    static int16_t ix[S][2 * NF][576];
    static mp3mi_frame_side side[S][NF];
    static int32_t state[S][STATE_WORDS];
    const int32_t kbps[S] = {128, 32, 320, 64, 128};
    int32_t listed = -1;
    memset(psy, 0, sizeof(psy));
    for (int s = 0; s < S; s++)
        for (int g = 0; g < 2 * NF; g++) {
            for (int b = 0; b < 21; b++) psy[s][g].ratio_l[b] = (s & 1) ? 0.0 : 1e-3;
            for (int b = 0; b < 36; b++) (&psy[s][g].ratio_s[0][0])[b] = (s & 1) ? 1e-3 : 0.0;
        }
    xr[0][0][0] = 0x1p-40;                     // q0 = 423: the bisection probes up to 422
    xr[1][1][575] = -0x1p-100;                 // q0 = 1087, in granule 1
    psy[1][1].block_type = 2;
    xr[2][0][3] = 0x1p-45; xr[2][0][40] = -0x1p-45; xr[2][0][300] = 0x1p-46; // q0 = 460: past the table by less than the bisection's first step
    psy[2][0].block_type = 1;
    for (int i = 0; i < 576; i++) xr[3][0][i] = 0.01 * sin(0.37 * i) * exp(-i / 150.0); // sound first, then frame 1 dies
    xr[3][2][17] = 0x1p-60;
    xr[4][0][0] = 0x1p-37;                     // q0 = 390: inside the table, and dies all the same
    const int32_t want[S] = {1, 1, 1, 1 | 1 << 8, 1}; // MP3MI_STREAM_ABORT_GLOBAL_GAIN | frame << 8
    const int rc = mp3mi_debug_iteration_loop(44100, 1, 0, S, NF, kbps, &xr[0][0][0], psy, NULL, &ix[0][0][0], side, state, &listed);
    if (rc != 0) {
        fprintf(stderr, "loop_steps: the hook returned %d\n", rc);
        return 1;
    }
    int bad = 0;
    for (int s = 0; s < S; s++) {
        const int32_t st = state[s][STATE_WORDS - 1];
        static int16_t oix[2 * NF][576];
        static int32_t oside[NF][226], ostate[STATE_WORDS];
        if (mp3o_iteration_loop(44100, 1, kbps[s], 0, NF, &xr[s][0][0], psy[s], NULL, 0, &oix[0][0], &oside[0][0], ostate, NULL) != 0 ||
            ostate[STATE_WORDS - 1] != st) {
            printf("stream %d: the oracle's status %#x\n", s, ostate[STATE_WORDS - 1]);
            bad++;
        }
        printf("stream %d: status %#x (want %#x, the oracle's too), global_gain of its granules %d %d %d %d\n", s, st, want[s], side[s][0].gr[0][0].global_gain,
               side[s][0].gr[1][0].global_gain, side[s][1].gr[0][0].global_gain, side[s][1].gr[1][0].global_gain);
        bad += st != want[s];
    }
    printf("records redone by k_prep: %d\n", listed);
    return bad ? 1 : 0;
}
