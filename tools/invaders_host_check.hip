// Stand-alone host check of csrc/env_invaders.hip: the rules (si_step), the record codec (si_pack / si_unpack) and the image
// (si_image, all 64 lanes) run on the CPU against steps recorded from the map-form restatement (tests/invaders_ref.py).  No
// GPU is touched; build it with the host sanitizers to have every shift and index of the packed-word arithmetic checked:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -Iprism_amd/csrc \
//         -x hip tools/invaders_host_check.hip -o invaders_host_check && ./invaders_host_check records.txt
// A record is two lines: the 8 state words before the step, the game's action (0..5, after the action map and the sticky
// coin) and the step limit; then the 8 words after the step (after the reset, where the episode ended), the reward, done,
// truncated and the 600 elements of the returned image as '0' / '1'.  tests/test_invaders_rules_host.py writes them.
#include "env_invaders.hip"

#include <cstdio>
#include <cstring>

namespace prism {
void set_error(const char *, ...) {}          // (the entry points of the included file are not called)
}

int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    long n = 0, bad = 0;
    for (;;) {
        uint32_t w[8], want[8], out[8];
        int a, limit, done, trunc;
        float reward;
        char img[604], got[601];
        if (fscanf(f, "%u %u %u %u %u %u %u %u %d %d", &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &w[6], &w[7], &a, &limit) != 10) break;
        if (fscanf(f, "%u %u %u %u %u %u %u %u %f %d %d %603s", &want[0], &want[1], &want[2], &want[3], &want[4], &want[5], &want[6], &want[7],
                   &reward, &done, &trunc, img) != 12)
            return 3;
        SiState s;
        si_unpack(w, s);
        s.last_action = a;
        float r = 0.f;
        const bool terminal = si_step(s, a, r);
        s.ep_steps += 1u;
        s.t += 1ull;
        const bool truncated = limit > 0 && s.ep_steps >= (uint32_t)limit && !terminal;
        memset(got, '?', 600);
        got[600] = 0;
        for (int lane = 0; lane < WAVE; ++lane) {
            const uint32_t im = si_image(s, lane);
            for (int j = 0; j < 3; ++j)
                for (int b = 0; b < 4 && lane + 64 * j < SI_CHUNKS; ++b) got[4 * (lane + 64 * j) + b] = ((im >> (4 * j + b)) & 1u) ? '1' : '0';
        }
        if (terminal || truncated) si_reset(s);
        si_pack(s, out);
        const bool ok = !memcmp(out, want, sizeof out) && r == reward && (int)terminal == done && (int)truncated == trunc && !strcmp(got, img);
        if (!ok && bad++ < 5) {
            printf("MISMATCH at record %ld: action %d, reward %g / %g, done %d / %d, truncated %d / %d, image %s\n", n, a, r, reward, (int)terminal,
                   done, (int)truncated, trunc, strcmp(got, img) ? "differs" : "same");
            for (int i = 0; i < 8; ++i) printf("  word %d: in %08x got %08x want %08x\n", i, w[i], out[i], want[i]);
        }
        ++n;
    }
    fclose(f);
    printf("%ld records, %ld mismatches\n", n, bad);
    return bad || !n ? 1 : 0;
}
