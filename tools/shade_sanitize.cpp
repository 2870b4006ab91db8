// A stand-alone program for a sanitizer run of the shading rule's HOST code (csrc/kernels/shade.h: the per-ray functions
// shade_kernel calls - the texel filter, the drawn row, the shadow test, the lights' sum, the triple - through ms_host_shade): no
// GPU, no Python.  Build the library's translation unit and this file with the host sanitizers and run the result, as
// tools/navzone_sanitize.cpp's header describes:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/shade_sanitize.cpp -o /tmp/shade_sanitize
//     /tmp/shade_sanitize
//
// Hand-made worlds of two agents - a box with pillars under three lights, one of intensity 0; a dark box; a box under 65 lights;
// a single wall; lines of one texel among lines of up to eight - every store allocated to the byte, so that a read or write past
// a store's end is a report.  Rays of R = 1, 37, 64 and 200 an env: indices from -1 to the env's line count and INT_MIN / INT_MAX,
// locations in [0, 1] with exactly 0 and 1, and NaN, infinities, negatives and 1e30 among them (black), with and without agents.
// After each call the triples are checked, bit for bit, against a plain statement of the rule written here, apart from the
// library's text (on a body: that the triple is a colour - the lights are tests/test_shade_host.py's business).  Exit status 0 and no report from the sanitizers: clean.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) & 0xffff)/65536.f; }
static unsigned bits_of(float v) { unsigned u; memcpy(&u, &v, sizeof u); return u; }

// a store of exactly n elements, 16-byte aligned at its start (the end is what the sanitizer watches)
template <typename T> static T* store(size_t n) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, n*sizeof(T) ? n*sizeof(T) : 1)) abort();
    memset(p, 0, n*sizeof(T));
    return (T*)p;
}

static float min_f(float a, float b) { if (a != a) return b; return b < a ? b : a; }
static float max_f(float a, float b) { if (a != a) return b; return b > a ? b : a; }

int main() {
    unsigned seed = 31;
    const int A = 2, M = 3, AF = A*M, N = 4;
    const float model_rows[M][4] = {{-.125f, 0.f, .125f, 0.f}, {0.f, -.1f, .1f, .1f}, {.1f, .1f, -.1f, .1f}};
    const int n_pillars = 4;
    const int walls_of[N] = {4 + 4*n_pillars, 4, 4 + 4*n_pillars, 1}, lights_of[N] = {3, 0, 65, 1};
    std::vector<int> lw(N), ls(N), liw(N), lis(N);
    int n_lines = 0, n_lights = 0;
    for (int n = 0; n < N; n++) { lw[n] = AF + walls_of[n]; ls[n] = n_lines; n_lines += lw[n]; liw[n] = lights_of[n]; lis[n] = n_lights; n_lights += liw[n]; }
    float* const lines = store<float>((size_t)4*n_lines);
    float* const lights = store<float>((size_t)3*n_lights);
    float* const model = store<float>((size_t)4*M);
    memcpy(model, model_rows, sizeof model_rows);
    const float box[4][4] = {{1, 1, 6, 1}, {6, 1, 6, 6}, {6, 6, 1, 6}, {1, 6, 1, 1}};
    for (int n = 0; n < N; n++) {
        float* w = lines + 4*(ls[n] + AF);
        for (int k = 0; k < walls_of[n] && k < 4; k++) memcpy(w + 4*k, box[k], sizeof box[k]);
        for (int p = 0; 4 + 4*p < walls_of[n]; p++) {
            const float x = uniform(seed, 1.5f, 5.f), y = uniform(seed, 1.5f, 5.f), d = .3f;
            const float sq[4][4] = {{x, y, x + d, y}, {x + d, y, x + d, y + d}, {x + d, y + d, x, y + d}, {x, y + d, x, y}};
            memcpy(w + 4*(4 + 4*p), sq, sizeof sq);
        }
        for (int i = 0; i < liw[n]; i++) {
            float* l = lights + 3*(lis[n] + i);
            l[0] = uniform(seed, 1.2f, 5.8f); l[1] = uniform(seed, 1.2f, 5.8f); l[2] = liw[n] > 8 ? uniform(seed, .002f, .03f) : uniform(seed, .2f, 1.f);
        }
    }
    lights[3*1 + 2] = 0.f;                                                  // env 0's second light: intensity 0
    int* const tw = store<int>(n_lines);
    int* const ts = store<int>(n_lines);
    int n_texels = 0;
    for (int l = 0; l < n_lines; l++) { tw[l] = (l % 5 == 0) ? 1 : 1 + (int)(next_random(seed) % 8); ts[l] = n_texels; n_texels += tw[l]; }
    float* const tex = store<float>((size_t)3*n_texels);
    float* const baked = store<float>(n_texels);
    for (int t = 0; t < n_texels; t++) { baked[t] = uniform(seed, 0.f, 1.f); for (int k = 0; k < 3; k++) tex[3*t + k] = uniform(seed, 0.f, 1.f); }
    float* const angles = store<float>(N*A);
    float* const positions = store<float>(2*N*A);
    float* const still = store<float>(2*N*A);
    for (int i = 0; i < N*A; i++) { angles[i] = uniform(seed, -180.f, 180.f); positions[2*i] = uniform(seed, 1.5f, 5.5f); positions[2*i + 1] = uniform(seed, 1.5f, 5.5f); }

    MsScenery sc;
    memset(&sc, 0, sizeof sc);
    sc.n_envs = N; sc.n_agents = A; sc.n_model = M;
    sc.lights_vals = lights; sc.lights_widths = liw.data(); sc.lights_starts = lis.data();
    sc.lines_vals = lines; sc.lines_widths = lw.data(); sc.lines_starts = ls.data();
    sc.textures_vals = tex; sc.textures_widths = tw; sc.textures_starts = ts;
    sc.model = model; sc.baked_vals = baked;
    sc.n_lines_total = n_lines; sc.n_lights_total = n_lights; sc.n_texels_total = n_texels;
    MsAgents ag;
    memset(&ag, 0, sizeof ag);
    ag.angles = angles; ag.positions = positions; ag.angvelocity = still; ag.velocity = still;

    const float odd_locations[] = {NAN, INFINITY, -INFINITY, -1.f, 2.f, 1e30f, -0.f, 1e-45f};
    const int ray_counts[] = {1, 37, 64, 200};
    int failures = 0, calls = 0;
    long long checked = 0;
    for (int R : ray_counts)
        for (int with_agents = 0; with_agents < 2; with_agents++) {
            int* const idx = store<int>((size_t)N*R);
            float* const loc = store<float>((size_t)N*R);
            float* const dots = store<float>((size_t)N*R);
            float* const screen = store<float>((size_t)3*N*R);
            for (int n = 0; n < N; n++)
                for (int r = 0; r < R; r++) {
                    const int i = n*R + r, kind = (int)(next_random(seed) % 16);
                    idx[i] = kind < 6 ? (int)(next_random(seed) % AF) : kind == 6 ? -1 : kind == 7 ? lw[n] : kind == 8 ? INT_MIN : kind == 9 ? INT_MAX
                                      : (int)(next_random(seed) % (lw[n] + 2)) - 1;
                    const int lk = (int)(next_random(seed) % 16);
                    loc[i] = lk == 0 ? 0.f : lk == 1 ? 1.f : lk == 2 ? odd_locations[next_random(seed) % 8] : uniform(seed, 0.f, 1.f);
                    dots[i] = uniform(seed, -1.f, 1.f);
                    for (int k = 0; k < 3; k++) screen[3*i + k] = NAN;
                }
            MsShade q;
            q.n_rays = R; q.indices = idx; q.locations = loc; q.dots = dots; q.screen = screen;
            const int rc = ms_host_shade(&sc, with_agents ? &ag : nullptr, &q);
            calls++;
            if (rc != MS_OK) { printf("R %d agents %d: ms_host_shade returned %d\n", R, with_agents, rc); failures++; }
            for (int n = 0; n < N && rc == MS_OK; n++)
                for (int r = 0; r < R; r++) {
                    const int i = n*R + r, l = idx[i];
                    float want[3] = {0.f, 0.f, 0.f};
                    const bool black = l < 0 || l >= lw[n] || (l < AF && !with_agents) || !(loc[i] >= 0.f && loc[i] <= 1.f);
                    if (!black) {
                        const int w = tw[ls[n] + l], t0 = ts[ls[n] + l];
                        const float x = loc[i];
                        const float y = min_f(x*(w + 1), (float)(w - 1));
                        const int fl = (int)max_f(y - 1, 0.f), fr = (int)min_f(y, (float)(w - 1));
                        const float ld = fabsf(y - (fl + 1)) + 1.e-3f, rd = fabsf(y - (fr + 1)) + 1.e-3f;
                        const float wl = rd/(ld + rd), wr = ld/(ld + rd);
                        float intensity;
                        if (l < AF) {
                            // (the lights on a body are the tests' business - tests/test_shade_host.py holds them to the numpy rule; here:
                            // the triple is a finite number in [0, 1.001])
                            for (int k = 0; k < 3; k++)
                                if (!(screen[3*i + k] >= 0.f && screen[3*i + k] <= 1.001f)) { printf("env %d ray %d: %g on a body\n", n, r, screen[3*i + k]); failures++; }
                            checked++;
                            continue;
                        }
                        intensity = wl*baked[t0 + fl] + wr*baked[t0 + fr];
                        const float dn = 1 - dots[i]*dots[i];
                        for (int k = 0; k < 3; k++) want[k] = dn*intensity*(wl*tex[3*(t0 + fl) + k] + wr*tex[3*(t0 + fr) + k]);
                    }
                    for (int k = 0; k < 3; k++)
                        if (bits_of(screen[3*i + k]) != bits_of(want[k])) {
                            if (failures < 10) printf("R %d agents %d env %d ray %d channel %d: %g, want %g\n", R, with_agents, n, r, k, screen[3*i + k], want[k]);
                            failures++;
                        }
                    checked++;
                }
            free(idx); free(loc); free(dots); free(screen);
        }
    // what the call refuses: nothing is read or written
    MsShade q;
    memset(&q, 0, sizeof q);
    if (ms_host_shade(&sc, &ag, &q) != MS_EINVAL || ms_host_shade(nullptr, &ag, &q) != MS_EINVAL || ms_host_shade(&sc, &ag, nullptr) != MS_EINVAL) {
        printf("a call without planes was not refused\n");
        failures++;
    }
    free(lines); free(lights); free(model); free(tw); free(ts); free(tex); free(baked); free(angles); free(positions); free(still);
    printf("shade_sanitize: %d calls, %lld rays checked, %d failures\n", calls, checked, failures);
    return failures ? 1 : 0;
}
