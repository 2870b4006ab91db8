// A stand-alone program for a sanitizer run of the age maps' HOST code (csrc/kernels/navage.h over navseen.h's ray and sample,
// through ms_host_nav_ages): no GPU, no Python.  Build the library's translation unit and this file with the host sanitizers
// and run the result, as tools/navcost_sanitize.cpp's header describes:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/navage_sanitize.cpp -o /tmp/navage_sanitize
//     /tmp/navage_sanitize
//
// Hand-made grids - one cell, one row, one column, and 31, 32, 33, 63, 64 and 65 cells, the edges of the words of the marks'
// bitmask - every store allocated to the byte, so that a read or write past a store's end is a report.  Per grid two maps and
// three viewers take six calls: fans of rays from inside and from outside the grid, with slots that skip viewers, resets, NaN
// and infinite origins, directions and distances, rays cut by max_range and rays of over 2^20 samples; a call with only some
// of the outputs; a survey alone; a clock at 2^24 - 1.  After each call the numbers are checked against each other: the ages
// against the ticks and the clock, the counts against the stale bytes.  Exit status 0 and no report from the sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

int main() {
    unsigned seed = 23;
    const float cell = .1f;
    const int shapes[][2] = {{1, 1}, {1, 40}, {40, 1}, {31, 1}, {32, 1}, {33, 1}, {9, 7}, {8, 8}, {13, 5}, {0, 0}};
    const int S = 2, P = 3, R = 13, T = 3;
    int failures = 0;
    long long marks = 0;
    for (int shape = 0; shape < 10; shape++) {
        const int nx = shapes[shape][0], ny = shapes[shape][1], cells = nx*ny;
        const int geom[4] = {-4 + shape, 3 - shape, nx, ny};
        const size_t spare = cells ? 0 : 1;                              // (an env without cells still has to point somewhere)
        std::vector<unsigned char> countable((size_t)cells + spare), stale((size_t)S*cells + spare, 9);
        for (int k = 0; k < cells; k++) countable[k] = (unsigned char)((next_random(seed) % 5 ? 1 : 0) | 2);
        std::vector<float> last((size_t)S*cells + spare, 0.f), ages((size_t)S*cells + spare, -7.f);
        std::vector<int> clock(S, 0), swept(S), gained(S), oldest(S), n_stale(S);
        std::vector<long long> idle(S), total(S);
        clock[1] = (1 << 24) - 1;
        for (int call = 0; call < 6; call++) {
            std::vector<float> origins((size_t)P*2), dirs((size_t)P*R*2), distances((size_t)P*R);
            std::vector<int> slot(P);
            std::vector<unsigned char> reset(S);
            for (int p = 0; p < P; p++) {
                const bool outside = p == 2 && call % 2;
                origins[2*p] = ((float)geom[0] + (outside ? -3.f : uniform(seed, 0.f, (float)(nx > 0 ? nx : 1))))*cell;
                origins[2*p + 1] = ((float)geom[1] + (outside ? (float)ny + 2.f : uniform(seed, 0.f, (float)(ny > 0 ? ny : 1))))*cell;
                slot[p] = (int)(next_random(seed) % 4) - 1;              // (-1 and 2: nobody's map)
                for (int r = 0; r < R; r++) {
                    const float angle = uniform(seed, 0.f, 6.2831853f), length = uniform(seed, .01f, 50.f);
                    dirs[2*(p*R + r)] = cosf(angle)*length;
                    dirs[2*(p*R + r) + 1] = sinf(angle)*length;
                    distances[p*R + r] = uniform(seed, .01f, 6.f);
                }
            }
            if (call == 2) {
                const float odd[6] = {NAN, INFINITY, -INFINITY, 0.f, -2.f, 3e38f};
                for (int r = 0; r < 6; r++) distances[r] = odd[r];
                dirs[2*(R + 1)] = NAN; dirs[2*(R + 2) + 1] = INFINITY; dirs[2*(R + 3)] = dirs[2*(R + 3) + 1] = 0.f;
                dirs[2*(R + 4)] = dirs[2*(R + 4) + 1] = 3e38f;
                origins[4] = NAN;
            }
            if (call == 4) origins[0] = INFINITY, origins[3] = -3e38f;
            for (int s = 0; s < S; s++) reset[s] = call == 3 && s == 0;
            MsNavAges a;
            memset(&a, 0, sizeof a);
            a.n_maps = S; a.n_viewers = P; a.n_rays = R;
            a.origins = origins.data(); a.dirs = dirs.data(); a.distances = distances.data(); a.slot = slot.data();
            a.max_range = call == 1 ? .35f : call == 5 ? 3e5f : 10.f;   // (3e5 m: over 2^20 samples a ray at this cell - skipped)
            a.reset = call >= 3 ? reset.data() : nullptr;
            a.countable = countable.data();
            a.advance = 1; a.threshold = T;
            a.last = last.data(); a.clock = clock.data();
            a.swept = swept.data(); a.gained = gained.data(); a.idle = idle.data();
            const bool survey = call != 1;                               // (call 1: the marks alone)
            if (survey) { a.oldest = oldest.data(); a.total_age = total.data(); a.n_stale = n_stale.data(); a.stale = stale.data(); a.ages = ages.data(); }
            if (call == 4) a.ages = nullptr, a.idle = nullptr;           // (only some of the outputs)
            const std::vector<int> before = clock;
            if (ms_host_nav_ages(geom, cell, &a) != MS_OK) { printf("shape %d call %d: refused\n", shape, call); failures++; continue; }
            if (call == 4) {                                             // the survey alone, with every output: the ages of call 4
                a.advance = 0; a.n_viewers = a.n_rays = 0; a.origins = a.dirs = a.distances = nullptr; a.slot = nullptr; a.reset = nullptr;
                a.ages = ages.data(); a.idle = idle.data();
                const std::vector<float> kept = last;
                if (ms_host_nav_ages(geom, cell, &a) != MS_OK || kept != last) { printf("shape %d: the survey alone\n", shape); failures++; }
            }
            for (int s = 0; s < S; s++) {
                const int start = call >= 3 && reset[s] ? 0 : before[s];
                const int now = start + 1 < (1 << 24) ? start + 1 : 1 << 24;
                if (clock[s] != now) { printf("shape %d call %d map %d: clock %d, not %d\n", shape, call, s, clock[s], now); failures++; }
                if (gained[s] > swept[s] || swept[s] > cells) { printf("shape %d call %d map %d: counts\n", shape, call, s); failures++; }
                marks += swept[s];
                if (!survey) continue;
                int old = 0, worst = 0;
                long long sum = 0;
                for (int k = 0; k < cells; k++) {
                    const int age = now - (int)last[(size_t)s*cells + k];
                    if (ages[(size_t)s*cells + k] != (float)age) { printf("shape %d call %d map %d cell %d: age\n", shape, call, s, k); failures++; }
                    const bool is = (countable[k] & 1) && age >= T;
                    if (stale[(size_t)s*cells + k] != (is ? 1 : 0)) { printf("shape %d call %d map %d cell %d: stale\n", shape, call, s, k); failures++; }
                    if (countable[k] & 1) { old += is; sum += age; worst = age > worst ? age : worst; }
                }
                if (old != n_stale[s] || sum != total[s] || worst != oldest[s]) { printf("shape %d call %d map %d: survey\n", shape, call, s); failures++; }
            }
        }
    }
    // refusals
    {
        const int geom[4] = {0, 0, 2, 2};
        unsigned char countable[4] = {1, 1, 1, 1};
        float last[4] = {0.f, 0.f, 0.f, 0.f};
        int clock = 0;
        MsNavAges a;
        memset(&a, 0, sizeof a);
        a.n_maps = 1; a.max_range = 10.f; a.threshold = 1; a.countable = countable; a.last = last; a.clock = &clock;
        if (ms_host_nav_ages(geom, cell, &a) != MS_OK || clock != 0) { printf("a call that does nothing\n"); failures++; }
        a.advance = 1;
        if (ms_host_nav_ages(geom, cell, &a) != MS_EINVAL) { printf("no viewers\n"); failures++; }
        a.advance = 0; a.threshold = 0;
        if (ms_host_nav_ages(geom, cell, &a) != MS_EINVAL) { printf("threshold 0\n"); failures++; }
        a.threshold = 1; a.last = nullptr;
        if (ms_host_nav_ages(geom, cell, &a) != MS_EINVAL || ms_host_nav_ages(geom, cell, nullptr) != MS_EINVAL) { printf("NULL\n"); failures++; }
    }
    printf("%lld countable cells swept\n", marks);
    if (marks < 100) { printf("too few marks to mean anything\n"); failures++; }
    printf(failures ? "FAILED\n" : "clean\n");
    return failures ? 1 : 0;
}
