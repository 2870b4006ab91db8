// A stand-alone program for a sanitizer run of the walkers' HOST code (csrc/kernels/walker.h over step.h and math.h, through
// ms_host_walkers): no GPU, no Python.  Build the library's translation unit and this file with the host sanitizers and run the
// result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/walker_sanitize.cpp -o /tmp/walker_sanitize
//     /tmp/walker_sanitize
//
// It looks at hand-made rooms - a box with a diagonal partition and a row of NaN, random oblique walls, an env without walls - with
// 1, 5 and 64 agents (a NaN and an infinite position among them) and 1, 64, 65 and 1024 slots: eight ticks each, a reset in the
// fifth, walkers at rest, NaN and infinite velocities, speeds and targets, every buffer of exactly its size and each record left
// out in turn, checked for the invariants of the rule: progress within [0, 1] and NaN exactly on an absent slot, blocked within
// 0 .. 4 and 0 exactly where progress is 1, a stopped walker at rest, an absent slot untouched, a present one present and finite
// afterwards and no further than its speed allows, bumps the count of blocked == 1 at least, close and bumps within [0, P].
// Exit status 0 and no report from the sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

static long long failures = 0, ticks = 0, stopped_total = 0, bumps_total = 0;
#define EXPECT(c) do { if (!(c)) { failures++; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

int main() {
    const int N = 3;
    unsigned seed = 29u;
    std::vector<float> walls;
    long long wall_starts[N + 1] = {0};
    const float box[6][4] = {{0, 0, 8, 0}, {8, 0, 8, 4}, {8, 4, 0, 4}, {NAN, 1, 3, NAN}, {0, 4, 0, 0}, {4, 1, 6, 3}};
    for (auto& r : box) walls.insert(walls.end(), r, r + 4);
    wall_starts[1] = 6;
    for (int l = 0; l < 40; l++) { const float x = uniform(seed, 0, 8), y = uniform(seed, 0, 4); const float w[4] = {x, y, x + uniform(seed, -1, 1), y + uniform(seed, -1, 1)}; walls.insert(walls.end(), w, w + 4); }
    wall_starts[2] = 46;
    wall_starts[3] = 46;                                                // (env 2 has no walls)
    walls.resize(walls.size() + 4, 0.f);                                // (never empty)

    const int As[] = {1, 5, 64}, Ps[] = {1, 64, 65, 1024};
    for (int A : As) for (int P : Ps) for (int leave = 0; leave < 5; leave++) {
        std::vector<float> agents((size_t)N*A*2), positions((size_t)N*P*2), velocities((size_t)N*P*2), speeds((size_t)N*P), towards((size_t)N*P*2);
        for (size_t i = 0; i < agents.size(); i += 2) { agents[i] = uniform(seed, .2f, 7.8f); agents[i + 1] = uniform(seed, .2f, 3.8f); }
        if (A > 1) { agents[2] = NAN; agents[(size_t)2*A + 3] = INFINITY; }
        for (size_t at = 0; at < (size_t)N*P; at++) {
            const float span = P > 64 ? 1.f : 0.f;                      // (a crowded store: bodies meet)
            positions[2*at] = uniform(seed, 1.f + span, 7.f - span); positions[2*at + 1] = uniform(seed, .5f + span, 3.5f - span);
            if (next_random(seed) % 3 == 0) positions[2*at] = positions[2*at + 1] = NAN;
            velocities[2*at] = uniform(seed, -1.f, 1.f); velocities[2*at + 1] = next_random(seed) % 5 == 0 ? 0.f : uniform(seed, -1.f, 1.f);
            if (next_random(seed) % 40 == 0) velocities[2*at] = NAN;
            if (next_random(seed) % 40 == 0) velocities[2*at + 1] = INFINITY;
            speeds[at] = next_random(seed) % 30 == 0 ? NAN : uniform(seed, 0.f, 2.f);
            towards[2*at] = uniform(seed, -1.f, 9.f); towards[2*at + 1] = uniform(seed, -1.f, 5.f);
            if (next_random(seed) % 9 == 0) towards[2*at] = NAN;
            if (next_random(seed) % 50 == 0) towards[2*at + 1] = INFINITY;
        }
        std::vector<unsigned char> reset((size_t)N);
        reset[1] = 1;
        for (int tick = 0; tick < 8; tick++) {
            std::vector<float> progress((size_t)N*P, 7.f);
            std::vector<unsigned char> blocked((size_t)N*P, 9);
            std::vector<int> bumps((size_t)N*A, -7), close((size_t)N*A, -7);
            const std::vector<float> before = positions, vbefore = velocities;
            MsWalkers w{};
            w.n_slots = P; w.positions = positions.data(); w.velocities = velocities.data(); w.speeds = speeds.data(); w.towards = towards.data();
            w.reset = tick == 4 ? reset.data() : nullptr;
            w.personal = .6f; w.push = tick % 3 ? 1.f : 0.f; w.keep = tick % 2 ? .5f : 0.f; w.agents_push = tick % 4 < 2; w.fps = 10.f; w.agent_radius = .15f;
            w.progress = leave == 1 ? nullptr : progress.data(); w.blocked = leave == 2 ? nullptr : blocked.data();
            w.bumps = leave == 3 ? nullptr : bumps.data(); w.close = leave == 4 ? nullptr : close.data();
            EXPECT(ms_host_walkers(&w, N, A, agents.data(), walls.data(), wall_starts) == MS_OK);
            ticks++;
            std::vector<int> by_agent((size_t)N, 0);
            for (int n = 0; n < N; n++) for (int k = 0; k < P; k++) {
                const size_t at = (size_t)n*P + k;
                const bool was = std::isfinite(before[2*at]) && std::isfinite(before[2*at + 1]);
                const bool is = std::isfinite(positions[2*at]) && std::isfinite(positions[2*at + 1]);
                const bool wiped = w.reset && w.reset[n];
                if (wiped) { EXPECT(!is); if (w.blocked) EXPECT(blocked[at] == 4); if (w.progress) EXPECT(std::isnan(progress[at])); continue; }
                EXPECT(is == was);
                if (!was) EXPECT(!memcmp(&positions[2*at], &before[2*at], 8) && !memcmp(&velocities[2*at], &vbefore[2*at], 8));
                if (w.progress) EXPECT(was ? (progress[at] >= 0.f && progress[at] <= 1.f) : std::isnan(progress[at]));
                if (w.blocked) EXPECT(blocked[at] <= 4 && (blocked[at] == 4) == !was);
                if (w.progress && w.blocked && was) EXPECT((blocked[at] == 0) == (progress[at] == 1.f));
                if (!was) continue;
                EXPECT(std::isfinite(velocities[2*at]) && std::isfinite(velocities[2*at + 1]));
                if (w.progress && progress[at] < 1.f) { EXPECT(velocities[2*at] == 0.f && velocities[2*at + 1] == 0.f); stopped_total++; }
                if (w.blocked && blocked[at] == 1) by_agent[(size_t)n]++;
                // no further than the blend allows: keep |v_old| + (1 - keep) speed, a tick of it; a stored velocity that is not finite: it stood
                const float vo = std::hypot(vbefore[2*at], vbefore[2*at + 1]), moved = std::hypot(positions[2*at] - before[2*at], positions[2*at + 1] - before[2*at + 1]);
                if (std::isfinite(vo) && std::isfinite(speeds[at])) EXPECT(moved <= (w.keep*vo + (1.f - w.keep)*speeds[at])/w.fps*1.001f + 1e-6f);
                else if (!std::isfinite(vo)) EXPECT(moved == 0.f);
            }
            for (int n = 0; n < N; n++) {
                int sum = 0;
                for (int a = 0; a < A; a++) {
                    const size_t at = (size_t)n*A + a;
                    if (w.bumps) { EXPECT(bumps[at] >= 0 && bumps[at] <= P); sum += bumps[at]; bumps_total += bumps[at]; }
                    if (w.close) EXPECT(close[at] >= 0 && close[at] <= P);
                }
                if (w.bumps && w.blocked && !(w.reset && w.reset[n])) EXPECT(sum >= by_agent[(size_t)n]);
            }
        }
    }
    printf("%lld ticks (%lld stops, %lld bumps), %lld failures\n", ticks, stopped_total, bumps_total, failures);
    return failures ? 1 : 0;
}
