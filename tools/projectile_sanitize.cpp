// A stand-alone program for a sanitizer run of the projectiles' HOST code (csrc/kernels/projectile.h over raycast.h, shade.h and
// items.h, through ms_host_projectiles): no GPU, no Python.  Build the library's translation unit and this file with the host
// sanitizers and run the result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/projectile_sanitize.cpp -o /tmp/projectile_sanitize
//     /tmp/projectile_sanitize
//
// It looks at hand-made worlds - a box with a diagonal partition and a row of NaN, random oblique walls, an env without walls -
// with 1, 4 and 64 agents (NaN and infinite poses among them) and 1, 3 and 16 slots an agent: eight ticks each with fire every
// other tick, a reset in the fifth, shots at rest, NaN and infinite velocities, every buffer of exactly its size and each record
// left out in turn, checked for the invariants of the rule: struck within [-1, A) and never the owner, ended within 0 .. 4 and
// consistent with struck and with presence, a slot that was absent and not fired into untouched, hits and scored the counts of
// struck, bounces never negative and never rising, a timer falling by one.  Exit status 0 and no report from the sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

static long long failures = 0, ticks = 0, struck_total = 0, bounced_total = 0;
#define EXPECT(c) do { if (!(c)) { failures++; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

int main() {
    const int N = 3, M = 8;
    unsigned seed = 23u;
    std::vector<float> walls;
    long long wall_starts[N + 1] = {0};
    const float box[6][4] = {{0, 0, 8, 0}, {8, 0, 8, 4}, {8, 4, 0, 4}, {NAN, 1, 3, NAN}, {0, 4, 0, 0}, {4, 1, 6, 3}};
    for (auto& r : box) walls.insert(walls.end(), r, r + 4);
    wall_starts[1] = 6;
    for (int l = 0; l < 40; l++) { const float x = uniform(seed, 0, 8), y = uniform(seed, 0, 4); const float w[4] = {x, y, x + uniform(seed, -1, 1), y + uniform(seed, -1, 1)}; walls.insert(walls.end(), w, w + 4); }
    wall_starts[2] = 46;
    wall_starts[3] = 46;                                                // (env 2 has no walls)
    walls.resize(walls.size() + 4, 0.f);                                // (never empty)
    std::vector<float> model((size_t)M*4);
    for (int m = 0; m < M; m++) {                                       // an octagon of radius .15
        const float a0 = 6.2831853f*m/M, a1 = 6.2831853f*(m + 1)/M;
        const float row[4] = {.15f*cosf(a0), .15f*sinf(a0), .15f*cosf(a1), .15f*sinf(a1)};
        memcpy(&model[(size_t)4*m], row, sizeof row);
    }

    const int As[] = {1, 4, 64}, Ss[] = {1, 3, 16};
    for (int A : As) for (int S : Ss) for (int leave = 0; leave < 6; leave++) {
        const int P = A*S;
        std::vector<float> agents((size_t)N*A*2), angles((size_t)N*A), positions((size_t)N*P*2), velocities((size_t)N*P*2);
        for (size_t i = 0; i < agents.size(); i += 2) { agents[i] = uniform(seed, .2f, 7.8f); agents[i + 1] = uniform(seed, .2f, 3.8f); }
        for (auto& v : angles) v = uniform(seed, -180.f, 180.f);
        if (A > 1) { agents[2] = NAN; angles[(size_t)A + 2] = INFINITY; }
        std::vector<int> owners((size_t)N*P), timers((size_t)N*P), bounces((size_t)N*P);
        for (size_t at = 0; at < (size_t)N*P; at++) {
            positions[2*at] = uniform(seed, -.5f, 8.5f); positions[2*at + 1] = uniform(seed, -.5f, 4.5f);
            if (next_random(seed) % 3 == 0) positions[2*at] = positions[2*at + 1] = NAN;
            const float a = uniform(seed, 0, 6.2831853f), sp = next_random(seed) % 5 == 0 ? 0.f : uniform(seed, .1f, 90.f);
            velocities[2*at] = sp*cosf(a); velocities[2*at + 1] = sp*sinf(a);
            if (next_random(seed) % 40 == 0) velocities[2*at] = NAN;
            if (next_random(seed) % 40 == 0) velocities[2*at + 1] = INFINITY;
            owners[at] = (int)(at % (size_t)P)/S; timers[at] = (int)(next_random(seed) % 6u); bounces[at] = (int)(next_random(seed) % 4u);
        }
        std::vector<unsigned char> fire((size_t)N*A), reset((size_t)N);
        reset[1] = 1;
        for (int tick = 0; tick < 8; tick++) {
            for (auto& f : fire) f = next_random(seed) % 2;
            std::vector<int> struck((size_t)N*P, -7), hits((size_t)N*A, -7), scored((size_t)N*A, -7);
            std::vector<unsigned char> ended((size_t)N*P, 9), misfires((size_t)N*A, 9);
            const std::vector<float> before = positions, vbefore = velocities;
            const std::vector<int> tbefore = timers, bbefore = bounces;
            MsProjectiles p{};
            p.n_slots = P; p.per_agent = S; p.positions = positions.data(); p.velocities = velocities.data(); p.owners = owners.data();
            p.timers = timers.data(); p.bounces = bounces.data(); p.fire = tick % 2 ? nullptr : fire.data(); p.reset = tick == 4 ? reset.data() : nullptr;
            p.speed = 8.f; p.muzzle = .25f; p.life = 5; p.n_bounces = 2; p.restitution = tick % 3 ? 1.f : .5f; p.fps = 10.f;
            p.struck = leave == 1 ? nullptr : struck.data(); p.ended = leave == 2 ? nullptr : ended.data(); p.hits = leave == 3 ? nullptr : hits.data();
            p.scored = leave == 4 ? nullptr : scored.data(); p.misfires = leave == 5 ? nullptr : misfires.data();
            EXPECT(ms_host_projectiles(&p, N, A, agents.data(), angles.data(), model.data(), M, walls.data(), wall_starts) == MS_OK);
            ticks++;
            std::vector<int> tally_hits((size_t)N*A, 0), tally_scored((size_t)N*A, 0);
            for (int n = 0; n < N; n++) for (int k = 0; k < P; k++) {
                const size_t at = (size_t)n*P + k;
                const bool was = std::isfinite(before[2*at]) && std::isfinite(before[2*at + 1]);
                const bool is = std::isfinite(positions[2*at]) && std::isfinite(positions[2*at + 1]);
                const bool wiped = p.reset && p.reset[n];
                if (wiped) { EXPECT(!is && timers[at] == 0 && bounces[at] == 0); }
                const bool tame = std::isfinite(vbefore[2*at]) && std::isfinite(vbefore[2*at + 1]);     // (an infinite velocity flies to infinity)
                if (p.ended) EXPECT(ended[at] <= 4 && ((ended[at] == 0) == is || (was && !tame)));
                if (p.struck) EXPECT(struck[at] >= -1 && struck[at] < A && (struck[at] < 0 || struck[at] != owners[at]));
                if (p.struck && p.ended) EXPECT((struck[at] >= 0) == (ended[at] == 1));
                if (!wiped && !was && !p.fire) EXPECT(!is && timers[at] == tbefore[at] && bounces[at] == bbefore[at] && !memcmp(&velocities[2*at], &vbefore[2*at], 8));
                if (!wiped && was) { EXPECT(bounces[at] >= 0 && bounces[at] <= bbefore[at]); bounced_total += bbefore[at] - bounces[at]; }
                if (!wiped && was && is) EXPECT(timers[at] == tbefore[at] - 1 && timers[at] != 0);
                if (p.struck && struck[at] >= 0) { tally_hits[(size_t)n*A + struck[at]]++; tally_scored[(size_t)n*A + owners[at]]++; struck_total++; }
            }
            if (p.struck && p.hits) EXPECT(hits == tally_hits);
            if (p.struck && p.scored) EXPECT(scored == tally_scored);
            if (p.misfires) for (auto m : misfires) EXPECT(m <= 1);
        }
    }
    printf("%lld ticks (%lld strikes, %lld bounces), %lld failures\n", ticks, struck_total, bounced_total, failures);
    return failures ? 1 : 0;
}
