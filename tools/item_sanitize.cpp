// A stand-alone program for a sanitizer run of the items' HOST code (csrc/kernels/items.h over navview.h and raycast.h, through
// ms_host_item_collect and ms_host_item_overlay): no GPU, no Python.  Build the library's translation unit and this file with the
// host sanitizers and run the result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/item_sanitize.cpp -o /tmp/item_sanitize
//     /tmp/item_sanitize
//
// It looks at hand-made worlds - a box with a partition and a door and a row of NaN, random oblique walls, an env without walls -
// with 1, 4 and 64 agents (NaN and infinite ones among them) and 1, 63, 64, 65 and 1024 items (absent ones, and items on an agent,
// among them): the collect with and without takers, reset and through_walls, for delays of 0, 1 and -1 over four calls each, every
// output in a buffer of exactly its size and each left out in turn, checked against a plain loop over every item, agent and wall;
// and the overlay at 1, 37, 64, 65 and 200 rays an origin, as a fan's rays (Q = A) and as a cast's (Q = R), every optional plane
// left out in turn, checked for the invariants of the rule: items within [-1, P), a shown item present, its distance below what
// the plane held, every other ray untouched.  Exit status 0 and no report from the sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

// the wall test, plainly
static bool blocks(float px, float py, float x, float y, const float* w) {
    const float ax = w[0], ay = w[1], bx = w[2], by = w[3];
    if (!(fminf(ax, bx) <= fmaxf(px, x) && fmaxf(ax, bx) >= fminf(px, x) && fminf(ay, by) <= fmaxf(py, y) && fmaxf(ay, by) >= fminf(py, y))) return false;
    const float rx = x - px, ry = y - py, vx = bx - ax, vy = by - ay;
    const float o1 = vx*(py - ay) - vy*(px - ax), o2 = vx*(y - ay) - vy*(x - ax);
    if (!((o1 < 0 && o2 > 0) || (o1 > 0 && o2 < 0))) return false;
    const float o3 = rx*(ay - py) - ry*(ax - px), o4 = rx*(by - py) - ry*(bx - px);
    return (o3 <= 0 && o4 >= 0) || (o3 >= 0 && o4 <= 0);
}

static long long failures = 0, collects = 0, overlays = 0, taken_total = 0, shown_total = 0;
#define EXPECT(c) do { if (!(c)) { failures++; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

int main() {
    const int N = 3;
    unsigned seed = 17u;
    std::vector<float> walls;
    long long wall_starts[N + 1] = {0};
    const float box[7][4] = {{0, 0, 8, 0}, {8, 0, 8, 4}, {8, 4, 0, 4}, {NAN, 1, 3, NAN}, {0, 4, 0, 0}, {4, 0, 4, 1.5f}, {4, 2.5f, 4, 4}};
    for (auto& r : box) walls.insert(walls.end(), r, r + 4);
    wall_starts[1] = 7;
    for (int l = 0; l < 40; l++) { const float x = uniform(seed, 0, 8), y = uniform(seed, 0, 4); const float w[4] = {x, y, x + uniform(seed, -1, 1), y + uniform(seed, -1, 1)}; walls.insert(walls.end(), w, w + 4); }
    wall_starts[2] = 47;
    wall_starts[3] = 47;                                                // (env 2 has no walls)
    walls.resize(walls.size() + 4, 0.f);                                // (never empty)

    const int As[] = {1, 4, 64}, Ps[] = {1, 63, 64, 65, 1024};
    for (int A : As) for (int P : Ps) {
        std::vector<float> agents((size_t)N*A*2), start((size_t)N*P*2);
        for (auto& v : agents) v = uniform(seed, .1f, 3.9f);
        for (size_t i = 0; i < agents.size(); i += 2) agents[i] *= 2.f;
        if (A > 1) { agents[2] = NAN; agents[5] = INFINITY; }
        for (size_t i = 0; i < start.size(); i += 2) {
            const int a = (int)(next_random(seed) % (unsigned)(N*A));
            const bool by = next_random(seed) % 3 == 0;
            start[i] = by ? agents[(size_t)2*a] + uniform(seed, -.3f, .3f) : uniform(seed, -.5f, 8.5f);
            start[i + 1] = by ? agents[(size_t)2*a + 1] + uniform(seed, -.3f, .3f) : uniform(seed, -.5f, 4.5f);
            if (next_random(seed) % 6 == 0) start[i] = start[i + 1] = NAN;
            if (next_random(seed) % 40 == 0 && A > 0) { start[i] = agents[0]; start[i + 1] = agents[1]; }
        }
        std::vector<int> kinds((size_t)N*P), timers0((size_t)N*P);
        for (auto& k : kinds) k = (int)(next_random(seed) % 9u);       // (8: outside [0, K), counted nowhere)
        for (auto& t : timers0) t = (int)(next_random(seed) % 5u) - 1;
        std::vector<unsigned char> takers((size_t)N*A), reset((size_t)N);
        for (auto& t : takers) t = next_random(seed) % 5 != 0;
        reset[1] = 1;
        const int K = 8;
        for (int variant = 0; variant < 12; variant++) {
            const int delay = variant % 3 - 1, through = (variant/3) % 2, masked = variant/6;
            const int leave = variant % 4;                              // 1: no taker, 2: no counts, 3: no due
            std::vector<float> positions = start;
            std::vector<int> timers = timers0;
            const float reach = .35f, reach2 = reach*reach;
            for (int call = 0; call < 4; call++) {
                std::vector<int> taker((size_t)N*P, -7), counts((size_t)N*A*K, -7);
                std::vector<unsigned char> due((size_t)N*P, 9);
                const std::vector<float> before = positions;
                const std::vector<int> timers_before = timers;
                MsItemCollect c{};
                c.n_items = P; c.n_kinds = K; c.positions = positions.data(); c.timers = timers.data(); c.kinds = kinds.data();
                c.takers = masked ? takers.data() : nullptr; c.reset = (masked && call == 2) ? reset.data() : nullptr;
                c.reach = reach; c.delay = delay; c.through_walls = through;
                c.taker = leave == 1 ? nullptr : taker.data(); c.counts = leave == 2 ? nullptr : counts.data(); c.due = leave == 3 ? nullptr : due.data();
                EXPECT(ms_host_item_collect(&c, N, A, agents.data(), walls.data(), wall_starts) == MS_OK);
                collects++;
                std::vector<int> tally((size_t)N*A*K, 0);
                for (int n = 0; n < N; n++) for (int k = 0; k < P; k++) {
                    const size_t at = (size_t)n*P + k;
                    const float x = before[2*at], y = before[2*at + 1];
                    const bool present = std::isfinite(x) && std::isfinite(y), wiped = c.reset && c.reset[n];
                    int who = -1; unsigned best = 0xffffffffu;
                    if (present && !wiped)
                        for (int a = 0; a < A; a++) {
                            const float px = agents[2*((size_t)n*A + a)], py = agents[2*((size_t)n*A + a) + 1];
                            if ((c.takers && !c.takers[(size_t)n*A + a]) || !std::isfinite(px) || !std::isfinite(py)) continue;
                            const float rx = x - px, ry = y - py, rr = rx*rx + ry*ry;
                            if (!(rr <= reach2)) continue;
                            bool blocked = false;
                            if (!through) for (long long l = wall_starts[n]; l < wall_starts[n + 1] && !blocked; l++) blocked = blocks(px, py, x, y, &walls[(size_t)4*l]);
                            unsigned bits; memcpy(&bits, &rr, 4);
                            if (!blocked && bits < best) { best = bits; who = a; }
                        }
                    int timer = timers_before[at];
                    bool absent = !present;
                    if (wiped) { timer = 0; absent = true; } else if (who >= 0) { timer = delay; absent = true; } else if (!present && timer > 0) timer--;
                    if (c.taker) EXPECT(taker[at] == who);
                    if (c.due) EXPECT(due[at] == (absent && timer == 0 ? 1 : 0));
                    EXPECT(timers[at] == timer);
                    EXPECT((std::isfinite(positions[2*at]) && std::isfinite(positions[2*at + 1])) == !absent);
                    if (wiped || who >= 0) EXPECT(std::isnan(positions[2*at]) && std::isnan(positions[2*at + 1]));
                    if (!absent) EXPECT(!memcmp(&positions[2*at], &before[2*at], 8));
                    if (who >= 0 && kinds[at] >= 0 && kinds[at] < K) tally[((size_t)n*A + who)*K + kinds[at]]++;
                    taken_total += who >= 0;
                }
                if (c.counts) EXPECT(counts == tally);
                // the return step: every other due item comes back next to an agent
                for (size_t at = 0; at < (size_t)N*P; at++)
                    if (!(std::isfinite(positions[2*at]) && std::isfinite(positions[2*at + 1])) && timers[at] == 0 && at % 2 == 0) {
                        positions[2*at] = uniform(seed, .2f, 7.8f); positions[2*at + 1] = uniform(seed, .2f, 3.8f);
                    }
            }
        }
    }

    // the overlay
    const int pers[] = {1, 37, 64, 65, 200}, Po[] = {1, 64, 65, 256, 1024};
    for (int per : pers) for (int P : Po) for (int cast = 0; cast < 2; cast++) {
        const int A = 3, R = A*per, Q = cast ? R : A;
        std::vector<float> positions((size_t)N*P*2), colors((size_t)N*P*3), origins((size_t)N*Q*2), dirs((size_t)N*R*2);
        for (size_t i = 0; i < positions.size(); i += 2) {
            positions[i] = uniform(seed, -.5f, 8.5f); positions[i + 1] = uniform(seed, -.5f, 4.5f);
            if (next_random(seed) % 5 == 0) positions[i] = positions[i + 1] = NAN;
        }
        if (P > 1) for (int k = 0; k < P; k++) positions[2*((size_t)2*P + k)] = NAN;     // (env 2: nothing present, but for P = 1)
        for (auto& v : colors) v = uniform(seed, 0, 1);
        for (size_t i = 0; i < origins.size(); i += 2) {
            if (cast && (i/2) % (size_t)per) { origins[i] = origins[i - 2]; origins[i + 1] = origins[i - 1]; continue; }
            origins[i] = uniform(seed, .2f, 7.8f); origins[i + 1] = uniform(seed, .2f, 3.8f);
        }
        origins[0] = positions[0]; origins[1] = positions[1];           // (an origin on an item, or a NaN origin)
        for (size_t i = 0; i < dirs.size(); i += 2) {
            const float a = uniform(seed, 0, 6.2831853f), l = uniform(seed, .5f, 2.f);
            dirs[i] = l*cosf(a); dirs[i + 1] = l*sinf(a);
        }
        if (R > 2) { dirs[2] = dirs[3] = 0.f; dirs[4] = NAN; }          // (a ray without a direction, a NaN ray)
        const int widths[N] = {13, 46, 6};
        for (int leave = 0; leave < 6; leave++) {
            std::vector<float> distances((size_t)N*R), locations((size_t)N*R, .5f), dots((size_t)N*R, .25f), screen((size_t)N*R*3, .125f);
            std::vector<int> indices((size_t)N*R, 3), items((size_t)N*R, -7);
            for (auto& d : distances) d = next_random(seed) % 4 == 0 ? INFINITY : uniform(seed, .2f, 6.f);
            const std::vector<float> held = distances;
            MsItemOverlay o{};
            o.n_items = P; o.n_rays = R; o.n_origins = Q; o.positions = positions.data(); o.colors = colors.data(); o.origins = origins.data();
            o.dirs = dirs.data(); o.radius = .1f; o.near_plane = .1f; o.distances = distances.data();
            o.indices = leave == 1 ? nullptr : indices.data(); o.locations = leave == 2 ? nullptr : locations.data();
            o.dots = leave == 3 ? nullptr : dots.data(); o.screen = leave == 4 ? nullptr : screen.data(); o.items = leave == 5 ? nullptr : items.data();
            if (leave == 4) o.colors = nullptr;
            EXPECT(ms_host_item_overlay(&o, N, o.indices ? widths : nullptr) == MS_OK);
            overlays++;
            for (int n = 0; n < N; n++) for (int r = 0; r < R; r++) {
                const size_t i = (size_t)n*R + r;
                const bool drawn = memcmp(&distances[i], &held[i], 4) != 0;
                if (o.items) {
                    const int k = items[i];
                    EXPECT(k >= -1 && k < P && (k >= 0) == drawn);
                    if (k >= 0) EXPECT(std::isfinite(positions[2*((size_t)n*P + k)]) && distances[i] < held[i] && distances[i] > 0.f);
                    if (k >= 0 && o.indices) EXPECT(indices[i] == widths[n] + k);
                    if (k >= 0 && o.locations) EXPECT(locations[i] >= 0.f && locations[i] <= 1.f);
                    if (k >= 0 && o.dots) EXPECT(fabsf(dots[i]) <= 1.f);
                    shown_total += k >= 0;
                }
                if (!drawn) {
                    if (o.indices) EXPECT(indices[i] == 3);
                    if (o.locations) EXPECT(locations[i] == .5f);
                    if (o.dots) EXPECT(dots[i] == .25f);
                    if (o.screen) EXPECT(screen[3*i] == .125f && screen[3*i + 1] == .125f && screen[3*i + 2] == .125f);
                }
                if (P > 1 && n == 2 && o.items) EXPECT(items[i] == -1);
            }
        }
    }
    printf("%lld collects (%lld items taken), %lld overlays (%lld rays on an item), %lld failures\n", collects, taken_total, overlays, shown_total, failures);
    return failures ? 1 : 0;
}
