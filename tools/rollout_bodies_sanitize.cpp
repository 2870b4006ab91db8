// A stand-alone program for a sanitizer run of the rollouts among bodies' HOST code (csrc/kernels/rollout_bodies.h over math.h,
// step.h, bodies.h and rollout.h, through ms_host_rollouts_bodies): no GPU, no Python.  Build the library's translation unit and
// this file with the host sanitizers and run the result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/rollout_bodies_sanitize.cpp -o /tmp/rollout_bodies_sanitize
//     /tmp/rollout_bodies_sanitize
//
// A hand-made room - a box with a pillar and a diagonal - and an env without a wall, every array allocated to the byte
// (std::vector: a read or write past an end is a report); one, two and five agents at random poses, at NaN and too fast; stores of
// 1, 7, 64, 65 and 1024 slots - scattered, clustered on the agents, absent, at NaN and at infinity, at rest and with velocities (a
// NaN among them); 1, 3 and 65 candidates over 1, 6 and 64 steps, shared plans and plans of their own, wild actions, a mask, with
// and without each optional output.  Checked on the way: progress in [0, 1]; body_stops within stops; first_blocker -1 or a
// present slot, and there exactly where body_stops is not 0; the store and the agents untouched; and the refusals.  Exit status 0
// and no report from the sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

static int failures = 0;
static long long rolled = 0, stopped = 0, by_body = 0;

#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void box(std::vector<float>& w, float x0, float y0, float x1, float y1) {
    const float rows[16] = {x0, y0, x1, y0, x1, y0, x1, y1, x1, y1, x0, y1, x0, y1, x0, y0};
    w.insert(w.end(), rows, rows + 16);
}

static const float TABLE[8*3] = {0, 0, 0, 0, 3, 0, 0, -3, 0, 3, 0, 0, -3, 0, 0, 0, 0, 90, 0, 0, -90, 0, 20, 0};
static const MsConfig CFG = {.106f, 8, 90.f, 10.f};

static void roll(const std::vector<float>& walls, int A, int P, int K, int H, bool moving, bool shared, bool masked, int outputs, unsigned& seed) {
    std::vector<float> angles(A), positions(2*A), angvelocity(A), velocity(2*A);
    for (int a = 0; a < A; a++) {
        const unsigned kind = next_random(seed) % 8;
        positions[2*a] = uniform(seed, .2f, 3.8f); positions[2*a + 1] = uniform(seed, .2f, 3.8f);
        velocity[2*a] = uniform(seed, -3.f, 3.f); velocity[2*a + 1] = uniform(seed, -3.f, 3.f);
        angles[a] = uniform(seed, -180.f, 180.f); angvelocity[a] = uniform(seed, -90.f, 90.f);
        if (kind == 0) positions[2*a] = NAN;
        if (kind == 1) velocity[2*a] *= 30.f;
        if (kind == 2) { velocity[2*a] = 0.f; velocity[2*a + 1] = 0.f; }
    }
    std::vector<float> bp(2*(size_t)P), bv(2*(size_t)P);
    for (int k = 0; k < P; k++) {
        const unsigned kind = next_random(seed) % 10;
        const int a = (int)(next_random(seed) % A);
        bp[2*k] = uniform(seed, .2f, 3.8f); bp[2*k + 1] = uniform(seed, .2f, 3.8f);
        bv[2*k] = uniform(seed, -2.f, 2.f); bv[2*k + 1] = uniform(seed, -2.f, 2.f);
        if (kind < 4) { bp[2*k] = positions[2*a] + uniform(seed, -.5f, .5f); bp[2*k + 1] = positions[2*a + 1] + uniform(seed, -.5f, .5f); }
        if (kind == 4) bp[2*k] = NAN;
        if (kind == 5) bp[2*k + 1] = INFINITY;
        if (kind == 6) bv[2*k + 1] = NAN;
        if (kind == 7) { bv[2*k] = 0.f; bv[2*k + 1] = 0.f; }
    }
    const std::vector<float> bp0 = bp, bv0 = bv, positions0 = positions, velocity0 = velocity;
    const size_t n = (size_t)A*K;
    std::vector<long long> actions((shared ? (size_t)K : n)*H);
    for (auto& x : actions) x = (long long)(next_random(seed) % 10) - 1;
    std::vector<unsigned char> mask(A);
    for (auto& x : mask) x = (unsigned char)(next_random(seed) % 3 != 0);
    std::vector<float> p(2*n, -9.f), ang(n, -9.f), v(2*n, -9.f), w(n, -9.f), progress(n, -9.f), trail(2*n*H, -9.f);
    std::vector<int> stops(n, -9), first(n, -9), body_stops(n, -9), blocker(n, -9);
    MsRollouts r = {K, H, actions.data(), shared ? 1 : 0, TABLE, 8, (rolled % 2) ? .875f : 0.f, A > 1 ? 1 : 0, masked ? mask.data() : nullptr,
                    p.data(), ang.data(), v.data(), w.data(), progress.data(), stops.data(), first.data(), (outputs & 4) ? trail.data() : nullptr,
                    0, 0.f, nullptr};
    MsRolloutBodies rb = {P, bp.data(), moving ? bv.data() : nullptr, (outputs & 1) ? body_stops.data() : nullptr, (outputs & 2) ? blocker.data() : nullptr};
    MsAgents view = {angles.data(), positions.data(), angvelocity.data(), velocity.data(), nullptr, nullptr};
    const int status = ms_host_rollouts_bodies(walls.empty() ? nullptr : walls.data(), (int)(walls.size()/4), &view, A, &r, &rb, &CFG);
    CHECK(status == MS_OK, "status %d", status);
    CHECK(std::memcmp(bp.data(), bp0.data(), bp.size()*sizeof(float)) == 0, "the store's positions were written");
    CHECK(std::memcmp(bv.data(), bv0.data(), bv.size()*sizeof(float)) == 0, "the store's velocities were written");
    CHECK(std::memcmp(positions.data(), positions0.data(), positions.size()*sizeof(float)) == 0 &&
          std::memcmp(velocity.data(), velocity0.data(), velocity.size()*sizeof(float)) == 0, "the agents were written");
    for (size_t i = 0; i < n; i++) {
        if (masked && !mask[i/K]) { CHECK(progress[i] == -9.f && stops[i] == -9 && body_stops[i] == -9 && blocker[i] == -9, "an agent left out was written"); continue; }
        rolled++;
        CHECK(progress[i] >= 0.f && progress[i] <= 1.f, "progress %g", progress[i]);
        CHECK(stops[i] >= 0 && stops[i] <= H && first[i] >= 0 && first[i] <= H, "stops %d, first_stop %d", stops[i], first[i]);
        stopped += stops[i] > 0;
        if (outputs & 1) { CHECK(body_stops[i] >= 0 && body_stops[i] <= stops[i], "body_stops %d of %d stops", body_stops[i], stops[i]); by_body += body_stops[i] > 0; }
        if (outputs & 2) {
            const int k = blocker[i];
            CHECK(k >= -1 && k < P && (k < 0 || (std::isfinite(bp[2*k]) && std::isfinite(bp[2*k + 1]))), "first_blocker %d", k);
            CHECK(!(outputs & 1) || (k >= 0) == (body_stops[i] > 0), "first_blocker %d with %d body stops", k, body_stops[i]);
        }
    }
}

int main() {
    unsigned seed = 4321u;
    std::vector<float> room, none;
    box(room, 0, 0, 4, 4); box(room, 1.5f, 1.5f, 2, 2);
    const float diagonal[4] = {3, 0, 4, 1};
    room.insert(room.end(), diagonal, diagonal + 4);
    int round = 0;
    for (int A : {1, 2, 5})
        for (int P : {1, 7, 64, 65, 1024})
            for (int K : {1, 3, 65})
                for (int H : {1, 6, 64}) {
                    if (P == 1024 && K == 65 && H == 64) continue;       // (minutes under the sanitizers, and no path the others leave out)
                    roll(round % 5 ? room : none, A, P, K, H, round % 2 == 0, round % 3 == 0, round % 4 == 1, round % 8, seed);
                    round++;
                }
    // the refusals
    {
        std::vector<float> agents(4, 1.f), slots(2*8 + 1, 1.f), out(4*6);
        std::vector<int> books(3);
        std::vector<long long> actions(2, 1);
        MsAgents view = {agents.data(), agents.data(), agents.data(), agents.data(), nullptr, nullptr};
        int* const ints = reinterpret_cast<int*>(out.data());
        const MsRollouts plain = {1, 2, actions.data(), 1, TABLE, 8, 0.f, 0, nullptr, out.data(), out.data() + 2, out.data() + 4, out.data() + 6,
                                  out.data() + 7, ints + 8, ints + 9, nullptr, 0, 0.f, nullptr};
        const MsRolloutBodies good = {8, slots.data(), nullptr, books.data(), books.data() + 1};
        const auto call = [&](const MsRollouts* r, const MsRolloutBodies* rb) {
            return ms_host_rollouts_bodies(room.data(), (int)(room.size()/4), &view, 1, r, rb, &CFG);
        };
        CHECK(call(&plain, &good) == MS_OK, "a sound call");
        CHECK(call(&plain, nullptr) == MS_EINVAL && call(nullptr, &good) == MS_EINVAL, "no struct");
        MsRolloutBodies bad = good; bad.positions = nullptr;
        CHECK(call(&plain, &bad) == MS_EINVAL, "no positions");
        bad = good; bad.positions = slots.data() + 1;
        CHECK(call(&plain, &bad) == MS_EINVAL, "positions off 8 bytes");
        bad = good; bad.velocities = slots.data() + 1;
        CHECK(call(&plain, &bad) == MS_EINVAL, "velocities off 8 bytes");
        bad = good; bad.body_stops = reinterpret_cast<int*>(reinterpret_cast<char*>(books.data()) + 2);
        CHECK(call(&plain, &bad) == MS_EINVAL, "body_stops off 4 bytes");
        bad = good; bad.first_blocker = reinterpret_cast<int*>(reinterpret_cast<char*>(books.data()) + 2);
        CHECK(call(&plain, &bad) == MS_EINVAL, "first_blocker off 4 bytes");
        for (int P : {0, -1, 1025}) { bad = good; bad.n_slots = P; CHECK(call(&plain, &bad) == MS_EINVAL, "%d slots", P); }
        MsRollouts sliding = plain; sliding.slide = 1; sliding.bounce = .05f;
        CHECK(call(&sliding, &good) == MS_EINVAL, "a sliding rollout");
        CHECK(ms_debug_rollout_scheme(1) == MS_OK && call(&plain, &good) == MS_EINVAL, "the lane-a-wall scheme pinned");
        CHECK(ms_debug_rollout_scheme(0) == MS_OK && call(&plain, &good) == MS_OK && ms_debug_rollout_scheme(-1) == MS_OK, "the lane-a-candidate scheme pinned");
        CHECK(ms_rollouts_bodies(nullptr, &view, &plain, &good, &CFG, nullptr) == MS_EINVAL, "the device entry without a scenery");
    }
    std::printf("%lld candidates rolled: %lld stopped, %lld of them by a body; %d failures\n", rolled, stopped, by_body, failures);
    return failures ? 1 : 0;
}
