// A stand-alone program for a sanitizer run of the step among bodies' HOST code (csrc/kernels/bodies.h over math.h and step.h,
// through ms_host_bodies): no GPU, no Python.  Build the library's translation unit and this file with the host sanitizers and run
// the result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/bodies_sanitize.cpp -o /tmp/bodies_sanitize
//     /tmp/bodies_sanitize
//
// Hand-made worlds - a room with a pillar and a diagonal, a corridor, an env without a wall - every array allocated to the byte
// (std::vector: a read or write past an end is a report); one, two, five and 64 agents an env at random poses, pressed against a
// wall, far outside, at NaN and at infinity, crawling and too fast; stores of 1, 7, 64, 65 and 1024 slots - scattered, clustered on
// the agents, absent, at NaN and at infinity, at rest and with velocities (a NaN among them) - with and without the movement
// prologue, respawns, lifespans and the IMU reading, with and without each optional output.  Checked on the way: progress in
// [0, 1]; blocker -1 or a present slot, and only where the agent was blocked and had a contact; contacts within the store; a
// blocked agent at rest; the store untouched; and the refusals.  Exit status 0 and no report from the sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

static int failures = 0;
static long long stepped = 0, blocked = 0, by_body = 0, touched = 0;

#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void box(std::vector<float>& w, float x0, float y0, float x1, float y1) {
    const float rows[16] = {x0, y0, x1, y0, x1, y0, x1, y1, x1, y1, x0, y1, x0, y1, x0, y0};
    w.insert(w.end(), rows, rows + 16);
}

static const float TABLE[8*3] = {0, 0, 0, 0, 3, 0, 0, -3, 0, 3, 0, 0, -3, 0, 0, 0, 0, 90, 0, 0, -90, 0, 20, 0};
static const MsConfig CFG = {.106f, 8, 90.f, 10.f};

static void step(const std::vector<std::vector<float>>& envs, int A, int P, bool moving, bool moved, int extras, int outputs, unsigned& seed) {
    const int N = (int)envs.size();
    std::vector<float> walls;
    std::vector<long long> starts(1, 0);
    for (const auto& w : envs) { walls.insert(walls.end(), w.begin(), w.end()); starts.push_back((long long)walls.size()/4); }
    walls.resize(walls.size() + 4, 0.f);                                 // (a row behind the last: the pointer of an env without walls)
    const size_t n = (size_t)N*A, m = (size_t)N*P;
    std::vector<float> angles(n), positions(2*n), angvelocity(n), velocity(2*n);
    for (size_t a = 0; a < n; a++) {
        const unsigned kind = next_random(seed) % 12;
        positions[2*a] = uniform(seed, .2f, 3.8f); positions[2*a + 1] = uniform(seed, .2f, 3.8f);
        velocity[2*a] = uniform(seed, -3.f, 3.f); velocity[2*a + 1] = uniform(seed, -3.f, 3.f);
        angles[a] = uniform(seed, -180.f, 180.f); angvelocity[a] = uniform(seed, -90.f, 90.f);
        if (kind == 0) { positions[2*a] = .106f; velocity[2*a] = -2.f; }
        if (kind == 1) { positions[2*a] = -30.f; positions[2*a + 1] = 1e4f; }
        if (kind == 2) positions[2*a] = NAN;
        if (kind == 3) positions[2*a + 1] = INFINITY;
        if (kind == 4) { velocity[2*a] *= 1e-7f; velocity[2*a + 1] *= 1e-7f; }
        if (kind == 5) velocity[2*a] *= 30.f;
        if (kind == 6) { velocity[2*a] = NAN; angles[a] = 1e30f; }
        if (kind == 7) { velocity[2*a] = 0.f; velocity[2*a + 1] = 0.f; }
    }
    std::vector<float> bp(2*m), bv(2*m);
    for (size_t k = 0; k < m; k++) {
        const unsigned kind = next_random(seed) % 10;
        const size_t a = (k/P)*A + next_random(seed) % A;                // (an agent of the body's env)
        bp[2*k] = uniform(seed, .2f, 3.8f); bp[2*k + 1] = uniform(seed, .2f, 3.8f);
        bv[2*k] = uniform(seed, -2.f, 2.f); bv[2*k + 1] = uniform(seed, -2.f, 2.f);
        if (kind < 4) { bp[2*k] = positions[2*a] + uniform(seed, -.5f, .5f); bp[2*k + 1] = positions[2*a + 1] + uniform(seed, -.5f, .5f); }
        if (kind == 4) bp[2*k] = NAN;
        if (kind == 5) bp[2*k + 1] = INFINITY;
        if (kind == 6) { bp[2*k] = positions[2*a]; bp[2*k + 1] = positions[2*a + 1]; }
        if (kind == 7) bv[2*k + 1] = NAN;
        if (kind == 8) { bv[2*k] = 0.f; bv[2*k + 1] = 0.f; }
    }
    const std::vector<float> bp0 = bp, bv0 = bv;
    std::vector<long long> actions(n), choice(n);
    for (auto& x : actions) x = (long long)(next_random(seed) % 10) - 1;
    const int S = 3;
    std::vector<unsigned char> mask(n);
    std::vector<float> spawn_p(n*S*2), spawn_a(n*S), imu(3*n, -9.f);
    std::vector<int> life(n), max_life(n, 4), fresh(n, 7);
    for (size_t i = 0; i < n; i++) { mask[i] = (unsigned char)(next_random(seed) % 4 == 0); choice[i] = (long long)(next_random(seed) % 5) - 1; life[i] = (int)(next_random(seed) % 5); }
    for (auto& x : spawn_p) x = uniform(seed, .3f, 3.7f);
    for (auto& x : spawn_a) x = uniform(seed, -180.f, 180.f);
    MsMovement mv = {actions.data(), TABLE, 8, (stepped % 2) ? .875f : 0.f};
    MsStepExtras ex;
    std::memset(&ex, 0, sizeof ex);
    ex.imu_ang_scale = 360.f; ex.imu_speed_scale = 10.f;
    if (extras >= 1) { ex.respawn_mask = mask.data(); ex.respawn_choice = choice.data(); ex.spawn_positions = spawn_p.data(); ex.spawn_angles = spawn_a.data();
                       ex.n_spawns = S; ex.respawn_after = extras == 2; ex.imu = imu.data(); }
    if (extras >= 2) { ex.lifespans = life.data(); ex.max_lifespans = max_life.data(); ex.fresh_max = fresh.data(); }
    std::vector<float> progress(n, -9.f);
    std::vector<int> blocker(n, -9), contacts(n, -9);
    MsBodies bd = {P, bp.data(), moving ? bv.data() : nullptr, (outputs & 1) ? blocker.data() : nullptr, (outputs & 2) ? contacts.data() : nullptr};
    MsAgents view = {angles.data(), positions.data(), angvelocity.data(), velocity.data(), nullptr, nullptr};
    const int status = ms_host_bodies(walls.data(), starts.data(), N, A, &view, moved ? &mv : nullptr, extras ? &ex : nullptr, &bd, progress.data(), &CFG);
    CHECK(status == MS_OK, "status %d", status);
    CHECK(std::memcmp(bp.data(), bp0.data(), bp.size()*sizeof(float)) == 0 && std::memcmp(bv.data(), bv0.data(), bv.size()*sizeof(float)) == 0, "the store was written");
    for (size_t i = 0; i < n; i++) {
        stepped++;
        CHECK(progress[i] >= 0.f && progress[i] <= 1.f, "progress %g", progress[i]);
        blocked += progress[i] < 1.f;
        if (outputs & 2) { CHECK(contacts[i] >= 0 && contacts[i] <= P, "contacts %d", contacts[i]); touched += contacts[i]; }
        if (outputs & 1) {
            const int k = blocker[i];
            CHECK(k >= -1 && k < P, "blocker %d", k);
            if (k >= 0) {
                const size_t at = (i/A)*P + k;
                CHECK(progress[i] < 1.f && std::isfinite(bp[2*at]) && std::isfinite(bp[2*at + 1]), "blocker %d at progress %g", k, progress[i]);
                CHECK(!(outputs & 2) || contacts[i] > 0, "a blocker without a contact");
                by_body++;
            }
        }
        if (progress[i] < 1.f && !(extras == 2 && mask[i]))
            CHECK(velocity[2*i] == 0.f && velocity[2*i + 1] == 0.f && angvelocity[i] == 0.f, "a blocked agent moves");
    }
}

int main() {
    unsigned seed = 4321u;
    std::vector<float> room, corridor, none;
    box(room, 0, 0, 4, 4); box(room, 1.5f, 1.5f, 2, 2);
    const float diagonal[4] = {3, 0, 4, 1};
    room.insert(room.end(), diagonal, diagonal + 4);
    box(corridor, 0, 0, 6, .5f);
    int round = 0;
    for (int A : {1, 2, 5, 64})
        for (int P : {1, 7, 64, 65, 1024})
            for (int extras = 0; extras < 3; extras++, round++) {
                step({room}, A, P, round % 2 == 0, round % 3 == 0, extras, 3, seed);
                step({corridor, none, room}, A, P, round % 2 == 1, round % 3 != 0, extras, round % 4, seed);
            }
    // the refusals
    {
        std::vector<float> agents(2*65, 1.f), slots(2*8 + 1, 1.f), progress(65);
        std::vector<int> out(66);
        MsAgents view = {agents.data(), agents.data(), agents.data(), agents.data(), nullptr, nullptr};
        const long long starts[2] = {0, (long long)room.size()/4};
        const MsBodies good = {8, slots.data(), nullptr, out.data(), out.data()};
        const auto call = [&](const MsBodies* bd, int A) { return ms_host_bodies(room.data(), starts, 1, A, &view, nullptr, nullptr, bd, progress.data(), &CFG); };
        CHECK(call(&good, 1) == MS_OK && call(&good, 64) == MS_OK, "a sound call");
        CHECK(call(nullptr, 1) == MS_EINVAL, "no MsBodies");
        CHECK(call(&good, 65) == MS_EINVAL, "65 agents");
        MsBodies bad = good; bad.positions = nullptr;
        CHECK(call(&bad, 1) == MS_EINVAL, "no positions");
        bad = good; bad.positions = slots.data() + 1;
        CHECK(call(&bad, 1) == MS_EINVAL, "positions off 8 bytes");
        bad = good; bad.velocities = slots.data() + 1;
        CHECK(call(&bad, 1) == MS_EINVAL, "velocities off 8 bytes");
        bad = good; bad.blocker = reinterpret_cast<int*>(reinterpret_cast<char*>(out.data()) + 2);
        CHECK(call(&bad, 1) == MS_EINVAL, "blocker off 4 bytes");
        bad = good; bad.contacts = reinterpret_cast<int*>(reinterpret_cast<char*>(out.data()) + 2);
        CHECK(call(&bad, 1) == MS_EINVAL, "contacts off 4 bytes");
        for (int P : {0, -1, 1025}) { bad = good; bad.n_slots = P; CHECK(call(&bad, 1) == MS_EINVAL, "%d slots", P); }
    }
    std::printf("%lld agent steps: %lld blocked, %lld of them by a body, %lld contacts; %d failures\n", stepped, blocked, by_body, touched, failures);
    return failures ? 1 : 0;
}
