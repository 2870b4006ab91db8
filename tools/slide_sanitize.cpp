// A stand-alone program for a sanitizer run of the sliding step's HOST code (csrc/kernels/slide.h and rollout.h over math.h, step.h
// and physics.h, through ms_host_slide and ms_host_rollouts with slide on): no GPU, no Python.  Build the library's translation unit and
// this file with the host sanitizers and run the result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/slide_sanitize.cpp -o /tmp/slide_sanitize
//     /tmp/slide_sanitize
//
// Hand-made worlds - a room with a pillar, a corridor narrower than two steps, an env without a wall, one wall of no length, the
// same wall twice and walls with a NaN or an infinity among their coordinates - every array allocated to the byte (std::vector: a
// read or write past an end is a report); one, two, five and 64 agents an env, one to three envs, at random poses, pressed against
// a wall, far outside, at NaN and at infinity, crawling and faster than any list; bounce 0, 0.05 and 1; with and without the
// movement prologue, respawns before and after, lifespans and the IMU reading; rollouts of K 1, 7, 65 and H 1, 5 with and without
// the others.  Checked on the way: progress and slid in [0, 1], slid only where blocked, a stopped agent at rest, stopped and slid
// written everywhere, the rollouts' counts within their bounds, and the refusals.  Exit status 0 and no report from the
// sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

static int failures = 0;
static long long stepped = 0, blocked = 0, slid_count = 0, stopped_count = 0, rolled = 0, rolled_slides = 0;

#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void box(std::vector<float>& w, float x0, float y0, float x1, float y1) {
    const float rows[16] = {x0, y0, x1, y0, x1, y0, x1, y1, x1, y1, x0, y1, x0, y1, x0, y0};
    w.insert(w.end(), rows, rows + 16);
}

static const float TABLE[8*3] = {0, 0, 0, 0, 3, 0, 0, -3, 0, 3, 0, 0, -3, 0, 0, 0, 0, 90, 0, 0, -90, 0, 20, 0};
static const MsConfig CFG = {.106f, 8, 90.f, 10.f};

struct Agents {
    std::vector<float> angles, positions, angvelocity, velocity;
    Agents(int n, unsigned& seed) : angles((size_t)n), positions((size_t)2*n), angvelocity((size_t)n), velocity((size_t)2*n) {
        for (int a = 0; a < n; a++) {
            const unsigned kind = next_random(seed) % 12;
            positions[2*a] = uniform(seed, .2f, 3.8f); positions[2*a + 1] = uniform(seed, .2f, 3.8f);
            velocity[2*a] = uniform(seed, -3.f, 3.f); velocity[2*a + 1] = uniform(seed, -3.f, 3.f);
            angles[a] = uniform(seed, -180.f, 180.f); angvelocity[a] = uniform(seed, -90.f, 90.f);
            if (kind == 0) { positions[2*a] = .106f; velocity[2*a] = -2.f; }
            if (kind == 1) { positions[2*a] = -30.f; positions[2*a + 1] = 1e4f; }
            if (kind == 2) { positions[2*a] = NAN; }
            if (kind == 3) { positions[2*a + 1] = INFINITY; }
            if (kind == 4) { velocity[2*a] *= 1e-7f; velocity[2*a + 1] *= 1e-7f; }
            if (kind == 5) { velocity[2*a] *= 30.f; }
            if (kind == 6) { velocity[2*a] = NAN; angles[a] = 1e30f; }
            if (kind == 7 && a > 0) { positions[2*a] = positions[2*a - 2] + .22f; positions[2*a + 1] = positions[2*a - 1]; }
        }
    }
    MsAgents view() { return MsAgents{angles.data(), positions.data(), angvelocity.data(), velocity.data(), nullptr, nullptr}; }
};

static void step(const std::vector<std::vector<float>>& envs, int A, float bounce, bool moved, int extras, unsigned& seed) {
    const int N = (int)envs.size();
    std::vector<float> walls;
    std::vector<long long> starts(1, 0);
    for (const auto& w : envs) { walls.insert(walls.end(), w.begin(), w.end()); starts.push_back((long long)walls.size()/4); }
    walls.resize(walls.size() + 4, 0.f);                                 // (a row behind the last: the pointer of an env without walls)
    const size_t n = (size_t)N*A;
    Agents ag((int)n, seed);
    std::vector<long long> actions(n), choice(n);
    for (auto& x : actions) x = next_random(seed) % 23 == 0 ? (next_random(seed) % 2 ? 1 : -1)*(1LL << 40) : (long long)(next_random(seed) % 9) - 1;
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
                       ex.n_spawns = S; ex.respawn_after = extras == 2; }
    if (extras >= 2) { ex.lifespans = life.data(); ex.max_lifespans = max_life.data(); ex.fresh_max = fresh.data(); }
    if (extras >= 1) ex.imu = imu.data();
    std::vector<float> progress(n, -9.f), slid(n, -9.f);
    std::vector<unsigned char> stopped(n, 9);
    MsSlide sl = {bounce, slid.data(), stopped.data()};
    MsAgents view = ag.view();
    const int status = ms_host_slide(walls.data(), starts.data(), N, A, &view, moved ? &mv : nullptr, extras ? &ex : nullptr, &sl, progress.data(), &CFG);
    CHECK(status == MS_OK, "status %d", status);
    for (size_t i = 0; i < n; i++) {
        stepped++;
        CHECK(progress[i] >= 0.f && progress[i] <= 1.f, "progress %g", progress[i]);
        CHECK(slid[i] >= 0.f && slid[i] <= 1.f, "slid %g", slid[i]);
        CHECK(stopped[i] <= 1, "stopped %d", (int)stopped[i]);
        CHECK(!(slid[i] > 0.f) || progress[i] < 1.f, "slid %g at progress %g", slid[i], progress[i]);
        CHECK(!stopped[i] || progress[i] < 1.f, "stopped at progress %g", progress[i]);
        const bool respawned_after = extras == 2 && mask[i];
        if (stopped[i] && !respawned_after) CHECK(ag.velocity[2*i] == 0.f && ag.velocity[2*i + 1] == 0.f && ag.angvelocity[i] == 0.f, "a stopped agent moves");
        blocked += progress[i] < 1.f; slid_count += slid[i] > 0.f; stopped_count += stopped[i];
    }
}

static void roll(const std::vector<float>& walls, int A, int K, int H, int others, float bounce, unsigned& seed) {
    Agents ag(A, seed);
    std::vector<long long> actions((size_t)A*K*H);
    for (auto& x : actions) x = (long long)(next_random(seed) % 9) - 1;
    const size_t C = (size_t)A*K;
    std::vector<float> p(2*C, -9.f), ang(C, -9.f), v(2*C, -9.f), w(C, -9.f), progress(C, -9.f), trail(2*C*H, -9.f);
    std::vector<int> stops(C, -9), first(C, -9), slides(C, -9);
    MsAgents view = ag.view();
    MsRollouts r = {K, H, actions.data(), 0, TABLE, 8, .875f, others, nullptr, p.data(), ang.data(), v.data(), w.data(), progress.data(),
                    stops.data(), first.data(), trail.data(), 1, bounce, slides.data()};
    const int status = ms_host_rollouts(walls.empty() ? nullptr : walls.data(), (int)walls.size()/4, &view, A, &r, &CFG);
    CHECK(status == MS_OK, "status %d", status);
    for (size_t c = 0; c < C; c++) {
        rolled++;
        CHECK(progress[c] >= 0.f && progress[c] <= 1.f, "progress %g", progress[c]);
        CHECK(stops[c] >= 0 && slides[c] >= 0 && stops[c] + slides[c] <= H, "stops %d slides %d of %d", stops[c], slides[c], H);
        CHECK((first[c] == H) == (stops[c] == 0) && first[c] >= 0 && first[c] <= H, "first_stop %d with %d stops", first[c], stops[c]);
        rolled_slides += slides[c];
    }
}

int main() {
    unsigned seed = 12345u;
    std::vector<float> room, corridor, none, odd;
    box(room, 0, 0, 4, 4); box(room, 1.5f, 1.5f, 2, 2);
    const float diagonal[4] = {3, 0, 4, 1};
    room.insert(room.end(), diagonal, diagonal + 4);
    box(corridor, 0, 0, 6, .5f);
    box(odd, 0, 0, 4, 4);
    const float rows[20] = {2, 2, 2, 2, 0, 0, 4, 0, NAN, 1, 2, NAN, 1, INFINITY, 3, 3, 0, 0, 4, 0};
    odd.insert(odd.end(), rows, rows + 20);
    const float bounces[3] = {0.f, .05f, 1.f};
    for (int round = 0; round < 40; round++) {
        for (int A : {1, 2, 5, 64}) {
            for (int extras = 0; extras < 3; extras++) {
                step({room}, A, bounces[round % 3], round % 2 == 0, extras, seed);
                step({corridor, none, odd}, A, bounces[(round + 1) % 3], round % 2 == 1, extras, seed);
            }
        }
    }
    for (int round = 0; round < 6; round++) {
        for (int K : {1, 7, 65}) {
            for (int H : {1, 5}) {
                roll(room, 1 + round % 3, K, H, round % 2, bounces[round % 3], seed);
                roll(round % 2 ? odd : corridor, 2, K, H, 1, .05f, seed);
                roll(none, 2, K, H, 1, .05f, seed);
            }
        }
    }
    // the refusals
    {
        Agents ag(65, seed);
        MsAgents view = ag.view();
        std::vector<float> progress(65);
        const long long starts[2] = {0, (long long)room.size()/4};
        MsSlide sl = {.05f, nullptr, nullptr};
        CHECK(ms_host_slide(room.data(), starts, 1, 65, &view, nullptr, nullptr, &sl, progress.data(), &CFG) == MS_EUNSUPPORTED, "65 agents");
        CHECK(ms_host_slide(room.data(), starts, 1, 64, &view, nullptr, nullptr, &sl, progress.data(), &CFG) == MS_OK, "64 agents");
        for (float b : {-.01f, 1.01f, NAN}) {
            MsSlide bad = {b, nullptr, nullptr};
            CHECK(ms_host_slide(room.data(), starts, 1, 1, &view, nullptr, nullptr, &bad, progress.data(), &CFG) == MS_EINVAL, "bounce %g", b);
        }
        CHECK(ms_host_slide(room.data(), starts, 1, 1, &view, nullptr, nullptr, nullptr, progress.data(), &CFG) == MS_EINVAL, "no MsSlide");
        CHECK(ms_host_slide(nullptr, starts, 1, 1, &view, nullptr, nullptr, &sl, progress.data(), &CFG) == MS_EINVAL, "no walls");
        CHECK(ms_host_slide(room.data(), starts, 0, 1, &view, nullptr, nullptr, &sl, progress.data(), &CFG) == MS_EINVAL, "no envs");
    }
    std::printf("%lld agent steps: %lld blocked, %lld slid, %lld stopped dead; %lld candidates rolled, %lld whole slides; %d failures\n",
                stepped, blocked, slid_count, stopped_count, rolled, rolled_slides, failures);
    return failures ? 1 : 0;
}
