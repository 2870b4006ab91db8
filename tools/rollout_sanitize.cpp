// A stand-alone program for a sanitizer run of the rollouts' HOST code (csrc/kernels/rollout.h over math.h, step.h and physics.h, through
// ms_host_rollouts and ms_host_move_velocity): no GPU, no Python.  Build the library's translation unit and this file with the host
// sanitizers and run the result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/rollout_sanitize.cpp -o /tmp/rollout_sanitize
//     /tmp/rollout_sanitize
//
// Hand-made worlds - a room with a pillar, a corridor narrower than two steps, an env without a wall, one wall of no length and
// walls with a NaN or an infinity among their coordinates - every array allocated to the byte (std::vector: a read or write past
// an end is a report); one, two and five agents, at random poses, pressed against a wall, far outside, at NaN and at infinity,
// crawling and faster than any list; K of 1, 7, 64, 65 and 256, H of 1, 5 and 64; per-agent and shared plans, actions far outside
// the table; with and without the other agents, a mask, a trail.  Checked on the way: progress in [0, 1], the counts' bounds,
// first_stop against stops, a stopped candidate at rest, the trail's last point the end pose, masked rows untouched, and the
// refusals.  Exit status 0 and no report from the sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

static int failures = 0;
static long long rolled = 0, stopped = 0;

static void box(std::vector<float>& w, float x0, float y0, float x1, float y1) {
    const float rows[16] = {x0, y0, x1, y0, x1, y0, x1, y1, x1, y1, x0, y1, x0, y1, x0, y0};
    w.insert(w.end(), rows, rows + 16);
}

static void roll(const std::vector<float>& walls, int A, int K, int H, bool shared, int others, bool masked, bool trailed, unsigned& seed) {
    const float table[8*3] = {0, 0, 0, 0, 3, 0, 0, -3, 0, 3, 0, 0, -3, 0, 0, 0, 0, 90, 0, 0, -90, 0, 20, 0};
    std::vector<float> angles((size_t)A), positions((size_t)2*A), angvelocity((size_t)A), velocity((size_t)2*A);
    for (int a = 0; a < A; a++) {
        const unsigned kind = next_random(seed) % 10;
        positions[2*a] = uniform(seed, .2f, 3.8f); positions[2*a + 1] = uniform(seed, .2f, 3.8f);
        velocity[2*a] = uniform(seed, -3.f, 3.f); velocity[2*a + 1] = uniform(seed, -3.f, 3.f);
        angles[a] = uniform(seed, -180.f, 180.f); angvelocity[a] = uniform(seed, -90.f, 90.f);
        if (kind == 0) { positions[2*a] = .101f; }
        if (kind == 1) { positions[2*a] = -30.f; positions[2*a + 1] = 1e4f; }
        if (kind == 2) { positions[2*a] = NAN; }
        if (kind == 3) { positions[2*a + 1] = INFINITY; }
        if (kind == 4) { velocity[2*a] *= 1e-7f; velocity[2*a + 1] *= 1e-7f; }
        if (kind == 5) { velocity[2*a] *= 30.f; }
        if (kind == 6) { velocity[2*a] = NAN; angles[a] = 1e30f; }
    }
    std::vector<long long> actions((size_t)(shared ? 1 : A)*K*H);
    for (auto& x : actions) x = next_random(seed) % 23 == 0 ? (next_random(seed) % 2 ? 1 : -1)*(1LL << 40) : (long long)(next_random(seed) % 9) - 1;
    std::vector<unsigned char> mask((size_t)A);
    for (auto& m : mask) m = (unsigned char)(next_random(seed) % 3 ? 1 : 0);
    const size_t C = (size_t)A*K;
    std::vector<float> p(2*C, -9.f), ang(C, -9.f), v(2*C, -9.f), w(C, -9.f), progress(C, -9.f), trail(trailed ? 2*C*H : 0, -9.f);
    std::vector<int> stops(C, -9), first(C, -9);
    MsAgents ag = {angles.data(), positions.data(), angvelocity.data(), velocity.data(), nullptr, nullptr};
    MsRollouts r = {K, H, actions.data(), shared ? 1 : 0, table, 8, (rolled % 2) ? .875f : 0.f, others, masked ? mask.data() : nullptr,
                    p.data(), ang.data(), v.data(), w.data(), progress.data(), stops.data(), first.data(), trailed ? trail.data() : nullptr};
    const MsConfig cfg = {.1f, 8, 90.f, 10.f};
    if (ms_host_rollouts(walls.empty() ? nullptr : walls.data(), (int)(walls.size()/4), &ag, A, &r, &cfg) != MS_OK) { printf("refused a good call\n"); failures++; return; }
    for (int a = 0; a < A; a++) {
        for (int k = 0; k < K; k++) {
            const size_t c = (size_t)a*K + k;
            if (masked && !mask[a]) {
                if (progress[c] != -9.f || stops[c] != -9 || p[2*c] != -9.f) { printf("a masked row was written\n"); failures++; }
                continue;
            }
            rolled++;
            stopped += stops[c] > 0;
            if (!(progress[c] >= 0.f && progress[c] <= 1.f)) { printf("progress %g\n", progress[c]); failures++; }
            if (stops[c] < 0 || stops[c] > H || first[c] < 0 || first[c] > H || (stops[c] == 0) != (first[c] == H) ||
                (stops[c] > 0) != (progress[c] < 1.f) || first[c] + stops[c] > H) { printf("stops %d, first %d, H %d\n", stops[c], first[c], H); failures++; }
            if (trailed && memcmp(&trail[2*(c*H + H - 1)], &p[2*c], 2*sizeof(float))) { printf("the trail does not end on the pose\n"); failures++; }
            if (ang[c] == ang[c] && std::isfinite(ang[c]) && !(ang[c] >= -180.f && ang[c] <= 180.f)) { printf("angle %g\n", ang[c]); failures++; }
        }
    }
    // the refusals: limits and NULL pointers, nothing written
    MsRollouts bad = r;
    bad.n_candidates = 0;   if (ms_host_rollouts(walls.data(), (int)(walls.size()/4), &ag, A, &bad, &cfg) != MS_EINVAL) { printf("K = 0\n"); failures++; }
    bad.n_candidates = 257; if (ms_host_rollouts(walls.data(), (int)(walls.size()/4), &ag, A, &bad, &cfg) != MS_EINVAL) { printf("K = 257\n"); failures++; }
    bad = r; bad.horizon = 65; if (ms_host_rollouts(walls.data(), (int)(walls.size()/4), &ag, A, &bad, &cfg) != MS_EINVAL) { printf("H = 65\n"); failures++; }
    bad = r; bad.n_actions = 0; if (ms_host_rollouts(walls.data(), (int)(walls.size()/4), &ag, A, &bad, &cfg) != MS_EINVAL) { printf("no actions\n"); failures++; }
    bad = r; bad.others = 2;   if (ms_host_rollouts(walls.data(), (int)(walls.size()/4), &ag, A, &bad, &cfg) != MS_EINVAL) { printf("others\n"); failures++; }
    bad = r; bad.stops = nullptr; if (ms_host_rollouts(walls.data(), (int)(walls.size()/4), &ag, A, &bad, &cfg) != MS_EINVAL) { printf("NULL stops\n"); failures++; }
    if (ms_host_rollouts(walls.data(), (int)(walls.size()/4), &ag, 0, &r, &cfg) != MS_EINVAL || ms_host_rollouts(nullptr, 3, &ag, A, &r, &cfg) != MS_EINVAL ||
        ms_rollouts(nullptr, &ag, &r, &cfg, nullptr) != MS_EINVAL) { printf("refusals\n"); failures++; }
}

int main() {
    unsigned seed = 29;
    std::vector<std::vector<float>> worlds(5);
    box(worlds[0], 0, 0, 4, 4); box(worlds[0], 1.5f, 1.5f, 2, 2);                       // a room with a pillar
    box(worlds[1], 0, 0, 6, .5f);                                                        // a corridor narrower than two steps
    /* worlds[2]: no wall at all */
    box(worlds[3], 0, 0, 4, 4);
    { const float odd[12] = {2, 2, 2, 2, NAN, 1, 3, 1, 1, 3, INFINITY, 3}; worlds[3].insert(worlds[3].end(), odd, odd + 12); }
    for (int k = 0; k < 300; k++) { const float x = uniform(seed, 0, 4), y = uniform(seed, 0, 4); const float row[4] = {x, y, x + uniform(seed, -.3f, .3f), y + uniform(seed, -.3f, .3f)}; worlds[4].insert(worlds[4].end(), row, row + 4); }
    const int Ks[5] = {1, 7, 64, 65, 256}, Hs[3] = {1, 5, 64}, As[3] = {1, 2, 5};
    int calls = 0;
    for (const auto& walls : worlds)
        for (int a = 0; a < 3; a++)
            for (int k = 0; k < 5; k++)
                for (int h = 0; h < 3; h++) {
                    if (Ks[k]*Hs[h] > 4096 && (a || &walls != &worlds[0])) continue;    // (the largest shape once)
                    calls++;
                    roll(walls, As[a], Ks[k], Hs[h], calls % 3 == 0, calls % 2, calls % 5 == 0, calls % 4 != 0, seed);
                }
    float vel[2] = {1.f, -2.f}, spin = 3.f;
    const float delta[3] = {0.f, 3.f, 90.f};
    ms_host_move_velocity(.875f, 45.f, delta, vel, &spin);
    if (!(spin == .875f*3.f + 90.f) || !(vel[0] == vel[0])) { printf("move_velocity\n"); failures++; }
    if (ms_debug_rollout_scheme(2) != MS_EINVAL || ms_debug_rollout_scheme(1) != MS_OK || ms_debug_rollout_scheme(-1) != MS_OK) { printf("scheme\n"); failures++; }
    printf("%d calls, %lld candidates rolled, %lld of them stopped at least once\n", calls, rolled, stopped);
    if (stopped == 0 || stopped == rolled) { printf("every candidate alike\n"); failures++; }
    printf(failures ? "FAILED\n" : "clean\n");
    return failures ? 1 : 0;
}
