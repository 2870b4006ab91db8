// A stand-alone program for a sanitizer run of the scenarios' HOST code (csrc/kernels/scenario.h over rollout.h, math.h, step.h and
// physics.h, through ms_host_scenarios): no GPU, no Python.  Build the library's translation unit and this file with the host
// sanitizers and run the result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/scenario_sanitize.cpp -o /tmp/scenario_sanitize
//     /tmp/scenario_sanitize
//
// Hand-made worlds - a room with a pillar, a corridor narrower than two steps, an env without a wall, walls with a NaN or an
// infinity among their coordinates - every array allocated to the byte (std::vector: a read or write past an end is a report);
// 1, 2, 5 and 64 agents an env, in a huddle a step across so that they meet, some pressed against a wall, far outside, at NaN and
// at infinity, crawling and faster than any list; S (focal: K) of 1, 7, 65 and 256, H of 1, 5 and 64; the joint mode with its own
// and with shared actions, the focal mode with its own and with shared plans; actions far outside the table; masks; a trail.
// Checked on the way: progress in [0, 1], the counts' bounds, first_stop against stops, a stopped agent at rest, the trail's last
// point the end pose, rows the mask leaves out untouched, focal = joint on the expanded tensor as bytes, and the refusals.
// Exit status 0 and no report from the sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

static int failures = 0;
static long long rolled = 0, agents_rolled = 0, stopped = 0;

static void box(std::vector<float>& w, float x0, float y0, float x1, float y1) {
    const float rows[16] = {x0, y0, x1, y0, x1, y0, x1, y1, x1, y1, x0, y1, x0, y1, x0, y0};
    w.insert(w.end(), rows, rows + 16);
}

struct Out {
    std::vector<float> p, ang, v, w, progress, trail;
    std::vector<int> stops, first;
    Out(size_t rows, int H, bool trailed) : p(2*rows, -9.f), ang(rows, -9.f), v(2*rows, -9.f), w(rows, -9.f), progress(rows, -9.f),
                                             trail(trailed ? 2*rows*H : 0, -9.f), stops(rows, -9), first(rows, -9) {}
    void into(MsScenarios& q, bool trailed) {
        q.positions = p.data(); q.angles = ang.data(); q.velocity = v.data(); q.angvelocity = w.data(); q.progress = progress.data();
        q.stops = stops.data(); q.first_stop = first.data(); q.trail = trailed ? trail.data() : nullptr;
    }
};

static void check_row(const Out& o, size_t c, int H, bool trailed) {
    agents_rolled++;
    stopped += o.stops[c] > 0;
    if (!(o.progress[c] >= 0.f && o.progress[c] <= 1.f)) { printf("progress %g\n", o.progress[c]); failures++; }
    if (o.stops[c] < 0 || o.stops[c] > H || o.first[c] < 0 || o.first[c] > H || (o.stops[c] == 0) != (o.first[c] == H) ||
        (o.stops[c] > 0) != (o.progress[c] < 1.f) || o.first[c] + o.stops[c] > H) { printf("stops %d, first %d, H %d\n", o.stops[c], o.first[c], H); failures++; }
    if (trailed && memcmp(&o.trail[2*(c*H + H - 1)], &o.p[2*c], 2*sizeof(float))) { printf("the trail does not end on the pose\n"); failures++; }
    if (o.ang[c] == o.ang[c] && std::isfinite(o.ang[c]) && !(o.ang[c] >= -180.f && o.ang[c] <= 180.f)) { printf("angle %g\n", o.ang[c]); failures++; }
}

static void roll(const std::vector<float>& walls, int A, int S, int H, bool focal, bool shared, bool masked, bool trailed, unsigned& seed) {
    const float table[8*3] = {0, 0, 0, 0, 3, 0, 0, -3, 0, 3, 0, 0, -3, 0, 0, 0, 0, 90, 0, 0, -90, 0, 20, 0};
    const int n_walls = (int)(walls.size()/4);
    const float* wp = walls.empty() ? nullptr : walls.data();
    std::vector<float> angles((size_t)A), positions((size_t)2*A), angvelocity((size_t)A), velocity((size_t)2*A);
    const float cx = uniform(seed, .6f, 3.4f), cy = uniform(seed, .6f, 3.4f);
    for (int a = 0; a < A; a++) {
        const unsigned kind = next_random(seed) % 12;
        positions[2*a] = cx + uniform(seed, -.5f, .5f); positions[2*a + 1] = cy + uniform(seed, -.5f, .5f);   // a huddle: they meet
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
    auto draw = [&](std::vector<long long>& xs) {
        for (auto& x : xs) x = next_random(seed) % 23 == 0 ? (next_random(seed) % 2 ? 1 : -1)*(1LL << 40) : (long long)(next_random(seed) % 9) - 1;
    };
    // focal: plans (A, K, H) or (K, H), base (A, H); joint: actions (S, A, H) - the host statement's one env reads `shared` alike
    std::vector<long long> actions(focal ? (size_t)(shared ? 1 : A)*S*H : (size_t)S*A*H), base(focal ? (size_t)A*H : 0);
    draw(actions); draw(base);
    std::vector<unsigned char> mask((size_t)(focal ? A : 1));
    for (auto& m : mask) m = (unsigned char)(next_random(seed) % 3 ? 1 : 0);
    const size_t rows = focal ? (size_t)A*S : (size_t)S*A;
    Out o(rows, H, trailed);
    MsAgents ag = {angles.data(), positions.data(), angvelocity.data(), velocity.data(), nullptr, nullptr};
    MsScenarios q = {};
    q.n_scenarios = S; q.horizon = H; q.focal = focal ? 1 : 0; q.actions = actions.data(); q.shared = (focal && shared) ? 1 : 0;
    q.base = focal ? base.data() : nullptr; q.table = table; q.n_actions = 8; q.keep = (rolled % 2) ? .875f : 0.f;
    q.mask = masked ? mask.data() : nullptr;
    o.into(q, trailed);
    const MsConfig cfg = {.1f, 8, 90.f, 10.f};
    if (ms_host_scenarios(wp, n_walls, &ag, A, &q, &cfg) != MS_OK) { printf("refused a good call\n"); failures++; return; }
    for (size_t c = 0; c < rows; c++) {
        const bool out_of_mask = masked && !mask[focal ? c/S : 0];
        if (out_of_mask) {
            if (o.progress[c] != -9.f || o.stops[c] != -9 || o.p[2*c] != -9.f) { printf("a masked row was written\n"); failures++; }
            continue;
        }
        check_row(o, c, H, trailed);
    }
    rolled += (masked && !focal && !mask[0]) ? 0 : (focal ? (long long)A*S : S);
    // focal = joint on the expanded tensor, byte for byte (where the expansion is within the limits)
    if (focal && (long long)A*S <= 256) {
        const int SJ = A*S;
        std::vector<long long> joint((size_t)SJ*A*H);
        for (int f = 0; f < A; f++) for (int k = 0; k < S; k++) for (int b = 0; b < A; b++) for (int h = 0; h < H; h++)
            joint[(((size_t)f*S + k)*A + b)*H + h] = b == f ? actions[((shared ? (size_t)0 : (size_t)f*S) + k)*H + h] : base[(size_t)b*H + h];
        Out j((size_t)SJ*A, H, trailed);
        MsScenarios qj = q;
        qj.n_scenarios = SJ; qj.focal = 0; qj.shared = 0; qj.actions = joint.data(); qj.base = nullptr; qj.mask = nullptr;
        j.into(qj, trailed);
        if (ms_host_scenarios(wp, n_walls, &ag, A, &qj, &cfg) != MS_OK) { printf("refused the expanded call\n"); failures++; return; }
        for (int f = 0; f < A; f++) for (int k = 0; k < S; k++) {
            if (masked && !mask[f]) continue;
            const size_t c = (size_t)f*S + k, cj = ((size_t)f*S + k)*A + f;
            if (memcmp(&o.p[2*c], &j.p[2*cj], 8) || memcmp(&o.ang[c], &j.ang[cj], 4) || memcmp(&o.v[2*c], &j.v[2*cj], 8) || memcmp(&o.w[c], &j.w[cj], 4) ||
                memcmp(&o.progress[c], &j.progress[cj], 4) || o.stops[c] != j.stops[cj] || o.first[c] != j.first[cj] ||
                (trailed && memcmp(&o.trail[2*c*H], &j.trail[2*cj*H], 8*(size_t)H))) { printf("focal differs from joint at (%d, %d)\n", f, k); failures++; }
        }
    }
    // the refusals: limits and NULL pointers, nothing written
    auto refuses = [&](const MsScenarios& bad, int n_agents, int code, const char* what) {
        if (ms_host_scenarios(wp, n_walls, &ag, n_agents, &bad, &cfg) != code) { printf("%s\n", what); failures++; }
    };
    MsScenarios bad = q;
    bad.n_scenarios = 0; refuses(bad, A, MS_EINVAL, "S = 0");
    bad.n_scenarios = 257; refuses(bad, A, MS_EINVAL, "S = 257");
    bad = q; bad.horizon = 65; refuses(bad, A, MS_EINVAL, "H = 65");
    bad = q; bad.horizon = 0; refuses(bad, A, MS_EINVAL, "H = 0");
    bad = q; bad.n_actions = 0; refuses(bad, A, MS_EINVAL, "no actions");
    bad = q; bad.keep = NAN; refuses(bad, A, MS_EINVAL, "keep");
    bad = q; bad.focal = 2; refuses(bad, A, MS_EINVAL, "focal");
    bad = q; bad.focal = 1; bad.base = nullptr; refuses(bad, A, MS_EINVAL, "NULL base");
    bad = q; bad.stops = nullptr; refuses(bad, A, MS_EINVAL, "NULL stops");
    bad = q; bad.actions = nullptr; refuses(bad, A, MS_EINVAL, "NULL actions");
    refuses(q, 0, MS_EINVAL, "no agents");
    refuses(q, 65, MS_EUNSUPPORTED, "65 agents");
    if (ms_host_scenarios(nullptr, 3, &ag, A, &q, &cfg) != MS_EINVAL || ms_scenarios(nullptr, &ag, &q, &cfg, nullptr) != MS_EINVAL) { printf("refusals\n"); failures++; }
}

int main() {
    unsigned seed = 31;
    std::vector<std::vector<float>> worlds(4);
    box(worlds[0], 0, 0, 4, 4); box(worlds[0], 1.5f, 1.5f, 2, 2);                       // a room with a pillar
    box(worlds[1], 0, 0, 6, .5f);                                                        // a corridor narrower than two steps
    /* worlds[2]: no wall at all */
    box(worlds[3], 0, 0, 4, 4);
    { const float odd[12] = {2, 2, 2, 2, NAN, 1, 3, 1, 1, 3, INFINITY, 3}; worlds[3].insert(worlds[3].end(), odd, odd + 12); }
    const int Ss[4] = {1, 7, 65, 256}, Hs[3] = {1, 5, 64}, As[4] = {1, 2, 5, 64};
    int calls = 0;
    for (const auto& walls : worlds)
        for (int a = 0; a < 4; a++)
            for (int s = 0; s < 4; s++)
                for (int h = 0; h < 3; h++) {
                    // (the work of a call goes as A^2 S H, in focal mode A^3 K H: the largest shapes once, in the first world)
                    const long long joint_work = (long long)As[a]*As[a]*Ss[s]*Hs[h];
                    for (int focal = 0; focal < 2; focal++) {
                        const long long work = focal ? joint_work*As[a] : joint_work;
                        if (work > 400000 && &walls != &worlds[0]) continue;
                        if (work > 30000000) continue;
                        calls++;
                        roll(walls, As[a], Ss[s], Hs[h], focal != 0, calls % 3 == 0, calls % 5 == 0, calls % 4 != 0, seed);
                    }
                }
    printf("%d calls, %lld scenarios rolled, %lld agents' rows checked, %lld of them stopped at least once\n", calls, rolled, agents_rolled, stopped);
    if (stopped == 0 || stopped == agents_rolled) { printf("every agent alike\n"); failures++; }
    printf(failures ? "FAILED\n" : "clean\n");
    return failures ? 1 : 0;
}
