// A stand-alone program for a sanitizer run of the percepts' HOST code (csrc/kernels/percept.h over navview.h, through
// ms_host_percepts): no GPU, no Python.  Build the library's translation unit and this file with the host sanitizers and run the
// result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/percept_sanitize.cpp -o /tmp/percept_sanitize
//     /tmp/percept_sanitize
//
// It looks at hand-made worlds - a box with a partition and a door and a row of NaN, random oblique walls, an env without walls -
// from 1, 4, 5 and 64 eyes (NaN and infinite ones among them) at 1, 63, 64, 65, 200 and 1024 points (NaN ones, and points on an eye,
// among them), with and without a cone (zero and NaN headings among them), valid, pairs in both shapes and a mask, for K of 0, 1 and
// 16, at three ranges, every output in buffers of exactly its size, with the kernel's wall capacity and with room for two rows (the
// walk over all walls), and checks the two wall paths against each other and against a plain loop over every pair and wall.  Exit
// status 0 and no report from the sanitizers: clean.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

// the rule, plainly: every pair against every wall
static bool blocks(float px, float py, float x, float y, const float* w) {
    const float ax = w[0], ay = w[1], bx = w[2], by = w[3];
    if (!(fminf(ax, bx) <= fmaxf(px, x) && fmaxf(ax, bx) >= fminf(px, x) && fminf(ay, by) <= fmaxf(py, y) && fmaxf(ay, by) >= fminf(py, y))) return false;
    const float rx = x - px, ry = y - py, vx = bx - ax, vy = by - ay;
    const float o1 = vx*(py - ay) - vy*(px - ax), o2 = vx*(y - ay) - vy*(x - ax);
    if (!((o1 < 0 && o2 > 0) || (o1 > 0 && o2 < 0))) return false;
    const float o3 = rx*(ay - py) - ry*(ax - px), o4 = rx*(by - py) - ry*(bx - px);
    return (o3 <= 0 && o4 >= 0) || (o3 >= 0 && o4 <= 0);
}

struct Out {
    std::vector<unsigned char> visible;
    std::vector<float> squares, offsets, near_offsets, near_distances;
    std::vector<int> counts, nearest;
    Out(int N, int E, int P, int K)
        : visible((size_t)N*E*P, 9), squares((size_t)N*E*P, -7.f), offsets((size_t)N*E*P*2, -7.f), near_offsets((size_t)N*E*K*2, -7.f),
          near_distances((size_t)N*E*K, -7.f), counts((size_t)N*E, -7), nearest((size_t)N*E*K, -7) {}
    static bool bits(const std::vector<float>& a, const std::vector<float>& b) {       // (as bits: a NaN equals a NaN)
        return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), 4*a.size()));
    }
    bool same(const Out& o) const {
        return visible == o.visible && counts == o.counts && nearest == o.nearest && bits(squares, o.squares) && bits(offsets, o.offsets) &&
               bits(near_offsets, o.near_offsets) && bits(near_distances, o.near_distances);
    }
};

int main() {
    const int N = 3;
    unsigned seed = 11u;
    std::vector<float> walls;
    long long wall_starts[N + 1] = {0};
    const float box[7][4] = {{0, 0, 8, 0}, {8, 0, 8, 4}, {8, 4, 0, 4}, {NAN, 1, 3, NAN}, {0, 4, 0, 0}, {4, 0, 4, 1.5f}, {4, 2.5f, 4, 4}};
    for (auto& w : box) walls.insert(walls.end(), w, w + 4);
    wall_starts[1] = 7;
    for (int k = 0; k < 40; k++) for (int t = 0; t < 4; t++) walls.push_back(uniform(seed, 0.f, 8.f));
    wall_starts[2] = wall_starts[3] = 47;
    walls.resize(walls.size() + 4, 0.f);
    const int eyes_of[4] = {1, 4, 5, 64}, points_of[6] = {1, 63, 64, 65, 200, 1024}, nearest_of[3] = {0, 1, 16};
    const float ranges[3] = {.5f, 3.f, 1e6f};
    int failures = 0, calls = 0;
    long long pairs_checked = 0;
    for (int ei = 0; ei < 4; ei++)
        for (int pi = 0; pi < 6; pi++) {
            const int E = eyes_of[ei], P = points_of[pi];
            // (vectors of exactly the size the call may touch: a read or a write past an end is the sanitizer's to find)
            std::vector<float> eyes((size_t)N*E*2), headings((size_t)N*E*2), points((size_t)N*P*2);
            std::vector<unsigned char> valid((size_t)N*P), shared((size_t)E*P), each((size_t)N*E*P), mask((size_t)N*E);
            for (auto& v : eyes) v = uniform(seed, -.5f, 8.5f);
            for (auto& v : headings) v = uniform(seed, -2.f, 2.f);
            for (auto& v : points) v = uniform(seed, -.5f, 8.5f);
            for (auto& v : valid) v = (unsigned char)(next_random(seed) % 8 ? 1 + next_random(seed) % 3 : 0);
            for (auto& v : shared) v = (unsigned char)(next_random(seed) % 8 ? 1 : 0);
            for (auto& v : each) v = (unsigned char)(next_random(seed) % 8 ? 255 : 0);
            for (auto& v : mask) v = (unsigned char)(next_random(seed) % 4 ? 1 : 0);
            mask[0] = 1;
            if (E > 1) { eyes[2] = NAN; headings[0] = headings[1] = 0.f; }
            if (E > 4) { eyes[2*4 + 1] = INFINITY; headings[2*3] = NAN; }
            points[0] = eyes[0]; points[1] = eyes[1];                                   // (a point on an eye)
            if (P > 1) points[2] = NAN;
            if (P > 64) { points[2*64 + 1] = NAN; points[2*65] = eyes[0]; points[2*65 + 1] = eyes[1]; }
            for (int ki = 0; ki < 3; ki++)
                for (int r = 0; r < 3; r++)
                    for (int variant = 0; variant < 4; variant++) {
                        const int K = nearest_of[ki];
                        const bool cone = variant & 1, gated = variant & 2;
                        const int shape = gated ? 1 + (variant == 3 ? 1 : (r & 1)) : 0;
                        const unsigned char* const pairs = shape == 0 ? nullptr : shape == 1 ? shared.data() : each.data();
                        Out out[2] = {Out(N, E, P, K), Out(N, E, P, K)};
                        for (int path = 0; path < 2; path++) {
                            Out& o = out[path];
                            MsPercepts q = {E, P, K, eyes.data(), cone ? headings.data() : nullptr, points.data(), gated ? valid.data() : nullptr, pairs,
                                            shape, gated ? mask.data() : nullptr, ranges[r], -.25f, o.visible.data(), o.squares.data(), o.offsets.data(),
                                            o.counts.data(), K ? o.nearest.data() : nullptr, K ? o.near_offsets.data() : nullptr,
                                            K ? o.near_distances.data() : nullptr};
                            if (ms_host_percepts(&q, N, walls.data(), wall_starts, path ? 2 : 0) != 0) { printf("ms_host_percepts refused\n"); return 2; }
                            calls++;
                        }
                        if (!out[0].same(out[1])) failures++;
                        // the plain loop
                        const float R2 = ranges[r]*ranges[r];
                        for (int n = 0; n < N; n++)
                            for (int e = 0; e < E; e++) {
                                const size_t at = (size_t)n*E + e;
                                if (gated && !mask[at]) { failures += out[0].counts[at] != -7 || (K && out[0].nearest[at*K] != -7) || out[0].visible[at*P] != 9; continue; }
                                const float px = eyes[2*at], py = eyes[2*at + 1], hx = headings[2*at], hy = headings[2*at + 1];
                                const float hlen = sqrtf(hx*hx + hy*hy);
                                const bool live = std::isfinite(px) && std::isfinite(py) && (!cone || (std::isfinite(hlen) && hlen > 0));
                                std::vector<std::pair<unsigned long long, int>> order;
                                int count = 0;
                                for (int p = 0; p < P; p++) {
                                    const float x = points[2*((size_t)n*P + p)], y = points[2*((size_t)n*P + p) + 1];
                                    const float rx = x - px, ry = y - py, rr = rx*rx + ry*ry;
                                    bool visible = live && rr <= R2;
                                    if (gated) visible = visible && valid[(size_t)n*P + p] && (shape == 1 ? shared[(size_t)e*P + p] : each[at*P + p]);
                                    if (visible && cone) visible = hx*rx + hy*ry >= (-.25f*sqrtf(rr))*hlen;
                                    for (long long l = wall_starts[n]; l < wall_starts[n + 1] && visible; l++) visible = !blocks(px, py, x, y, &walls[4*l]);
                                    pairs_checked++;
                                    if (out[0].visible[at*P + p] != (visible ? 1 : 0)) failures++;
                                    if (visible) {
                                        unsigned bits; memcpy(&bits, &rr, 4);
                                        order.push_back({((unsigned long long)bits << 32) | (unsigned)p, p});
                                        if (out[0].squares[at*P + p] != rr || out[0].offsets[2*(at*P + p)] != rx || out[0].offsets[2*(at*P + p) + 1] != ry) failures++;
                                    } else if (out[0].squares[at*P + p] != INFINITY || !std::isnan(out[0].offsets[2*(at*P + p)])) failures++;
                                    count += visible;
                                }
                                if (out[0].counts[at] != count) failures++;
                                std::sort(order.begin(), order.end());
                                for (int k = 0; k < K; k++) {
                                    const int want = k < (int)order.size() ? order[(size_t)k].second : -1;
                                    if (out[0].nearest[at*K + k] != want) failures++;
                                    if (want < 0 ? out[0].near_distances[at*K + k] != INFINITY || !std::isnan(out[0].near_offsets[2*(at*K + k)])
                                                 : out[0].near_distances[at*K + k] != sqrtf(out[0].squares[at*P + want]) ||
                                                   out[0].near_offsets[2*(at*K + k)] != out[0].offsets[2*(at*P + want)]) failures++;
                                }
                            }
                    }
        }
    printf("%d calls, %lld pairs: %s\n", calls, pairs_checked,
           failures ? "MISMATCH" : "clean: staged walls, the walk over all walls and the plain loop agree");
    return failures ? 1 : 0;
}
