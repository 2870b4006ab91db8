// A stand-alone program for a sanitizer run of the cost fields' HOST code (csrc/kernels/navfield.h and navpath.h through
// ms_host_nav_cost_field, ms_host_nav_cost_waypoint and ms_host_nav_cost_path): no GPU, no Python.  Build the library's translation
// unit and this file with the host sanitizers and run the result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/navcost_sanitize.cpp -o /tmp/navcost_sanitize
//     /tmp/navcost_sanitize
//
// Hand-made grids - open floor, random blocked cells, a single row, a single column, a single cell, an all-blocked grid - every
// store allocated to the byte, so that a read or write past a store's end is a report; cost layers that are a gradient, noise, all
// ones, and salted with +inf, NaN, negative and subnormal values.  The framed sweep (the multipliers beside the framed copy) and
// the stored one are checked against each other bit for bit, a layer of ones against ms_host_nav_seed_field, the salted layer
// against its clamped twin; then the followers from every cell's centre and from points outside the grid, on the settled field and
// on a garbage one, every look-ahead from 1 to 64 on a few.  Exit status 0 and no report from the sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

int main() {
    unsigned seed = 11;
    const float cell = .1f;
    const int shapes[][2] = {{23, 17}, {31, 29}, {40, 1}, {1, 40}, {1, 1}, {6, 5}};
    int failures = 0, chains = 0, broken = 0;
    for (int s = 0; s < 6; s++) {
        const int nx = shapes[s][0], ny = shapes[s][1], cells = nx*ny;
        const int geom[4] = {-4 + s, 3 - s, nx, ny};
        std::vector<unsigned char> free_cells((size_t)cells), marks((size_t)cells), among((size_t)cells);
        for (int k = 0; k < cells; k++) {
            free_cells[k] = s == 5 ? 0 : (s == 0 || next_random(seed) % 5 ? 1 : 0);
            marks[k] = (unsigned char)((next_random(seed) % 40 == 0 ? 1 : 0) | 2);
            among[k] = (unsigned char)(next_random(seed) % 4 ? 1 : 0);
        }
        marks[cells/2] |= 1; free_cells[cells/2] = s == 5 ? 0 : 1;
        std::vector<float> gradient((size_t)cells), noise((size_t)cells), ones((size_t)cells, 1.f), salted((size_t)cells), clamped((size_t)cells);
        for (int k = 0; k < cells; k++) {
            gradient[k] = 1.f + .3f*(float)(k / nx) + .2f*(float)(k % nx);
            noise[k] = expf(uniform(seed, -1.f, 6.f));
            const unsigned pick = next_random(seed) % 10;
            const float odd[7] = {INFINITY, NAN, 1e30f, -3.f, 0.f, 1e-40f, -INFINITY};
            salted[k] = pick < 7 ? odd[pick] : noise[k];
            clamped[k] = pick < 3 ? 256.f : pick < 7 ? 1.f : noise[k] > 256.f ? 256.f : noise[k] < 1.f ? 1.f : noise[k];
        }
        const std::vector<float>* layers[4] = {&gradient, &noise, &salted, &clamped};
        std::vector<std::vector<float>> D(4, std::vector<float>((size_t)cells, -3.f));
        for (int l = 0; l < 4; l++) {
            for (int with_among = 0; with_among < 2; with_among++) {
                std::vector<float> framed((size_t)cells, -5.f);
                int n0 = -1, n1 = -1;
                const int a = ms_host_nav_cost_field(geom, cell, free_cells.data(), marks.data(), 1, with_among ? among.data() : nullptr, layers[l]->data(), 0, D[l].data(), &n0);
                const int b = ms_host_nav_cost_field(geom, cell, free_cells.data(), marks.data(), 1, with_among ? among.data() : nullptr, layers[l]->data(), 1, framed.data(), &n1);
                if (a < 1 || b < 1 || n0 != n1 || memcmp(D[l].data(), framed.data(), (size_t)cells*4)) { printf("shape %d layer %d: framed and stored differ\n", s, l); failures++; }
            }
            // (D[l] is now the field among the `among` cells)
        }
        if (memcmp(D[2].data(), D[3].data(), (size_t)cells*4)) { printf("shape %d: the salted layer differs from its clamped twin\n", s); failures++; }
        std::vector<float> seeded((size_t)cells, -3.f), unit((size_t)cells, -3.f);
        ms_host_nav_seed_field(geom, cell, free_cells.data(), marks.data(), 1, among.data(), 1, seeded.data(), nullptr);
        ms_host_nav_cost_field(geom, cell, free_cells.data(), marks.data(), 1, among.data(), ones.data(), 1, unit.data(), nullptr);
        if (memcmp(seeded.data(), unit.data(), (size_t)cells*4)) { printf("shape %d: a cost of one differs from the seeded field\n", s); failures++; }
        // the followers
        std::vector<float> garbage((size_t)cells);
        for (int k = 0; k < cells; k++) garbage[k] = next_random(seed) % 7 ? uniform(seed, -2.f, 9.f) : (next_random(seed) % 2 ? NAN : 0.f);
        for (int l = 0; l < 3; l++) {
            for (int junk = 0; junk < 2; junk++) {
                const float* field = junk ? garbage.data() : D[l].data();
                for (int k = -3; k < cells + 3; k++) {
                    float p[2] = {((float)(geom[0] + (k < 0 ? -2 : k % nx)) + .5f)*cell + uniform(seed, -.04f, .04f),
                                  ((float)(geom[1] + (k >= cells ? ny + 2 : k < 0 ? 0 : k / nx)) + .5f)*cell + uniform(seed, -.04f, .04f)};
                    if (k == 7) p[0] = NAN;
                    float way[2];
                    std::vector<float> path(2*5);
                    for (int L = (k % 19 == 0 ? 1 : 16); L <= (k % 19 == 0 ? 64 : 16); L++) {
                        const int hops = ms_host_nav_cost_waypoint(geom, cell, free_cells.data(), field, layers[l]->data(), p, L, way);
                        if (hops >= L || (hops < 0) != (way[0] != way[0])) { printf("shape %d: waypoint %d of look-ahead %d\n", s, hops, L); failures++; }
                    }
                    const int count = ms_host_nav_cost_path(geom, cell, free_cells.data(), field, layers[l]->data(), p, 5, path.data());
                    chains++;
                    if (count < 0) broken++;
                    if (count < 0 && !junk) { printf("shape %d layer %d: a chain broke on a settled field\n", s, l); failures++; }
                    if (abs(count) > cells + 2) { printf("shape %d: a path of %d points in %d cells\n", s, count, cells); failures++; }
                }
            }
        }
    }
    int caps[3];
    if (ms_host_nav_cost_capacity(caps) != MS_OK || caps[0] <= 0 || ms_host_nav_cost_capacity(nullptr) != MS_EINVAL) { printf("capacity\n"); failures++; }
    printf("%d chains followed, %d of them broken (garbage fields only)\n", chains, broken);
    printf(failures ? "FAILED\n" : "clean\n");
    return failures ? 1 : 0;
}
