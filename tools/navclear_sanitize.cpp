// A stand-alone program for a sanitizer run of the clearance HOST code (csrc/kernels/navclear.h through ms_host_nav_clearance and
// ms_host_nav_clear_query): no GPU, no Python.  Build the library's translation unit and this file with the host sanitizers and run
// the result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/navclear_sanitize.cpp -o /tmp/navclear_sanitize
//     /tmp/navclear_sanitize
//
// A ragged hand-made world - random oblique walls with a NaN row and a zero-length one, 1100 walls round one tile (the list is
// folded and emptied on the way), a single row of cells, an env without walls, an env without cells - every store allocated to the
// byte, so that a write past a store's end is a report; brute force, the tile cull and both culls are checked against each other
// bit for bit, with a mask, with and without nearest and fits; then the query, serially and dealt to 64 bests, with agent rows,
// skips in and out of range, NaN points and a mask.  Exit status 0 and no report from the sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

int main() {
    unsigned seed = 7;
    const int N = 5;
    const float cell = .125f;
    // geom must be 16-byte aligned: an over-aligned array
    alignas(16) static int geom[N*4] = {0, 0, 40, 37,  -3, 2, 20, 18,  8, 8, 33, 1,  0, 0, 17, 16,  0, 0, 0, 0};
    std::vector<long long> starts(N + 1, 0);
    for (int n = 0; n < N; n++) starts[n + 1] = starts[n] + (long long)geom[4*n + 2]*geom[4*n + 3];
    const long long cells = starts[N];
    std::vector<float> walls;
    std::vector<long long> wall_starts(1, 0);
    auto wall = [&](float ax, float ay, float bx, float by) { walls.insert(walls.end(), {ax, ay, bx, by}); };
    for (int k = 0; k < 40; k++) { const float x = uniform(seed, 0, 5), y = uniform(seed, 0, 4.5f); wall(x, y, x + uniform(seed, -1, 1), y + uniform(seed, -1, 1)); }
    wall(NAN, 1, 2, 2); wall(1, 1, 1, 1); wall(INFINITY, 0, 1, 1);
    wall_starts.push_back((long long)walls.size()/4);
    for (int k = 0; k < 1100; k++) { const float x = uniform(seed, .2f, 1.8f), y = uniform(seed, .6f, 2.2f); wall(x, y, x + uniform(seed, -.05f, .05f), y + uniform(seed, -.05f, .05f)); }
    wall_starts.push_back((long long)walls.size()/4);
    for (int k = 0; k < 7; k++) { const float x = uniform(seed, 1, 5); wall(x, .5f, x + .3f, 1.5f); }
    wall_starts.push_back((long long)walls.size()/4);
    wall_starts.push_back((long long)walls.size()/4);                  // an env without walls
    wall(0, 0, 1, 1);
    wall_starts.push_back((long long)walls.size()/4);                  // an env without cells
    std::vector<unsigned char> free_cells((size_t)cells, 1);
    const int max_framed = 42*39;
    MsNavGrid grid{N, cell, .106f, geom, starts.data(), max_framed, free_cells.data()};
    const unsigned char mask[N] = {1, 1, 0, 1, 1};
    int failures = 0;
    for (int variant = 0; variant < 3; variant++) {
        const int K = variant == 0 ? 0 : variant == 1 ? 3 : 8;
        std::vector<std::vector<float>> values(3, std::vector<float>((size_t)cells, -3.f));
        std::vector<std::vector<int>> nearest(3, std::vector<int>((size_t)cells, -7));
        std::vector<std::vector<unsigned char>> fits(3, std::vector<unsigned char>((size_t)(K*cells), 9));
        for (int flags = 0; flags < 3; flags++) {
            MsNavClearance spec{};
            spec.max_range = variant == 2 ? .3f : 2.f;
            spec.n_radii = K;
            for (int k = 0; k < K; k++) spec.radii[k] = .05f + .03f*(float)k;
            spec.max_tiles = 9;
            spec.mask = variant == 1 ? mask : nullptr;
            spec.values = values[flags].data();
            spec.nearest = variant == 0 ? nullptr : nearest[flags].data();
            spec.fits = K ? fits[flags].data() : nullptr;
            if (ms_host_nav_clearance(&grid, &spec, walls.data(), wall_starts.data(), flags) != MS_OK) { printf("variant %d flags %d refused\n", variant, flags); failures++; }
        }
        for (int flags = 1; flags < 3; flags++)
            if (memcmp(values[0].data(), values[flags].data(), (size_t)cells*4) || memcmp(nearest[0].data(), nearest[flags].data(), (size_t)cells*4) ||
                (K && memcmp(fits[0].data(), fits[flags].data(), (size_t)(K*cells)))) { printf("variant %d: flags %d differ from brute force\n", variant, flags); failures++; }
        long long pairs = 0;
        const long long folds = ms_host_nav_clear_folds(&pairs);
        printf("variant %d: %lld of %lld (cell, row) pairs folded with both culls\n", variant, folds, pairs);
    }
    // the query: three agents of four rows each in front of each env's walls
    const int A = 3, M = 4, P = 6;
    std::vector<float> rows;
    std::vector<long long> row_starts(1, 0);
    for (int n = 0; n < N; n++) {
        for (int k = 0; k < A*M; k++) { const float x = uniform(seed, 0, 4), y = uniform(seed, 0, 4); rows.insert(rows.end(), {x, y, x + .2f, y + (k % 2 ? .2f : 0.f)}); }
        rows.insert(rows.end(), walls.begin() + 4*wall_starts[n], walls.begin() + 4*wall_starts[n + 1]);
        row_starts.push_back((long long)rows.size()/4);
    }
    std::vector<float> points(N*P*2);
    for (auto& v : points) v = uniform(seed, -1, 5);
    points[3] = NAN;
    std::vector<int> skip(N*P);
    for (int k = 0; k < N*P; k++) skip[k] = (int)(next_random(seed) % 7) - 2;     // -2 .. 4: in and out of 0 .. A - 1
    std::vector<unsigned char> pmask(N*P, 1);
    pmask[4] = pmask[11] = 0;
    for (int with_agents = 0; with_agents < 2; with_agents++) {
        std::vector<float> d[2], t[2];
        std::vector<int> l[2];
        for (int flags = 0; flags < 2; flags++) {
            d[flags].assign(N*P, -3.f); t[flags].assign(N*P*2, 5.f); l[flags].assign(N*P, -7);
            MsNavClearQuery q{N, P, points.data(), skip.data(), 1.5f, pmask.data(), d[flags].data(), l[flags].data(), t[flags].data()};
            if (ms_host_nav_clear_query(&q, rows.data(), row_starts.data(), A, M, with_agents, flags) != MS_OK) { printf("query refused\n"); failures++; }
        }
        if (memcmp(d[0].data(), d[1].data(), N*P*4) || memcmp(l[0].data(), l[1].data(), N*P*4) || memcmp(t[0].data(), t[1].data(), N*P*8)) {
            printf("query (agents %d): the dealt rows differ from the serial fold\n", with_agents); failures++;
        }
        if (d[0][4] != -3.f || l[0][11] != -7) { printf("a masked point was written\n"); failures++; }
    }
    printf(failures ? "FAILED\n" : "clean\n");
    return failures ? 1 : 0;
}
