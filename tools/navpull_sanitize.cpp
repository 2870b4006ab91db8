// A stand-alone program for a sanitizer run of the pulled paths' HOST code (csrc/kernels/navpull.h over navpath.h, through
// ms_host_nav_pull): no GPU, no Python.  Build the library's translation unit and this file with the host sanitizers and run the
// result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/navpull_sanitize.cpp -o /tmp/navpull_sanitize
//     /tmp/navpull_sanitize
//
// Hand-made grids - open floor, random blocked cells, a single row, a single column, a single cell, an all-blocked grid, a corridor
// of 300 cells - every store allocated to the byte, so that a read or write past a store's end is a report; seeded fields settled
// by ms_host_nav_seed_field and cost fields by ms_host_nav_cost_field, a field of a goal made by hand on the corridor, and a garbage
// field (random numbers, NaNs, zeros) over each; starts at every cell's centre, outside the grid and at NaN and infinite points;
// reach 1, 64 and 1024; max_points 2 (every longer path is cut) and 8; with and without indices.  Checked on the way: the count's
// bounds, reach 1 against ms_host_nav_seed_path / ms_host_nav_cost_path, a pulled length no longer than the chain's, NaN and -1 in
// every slot not written.  Exit status 0 and no report from the sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

static int failures = 0, pulls = 0, broken = 0, none = 0;

// One query at every reach and max_points; `chain`: the count of the whole chain (ms_host_nav_*_path's), 0 when unknown.
static void pull(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* goal, const float* costs,
                 const float* p, int cells, int chain, bool settled) {
    const int reaches[3] = {1, 64, 1024}, sizes[2] = {2, 8};
    float whole = 0.f;
    for (int r = 0; r < 3; r++) {
        for (int m = 0; m < 2; m++) {
            const int M = sizes[m];
            std::vector<float> vertices((size_t)2*M, -9.f);
            std::vector<int> indices((size_t)M, -9);
            float length = -9.f;
            const int count = ms_host_nav_pull(geom, cell, free_cells, D, goal, costs, p, reaches[r], M, vertices.data(),
                                               (r + m) % 2 ? indices.data() : nullptr, &length);
            pulls++;
            if (count < 0) broken++;
            if (count == 0) none++;
            const int got = abs(count), written = got < M ? got : M;
            if (got > cells + 2 || got == 1) { printf("a pulled path of %d vertices in %d cells\n", count, cells); failures++; }
            if (count < 0 && settled) { printf("a chain broke on a settled field\n"); failures++; }
            if ((count == 0) != (length == INFINITY) || length < 0.f || length != length) { printf("count %d, length %g\n", count, length); failures++; }
            if (count != 0 && (vertices[0] != p[0] || vertices[1] != p[1])) { printf("the first vertex is not the start\n"); failures++; }
            for (int k = 0; k < M; k++) {
                const bool nan = vertices[2*k] != vertices[2*k] && vertices[2*k + 1] != vertices[2*k + 1];
                if ((k >= written) != nan) { printf("slot %d of %d written: %g %g\n", k, written, vertices[2*k], vertices[2*k + 1]); failures++; }
                if ((r + m) % 2 && ((k >= written) != (indices[k] == -1) || (k < written && k && indices[k] <= indices[k - 1]) ||
                                    (k && k < written && indices[k] - indices[k - 1] > reaches[r]))) { printf("index %d: %d\n", k, indices[k]); failures++; }
            }
            if (reaches[r] == 1) {
                whole = length;
                if (chain && count != chain) { printf("reach 1 gave %d points, the path %d\n", count, chain); failures++; }
            } else if (count != 0 && !(length <= whole*(1.f + 1e-5f))) { printf("pulled %g, chain %g\n", length, whole); failures++; }
        }
    }
    if (ms_host_nav_pull(geom, cell, free_cells, D, goal, costs, p, 0, 8, &whole, nullptr, &whole) != -2 ||
        ms_host_nav_pull(geom, cell, free_cells, D, goal, costs, p, 1025, 8, &whole, nullptr, &whole) != -2 ||
        ms_host_nav_pull(geom, cell, free_cells, D, goal, costs, p, 64, 1, &whole, nullptr, &whole) != 0) { printf("refusals\n"); failures++; }
}

int main() {
    unsigned seed = 13;
    const float cell = .1f;
    const int shapes[][2] = {{23, 17}, {31, 29}, {40, 1}, {1, 40}, {1, 1}, {6, 5}, {304, 5}};
    for (int s = 0; s < 7; s++) {
        const int nx = shapes[s][0], ny = shapes[s][1], cells = nx*ny;
        const int geom[4] = {-4 + s, 3 - s, nx, ny};
        std::vector<unsigned char> free_cells((size_t)cells), marks((size_t)cells);
        for (int k = 0; k < cells; k++) {
            const int i = k / nx, j = k % nx;
            free_cells[k] = s == 5 ? 0 : s == 6 ? (i >= 1 && i <= 3 && j >= 1 && j <= 302) : (s == 0 || next_random(seed) % 5 ? 1 : 0);
            marks[k] = (unsigned char)((s != 6 && next_random(seed) % 60 == 0 ? 1 : 0) | 2);
        }
        const int seed_cell = s == 6 ? 2*nx + 301 : cells/2;
        marks[seed_cell] |= 1; free_cells[seed_cell] = s == 5 ? 0 : 1;
        std::vector<float> costs((size_t)cells), seeded((size_t)cells, -3.f), priced((size_t)cells, -3.f), garbage((size_t)cells);
        for (int k = 0; k < cells; k++) {
            const unsigned pick = next_random(seed) % 12;
            const float odd[4] = {INFINITY, NAN, -3.f, 1e-40f};
            costs[k] = pick < 4 ? odd[pick] : expf(uniform(seed, -1.f, 4.f));
            garbage[k] = next_random(seed) % 7 ? uniform(seed, -2.f, 9.f) : (next_random(seed) % 2 ? NAN : 0.f);
        }
        ms_host_nav_seed_field(geom, cell, free_cells.data(), marks.data(), 1, nullptr, 1, seeded.data(), nullptr);
        ms_host_nav_cost_field(geom, cell, free_cells.data(), marks.data(), 1, nullptr, costs.data(), 1, priced.data(), nullptr);
        // on the corridor the seeded field is a goal's too, up to its legs: the goal at the seed's centre makes D[seed] = leg = 0
        const float goal[2] = {((float)(geom[0] + seed_cell % nx) + .5f)*cell, ((float)(geom[1] + seed_cell / nx) + .5f)*cell};
        const int stride = s == 6 ? 97 : 1;
        for (int k = -3; k < cells + 3; k += (k >= 0 && k < cells ? stride : 1)) {
            float p[2] = {((float)(geom[0] + (k < 0 ? -2 : k % nx)) + .5f)*cell + uniform(seed, -.04f, .04f),
                          ((float)(geom[1] + (k >= cells ? ny + 2 : k < 0 ? 0 : k / nx)) + .5f)*cell + uniform(seed, -.04f, .04f)};
            if (k == 7) p[0] = NAN;
            if (k == 8) p[1] = INFINITY;
            if (k == 9) { p[0] = -3e38f; p[1] = 3e38f; }
            std::vector<float> path(2*2);
            pull(geom, cell, free_cells.data(), seeded.data(), nullptr, nullptr, p, cells,
                 ms_host_nav_seed_path(geom, cell, free_cells.data(), seeded.data(), p, 2, path.data()), true);
            pull(geom, cell, free_cells.data(), priced.data(), nullptr, costs.data(), p, cells,
                 ms_host_nav_cost_path(geom, cell, free_cells.data(), priced.data(), costs.data(), p, 2, path.data()), true);
            pull(geom, cell, free_cells.data(), garbage.data(), nullptr, k % 2 ? costs.data() : nullptr, p, cells, 0, false);
            pull(geom, cell, free_cells.data(), garbage.data(), goal, nullptr, p, cells, 0, false);
            if (s == 6) pull(geom, cell, free_cells.data(), seeded.data(), goal, nullptr, p, cells,
                             ms_host_nav_path(geom, cell, free_cells.data(), seeded.data(), goal, p, 2, path.data()), true);
        }
    }
    if (ms_debug_nav_pull_scheme(2) != MS_EINVAL || ms_debug_nav_pull_scheme(1) != MS_OK || ms_debug_nav_pull_scheme(-1) != MS_OK) { printf("scheme\n"); failures++; }
    printf("%d pulls, %d of them of broken chains (garbage fields only), %d without a path\n", pulls, broken, none);
    printf(failures ? "FAILED\n" : "clean\n");
    return failures ? 1 : 0;
}
