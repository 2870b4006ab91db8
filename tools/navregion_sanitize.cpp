// A stand-alone program for a sanitizer run of the regions' HOST code (csrc/kernels/navregion.h through ms_host_nav_regions,
// ms_host_nav_region_query and ms_host_nav_region_masks): no GPU, no Python.  Build the library's translation unit and this file
// with the host sanitizers and run the result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/navregion_sanitize.cpp -o /tmp/navregion_sanitize
//     /tmp/navregion_sanitize
//
// It labels a ragged grid - a serpentine corridor, a random mask, a checkerboard, a single row, an env without cells - framed (the
// launch that fits) and as stored (max_framed = 0: the smallest launch), with and without marks, checks the two against each other
// and against a flood fill, asks the labels at points on and off the grid, and writes masks.  Exit status 0 and no report from the
// sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }

static void flood(const std::vector<unsigned char>& open, int nx, int ny, std::vector<int>& labels) {
    labels.assign((size_t)nx*ny, -1);
    std::vector<int> stack;
    for (int start = 0; start < nx*ny; start++) {
        if (!open[start] || labels[start] >= 0) continue;
        labels[start] = start;
        stack.push_back(start);
        while (!stack.empty()) {
            const int k = stack.back(); stack.pop_back();
            const int i = k / nx, j = k % nx;
            const int other[4] = {j > 0 ? k - 1 : -1, j < nx - 1 ? k + 1 : -1, i > 0 ? k - nx : -1, i < ny - 1 ? k + nx : -1};
            for (int t = 0; t < 4; t++)
                if (other[t] >= 0 && open[other[t]] && labels[other[t]] < 0) { labels[other[t]] = start; stack.push_back(other[t]); }
        }
    }
}

int main() {
    const int N = 5, G = 2;
    alignas(16) int geom[N*4] = {-16, -16, 33, 33,  -50, 7, 131, 97,  0, -7, 11, 9,  -2000, 0, 4097, 1,  3, 4, 0, 7};
    long long starts[N + 1] = {0};
    for (int n = 0; n < N; n++) starts[n + 1] = starts[n] + (geom[4*n + 2] > 0 && geom[4*n + 3] > 0 ? (long long)geom[4*n + 2]*geom[4*n + 3] : 0);
    const long long cells = starts[N];
    std::vector<unsigned char> free_cells((size_t)cells + 1, 0), marks((size_t)G*cells + 1, 0), among((size_t)cells + 1, 0);
    unsigned seed = 7u;
    for (int n = 0; n < N; n++) {
        const int nx = geom[4*n + 2], ny = geom[4*n + 3];
        for (long long k = 0; k < starts[n + 1] - starts[n]; k++) {
            const int i = (int)(k / nx), j = (int)(k % nx);
            bool open = true;
            if (n == 0) open = i % 2 == 0 || (i % 4 == 1 ? j == nx - 1 : j == 0);
            if (n == 1) open = next_random(seed) % 100 < 62;
            if (n == 2) open = (i + j) % 2 == 0;
            free_cells[starts[n] + k] = open ? (next_random(seed) % 2 ? 1 : 3) : (next_random(seed) % 2 ? 0 : 2);
            among[starts[n] + k] = next_random(seed) % 100 < 85;
            for (int g = 0; g < G; g++) marks[G*starts[n] + (long long)g*nx*ny + k] = g == 0 ? 1 : (unsigned char)(next_random(seed) % 4);
        }
        (void)ny;
    }
    int failures = 0;
    for (int with_marks = 0; with_marks < 2; with_marks++) {
        const int fields = with_marks ? G : 1;
        std::vector<int> labels[2];
        for (int stored = 0; stored < 2; stored++) {
            int framed = 0;
            for (int n = 0; n < N; n++)
                if (geom[4*n + 2] > 0 && geom[4*n + 3] > 0 && (geom[4*n + 2] + 2)*(geom[4*n + 3] + 2) > framed) framed = (geom[4*n + 2] + 2)*(geom[4*n + 3] + 2);
            MsNavGrid grid = {N, .125f, .106f, geom, starts, stored ? 0 : framed, free_cells.data()};
            labels[stored].assign((size_t)fields*cells + 1, -7);
            std::vector<float> areas((size_t)fields*cells + 1, -7.f);
            std::vector<int> counts(N*fields, -7), open_cells(N*fields, -7), largest(N*fields, -7), largest_cells(N*fields, -7), passes(N*fields, -7);
            MsNavRegions r = {fields, with_marks ? marks.data() : nullptr, 1, with_marks ? among.data() : nullptr, nullptr, labels[stored].data(), areas.data(),
                              counts.data(), open_cells.data(), largest.data(), largest_cells.data(), passes.data()};
            if (ms_host_nav_regions(&grid, &r) != 0) { printf("ms_host_nav_regions refused\n"); return 2; }
            for (int n = 0; n < N; n++)
                for (int g = 0; g < fields; g++) {
                    const int nx = geom[4*n + 2], ny = geom[4*n + 3];
                    const long long size = starts[n + 1] - starts[n], at = fields*starts[n] + g*size;
                    std::vector<unsigned char> open((size_t)size);
                    for (long long k = 0; k < size; k++)
                        open[k] = (free_cells[starts[n] + k] & 1) && (!with_marks || ((among[starts[n] + k] & 1) && (marks[at + k] & 1) == 1));
                    std::vector<int> want;
                    if (size) flood(open, nx, ny, want);
                    int regions = 0;
                    for (long long k = 0; k < size; k++) {
                        if (labels[stored][at + k] != want[k]) failures++;
                        regions += want[k] == k;
                    }
                    if (counts[n*fields + g] != regions) failures++;
                    printf("marks %d stored %d env %d field %d: %d regions, %d open, largest %d of %d cells, %d passes\n", with_marks, stored, n, g,
                           counts[n*fields + g], open_cells[n*fields + g], largest[n*fields + g], largest_cells[n*fields + g], passes[n*fields + g]);
                }
            // the labels at a few points - on the grid, off it, NaN, far - and the masks of the same points and of one label each
            const int P = 4;
            std::vector<float> points((size_t)N*P*2);
            for (int n = 0; n < N; n++) {
                const float x0 = (geom[4*n] + 1.f)*.125f, y0 = (geom[4*n + 1] + 1.f)*.125f;
                const float pts[P][2] = {{x0, y0}, {x0 - 10.f, y0}, {NAN, y0}, {4e9f, -4e9f}};
                memcpy(&points[(size_t)n*P*2], pts, sizeof pts);
            }
            std::vector<int> field((size_t)N*P), found((size_t)N*P*4, -7), wanted((size_t)N*P);
            for (int k = 0; k < N*P; k++) { field[k] = k % (fields + 2) - 1; wanted[k] = k % 3 - 1; }      // (-1 and G among them)
            MsNavRegionQuery q = {P, points.data(), field.data(), labels[stored].data(), fields, found.data()};
            if (ms_host_nav_region_query(&grid, &q) != 0) { printf("ms_host_nav_region_query refused\n"); return 2; }
            std::vector<unsigned char> out((size_t)P*cells + 1, 9);
            MsNavRegionMasks by_points = {P, points.data(), nullptr, field.data(), labels[stored].data(), fields, out.data()};
            MsNavRegionMasks by_labels = {P, nullptr, wanted.data(), field.data(), labels[stored].data(), fields, out.data()};
            if (ms_host_nav_region_masks(&grid, &by_points) != 0 || ms_host_nav_region_masks(&grid, &by_labels) != 0) { printf("masks refused\n"); return 2; }
            for (long long k = 0; k < (long long)P*cells; k++) if (out[k] > 1) failures++;
        }
        if (labels[0] != labels[1]) failures++;
    }
    printf("%s\n", failures ? "MISMATCH" : "clean: framed, stored and the flood fill agree");
    return failures ? 1 : 0;
}
