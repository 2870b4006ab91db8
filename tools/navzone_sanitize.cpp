// A stand-alone program for a sanitizer run of the zones' HOST code (csrc/kernels/navzone.h: the root test, the rank of a label in
// the list of roots, a cell's zone, mark and key, a zone's stores - through ms_host_nav_zones): no GPU, no Python.  Build the
// library's translation unit and this file with the host sanitizers and run the result, as tools/navcost_sanitize.cpp's header
// describes:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/navzone_sanitize.cpp -o /tmp/navzone_sanitize
//     /tmp/navzone_sanitize
//
// Hand-made ragged grids - one cell, one row, one column, 63, 64, 65, 255, 256 and 257 cells, a block, an env without cells between
// envs that have some - every store allocated to the byte, so that a read or write past a store's end is a report.  Per grid:
// ranked and direct labels salted with -1, INT_MIN, INT_MAX, labels beyond the env and labels of cells that are no root; values
// salted with +inf, NaN, negatives, -0 and subnormals; marks of any byte; every combination of one store or F = 3 stores a layer;
// K of 1, 5 and 256; where and within_marks on and off; a mask.  After each call the numbers are checked against a plain loop over
// the cells written here, apart from the library's text.  Exit status 0 and no report from the sanitizers: clean.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }

static unsigned bits_of(float v) { unsigned u; memcpy(&u, &v, sizeof u); return u; }

int main() {
    unsigned seed = 29;
    const float cell = .1f;
    const int shapes[][2] = {{1, 1}, {1, 40}, {40, 1}, {0, 3}, {63, 1}, {64, 1}, {65, 1}, {255, 1}, {256, 1}, {257, 1}, {3, 0}, {23, 17}};
    const int N = 12, F = 3;
    std::vector<int> geom((size_t)4*N + 4);
    int* const g = reinterpret_cast<int*>(((uintptr_t)geom.data() + 15) & ~(uintptr_t)15);       // (16-byte aligned)
    std::vector<long long> starts(N + 1, 0);
    int max_framed = 0;
    for (int n = 0; n < N; n++) {
        g[4*n] = -5 + n; g[4*n + 1] = 4 - 2*n; g[4*n + 2] = shapes[n][0]; g[4*n + 3] = shapes[n][1];
        const int cells = shapes[n][0]*shapes[n][1];
        starts[n + 1] = starts[n] + cells;
        if (cells > 0 && (shapes[n][0] + 2)*(shapes[n][1] + 2) > max_framed) max_framed = (shapes[n][0] + 2)*(shapes[n][1] + 2);
    }
    const long long total = starts[N];
    std::vector<unsigned char> free_cells((size_t)total, 1);
    MsNavGrid grid;
    memset(&grid, 0, sizeof grid);
    grid.n_envs = N; grid.cell = cell; grid.clearance = .09f; grid.geom = g; grid.starts = starts.data(); grid.max_framed = max_framed;
    grid.free_cells = free_cells.data();

    const float odd_values[] = {0.f, .125f, .125f, .5f, 2.f, INFINITY, NAN, -1.f, -0.f, -INFINITY, 1e-45f, -1e-45f, 3e38f};
    int failures = 0, calls = 0;
    long long counted = 0;
    for (int combo = 0; combo < 8; combo++)
        for (int ranked = 0; ranked < 2; ranked++)
            for (int ki = 0; ki < 3; ki++) {
                const int L = combo & 1 ? F : 1, V = combo & 2 ? F : 1, M = combo & 4 ? F : 1, K = ki == 0 ? 1 : ki == 1 ? 5 : 256;
                const int variant = (int)(next_random(seed) % 6);       // values and marks given or not, where, within_marks
                const bool with_values = variant != 0, with_marks = variant != 1;
                const int where = variant & 1, within = variant >= 3;
                std::vector<int> labels((size_t)L*total);
                std::vector<float> values((size_t)V*total);
                std::vector<unsigned char> marks((size_t)M*total), mask((size_t)N*F);
                for (int n = 0; n < N; n++) {
                    const int cells = (int)(starts[n + 1] - starts[n]);
                    for (int s = 0; s < L; s++) {
                        int* const lab = labels.data() + L*starts[n] + (long long)s*cells;
                        const int n_roots = 1 + (int)(next_random(seed) % 9);
                        for (int k = 0; k < cells; k++) {
                            const unsigned r = next_random(seed) % 16;
                            if (ranked) {
                                const int root = (int)((next_random(seed) % (unsigned)n_roots)*(unsigned)cells/(unsigned)n_roots);
                                lab[k] = r == 0 ? -1 : r == 1 ? INT_MIN : r == 2 ? INT_MAX : r == 3 ? cells + (int)(next_random(seed) % 5) : root;
                            } else
                                lab[k] = r == 0 ? -1 : r == 1 ? INT_MIN : r == 2 ? INT_MAX : r == 3 ? K : (int)(next_random(seed) % (unsigned)(K + 2));
                        }
                        if (ranked && cells > 0)                         // (the roots name themselves)
                            for (int t = 0; t < n_roots; t++) {
                                const int root = (int)((unsigned)t*(unsigned)cells/(unsigned)n_roots);
                                lab[root] = root;
                            }
                    }
                    for (long long k = V*starts[n]; k < V*starts[n + 1]; k++) values[k] = odd_values[next_random(seed) % 13];
                    for (long long k = M*starts[n]; k < M*starts[n + 1]; k++) marks[k] = (unsigned char)(next_random(seed) % 3 ? next_random(seed) % 256 : 0);
                }
                const bool masked = variant == 5;
                for (size_t k = 0; k < mask.size(); k++) mask[k] = (unsigned char)(masked ? next_random(seed) % 2 : 1);
                const size_t out = (size_t)N*F*K;
                std::vector<int> cells_out(out, -7), marked(out, -7), nearest(out, -7), roots(out, -7), n_zones((size_t)N*F, -7);
                std::vector<float> least(out, -7.f), points(2*out, -7.f);
                MsNavZones z;
                memset(&z, 0, sizeof z);
                z.n_fields = F; z.labels = labels.data(); z.n_labels = L;
                z.values = with_values ? values.data() : nullptr; z.n_values = V;
                z.marks = with_marks ? marks.data() : nullptr; z.n_marks = M; z.where = where; z.within_marks = within;
                z.ranked = ranked; z.max_zones = K; z.mask = masked ? mask.data() : nullptr;
                z.cells = cells_out.data(); z.marked = marked.data(); z.least = least.data(); z.nearest = nearest.data();
                z.points = points.data(); z.roots = roots.data(); z.n_zones = n_zones.data();
                calls++;
                if (ms_host_nav_zones(&grid, &z) != MS_OK) { printf("combo %d ranked %d K %d: refused\n", combo, ranked, K); failures++; continue; }
                // a plain loop over the cells
                for (int n = 0; n < N; n++)
                    for (int f = 0; f < F; f++) {
                        const size_t field = (size_t)n*F + f;
                        if (!mask[field]) {
                            bool kept = n_zones[field] == -7;
                            for (int k = 0; k < K; k++) kept = kept && cells_out[field*K + k] == -7 && least[field*K + k] == -7.f && points[2*(field*K + k)] == -7.f;
                            if (!kept) { printf("combo %d ranked %d K %d env %d field %d: a masked field was written\n", combo, ranked, K, n, f); failures++; }
                            continue;
                        }
                        const int cells = (int)(starts[n + 1] - starts[n]);
                        const int* const lab = labels.data() + L*starts[n] + (long long)(L == 1 ? 0 : f)*cells;
                        const float* const val = values.data() + V*starts[n] + (long long)(V == 1 ? 0 : f)*cells;
                        const unsigned char* const mk = marks.data() + M*starts[n] + (long long)(M == 1 ? 0 : f)*cells;
                        std::vector<int> list, count(K, 0), mcount(K, 0), best(K, -1);
                        int all_roots = 0;
                        if (ranked)
                            for (int k = 0; k < cells; k++)
                                if (lab[k] == k) { if ((int)list.size() < K) list.push_back(k); all_roots++; }
                        for (int k = 0; k < cells; k++) {
                            int zone = -1;
                            if (ranked) { for (size_t t = 0; t < list.size(); t++) if (list[t] == lab[k]) zone = (int)t; }
                            else if (lab[k] >= 0 && lab[k] < K) zone = lab[k];
                            if (zone < 0) continue;
                            const bool m = !with_marks || ((mk[k] != 0) == (where != 0));
                            count[zone]++; mcount[zone] += m;
                            if (with_values && (m || !within) && bits_of(val[k]) < 0x7f800000u &&
                                (best[zone] < 0 || bits_of(val[k]) < bits_of(val[best[zone]]))) best[zone] = k;
                        }
                        int used = 0;
                        for (int k = 0; k < K; k++) {
                            const size_t at = field*K + k;
                            used += count[k] > 0;
                            counted += count[k];
                            const int root = ranked ? (k < (int)list.size() ? list[k] : -1) : (count[k] > 0 ? k : -1);
                            bool ok = cells_out[at] == count[k] && marked[at] == mcount[k] && nearest[at] == best[k] && roots[at] == root;
                            if (best[k] >= 0) {
                                const int i = best[k]/shapes[n][0], j = best[k] - i*shapes[n][0];
                                ok = ok && bits_of(least[at]) == bits_of(val[best[k]]) && points[2*at] == ((float)(g[4*n] + j) + .5f)*cell &&
                                     points[2*at + 1] == ((float)(g[4*n + 1] + i) + .5f)*cell;
                            } else
                                ok = ok && least[at] == INFINITY && std::isnan(points[2*at]) && std::isnan(points[2*at + 1]);
                            if (!ok) { printf("combo %d ranked %d K %d env %d field %d zone %d: differs\n", combo, ranked, K, n, f, k); failures++; }
                        }
                        if (n_zones[field] != (ranked ? all_roots : used)) { printf("combo %d ranked %d K %d env %d field %d: n_zones\n", combo, ranked, K, n, f); failures++; }
                    }
            }
    // refusals
    {
        int labels[4] = {0, 0, 2, 2}, out[8];
        float fout[8];
        const int geom2[8] = {0, 0, 2, 2, 0, 0, 0, 0};
        int* const g2 = reinterpret_cast<int*>(((uintptr_t)geom.data() + 15) & ~(uintptr_t)15);
        memcpy(g2, geom2, sizeof(int)*4);
        long long starts2[2] = {0, 4};
        grid.n_envs = 1; grid.geom = g2; grid.starts = starts2; grid.max_framed = 16;
        MsNavZones z;
        memset(&z, 0, sizeof z);
        z.n_fields = 1; z.labels = labels; z.n_labels = 1; z.ranked = 1; z.max_zones = 2;
        z.cells = out; z.marked = out + 2; z.nearest = out + 4; z.roots = out + 6; z.least = fout; z.points = fout + 2;
        int n_zones = -7;
        z.n_zones = &n_zones;
        if (ms_host_nav_zones(&grid, &z) != MS_OK || n_zones != 2 || out[0] != 2 || out[1] != 2 || out[6] != 0 || out[7] != 2) { printf("the small call\n"); failures++; }
        MsNavZones bad = z;
        bad.max_zones = 257;
        if (ms_host_nav_zones(&grid, &bad) != MS_EINVAL) { printf("K = 257\n"); failures++; }
        bad = z; bad.max_zones = 0;
        if (ms_host_nav_zones(&grid, &bad) != MS_EINVAL) { printf("K = 0\n"); failures++; }
        bad = z; bad.n_labels = 2;
        if (ms_host_nav_zones(&grid, &bad) != MS_EINVAL) { printf("L = 2, F = 1\n"); failures++; }
        bad = z; bad.labels = nullptr;
        if (ms_host_nav_zones(&grid, &bad) != MS_EINVAL) { printf("NULL labels\n"); failures++; }
        bad = z; bad.points = nullptr;
        if (ms_host_nav_zones(&grid, &bad) != MS_EINVAL) { printf("NULL points\n"); failures++; }
        bad = z; bad.ranked = 2;
        if (ms_host_nav_zones(&grid, &bad) != MS_EINVAL) { printf("ranked = 2\n"); failures++; }
        if (ms_host_nav_zones(&grid, nullptr) != MS_EINVAL || ms_host_nav_zones(nullptr, &z) != MS_EINVAL) { printf("NULL structs\n"); failures++; }
    }
    printf("%d calls, %lld cells counted into zones, %d failures\n", calls, counted, failures);
    return failures ? 1 : 0;
}
