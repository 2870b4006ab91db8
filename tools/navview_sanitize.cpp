// A stand-alone program for a sanitizer run of the view fields' HOST code (csrc/kernels/navview.h through ms_host_nav_views): no
// GPU, no Python.  Build the library's translation unit and this file with the host sanitizers and run the result:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/navview_sanitize.cpp -o /tmp/navview_sanitize
//     /tmp/navview_sanitize
//
// It looks out over a ragged hand-made world - a box with a partition and a door and a row of NaN, random oblique walls, a single
// row of cells, an env without walls, an env without cells - from viewpoints on the grid, on its edges, far off it, NaN and
// infinite, with and without a cone (zero and NaN headings among them), with and without maps, slots (out of range among them),
// a mask and a byte store, at four ranges, with the kernel's wall capacity and with room for two rows (the sweep over all walls),
// and checks the two wall paths against each other and against a plain loop over every cell and wall.  Exit status 0 and no
// report from the sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }
static float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo)*(float)(next_random(s) % 65536)/65536.f; }

// the rule, plainly: every cell against every wall
static bool blocks(float px, float py, float x, float y, const float* w) {
    const float ax = w[0], ay = w[1], bx = w[2], by = w[3];
    if (!(fminf(ax, bx) <= fmaxf(px, x) && fmaxf(ax, bx) >= fminf(px, x) && fminf(ay, by) <= fmaxf(py, y) && fmaxf(ay, by) >= fminf(py, y))) return false;
    const float rx = x - px, ry = y - py, vx = bx - ax, vy = by - ay;
    const float o1 = vx*(py - ay) - vy*(px - ax), o2 = vx*(y - ay) - vy*(x - ax);
    if (!((o1 < 0 && o2 > 0) || (o1 > 0 && o2 < 0))) return false;
    const float o3 = rx*(ay - py) - ry*(ax - px), o4 = rx*(by - py) - ry*(bx - px);
    return (o3 <= 0 && o4 >= 0) || (o3 >= 0 && o4 <= 0);
}

int main() {
    const int N = 5, P = 6, S = 3;
    const float c = .125f;
    alignas(16) int geom[N*4] = {-1, -1, 67, 35,  -3, -3, 47, 46,  -2000, 0, 4097, 1,  -10, 5, 40, 24,  3, 4, 0, 7};
    long long starts[N + 1] = {0};
    for (int n = 0; n < N; n++) starts[n + 1] = starts[n] + (geom[4*n + 2] > 0 && geom[4*n + 3] > 0 ? (long long)geom[4*n + 2]*geom[4*n + 3] : 0);
    const long long cells = starts[N];
    unsigned seed = 11u;
    std::vector<float> walls;
    long long wall_starts[N + 1] = {0};
    const float box[7][4] = {{0, 0, 8, 0}, {8, 0, 8, 4}, {8, 4, 0, 4}, {NAN, 1, 3, NAN}, {0, 4, 0, 0}, {4, 0, 4, 1.5f}, {4, 2.5f, 4, 4}};
    for (auto& w : box) walls.insert(walls.end(), w, w + 4);
    wall_starts[1] = 7;
    for (int k = 0; k < 40; k++) for (int t = 0; t < 4; t++) walls.push_back(uniform(seed, 0.f, 5.f));
    wall_starts[2] = 47;
    const float row[2][4] = {{-100, -1, -100, 2}, {100, -1, 100.5f, 2}};
    for (auto& w : row) walls.insert(walls.end(), w, w + 4);
    wall_starts[3] = wall_starts[4] = wall_starts[5] = 49;
    walls.resize(walls.size() + 4, 0.f);
    std::vector<unsigned char> free_cells((size_t)cells + 1, 0), unseen((size_t)S*cells + 1, 0), mask((size_t)N*P, 1);
    for (long long k = 0; k < cells; k++) free_cells[k] = (unsigned char)(next_random(seed) % 4);
    for (long long k = 0; k < S*cells; k++) unseen[k] = (unsigned char)(next_random(seed) % 4);
    alignas(8) float points[N*P*2], headings[N*P*2];
    int slot[N*P];
    for (int n = 0; n < N; n++) {
        const float x0 = geom[4*n]*c, y0 = geom[4*n + 1]*c, x1 = x0 + geom[4*n + 2]*c, y1 = y0 + geom[4*n + 3]*c;
        const float pts[P][2] = {{uniform(seed, x0, x1), uniform(seed, y0, y1)}, {x0, y0}, {x1 + .01f, y1 - .01f}, {NAN, y0}, {4e9f, -4e9f}, {INFINITY, y1}};
        memcpy(&points[n*P*2], pts, sizeof pts);
        for (int p = 0; p < P; p++) {
            headings[(n*P + p)*2] = p == 1 ? 0.f : p == 2 ? NAN : uniform(seed, -2.f, 2.f);
            headings[(n*P + p)*2 + 1] = p == 1 ? -0.f : uniform(seed, -2.f, 2.f);
            slot[n*P + p] = (n + p) % (S + 2) - 1;                            // (-1 and S among them)
        }
    }
    mask[3] = mask[N*P - 2] = 0;
    int framed = 0;
    for (int n = 0; n < N; n++)
        if (geom[4*n + 2] > 0 && geom[4*n + 3] > 0 && (geom[4*n + 2] + 2)*(geom[4*n + 3] + 2) > framed) framed = (geom[4*n + 2] + 2)*(geom[4*n + 3] + 2);
    MsNavGrid grid = {N, c, .106f, geom, starts, framed, free_cells.data()};
    int failures = 0, calls = 0;
    const float ranges[4] = {.05f, 1.3f, 6.f, 1e6f};
    for (int r = 0; r < 4; r++)
        for (int variant = 0; variant < 4; variant++) {
            const bool cone = variant & 1, maps = variant & 2, store = variant != 3;
            std::vector<unsigned char> values[2];
            std::vector<int> counts[2], gains[2];
            for (int path = 0; path < 2; path++) {
                values[path].assign((size_t)P*cells + 1, 9);
                counts[path].assign(N*P, -7);
                gains[path].assign(N*P, -7);
                MsNavViews v = {P, points, cone ? headings : nullptr, ranges[r], -.25f, free_cells.data(), maps ? unseen.data() : nullptr, maps ? S : 0,
                                maps ? slot : nullptr, mask.data(), store ? values[path].data() : nullptr, counts[path].data(),
                                maps ? gains[path].data() : nullptr};
                if (ms_host_nav_views(&grid, &v, walls.data(), wall_starts, path ? 2 : 0) != 0) { printf("ms_host_nav_views refused\n"); return 2; }
                calls++;
            }
            if (values[0] != values[1] || counts[0] != counts[1] || gains[0] != gains[1]) failures++;
            if (values[0][(size_t)P*cells] != 9) failures++;                     // (nothing beyond the stores)
            // the plain loop
            const float R2 = ranges[r]*ranges[r];
            for (int n = 0; n < N; n++)
                for (int p = 0; p < P; p++) {
                    const int vp = n*P + p, nx = geom[4*n + 2], ny = geom[4*n + 3];
                    const long long size = starts[n + 1] - starts[n];
                    if (!mask[vp]) { failures += counts[0][vp] != -7; continue; }
                    const float px = points[2*vp], py = points[2*vp + 1], hx = headings[2*vp], hy = headings[2*vp + 1];
                    const float hlen = sqrtf(hx*hx + hy*hy);
                    const bool live = std::isfinite(px) && std::isfinite(py) && (!cone || (std::isfinite(hlen) && hlen > 0));
                    const int s = maps ? slot[vp] : -1;
                    int count = 0, gain = 0;
                    for (long long k = 0; k < size; k++) {
                        const int i = (int)(k / nx), j = (int)(k % nx);
                        const float x = ((float)(geom[4*n] + j) + .5f)*c, y = ((float)(geom[4*n + 1] + i) + .5f)*c;
                        const float rx = x - px, ry = y - py, rr = rx*rx + ry*ry;
                        bool visible = live && rr <= R2;
                        if (visible && cone) visible = hx*rx + hy*ry >= (-.25f*sqrtf(rr))*hlen;
                        for (long long l = wall_starts[n]; l < wall_starts[n + 1] && visible; l++) visible = !blocks(px, py, x, y, &walls[4*l]);
                        if (store && values[0][(size_t)(P*starts[n] + p*size + k)] != (visible ? 1 : 0)) failures++;
                        const bool counted = visible && (free_cells[starts[n] + k] & 1);
                        count += counted;
                        gain += counted && s >= 0 && s < S && !(unseen[(size_t)(S*starts[n] + s*size + k)] & 1);
                    }
                    (void)ny;
                    if (counts[0][vp] != count || (maps && gains[0][vp] != gain)) failures++;
                }
            printf("range %g cone %d maps %d store %d: counts", ranges[r], cone, maps, store);
            for (int k = 0; k < N*P; k += P) printf(" %d", counts[0][k]);
            printf("\n");
        }
    printf("%d calls: %s\n", calls, failures ? "MISMATCH" : "clean: staged walls, the sweep over all walls and the plain loop agree");
    return failures ? 1 : 0;
}
