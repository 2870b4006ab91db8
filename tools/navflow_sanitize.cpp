// A stand-alone program for a sanitizer run of the flow fields' HOST code (csrc/kernels/navflow.h over navpath.h's hop, start and
// sight, through ms_host_nav_flows and ms_host_nav_flow_query): no GPU, no Python.  Build the library's translation unit and this
// file with the host sanitizers and run the result, as tools/navcost_sanitize.cpp's header describes:
//
//     cd megastep_amd/csrc
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           -fsanitize=address,undefined -x hip megastep_hip.hip ../../tools/navflow_sanitize.cpp -o /tmp/navflow_sanitize
//     /tmp/navflow_sanitize
//
// Hand-made grids - one cell, one row, one column, rooms with a wall and a one-cell doorway, an env without cells - every store
// allocated to the byte, so that a read or write past a store's end is a report.  Per grid a seeded field (plain breadth-first
// sums of the hop's weights - a field need not be exact for the chains to be followed, only to fall) takes look-aheads 1, 2, 16
// and 64, once with the grid's own max_framed (the framed codes) and once on a grid that declares none, under which the largest env
// exceeds the launch's tier (the stores' path): the two must agree, every target must be -1 on a dead cell and a live cell of the env otherwise, and a seed must name itself.  Then
// the field is scrambled (a stale field), and queried with points inside, outside, NaN and infinite, against a store of wild
// targets too.  Exit status 0 and no report from the sanitizers: clean.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/megastep_hip_test.h"

static unsigned next_random(unsigned& s) { s = s*1664525u + 1013904223u; return s >> 8; }

int main() {
    unsigned seed = 11;
    const float cell = .25f;
    const int shapes[][2] = {{1, 1}, {40, 1}, {1, 40}, {12, 9}, {33, 17}, {130, 130}, {0, 0}};
    int failures = 0;
    long long live = 0;
    for (int shape = 0; shape < 7; shape++) {
        const int nx = shapes[shape][0], ny = shapes[shape][1], cells = nx*ny;
        const size_t spare = cells ? 0 : 1;                              // (an env without cells still has to point somewhere)
        alignas(16) int geom[4] = {-3 + shape, 2 - shape, nx, ny};
        const long long starts[2] = {0, cells};
        std::vector<unsigned char> free_cells((size_t)cells + spare, 1);
        if (nx > 4 && ny > 4)
            for (int i = 0; i < ny; i++) if (i != ny/2) free_cells[(size_t)i*nx + nx/2] = 0;       // a wall with a doorway one cell wide
        // a seeded field by breadth-first sums from cell 0 and the last cell
        std::vector<float> D((size_t)cells + spare, INFINITY);
        if (cells) D[0] = D[cells - 1] = 0.f;
        for (bool changed = cells > 0; changed;) {
            changed = false;
            for (int k = 0; k < cells; k++) {
                if (!free_cells[k]) continue;
                const int i = k/nx, j = k % nx;
                const float was = D[k];
                if (j + 1 < nx && free_cells[k + 1] && D[k + 1] + cell < D[k]) D[k] = D[k + 1] + cell;
                if (j > 0 && free_cells[k - 1] && D[k - 1] + cell < D[k]) D[k] = D[k - 1] + cell;
                if (i + 1 < ny && free_cells[k + nx] && D[k + nx] + cell < D[k]) D[k] = D[k + nx] + cell;
                if (i > 0 && free_cells[k - nx] && D[k - nx] + cell < D[k]) D[k] = D[k - nx] + cell;
                changed |= D[k] < was;
            }
        }
        MsNavGrid grid;
        memset(&grid, 0, sizeof grid);
        grid.n_envs = 1; grid.cell = cell; grid.clearance = .2f; grid.geom = geom; grid.starts = starts; grid.free_cells = free_cells.data();
        const int looks[4] = {1, 2, 16, 64};
        for (int stale = 0; stale < 2; stale++) {
            if (stale)
                for (int k = 0; k < cells; k += 3) D[k] = (float)(next_random(seed) % 100)*.1f;
            if (stale && cells > 5) D[5] = NAN;
            for (int l = 0; l < 4; l++) {
                std::vector<int> framed((size_t)cells + spare, -7), stored((size_t)cells + spare, -7);
                MsNavFlows f;
                memset(&f, 0, sizeof f);
                f.n_fields = 1; f.fields = D.data(); f.lookahead = looks[l];
                grid.max_framed = cells ? (nx + 2)*(ny + 2) : 0; f.targets = framed.data();
                const int a = ms_host_nav_flows(&grid, &f);
                grid.max_framed = 0; f.targets = stored.data();
                // (a grid that declares nothing picks the least tier: the 130 x 130 env does not fit it and takes the stores' path)
                const int b = ms_host_nav_flows(&grid, &f);
                if (a != MS_OK || b != MS_OK || framed != stored) { printf("shape %d L %d stale %d: the calls\n", shape, looks[l], stale); failures++; continue; }
                for (int k = 0; k < cells; k++) {
                    const bool is_live = free_cells[k] && D[k] < INFINITY;
                    const int t = framed[k];
                    if (is_live ? (t < 0 || t >= cells || !free_cells[t]) : t != -1) { printf("shape %d L %d cell %d: target %d\n", shape, looks[l], k, t); failures++; }
                    if (is_live && (D[k] == 0.f || looks[l] == 1) && t != k) { printf("shape %d L %d cell %d: a seed names %d\n", shape, looks[l], k, t); failures++; }
                    live += is_live;
                }
                // the query: points over and round the env, no numbers, far away; then against wild targets
                const int P = 24;
                std::vector<float> points((size_t)P*2), way((size_t)P*2, -7.f);
                std::vector<int> goal(P, 0), took(P, -7);
                for (int p = 0; p < P; p++) {
                    points[2*p] = ((float)geom[0] - 1.f + (float)(next_random(seed) % 1000)*.001f*(float)(nx + 2))*cell;
                    points[2*p + 1] = ((float)geom[1] - 1.f + (float)(next_random(seed) % 1000)*.001f*(float)(ny + 2))*cell;
                }
                points[0] = NAN; points[3] = INFINITY; points[4] = -3e38f; goal[3] = 1; goal[4] = -1;
                MsNavFlowQuery q;
                memset(&q, 0, sizeof q);
                q.n_points = P; q.points = points.data(); q.goal = goal.data(); q.fields = D.data(); q.n_fields = 1; q.targets = framed.data();
                q.waypoints = way.data(); q.took = took.data();
                grid.max_framed = cells ? (nx + 2)*(ny + 2) : 0;
                if (ms_host_nav_flow_query(&grid, &q) != MS_OK) { printf("shape %d: the query\n", shape); failures++; }
                for (int p = 0; p < P; p++)
                    if ((took[p] < 0) != std::isnan(way[2*p]) || took[p] < -1 || took[p] > 1) { printf("shape %d point %d: took %d\n", shape, p, took[p]); failures++; }
                std::vector<int> wild((size_t)cells + spare);
                for (size_t k = 0; k < wild.size(); k++) wild[k] = (int)(next_random(seed) % 7) == 0 ? (int)k : (int)next_random(seed) - (1 << 23);
                q.targets = wild.data(); q.took = nullptr;
                if (ms_host_nav_flow_query(&grid, &q) != MS_OK) { printf("shape %d: the wild query\n", shape); failures++; }
            }
        }
    }
    // refusals
    {
        alignas(16) const int geom[4] = {0, 0, 2, 2};
        const long long starts[2] = {0, 4};
        unsigned char free_cells[4] = {1, 1, 1, 1};
        float D[4] = {0.f, .25f, .25f, .35f};
        int targets[4];
        MsNavGrid grid;
        memset(&grid, 0, sizeof grid);
        grid.n_envs = 1; grid.cell = .25f; grid.clearance = .2f; grid.geom = geom; grid.starts = starts; grid.free_cells = free_cells; grid.max_framed = 16;
        MsNavFlows f;
        memset(&f, 0, sizeof f);
        f.n_fields = 1; f.fields = D; f.lookahead = 16; f.targets = targets;
        if (ms_host_nav_flows(&grid, &f) != MS_OK || targets[0] != 0 || targets[3] != 0) { printf("the 2 x 2 room\n"); failures++; }
        f.lookahead = 65;
        if (ms_host_nav_flows(&grid, &f) != MS_EINVAL) { printf("L 65\n"); failures++; }
        f.lookahead = 16; f.targets = (int*)D;
        if (ms_host_nav_flows(&grid, &f) != MS_EINVAL) { printf("aliasing\n"); failures++; }
        f.targets = nullptr;
        if (ms_host_nav_flows(&grid, &f) != MS_EINVAL || ms_host_nav_flows(&grid, nullptr) != MS_EINVAL) { printf("NULL\n"); failures++; }
    }
    printf("%lld live cells given targets\n", live);
    if (live < 1000) { printf("too few cells to mean anything\n"); failures++; }
    printf(failures ? "FAILED\n" : "clean\n");
    return failures ? 1 : 0;
}
