// kernels/navclear.h -- nav_clear_kernel, nav_clear_query_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navfield.h: a cell's
// centre is navfield.h's nav_centre, a line's d2 and the winner are overhead.h's ov_fold and OvBest, the culls its ov_keeps, an
// agent's row render.h's drawn_row); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// clearance: the distance to the nearest wall, per cell and per point              no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavClearance, MsNavClearQuery) and DESIGN.md section 3.23: what
// nav_free_kernel folds and throws away - the least d2 of MsOverhead's point-to-segment rule within R = max_range, ties to the
// lower row - kept: its root, its row, and the free byte of up to eight body sizes at once.  Every value has one writer and one
// definition; tests/test_navclear_host.py restates it in numpy (clear_rule) and the kernels - and their host instantiations,
// ms_host_nav_clearance / ms_host_nav_clear_query, which sweep the __host__ __device__ pieces below serially - are held to
// EQUALITY with it.
//
//   nav_clear_kernel<WAVE_CULL>   overhead_kernel's scheme on grid cells: a workgroup a 16 x 16 tile of an env's cells, a lane a
//                     cell (the grid is sized for the env of most tiles; an env of fewer leaves its spare blocks at once, one of
//                     more takes a tile after another).  The env's static rows WG at a time: those ov_keeps cannot rule out for
//                     the box of the tile's centres at R go into an LDS list with their indices, ascending; the list is folded
//                     when it could overflow and at the end.  ov_keeps drops a row only when no centre in the box can have
//                     d2 <= R*R with it, so the fold over the list is the fold over all rows, and ascending order keeps the
//                     tie rule.
//                     WAVE_CULL: the fold takes the list 64 rows at a time; a lane a row tests ov_keeps(the wave's own 16 x 4
//                     box, h, row) with h = sqrtf(the greatest best d2 of the wave's lanes) once every lane has a winner, and
//                     the wave folds only the rows some lane kept (a ballot: the loop is scalar).  Exact: ov_keeps at h keeps
//                     every row that can reach d2 <= h*h at a centre of the box, with slack r >= h*(1 + 1e-5) that covers the
//                     roundings of sqrtf and of h*h ten thousand times over; a dropped row has d2 above every lane's best and
//                     would lose; a later row of EQUAL d2 loses the tie anyway.
//   nav_clear_query_kernel   one wave a point: the lanes stride the env's rows (with agents: the A M agent rows at the agents'
//                     live poses first, drawn in registers, less those of the agent the point skips), a best each; the
//                     lexicographic minimum of (d2, row) by six xor shuffles - a minimum is order-free - and lane 0 stores.
//                     No LDS, no atomics.
constexpr int CLEAR_MAX_RADII = 8;
constexpr int CLEAR_BRUTE = 0, CLEAR_TILE = 1, CLEAR_TILE_WAVE = 2;     // which culls run (ms_debug_nav_clear_cull, the host hooks' flags)
constexpr int CLEAR_WAVE_ROWS = OV_TILE*OV_TILE/WAVE;                  // rows of the tile a wave holds: 4

struct ClearArgs {                                   // MsNavClearance, checked
    const unsigned char* mask;                       // (N,) or NULL
    float* values;
    int* nearest;                                    // or NULL
    unsigned char* fits;                             // NULL exactly when n_radii == 0
    int n_radii, cull;
    float R, R2;                                     // max_range and its square (binary32, as the rule squares it)
    float r2[CLEAR_MAX_RADII];                       // the radii's squares
};

struct ClearQueryArgs {                              // MsNavClearQuery, checked
    const float* points;                             // (N, P, 2)
    const int* skip;                                 // (N, P) or NULL
    const unsigned char* mask;                       // (N, P) or NULL
    float* distances; int* nearest; float* towards;  // any of them NULL: not wanted
    int n_points, with_agents;
    long long total;                                 // N P
    float R2;
};

// The box of the centres of rows i0..i1 and columns j0..j1 of an env's grid.  nav_centre is monotone in the index - a
// conversion, an addition and a product with c > 0, each monotone - so every centre of the range lies in the box of its corner
// centres, exactly: no slack.  `mag` as ov_footprint sets it, for ov_keeps' own slack.
__host__ __device__ inline OvBox clear_box(const NavCells& g, const int i0, const int j0, const int i1, const int j1) {
    const float xa = nav_centre(g.jx0, j0, g.c), xb = nav_centre(g.jx0, j1, g.c);
    const float ya = nav_centre(g.iy0, i0, g.c), yb = nav_centre(g.iy0, i1, g.c);
    OvBox b{fminf(xa, xb), fminf(ya, yb), fmaxf(xa, xb), fmaxf(ya, yb), 0.f, true};
    b.finite = isfinite(xa) && isfinite(xb) && isfinite(ya) && isfinite(yb);
    b.mag = fmaxf(fmaxf(fabsf(b.x0), fabsf(b.x1)), fmaxf(fabsf(b.y0), fabsf(b.y1)));
    return b;
}

// The second cull: may `row` still better the best of a lane whose centre lies in `box`, when the greatest best d2 of those
// lanes is `worst`?  (+inf: some lane has no winner yet - every row is kept.)
__host__ __device__ inline bool clear_wave_keeps(const OvBox& box, const float worst, const float4 row) {
    return !(worst < INFINITY) || ov_keeps(box, sqrtf(worst), row);
}

// Does best a come before best b: the winner's order, least d2 then least row.
__host__ __device__ inline bool clear_before(const OvBest& a, const OvBest& b) {
    return (a.d2 < b.d2) | ((a.d2 == b.d2) & (a.idx < b.idx));
}

// The stores of cell k of an env of `cells` cells whose first cell is `first`.
__host__ __device__ inline void clear_store(const ClearArgs& q, const long long first, const long long cells, const long long k, const OvBest& b) {
    const bool won = b.idx != INT_MAX;
    q.values[first + k] = won ? sqrtf(b.d2) : INFINITY;
    if (q.nearest) q.nearest[first + k] = won ? b.idx : -1;
    for (int r = 0; r < q.n_radii; r++) q.fits[q.n_radii*first + r*cells + k] = (won && b.d2 <= q.r2[r]) ? 0 : 1;
}

// The stores of point `at` = (x, y), `row` its winner's.  dx, dy: the winner's own - MsOverhead's px, py, vx, vy, dx, dy
// statements once more, from the winner's t, which are the bits ov_fold formed them from.
__host__ __device__ inline void clear_query_store(const ClearQueryArgs& q, const long long at, const float x, const float y, const OvBest& b,
                                                  const float4 row) {
    const bool won = b.idx != INT_MAX;
    const float d = won ? sqrtf(b.d2) : INFINITY;
    if (q.distances) q.distances[at] = d;
    if (q.nearest) q.nearest[at] = won ? b.idx : -1;
    if (q.towards) {
        float tx = 0.f, ty = 0.f;
        if (won && d > 0.f) {
            const float vx = row.z - row.x, vy = row.w - row.y, px = x - row.x, py = y - row.y;
            const float dx = px - b.t*vx, dy = py - b.t*vy;
            tx = -dx/d; ty = -dy/d;
        }
        q.towards[2*at] = tx; q.towards[2*at + 1] = ty;
    }
}

// The agent a point skips: skip[at] when it names one of the env's, else none (-1).
__host__ __device__ inline int clear_skipped(const int* skip, const long long at, const int n_agents) {
    const int s = skip ? skip[at] : -1;
    return ((s >= 0) & (s < n_agents)) ? s : -1;
}

// ms_host_nav_clearance: the kernel's tiles, windows, list and folds swept serially over host arrays - `walls` the STATIC rows of
// all envs, env n's wall_starts[n] .. wall_starts[n + 1] - 1, numbered from `first_row` on within their env.  mode: CLEAR_BRUTE
// (every tile keeps every row), CLEAR_TILE, CLEAR_TILE_WAVE (the second cull over the same 16 x 4 groups of cells and the same
// runs of 64 list rows, in the same order).  folds / pairs (or NULL): the (cell, row) pairs folded, and all there are.
inline void clear_serial(const NavArgs& a, const ClearArgs& q, const float4* walls, const long long* wall_starts, const int first_row, const int mode,
                         long long* folds, long long* pairs) {
    std::vector<float4> list(OV_CHUNK);
    std::vector<int> index(OV_CHUNK);
    std::vector<OvBest> best(WG);
    std::vector<float> xs(WG), ys(WG);
    long long folded = 0, all = 0;
    for (int e = 0; e < a.n_envs; e++) {
        if (q.mask && !q.mask[e]) continue;
        const NavCells g = nav_cells(a, e);
        const long long cells = nav_count(a, e);
        if (cells == 0) continue;
        const float4* const rows = walls + wall_starts[e];
        const long long L = wall_starts[e + 1] - wall_starts[e];
        const int tiles_x = (g.nx + OV_TILE - 1)/OV_TILE, tiles_y = (g.ny + OV_TILE - 1)/OV_TILE;
        for (int ty = 0; ty < tiles_y; ty++)
            for (int tx = 0; tx < tiles_x; tx++) {
                const int i0 = ty*OV_TILE, j0 = tx*OV_TILE;
                const int i1 = i0 + OV_TILE - 1 < g.ny - 1 ? i0 + OV_TILE - 1 : g.ny - 1, j1 = j0 + OV_TILE - 1 < g.nx - 1 ? j0 + OV_TILE - 1 : g.nx - 1;
                const OvBox box = clear_box(g, i0, j0, i1, j1);
                OvBox wbox[WAVES];
                for (int w = 0; w < WAVES; w++) {
                    const int ia = i0 + CLEAR_WAVE_ROWS*w < i1 ? i0 + CLEAR_WAVE_ROWS*w : i1;
                    const int ib = i0 + CLEAR_WAVE_ROWS*w + CLEAR_WAVE_ROWS - 1 < i1 ? i0 + CLEAR_WAVE_ROWS*w + CLEAR_WAVE_ROWS - 1 : i1;
                    wbox[w] = clear_box(g, ia, j0, ib, j1);
                }
                for (int t = 0; t < WG; t++) {                              // (a lane beyond the grid redoes a cell of the tile's edge)
                    const int i = i0 + t/OV_TILE < i1 ? i0 + t/OV_TILE : i1, j = j0 + t%OV_TILE < j1 ? j0 + t%OV_TILE : j1;
                    xs[t] = nav_centre(g.jx0, j, g.c); ys[t] = nav_centre(g.iy0, i, g.c);
                    best[t] = OvBest{INFINITY, INT_MAX, 0.f};
                }
                all += (long long)WG*L;
                int count = 0;
                for (long long l0 = 0; l0 < L; l0 += WG) {
                    for (long long l = l0; l < L && l < l0 + WG; l++)
                        if (mode == CLEAR_BRUTE || ov_keeps(box, q.R, rows[l])) { list[count] = rows[l]; index[count] = first_row + (int)l; count++; }
                    if (count > OV_CHUNK - WG || l0 + WG >= L) {
                        for (int w = 0; w < WAVES; w++)
                            for (int q0 = 0; q0 < count; q0 += WAVE) {
                                float worst = -INFINITY;
                                for (int t = w*WAVE; t < (w + 1)*WAVE; t++) worst = fmaxf(worst, best[t].d2);
                                for (int b = q0; b < count && b < q0 + WAVE; b++) {
                                    if (mode == CLEAR_TILE_WAVE && !clear_wave_keeps(wbox[w], worst, list[b])) continue;
                                    for (int t = w*WAVE; t < (w + 1)*WAVE; t++) ov_fold(xs[t], ys[t], list[b], index[b], q.R2, best[t]);
                                    folded += WAVE;
                                }
                            }
                        count = 0;
                    }
                }
                for (int t = 0; t < WG; t++) {
                    const int i = i0 + t/OV_TILE, j = j0 + t%OV_TILE;
                    if (i < g.ny && j < g.nx) clear_store(q, a.starts[e], cells, (long long)i*g.nx + j, best[t]);
                }
            }
    }
    if (folds) *folds = folded;
    if (pairs) *pairs = all;
}

// ms_host_nav_clear_query: the query swept serially over host arrays - `rows` ALL rows of all envs as they stand (the agents'
// first, at whatever pose the caller drew them: the host draws none), env n's row_starts[n] .. row_starts[n + 1] - 1.  dealt: the
// rows go to 64 bests, row by row as the kernel's lanes stride them, merged by the kernel's butterfly; else one serial fold.
inline void clear_query_serial(const ClearQueryArgs& q, const int n_agents, const int n_model, const float4* rows_all, const long long* row_starts,
                               const bool dealt) {
    const int AF = n_agents*n_model;
    for (long long at = 0; at < q.total; at++) {
        if (q.mask && !q.mask[at]) continue;
        const int e = (int)(at / q.n_points);
        const float4* const rows = rows_all + row_starts[e];
        const int L = (int)(row_starts[e + 1] - row_starts[e]);
        const float x = q.points[2*at], y = q.points[2*at + 1];
        const int s = q.with_agents ? clear_skipped(q.skip, at, n_agents) : -1;
        const int start = q.with_agents ? 0 : AF;
        OvBest lanes[WAVE];
        for (int t = 0; t < WAVE; t++) lanes[t] = OvBest{INFINITY, INT_MAX, 0.f};
        for (int l = start; l < L; l++) {
            if (s >= 0 && l >= s*n_model && l < (s + 1)*n_model) continue;
            ov_fold(x, y, rows[l], l, q.R2, lanes[dealt ? (l - start) % WAVE : 0]);
        }
        if (dealt)
            for (int o = WAVE/2; o; o >>= 1) {
                OvBest next[WAVE];
                for (int t = 0; t < WAVE; t++) next[t] = clear_before(lanes[t ^ o], lanes[t]) ? lanes[t ^ o] : lanes[t];
                for (int t = 0; t < WAVE; t++) lanes[t] = next[t];
            }
        const OvBest b = lanes[0];
        clear_query_store(q, at, x, y, b, b.idx != INT_MAX ? rows[b.idx] : make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

// The fold of the tile's list (see the head of the file).
template <bool WAVE_CULL>
__device__ inline void clear_fold_list(const float4* s_rows, const int* s_idx, const int count, const float x, const float y, const OvBox& wbox,
                                       const float R2, const int lane, OvBest& best) {
    if (!WAVE_CULL) {
        for (int k = 0; k < count; k++) ov_fold(x, y, s_rows[k], s_idx[k], R2, best);
    } else {
        for (int q0 = 0; q0 < count; q0 += WAVE) {
            float worst = best.d2;
            for (int o = WAVE/2; o; o >>= 1) worst = fmaxf(worst, __shfl_xor(worst, o));
            const int k = q0 + lane;
            unsigned long long kept = __ballot(k < count && clear_wave_keeps(wbox, worst, s_rows[k < count ? k : 0]));
            while (kept) {                                              // (uniform: ascending, so the tie rule holds)
                const int b = q0 + __ffsll((long long)kept) - 1;
                kept &= kept - 1;
                ov_fold(x, y, s_rows[b], s_idx[b], R2, best);
            }
        }
    }
}

template <bool WAVE_CULL>
__global__ __launch_bounds__(WG) void nav_clear_kernel(const MsScenery sc, const NavArgs a, const ClearArgs q) {
    __shared__ float4 s_rows[OV_CHUNK];
    __shared__ int s_idx[OV_CHUNK];
    __shared__ int s_wave[WAVES];
    const int e = blockIdx.y, tid = threadIdx.x, lane = tid % WAVE, wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    if (q.mask && !q.mask[e]) return;                                   // (uniform)
    const NavCells g = nav_cells(a, e);
    const long long cells = nav_count(a, e);
    if (cells == 0) return;
    const int tiles_x = (g.nx + OV_TILE - 1)/OV_TILE, tiles_y = (g.ny + OV_TILE - 1)/OV_TILE;
    const long long tiles = (long long)tiles_x*tiles_y;
    const long long first = a.starts[e];
    const int AF = sc.n_agents*sc.n_model;
    const int L = sc.lines_widths[e];
    const float4* const rows = reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[e];
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {                // (uniform: the grid is sized for the env of most tiles)
        const int ty = (int)(tile / tiles_x), tx = (int)(tile - (long long)ty*tiles_x);
        const int i0 = ty*OV_TILE, j0 = tx*OV_TILE, i1 = min(i0 + OV_TILE - 1, g.ny - 1), j1 = min(j0 + OV_TILE - 1, g.nx - 1);
        const int ir = i0 + tid / OV_TILE, jr = j0 + tid % OV_TILE;
        const bool live = (ir < g.ny) & (jr < g.nx);
        const int i = min(ir, i1), j = min(jr, j1);                     // (a lane beyond the grid redoes a cell of the tile's edge, stores nothing)
        const float x = nav_centre(g.jx0, j, g.c), y = nav_centre(g.iy0, i, g.c);
        const OvBox box = clear_box(g, i0, j0, i1, j1);
        const OvBox wbox = clear_box(g, min(i0 + CLEAR_WAVE_ROWS*wave, i1), j0, min(i0 + CLEAR_WAVE_ROWS*wave + CLEAR_WAVE_ROWS - 1, i1), j1);
        OvBest best{INFINITY, INT_MAX, 0.f};
        int count = 0;
        for (int l0 = AF; l0 < L; l0 += WG) {
            const int l = l0 + tid;
            bool keep = false;
            float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
            if (l < L) {
                row = rows[l];
                keep = !q.cull || ov_keeps(box, q.R, row);
            }
            // compaction: the wave's survivors by ballot, the waves' counts through LDS (overhead_kernel's)
            const unsigned long long m = __ballot(keep);
            if (lane == 0) s_wave[wave] = (int)__popcll(m);
            __syncthreads();
            int off = count, total = 0;
            for (int w = 0; w < WAVES; w++) {
                const int c = s_wave[w];
                off += w < wave ? c : 0;
                total += c;
            }
            off += (int)__popcll(m & ((1ull << lane) - 1ull));
            if (keep) { s_rows[off] = row; s_idx[off] = l; }
            count += total;
            __syncthreads();
            if (count > OV_CHUNK - WG || l0 + WG >= L) {                // (uniform) the list is full, or the env's rows are done
                clear_fold_list<WAVE_CULL>(s_rows, s_idx, count, x, y, wbox, q.R2, lane, best);
                count = 0;
                __syncthreads();
            }
        }
        if (live) clear_store(q, first, cells, (long long)ir*g.nx + jr, best);
    }
}

__global__ __launch_bounds__(WG) void nav_clear_query_kernel(const MsScenery sc, const AgentsK ag, const ClearQueryArgs q) {
    const int lane = threadIdx.x % WAVE;
    const long long at = (long long)blockIdx.x*WAVES + threadIdx.x / WAVE;      // the wave's point (n, p): n P + p
    if (at >= q.total) return;                                          // (uniform in the wave; the kernel has no barrier)
    if (q.mask && !q.mask[at]) return;
    const int e = (int)(at / q.n_points);
    const int A = sc.n_agents, M = sc.n_model, AF = A*M;
    const int L = sc.lines_widths[e];
    const float4* const rows = reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[e];
    const float2 p = reinterpret_cast<const float2*>(q.points)[at];
    const int s = q.with_agents ? clear_skipped(q.skip, at, A) : -1;
    // row l of the env as the query meets it: an agent's at its current pose, as ms_render draws it; a wall's as stored
    auto row_at = [&](const int l) {
        if (l >= AF) return rows[l];
        const int agent = l / M;
        float sn, cs;
        sincospi_f(ag.angles[e*A + agent]/180.f, sn, cs);
        const float2 pa = reinterpret_cast<const float2*>(ag.positions)[e*A + agent];
        return drawn_row(sn, cs, pa.x, pa.y, reinterpret_cast<const float4*>(sc.model)[l - agent*M]);
    };
    OvBest best{INFINITY, INT_MAX, 0.f};
    for (int l = (q.with_agents ? 0 : AF) + lane; l < L; l += WAVE) {
        if ((s >= 0) & (l >= s*M) & (l < (s + 1)*M)) continue;
        ov_fold(p.x, p.y, row_at(l), l, q.R2, best);
    }
    for (int o = WAVE/2; o; o >>= 1) {
        const OvBest other{__shfl_xor(best.d2, o), __shfl_xor(best.idx, o), __shfl_xor(best.t, o)};
        if (clear_before(other, best)) best = other;
    }
    if (lane == 0) clear_query_store(q, at, p.x, p.y, best, best.idx != INT_MAX ? row_at(best.idx) : make_float4(0.f, 0.f, 0.f, 0.f));
}
