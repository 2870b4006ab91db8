// kernels/navflow.h -- nav_flow_kernel, nav_flow_query_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navbasin.h; NavEnv, NavGoal,
// nav_hop, nav_start, nav_sight, nav_sight_samples, nav_furthest_seen and nav_waypoint_from are navpath.h's, the grid navfield.h's);
// not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// flow fields: every cell's look-ahead target                               no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavFlows, MsNavFlowQuery) and DESIGN.md section 3.38: the chain of a live
// cell v - x_0 its centre, x_{k+1} the centre of the cell nav_hop moves to, at most L points, the goal point q last where a
// single-goal chain ends with room left - and its target, the furthest x_k, k >= 1, that x_0 can see (k = 1 untested; a chain of one
// point names v itself).  tests/flow_rule.py restates it in numpy on path_rule's hop, sight and start.
//
//   nav_flow_kernel        one workgroup a field.  CODES: each lane computes, once, for its cells of the FRAMED env (a ring of BLOCKED
//                          round it) what nav_hop does there - from the field in global memory - as ONE BYTE in LDS: 0..7 the neighbour
//                          taken in nav_di / nav_dj order, FLOW_END, FLOW_BROKEN, FLOW_DEAD (free, D not < +inf) or FLOW_BLOCKED.  A
//                          free cell is any code but FLOW_BLOCKED: no second bitmap.  One barrier.  TARGETS: a lane a cell,
//                          tid + THREADS*r.  A hop is a byte load and an add; the lane walks to the chain's far end (at most L - 1 hops)
//                          and tests the sight from the far end down, a candidate nearer than the far end reached by walking again from
//                          the cell - no per-lane array of chain points, no scratch.  A sight sample's four cells are four LDS bytes;
//                          the frame spares the per-cell bounds test: only the sample's corner is tested against the frame.  In open
//                          floor the far end is in sight at the first try; lanes diverge near walls.  Each cell stores its own
//                          element: one writer an output.  Three instantiations by the LDS they declare (16, 64, 160 KiB; 256, 1024,
//                          1024 threads); an env whose framed cells exceed the launch's one takes its codes through nav_hop and its
//                          frees from global memory (FlowStored) - slower, the same result, no workspace.
//   nav_flow_query_kernel  one lane a point: nav_start, the target under the anchor, one sight from the point, else the L = 2
//                          waypoint (nav_waypoint_from<2>: at most one hop and one sight, round the anchor's eight neighbours).  No LDS.
constexpr int FLOW_GOAL = -2;
constexpr int FLOW_END = 8, FLOW_BROKEN = 9, FLOW_DEAD = 10, FLOW_BLOCKED = 11;
constexpr int FLOW_LDS[3] = {16*1024, 64*1024, 160*1024}, FLOW_THREADS[3] = {256, 1024, 1024};
constexpr int flow_capacity(const int lds_bytes) { return lds_bytes; }                                // framed cells: a byte each

// The code of cell (i, j): what nav_hop does there, in a byte.  (di, dj) -> the neighbour's number, a nibble an offset pair.
__host__ __device__ inline int flow_code(const NavEnv& g, const NavGoal& q, const int i, const int j) {
    const long long k = (long long)i*g.nx + j;
    if (!(g.free[k] & 1)) return FLOW_BLOCKED;
    if (!(g.D[k] < INFINITY)) return FLOW_DEAD;
    int ui = i, uj = j;
    const int state = nav_hop(g, q, ui, uj);
    if (state != 1) return state == 0 ? FLOW_END : FLOW_BROKEN;
    return (int)((0x415002736ULL >> 4*((ui - i + 1)*3 + (uj - j + 1))) & 15);
}

// The two places a chain is followed in.  `pos` is a cell in the place's own numbering; code(pos), step(pos, t) to neighbour t,
// the cell's (i, j), and clear(i0, j0): are the four cells of a sight sample's corner all free.
struct FlowFramed {                                  // the codes of the framed env, row pitch P = nx + 2 (LDS; a host array)
    const unsigned char* codes;
    int P, nx, ny;
    __host__ __device__ int at(const int i, const int j) const { return (i + 1)*P + j + 1; }
    __host__ __device__ int code(const int pos) const { return codes[pos]; }
    __host__ __device__ int step(const int pos, const int t) const { return pos + nav_di(t)*P + nav_dj(t); }
    __host__ __device__ void cell(const int pos, int& i, int& j) const { i = pos / P - 1; j = pos - (i + 1)*P - 1; }
    __host__ __device__ bool clear(const long long i0, const long long j0) const {
        if (((unsigned long long)(i0 + 1) > (unsigned long long)ny) | ((unsigned long long)(j0 + 1) > (unsigned long long)nx)) return false;    // outside the frame
        const unsigned char* const c = codes + (i0 + 1)*P + (j0 + 1);
        return (c[0] != FLOW_BLOCKED) & (c[1] != FLOW_BLOCKED) & (c[P] != FLOW_BLOCKED) & (c[P + 1] != FLOW_BLOCKED);
    }
};
struct FlowStored {                                  // the field and the free bytes where they are stored: every code a nav_hop
    const NavEnv& g;
    const NavGoal& q;
    __host__ __device__ int at(const int i, const int j) const { return i*g.nx + j; }
    __host__ __device__ int code(const int pos) const { return flow_code(g, q, pos / g.nx, pos % g.nx); }
    __host__ __device__ int step(const int pos, const int t) const { return pos + nav_di(t)*g.nx + nav_dj(t); }
    __host__ __device__ void cell(const int pos, int& i, int& j) const { i = pos / g.nx; j = pos - i*g.nx; }
    __host__ __device__ bool clear(const long long i0, const long long j0) const {
        return nav_is_free(g, i0, j0) && nav_is_free(g, i0, j0 + 1) && nav_is_free(g, i0 + 1, j0) && nav_is_free(g, i0 + 1, j0 + 1);
    }
};

// nav_sight from (px, py) to (x, y) - nav_sight_samples' count, nav_sample_clear's sample point and corner, operation for operation -
// with the four frees asked of `place`.
template <typename Place>
__host__ __device__ inline bool flow_sight(const Place& place, const NavEnv& g, const float px, const float py, const float x, const float y) {
    const float dx = x - px, dy = y - py;
    const int K = nav_sight_samples(g.c, dx, dy);
    if (K < 0) return false;
    for (int s = 1; s < K; s++) {
        const float t = (float)s/(float)K;
        const float sx = px + dx*t, sy = py + dy*t;
        long long i0, j0;
        if (!nav_anchor_corner(sx, sy, g.c, g.jx0, g.iy0, i0, j0) || !place.clear(i0, j0)) return false;
    }
    return true;
}

// The target of cell (i, j): -1 not live, FLOW_GOAL, or a cell's row-major index.  The chain is counted to its far end, then
// nav_furthest_seen chooses; the point of candidate k is q, the far end, or k hops from the cell again.
template <typename Place>
__host__ __device__ inline int flow_target(const Place& place, const NavEnv& g, const NavGoal& q, const int i, const int j, const int L) {
    const int v = place.at(i, j);
    if (place.code(v) >= FLOW_DEAD) return -1;
    int n = 1, far = v;
    bool to_goal = false;
    while (n < L) {
        const int c = place.code(far);
        if (c >= FLOW_END) {
            to_goal = (c == FLOW_END) & !q.seeded;                      // the goal point, with room left
            n += to_goal;
            break;
        }
        far = place.step(far, c);
        n++;
    }
    if (n == 1) return i*g.nx + j;                                      // a seed, a chain broken at once, L = 1
    const int far_hops = n - 1 - to_goal;
    const float x0 = nav_centre(g.jx0, j, g.c), y0 = nav_centre(g.iy0, i, g.c);
    int found = far;                                                    // the cell of the candidate last looked at
    const auto walk = [&](const int k) {
        if (k == far_hops) return far;
        int pos = v;
        for (int h = 0; h < k; h++) pos = place.step(pos, place.code(pos));      // (0..7 on every cell before the far end)
        return pos;
    };
    const int k = nav_furthest_seen(n, 1, [&](const int c) {
        float x = q.x, y = q.y;
        if (!(to_goal && c == n - 1)) {
            int ci, cj;
            found = walk(c);
            place.cell(found, ci, cj);
            x = nav_centre(g.jx0, cj, g.c); y = nav_centre(g.iy0, ci, g.c);
        }
        return flow_sight(place, g, x0, y0, x, y);
    });
    if (to_goal && k == n - 1) return FLOW_GOAL;
    int ti, tj;
    place.cell(k == 1 ? walk(1) : found, ti, tj);                       // (k > 1: the candidate the choice stopped at)
    return ti*g.nx + tj;
}

struct NavFlowArgs {                                 // MsNavFlows, checked
    const unsigned char* free_cells;
    const float* fields;
    const float* goals;                              // (N, G, 2); NULL: seeded or cost fields
    const float* costs;                              // NULL: unweighted
    const unsigned char* mask;                       // (N, G) or NULL
    int* targets;
    int n_fields, n_costs, lookahead;
};

// Field (e, gi)'s env, goal and first element; false: an env without cells.
__host__ __device__ inline bool flow_bind(const NavArgs& a, const unsigned char* free_cells, const float* fields, const float* goals, const float* costs,
                                          const int n_costs, const int n_fields, const int e, const int gi, NavEnv& g, NavGoal& goal, long long& first) {
    const NavCells c = nav_cells(a, e);
    const long long cells = nav_count(a, e);
    if (cells <= 0) return false;
    first = (long long)n_fields*a.starts[e] + (long long)gi*cells;
    g = NavEnv{c.jx0, c.iy0, c.nx, c.ny, c.c, free_cells + a.starts[e], fields + first, nullptr};
    if (costs) g.cost = costs + (n_costs == 1 ? a.starts[e] : first);
    goal = goals ? nav_goal(g, goals[2*((long long)e*n_fields + gi)], goals[2*((long long)e*n_fields + gi) + 1]) : nav_seeded();
    return true;
}

// One field, serially (host instantiation only): the kernel's two paths with the same pieces - the codes in a framed array when
// the env's framed cells fit `capacity`, else from the stores.
inline void flow_serial_field(const NavArgs& a, const NavFlowArgs& f, const long long field, const int capacity) {
    const int e = (int)(field / f.n_fields), gi = (int)(field - (long long)e*f.n_fields);
    NavEnv g;
    NavGoal goal;
    long long first;
    if (!flow_bind(a, f.free_cells, f.fields, f.goals, f.costs, f.n_costs, f.n_fields, e, gi, g, goal, first)) return;
    int* const out = f.targets + first;
    const int P = g.nx + 2;
    const long long framed = (long long)P*(g.ny + 2);
    if (framed <= capacity) {
        std::vector<unsigned char> codes((size_t)framed);
        for (int k = 0; k < (int)framed; k++) {
            const int fi = k / P, fj = k - fi*P;
            codes[k] = (unsigned char)(((fi >= 1) & (fi <= g.ny) & (fj >= 1) & (fj <= g.nx)) ? flow_code(g, goal, fi - 1, fj - 1) : FLOW_BLOCKED);
        }
        const FlowFramed place{codes.data(), P, g.nx, g.ny};
        for (int k = 0; k < g.nx*g.ny; k++) out[k] = flow_target(place, g, goal, k / g.nx, k % g.nx, f.lookahead);
    } else {
        const FlowStored place{g, goal};
        for (int k = 0; k < g.nx*g.ny; k++) out[k] = flow_target(place, g, goal, k / g.nx, k % g.nx, f.lookahead);
    }
}

inline void flow_serial(const NavArgs& a, const NavFlowArgs& f, const int capacity) {
    for (long long field = 0; field < (long long)a.n_envs*f.n_fields; field++)
        if (!f.mask || f.mask[field]) flow_serial_field(a, f, field, capacity);
}

template <int LDS_BYTES, int THREADS>
__global__ __launch_bounds__(THREADS) void nav_flow_kernel(const NavArgs a, const NavFlowArgs f) {
    constexpr int CAP = flow_capacity(LDS_BYTES);
    __shared__ unsigned char codes[CAP];
    const int tid = threadIdx.x;
    const long long field = blockIdx.x;                                // (n, g): n G + g
    const int e = (int)(field / f.n_fields), gi = (int)(field - (long long)e*f.n_fields);
    if (f.mask && !f.mask[field]) return;                               // (uniform) left as it is
    NavEnv g;
    NavGoal goal;
    long long first;
    if (!flow_bind(a, f.free_cells, f.fields, f.goals, f.costs, f.n_costs, f.n_fields, e, gi, g, goal, first)) return;      // (uniform)
    int* const out = f.targets + first;
    const int nx = g.nx, n = nx*g.ny, P = nx + 2, L = f.lookahead;      // (an env has fewer than 2^31 framed cells: MsNavGrid.max_framed is an int)
    const long long framed = (long long)P*(g.ny + 2);
    if (framed <= CAP) {                                                // (uniform)
        for (int k = tid; k < (int)framed; k += THREADS) {
            const int fi = k / P, fj = k - fi*P;
            codes[k] = (unsigned char)(((fi >= 1) & (fi <= g.ny) & (fj >= 1) & (fj <= nx)) ? flow_code(g, goal, fi - 1, fj - 1) : FLOW_BLOCKED);
        }
        __syncthreads();
        const FlowFramed place{codes, P, nx, g.ny};
        for (int k = tid; k < n; k += THREADS) {
            const int i = k / nx;
            out[k] = flow_target(place, g, goal, i, k - i*nx, L);
        }
    } else {
        const FlowStored place{g, goal};
        for (int k = tid; k < n; k += THREADS) {
            const int i = k / nx;
            out[k] = flow_target(place, g, goal, i, k - i*nx, L);
        }
    }
}

struct NavFlowQueryArgs {                            // MsNavFlowQuery, checked
    const float* points;                             // (N, P, 2)
    const int* goal;                                 // (N, P) or NULL
    const unsigned char* free_cells;
    const float* fields;
    const float* goals;                              // (N, G, 2) or NULL
    const float* costs;
    const int* targets;
    float* waypoints;                                // (N, P, 2)
    int* took;                                       // (N, P) or NULL
    int n_points, n_fields, n_costs;
    long long total;                                 // N P
};

// Point `at` = (e, k): the target of the anchor nav_start picks when the point sees it, else the L = 2 waypoint.
__host__ __device__ inline void flow_query_one(const NavArgs& a, const NavFlowQueryArgs& q, const long long at) {
    const int e = (int)(at / q.n_points), k = (int)(at - (long long)e*q.n_points);
    const int gi = q.goal ? q.goal[at] : k;
    const float px = q.points[2*at], py = q.points[2*at + 1];
    float wx = NAN, wy = NAN, leg0;
    int took = -1, i = 0, j = 0;
    NavEnv g;
    NavGoal goal;
    long long first;
    if ((gi >= 0) & (gi < q.n_fields) && flow_bind(a, q.free_cells, q.fields, q.goals, q.costs, q.n_costs, q.n_fields, e, gi, g, goal, first) &&
        nav_start(g, px, py, i, j, leg0)) {
        const int here = i*g.nx + j, t = q.targets[first + here];
        const bool named = t == FLOW_GOAL ? !goal.seeded : (t >= 0) & (t < g.nx*g.ny);          // (a stale store may hold anything)
        if (named) {
            const int ti = t < 0 ? 0 : t / g.nx;
            const float x = t < 0 ? goal.x : nav_centre(g.jx0, t - ti*g.nx, g.c), y = t < 0 ? goal.y : nav_centre(g.iy0, ti, g.c);
            if (t == here || nav_sight(g, px, py, x, y)) { wx = x; wy = y; took = 1; }
            else { nav_waypoint_from<2>(g, goal, px, py, i, j, leg0, 2, wx, wy); took = 0; }
        }
    }
    q.waypoints[2*at] = wx; q.waypoints[2*at + 1] = wy;
    if (q.took) q.took[at] = took;
}

__global__ __launch_bounds__(WG) void nav_flow_query_kernel(const NavArgs a, const NavFlowQueryArgs q) {
    const long long at = (long long)blockIdx.x*WG + threadIdx.x;
    if (at < q.total) flow_query_one(a, q, at);
}
