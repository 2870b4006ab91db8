// kernels/navpath.h -- nav_waypoint_kernel, nav_path_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navfield.h, whose
// nav_centre / nav_anchor_corner / nav_leg it reads the fields with); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// paths and look-ahead waypoints on the distance fields                    no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavWaypoints) and DESIGN.md section 3.15: from a point, the
// anchor a* the query's minimum is attained at, then the descent of the field cell by cell (the first of the eight
// neighbours that attains the least D[u] + w, which at a fixed point of the relaxation IS D[v]) down to the goal; the
// waypoint is the furthest of the first L points of that chain the point can see, a sight being a run of samples half a
// cell apart whose four surrounding cells are all free.  tests/test_navpath_host.py restates all of it in numpy (path_rule).
//
// The rule's pieces - nav_start, nav_hop_weights / nav_neighbour / nav_hop, nav_sight_samples / nav_sample_clear / nav_sight - are
// __host__ __device__ functions over plain pointers: ms_host_nav_waypoint / ms_host_nav_path run them on host arrays, so the
// CPU suite holds this very text to path_rule, bit for bit.
//
//   nav_waypoint_kernel  one WAVEFRONT a query (the per-step call: N x A queries, each a serial chain of dependent gathers -
//                        a lane a query would put 4096 of them on 64 waves of a 256-CU chip).  The hop: lanes 0-7 take a
//                        neighbour each (nav_neighbour), three xor-shuffles find the least value, a ballot its first lane.
//                        Lane k keeps chain point x_k (hence L <= 64).  The sight: candidates from the furthest down, the
//                        samples of one candidate a lane each (nav_sample_clear; at L = 16 a sight has at most some 50 of
//                        them, four byte gathers each), one ballot a round; the first candidate in sight is the largest
//                        admissible index, and the loop stops there.  Every branch is wave-uniform.
//   nav_path_kernel      one lane a path (not hot): nav_hop to the chain's end for the count, the first M points written.
// Both are instantiated on WEIGHTED: the fields are cost fields (MsNavCostFields) and a hop runs with the weights
// of the cell it leaves.
struct NavEnv {                                      // one env's grid and one of its fields: what the pieces read
    int jx0, iy0, nx, ny;
    float c;
    const unsigned char* free;                       // (ny, nx)
    const float* D;                                  // (ny, nx)
    const float* cost = nullptr;                     // (ny, nx) a cost field's costs (MsNavCostFields); NULL: every cell at 1
};
struct NavGoal {                                     // the field's goal q and its anchor corner
    float x, y;
    bool anchored;
    long long i0, j0;
    bool seeded;                                     // a seeded field (MsNavSeedFields): no goal point, a chain ends on a cell at 0
};

__host__ __device__ inline NavGoal nav_goal(const NavEnv& g, const float x, const float y) {
    NavGoal q{x, y, false, 0, 0, false};
    q.anchored = nav_anchor_corner(x, y, g.c, g.jx0, g.iy0, q.i0, q.j0);
    return q;
}
__host__ __device__ inline NavGoal nav_seeded() { return NavGoal{0.f, 0.f, false, 0, 0, true}; }

__host__ __device__ inline bool nav_is_free(const NavEnv& g, const long long i, const long long j) {
    return (i >= 0) & (i < g.ny) & (j >= 0) & (j < g.nx) && (g.free[i*g.nx + j] & 1);
}

// Start: the first of p's anchors (the query's order) that attains the least fl(D[a] + leg(p, a)); false: no path - exactly
// when nav_query_kernel's minimum stays +inf.
__host__ __device__ inline bool nav_start(const NavEnv& g, const float px, const float py, int& ai, int& aj, float& leg0) {
    long long i0, j0;
    if (!nav_anchor_corner(px, py, g.c, g.jx0, g.iy0, i0, j0)) return false;
    float best = INFINITY;
    for (int t = 0; t < 4; t++) {
        const long long i = i0 + (t >> 1), j = j0 + (t & 1);
        if ((i >= 0) & (i < g.ny) & (j >= 0) & (j < g.nx)) {
            const float d = g.D[i*g.nx + j];
            if (d < INFINITY) {
                const float leg = nav_leg(px, py, g.jx0, g.iy0, (int)i, (int)j, g.c);
                const float s = d + leg;
                if (s < best) { best = s; ai = (int)i; aj = (int)j; leg0 = leg; }
            }
        }
    }
    return best < INFINITY;
}

// Neighbour t of a hop, in the rule's order (0,+1) (+1,0) (0,-1) (-1,0) (+1,+1) (+1,-1) (-1,-1) (-1,+1): two bits an offset.
__host__ __device__ inline int nav_di(const int t) { return ((0xa19 >> 2*t) & 3) - 1; }
__host__ __device__ inline int nav_dj(const int t) { return ((0x8246 >> 2*t) & 3) - 1; }

// The value fl(D[u] + w) of neighbour u = t of cell (i, j), D[u] in du; +inf (never the least: the fold replaces on <
// from +inf) for a neighbour that does not count.  ws, wd: the hop's weights (nav_hop_weights).
__host__ __device__ inline float nav_neighbour(const NavEnv& g, const int i, const int j, const int t, const float ws, const float wd, float& du) {
    const int ui = i + nav_di(t), uj = j + nav_dj(t);
    du = INFINITY;
    if (!nav_is_free(g, ui, uj)) return INFINITY;
    if (t >= 4 && !(nav_is_free(g, ui, j) && nav_is_free(g, i, uj))) return INFINITY;      // no corner is cut
    du = g.D[(long long)ui*g.nx + uj];
    return du + (t < 4 ? ws : wd);
}

// The weights of a hop out of cell (i, j), formed once a hop: those of the cell the hop LEAVES - on a cost field c and
// c*1.41421356f times its multiplier (nav_cost_weights), which a NULL cost folds to the plain ones.
__host__ __device__ inline void nav_hop_weights(const NavEnv& g, const int i, const int j, float& ws, float& wd) {
    nav_cost_weights(g.c, g.cost ? nav_cost_multiplier(g.cost[(long long)i*g.nx + j]) : 1.f, ws, wd);
}

// Does the chain end at cell (i, j): one of the goal's anchor cells whose value is its own leg to the goal; on a seeded
// field, a seed - the cells at 0, every other one holding a sum of positive weights.
__host__ __device__ inline bool nav_chain_ends(const NavEnv& g, const NavGoal& q, const int i, const int j) {
    if (q.seeded) return g.D[(long long)i*g.nx + j] == 0.f;
    if (!q.anchored || i < q.i0 || i > q.i0 + 1 || j < q.j0 || j > q.j0 + 1) return false;
    return nav_leg(q.x, q.y, g.jx0, g.iy0, i, j, g.c) == g.D[(long long)i*g.nx + j];
}

// One hop from cell (i, j).  1: on to the next cell, now in (i, j); 0: the chain ends here, its last point is the goal
// itself (seeded: this cell's centre); -1: broken (no neighbour below D[v]: a stale or foreign field) - it stops.
__host__ __device__ inline int nav_hop(const NavEnv& g, const NavGoal& q, int& i, int& j) {
    if (nav_chain_ends(g, q, i, j)) return 0;
    float best = INFINITY, dbest = INFINITY, ws, wd;
    nav_hop_weights(g, i, j, ws, wd);
    int bt = -1;
    for (int t = 0; t < 8; t++) {
        float du;
        const float v = nav_neighbour(g, i, j, t, ws, wd, du);
        if (v < best) { best = v; bt = t; dbest = du; }
    }
    if (bt < 0 || !(dbest < g.D[(long long)i*g.nx + j])) return -1;
    i += nav_di(bt); j += nav_dj(bt);
    return 1;
}

// Sight: K = (int)ceilf(len/(0.5f*c)) samples' worth of segment; -1: a length no grid holds (or a NaN) - no sight.
__host__ __device__ inline int nav_sight_samples(const float c, const float dx, const float dy) {
    const float len = sqrtf(dx*dx + dy*dy);
    const float k = ceilf(len/(.5f*c));
    return k < 1048576.f ? (int)k : -1;
}

// Sample s of K: are the four cells round p + (s/K) d all in range and free?
__host__ __device__ inline bool nav_sample_clear(const NavEnv& g, const float px, const float py, const float dx, const float dy, const int s, const int K) {
    const float t = (float)s/(float)K;
    const float x = px + dx*t, y = py + dy*t;
    long long i0, j0;
    if (!nav_anchor_corner(x, y, g.c, g.jx0, g.iy0, i0, j0)) return false;
    return nav_is_free(g, i0, j0) && nav_is_free(g, i0, j0 + 1) && nav_is_free(g, i0 + 1, j0) && nav_is_free(g, i0 + 1, j0 + 1);
}

__host__ __device__ inline bool nav_sight(const NavEnv& g, const float px, const float py, const float x, const float y) {
    const float dx = x - px, dy = y - py;
    const int K = nav_sight_samples(g.c, dx, dy);
    if (K < 0) return false;
    for (int s = 1; s < K; s++)
        if (!nav_sample_clear(g, px, py, dx, dy, s, K)) return false;
    return true;
}

// The path from p: p, x_0, x_1, ..., q (seeded: ..., the seed's centre).  Walks the whole chain (at most `cells` hops: D falls
// at every one), writes the first M points to out (M x 2; NaN in the slots beyond) and returns the number of points: 0 without
// a path, negated for a broken chain.
__host__ __device__ inline int nav_path(const NavEnv& g, const NavGoal& q, const float px, const float py, const long long cells, const int M, float* out) {
    int count = 0, i = 0, j = 0, state = -1;
    float leg0;
    if (nav_start(g, px, py, i, j, leg0)) {
        out[0] = px; out[1] = py; count = 1;                            // (M >= 2)
        for (long long hops = 0; hops <= cells; hops++) {
            if (count < M) { out[2*count] = nav_centre(g.jx0, j, g.c); out[2*count + 1] = nav_centre(g.iy0, i, g.c); }
            count++;
            state = nav_hop(g, q, i, j);
            if (state != 1) break;
        }
        if (state == 0 && !q.seeded) {
            if (count < M) { out[2*count] = q.x; out[2*count + 1] = q.y; }
            count++;
        }
    }
    for (int k = count < M ? count : M; k < M; k++) { out[2*k] = NAN; out[2*k + 1] = NAN; }
    return state == 0 || count == 0 ? count : -count;
}

// The waypoint from p with look-ahead L, serially, as the wave does it side by side (host instantiation only: the chain's
// points live in an array).  Returns the chosen index k, -1 without a path.
inline int nav_waypoint_serial(const NavEnv& g, const NavGoal& q, const float px, const float py, const int L, float& wx, float& wy) {
    wx = wy = NAN;
    int i = 0, j = 0, n = 0;
    float leg0, xs[64], ys[64];
    if (!nav_start(g, px, py, i, j, leg0)) return -1;
    for (;;) {
        xs[n] = nav_centre(g.jx0, j, g.c); ys[n] = nav_centre(g.iy0, i, g.c); n++;
        if (n >= L) break;
        const int state = nav_hop(g, q, i, j);
        if (state == 0 && !q.seeded) { xs[n] = q.x; ys[n] = q.y; n++; }
        if (state != 1) break;
    }
    const int b = (leg0 <= .5f*g.c && n >= 2) ? 1 : 0;
    int k = n - 1;
    while (k > b && !nav_sight(g, px, py, xs[k], ys[k])) k--;
    wx = xs[k]; wy = ys[k];
    return k;
}

struct NavPathArgs {                                 // MsNavWaypoints / MsNavPaths, checked
    const float* points;                             // (N, P, 2)
    const int* goal;                                 // (N, P) or NULL
    const float* fields;
    const float* goals;                              // (N, G, 2); NULL: seeded fields, which have none
    const unsigned char* free_cells;
    float* waypoints;                                // (N, P, 2)
    int* hops;                                       // (N, P) or NULL
    float* paths;                                    // (N, P, M, 2)
    int* counts;                                     // (N, P)
    int n_points, n_goals, lookahead, max_points;
    long long total;                                 // N P
    const float* costs;                              // cost fields only (WEIGHTED): as NavFieldArgs'
    int n_costs;
};

// Query `at`'s env, field and goal; false: a goal index out of range or an env without cells - no path.  WEIGHTED: the field's
// costs too - every other instantiation builds its NavEnv with a literal null, and nav_neighbour's branch folds away.
template <bool WEIGHTED>
__device__ inline bool nav_bind(const NavArgs& a, const NavPathArgs& q, const long long at, NavEnv& g, NavGoal& goal, long long& cells) {
    const int e = (int)(at / q.n_points), k = (int)(at - (long long)e*q.n_points);
    const int gi = q.goal ? q.goal[at] : k;
    const int4 geom = reinterpret_cast<const int4*>(a.geom)[e];
    cells = (long long)geom.z*geom.w;
    if ((gi < 0) | (gi >= q.n_goals) || cells <= 0) return false;
    const long long first = (long long)q.n_goals*a.starts[e] + (long long)gi*cells;
    g = NavEnv{geom.x, geom.y, geom.z, geom.w, a.cell, q.free_cells + a.starts[e], q.fields + first, nullptr};
    if constexpr (WEIGHTED) g.cost = q.costs + (q.n_costs == 1 ? a.starts[e] : first);
    if (q.goals) {
        const float2 p = reinterpret_cast<const float2*>(q.goals)[(long long)e*q.n_goals + gi];
        goal = nav_goal(g, p.x, p.y);
    } else goal = nav_seeded();
    return true;
}

template <bool WEIGHTED>
__global__ __launch_bounds__(WG) void nav_waypoint_kernel(const NavArgs a, const NavPathArgs q) {
    const int lane = threadIdx.x & 63;
    const long long at = (long long)blockIdx.x*(WG/64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (at >= q.total) return;                                          // (uniform: a wave a query)
    const float2 p = reinterpret_cast<const float2*>(q.points)[at];
    NavEnv g;
    NavGoal goal;
    long long cells;
    float wx = NAN, wy = NAN, leg0 = 0.f;
    int chosen = -1, i = 0, j = 0;
    if (nav_bind<WEIGHTED>(a, q, at, g, goal, cells) && nav_start(g, p.x, p.y, i, j, leg0)) {
        // the chain: lane k keeps x_k
        const int L = q.lookahead;
        float mx = NAN, my = NAN;
        int n = 0;
        for (;;) {
            if (lane == n) { mx = nav_centre(g.jx0, j, g.c); my = nav_centre(g.iy0, i, g.c); }
            n++;
            if (n >= L) break;
            if (nav_chain_ends(g, goal, i, j)) {
                if (!goal.seeded) {                                     // (uniform: the launch's mode)
                    if (lane == n) { mx = goal.x; my = goal.y; }
                    n++;
                }
                break;
            }
            // nav_hop's fold, a neighbour a lane: the least value, then the first lane that holds it
            float du = INFINITY, ws, wd;
            nav_hop_weights(g, i, j, ws, wd);                           // (uniform: the cell the wave's hop leaves)
            const float v = lane < 8 ? nav_neighbour(g, i, j, lane, ws, wd, du) : INFINITY;
            float least = v < INFINITY ? v : INFINITY;                  // (a NaN is never the least)
            least = fminf(least, __shfl_xor(least, 1));
            least = fminf(least, __shfl_xor(least, 2));
            least = fminf(least, __shfl_xor(least, 4));
            const unsigned long long holders = __ballot((lane < 8) & (v < INFINITY) & (v == least));
            if (!holders) break;                                        // broken
            const int t = __ffsll((long long)holders) - 1;
            const float dbest = __shfl(du, t);
            if (!(dbest < g.D[(long long)i*g.nx + j])) break;           // broken
            i += nav_di(t); j += nav_dj(t);
        }
        // the sight: from the furthest candidate down, its samples a lane each; the first in sight is the largest admissible
        const int b = (leg0 <= .5f*g.c && n >= 2) ? 1 : 0;
        int k = n - 1;
        for (; k > b; k--) {
            const float dx = __shfl(mx, k) - p.x, dy = __shfl(my, k) - p.y;
            const int K = nav_sight_samples(g.c, dx, dy);
            bool sight = K >= 0;
            for (int s0 = 1; sight && s0 < K; s0 += 64) {
                const int s = s0 + lane;
                const bool blocked = s < K && !nav_sample_clear(g, p.x, p.y, dx, dy, s, K);
                if (__ballot(blocked)) sight = false;
            }
            if (sight) break;
        }
        wx = __shfl(mx, k); wy = __shfl(my, k); chosen = k;
    }
    if (lane == 0) {
        reinterpret_cast<float2*>(q.waypoints)[at] = make_float2(wx, wy);
        if (q.hops) q.hops[at] = chosen;
    }
}

template <bool WEIGHTED>
__global__ __launch_bounds__(WG) void nav_path_kernel(const NavArgs a, const NavPathArgs q) {
    const long long at = (long long)blockIdx.x*WG + threadIdx.x;
    if (at >= q.total) return;
    const float2 p = reinterpret_cast<const float2*>(q.points)[at];
    float* const out = q.paths + at*q.max_points*2;
    NavEnv g;
    NavGoal goal;
    long long cells;
    if (nav_bind<WEIGHTED>(a, q, at, g, goal, cells)) q.counts[at] = nav_path(g, goal, p.x, p.y, cells, q.max_points, out);
    else {
        for (int k = 0; k < 2*q.max_points; k++) out[k] = NAN;
        q.counts[at] = 0;
    }
}
