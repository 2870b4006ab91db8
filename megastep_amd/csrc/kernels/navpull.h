// kernels/navpull.h -- nav_pull_kernel, nav_pull_serial.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navpath.h, whose
// nav_start / nav_hop / nav_sight it pulls the chains with); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// pulled paths: a field's chain straightened by sight, its vertices and its length   no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavPulls) and DESIGN.md section 3.26: the points P_0 = p, P_1 = x_0,
// ... of the whole path (MsNavPaths'), and from the anchor a = 0 on, again and again, the LARGEST index k of the next `reach`
// points that a + 1 is or that P_a can see (nav_sight, unchanged) - greedy string pulling.  tests/test_navpull_host.py restates
// it in numpy (pull_rule); nav_pull_serial states it serially over navpath.h's pieces, and ms_host_nav_pull runs that on host
// arrays, so the CPU suite holds this text to pull_rule, bit for bit.
//
//   nav_pull_kernel   one WAVEFRONT a path, WG/64 paths a workgroup.  The hop is nav_waypoint_kernel's (lanes 0-7 a neighbour
//                     each, three xor-shuffles, a ballot) and every hop is taken ONCE: the chain's cells - an int a point, -1
//                     for the goal, which is no cell - go through a ring in LDS of the next power of two >= reach ints a wave
//                     (at most 4 KiB a wave, 16 KiB a workgroup); when the anchor moves to k only the points past the old
//                     window's end are walked.  A centre is formed again from its index (nav_centre: the same bits).  The
//                     sights, BY_SAMPLE = false: from the window's far end down, 64 candidates a batch, a lane a candidate
//                     walking its own samples with early exit (nav_pull_sight: nav_sight's verdict, four samples' gathers in
//                     flight a round), one ballot a batch - the highest index in sight is
//                     the lowest lane set, and the first batch with a sight ends the search.  BY_SAMPLE = true: the waypoint
//                     kernel's scheme, candidate after candidate, its samples a lane each (ms_debug_nav_pull_scheme, for A/B
//                     runs; the same bits).  Lane 0 writes the vertices; the length is summed in vertex order, the same sum
//                     in every lane.  Every branch is wave-uniform but the lanes' own sample walks.
struct NavPullArgs {                                 // MsNavPulls, checked
    NavPathArgs path;                                // the query as the followers read it; paths = vertices (N, P, M, 2), counts
    const unsigned char* mask;                       // (N, P) or NULL
    int* indices;                                    // (N, P, M) or NULL
    int* cells;                                      // (N, P) or NULL
    float* lengths;                                  // (N, P)
    int reach;                                       // R, 1..NAV_PULL_REACH
    int ring;                                        // the power of two >= R: a wave's ints of LDS
};

constexpr int NAV_PULL_REACH = 1024;                 // the largest reach: a 4 KiB ring a wave
constexpr int NAV_PULL_POINTS = 1 << 20;             // the most vertices a path may be given room for
constexpr int NAV_PULL_GOAL = -1;                    // the ring's entry for the goal q, which is no cell

__host__ __device__ inline int nav_pull_ring(const int reach) {
    int ring = 1;
    while (ring < reach) ring <<= 1;
    return ring;
}

// Chain point `cell` of the ring: the centre of that cell of its env, row-major, or the goal.
__host__ __device__ inline void nav_pull_point(const NavEnv& g, const NavGoal& q, const int cell, float& x, float& y) {
    if (cell == NAV_PULL_GOAL) { x = q.x; y = q.y; return; }
    const int i = cell/g.nx, j = cell - i*g.nx;
    x = nav_centre(g.jx0, j, g.c); y = nav_centre(g.iy0, i, g.c);
}

// One more segment of a pulled path, from (ax, ay) to (x, y): L = fl(L + sqrtf(fl(fl(dx*dx) + fl(dy*dy)))).
__host__ __device__ inline float nav_pull_add(const float L, const float ax, const float ay, const float x, const float y) {
    const float dx = x - ax, dy = y - ay;
    return L + sqrtf(dx*dx + dy*dy);
}

// The rule, serially (host instantiation only: the chain's points live in a vector).  Writes the first M vertices (NaN beyond)
// and, indices not NULL, their chain indices (-1 beyond); returns `counts`: the vertices, negated for a broken chain, 0 without
// a path.  cells_out, or NULL: MsNavPaths' count.
inline int nav_pull_serial(const NavEnv& g, const NavGoal& q, const float px, const float py, const int R, const int M, float* vertices,
                           int* indices, int* cells_out, float& length) {
    for (int k = 0; k < M; k++) {
        vertices[2*k] = vertices[2*k + 1] = NAN;
        if (indices) indices[k] = -1;
    }
    length = INFINITY;
    if (cells_out) *cells_out = 0;
    int i = 0, j = 0, state = 1;
    float leg0;
    if (!nav_start(g, px, py, i, j, leg0)) return 0;
    std::vector<int> chain;                                             // P_1 ..: a cell a point, the goal last
    const long long cells = (long long)g.nx*g.ny;
    for (long long hops = 0; hops <= cells; hops++) {
        chain.push_back(i*g.nx + j);
        state = nav_hop(g, q, i, j);
        if (state != 1) break;
    }
    if (state == 0 && !q.seeded) chain.push_back(NAV_PULL_GOAL);
    const int n = (int)chain.size() + 1;
    if (cells_out) *cells_out = state == 0 ? n : -n;
    vertices[0] = px; vertices[1] = py;                                 // (M >= 2)
    if (indices) indices[0] = 0;
    int a = 0, count = 1;
    float ax = px, ay = py, x, y;
    length = 0.f;
    while (a < n - 1) {
        const int hi = a + R < n - 1 ? a + R : n - 1;
        int k = hi;
        for (; k > a + 1; k--) {
            nav_pull_point(g, q, chain[k - 1], x, y);
            if (nav_sight(g, ax, ay, x, y)) break;
        }
        nav_pull_point(g, q, chain[k - 1], x, y);
        length = nav_pull_add(length, ax, ay, x, y);
        if (count < M) {
            vertices[2*count] = x; vertices[2*count + 1] = y;
            if (indices) indices[count] = k;
        }
        count++;
        a = k; ax = x; ay = y;
    }
    return state == 0 ? count : -count;
}

// nav_sample_clear without a branch: the four bytes are loaded whatever the sample (from the env's first cells when its block of
// four is not all in range) and the verdict is formed afterwards, so that the loads of several samples can be in flight at once.
__device__ inline bool nav_pull_sample_clear(const NavEnv& g, const float px, const float py, const float dx, const float dy, const int s, const int K) {
    const float t = (float)s/(float)K;
    const float x = px + dx*t, y = py + dy*t;
    long long i0 = 0, j0 = 0;
    const bool anchored = nav_anchor_corner(x, y, g.c, g.jx0, g.iy0, i0, j0);
    const bool inside = anchored & (i0 >= 0) & (i0 + 1 < g.ny) & (j0 >= 0) & (j0 + 1 < g.nx);
    const long long base = inside ? i0*g.nx + j0 : 0;
    const int right = inside ? 1 : 0, up = inside ? g.nx : 0;
    const unsigned char f = g.free[base] & g.free[base + right] & g.free[base + up] & g.free[base + up + right];
    return inside & (f & 1);
}

// nav_sight, the samples four a round (the last round's spare ones test sample K - 1 again): the same verdict - every sample
// clear - with four samples' gathers in flight where nav_sight waits for each sample's before it forms the next.
__device__ inline bool nav_pull_sight(const NavEnv& g, const float px, const float py, const float x, const float y) {
    const float dx = x - px, dy = y - py;
    const int K = nav_sight_samples(g.c, dx, dy);
    if (K < 0) return false;
    for (int s = 1; s < K; s += 4) {
        const int last = K - 1;
        const int clear = (int)nav_pull_sample_clear(g, px, py, dx, dy, s, K) & (int)nav_pull_sample_clear(g, px, py, dx, dy, s + 1 < last ? s + 1 : last, K) &
                          (int)nav_pull_sample_clear(g, px, py, dx, dy, s + 2 < last ? s + 2 : last, K) &
                          (int)nav_pull_sample_clear(g, px, py, dx, dy, s + 3 < last ? s + 3 : last, K);
        if (!clear) return false;
    }
    return true;
}

template <bool WEIGHTED, bool BY_SAMPLE>
__global__ __launch_bounds__(WG) void nav_pull_kernel(const NavArgs a, const NavPullArgs u) {
    extern __shared__ int s_pull[];                                     // WG/64 rings of u.ring ints
    const NavPathArgs& q = u.path;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long at = (long long)blockIdx.x*(WG/64) + wave;
    if (at >= q.total) return;                                          // (uniform: a wave a path)
    if (u.mask && !u.mask[at]) return;                                  // masked out: every output stays as it stands
    int* const ring = s_pull + wave*u.ring;
    const int wrap = u.ring - 1, M = q.max_points, R = u.reach;
    float* const vertices = q.paths + at*M*2;
    int* const indices = u.indices ? u.indices + at*M : nullptr;
    const float2 p = reinterpret_cast<const float2*>(q.points)[at];
    NavEnv g;
    NavGoal goal;
    long long cells;
    float L = INFINITY, leg0 = 0.f;
    int count = 0, n = 0, i = 0, j = 0;                                 // the vertices so far; the chain's points so far
    bool ended = false;
    if (nav_bind<WEIGHTED>(a, q, at, g, goal, cells) && nav_start(g, p.x, p.y, i, j, leg0)) {
        if (lane == 0) {
            vertices[0] = p.x; vertices[1] = p.y;                       // (M >= 2)
            if (indices) indices[0] = 0;
        }
        bool more = true, goal_next = false;                            // points to come, the next of them cell (i, j) - or the goal
        int anchor = 0;
        float ax = p.x, ay = p.y;
        n = 1; count = 1; L = 0.f;
        for (;;) {
            // the chain, up to the window's end: every hop once, its cell into the ring (slot of a point at or below the anchor)
            while (more && n <= anchor + R) {
                if (goal_next) {
                    if (lane == 0) ring[n & wrap] = NAV_PULL_GOAL;
                    n++; more = false; ended = true;
                    break;
                }
                if (lane == 0) ring[n & wrap] = i*g.nx + j;
                n++;
                if (nav_chain_ends(g, goal, i, j)) {
                    if (goal.seeded) { more = false; ended = true; }    // (uniform: the launch's mode)
                    else goal_next = true;
                    continue;
                }
                if (n - 1 > cells) { more = false; break; }             // (nav_path's bound: D falls at every hop)
                // nav_hop's fold, a neighbour a lane: the least value, then the first lane that holds it
                float du = INFINITY, ws, wd;
                nav_hop_weights(g, i, j, ws, wd);                       // (uniform: the cell the wave's hop leaves)
                const float v = lane < 8 ? nav_neighbour(g, i, j, lane, ws, wd, du) : INFINITY;
                float least = v < INFINITY ? v : INFINITY;              // (a NaN is never the least)
                least = fminf(least, __shfl_xor(least, 1));
                least = fminf(least, __shfl_xor(least, 2));
                least = fminf(least, __shfl_xor(least, 4));
                const unsigned long long holders = __ballot((lane < 8) & (v < INFINITY) & (v == least));
                if (!holders) { more = false; break; }                  // broken
                const int t = __ffsll((long long)holders) - 1;
                const float dbest = __shfl(du, t);
                if (!(dbest < g.D[(long long)i*g.nx + j])) { more = false; break; }        // broken
                i += nav_di(t); j += nav_dj(t);
            }
            if (n - 1 == anchor) break;                                 // the anchor is the chain's last point
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // the largest admissible index of the window: anchor + 1 is; any further one the anchor can see
            const int hi = anchor + R < n - 1 ? anchor + R : n - 1;
            int k = anchor + 1;
            if constexpr (BY_SAMPLE) {
                for (int c = hi; c > anchor + 1; c--) {
                    float x, y;
                    nav_pull_point(g, goal, ring[c & wrap], x, y);
                    const float dx = x - ax, dy = y - ay;
                    const int K = nav_sight_samples(g.c, dx, dy);
                    bool sight = K >= 0;
                    for (int s0 = 1; sight && s0 < K; s0 += 64) {
                        const int s = s0 + lane;
                        const bool blocked = s < K && !nav_sample_clear(g, ax, ay, dx, dy, s, K);
                        if (__ballot(blocked)) sight = false;
                    }
                    if (sight) { k = c; break; }
                }
            } else {
                for (int top = hi; top > anchor + 1; top -= 64) {
                    const int c = top - lane;
                    bool sight = false;
                    if (c > anchor + 1) {
                        float x, y;
                        nav_pull_point(g, goal, ring[c & wrap], x, y);
                        sight = nav_pull_sight(g, ax, ay, x, y);
                    }
                    const unsigned long long seen = __ballot(sight);
                    if (seen) { k = top - (__ffsll((long long)seen) - 1); break; }
                }
            }
            float x, y;
            nav_pull_point(g, goal, ring[k & wrap], x, y);              // (uniform)
            L = nav_pull_add(L, ax, ay, x, y);
            if (lane == 0 && count < M) {
                vertices[2*count] = x; vertices[2*count + 1] = y;
                if (indices) indices[count] = k;
            }
            count++;
            anchor = k; ax = x; ay = y;
            __builtin_amdgcn_wave_barrier();                            // (every lane has read before lane 0 writes on)
        }
    }
    for (int k = (count < M ? count : M) + lane; k < M; k += 64) {      // the slots not written
        vertices[2*k] = NAN; vertices[2*k + 1] = NAN;
        if (indices) indices[k] = -1;
    }
    if (lane == 0) {
        q.counts[at] = ended ? count : -count;
        if (u.cells) u.cells[at] = ended ? n : -n;
        u.lengths[at] = L;
    }
}
