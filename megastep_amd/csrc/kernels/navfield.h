// kernels/navfield.h -- nav_free_kernel, nav_relax_kernel (single-goal and seeded), nav_query_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after overhead.h: a cell
// is blocked by overhead.h's ov_fold, the very statements of MsOverhead's rule); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// shortest-path distance fields on the floorplans                          no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavGrid) and DESIGN.md section 3.14: a grid of square cells over
// every env's static walls, a cell blocked when a wall comes within the clearance of its centre; free cells joined to their
// free 4-neighbours (weight c) and, where no corner is cut, to their diagonal ones (weight c*1.41421356f); the field of a
// goal is the least fixed point of D[v] = min(D[v], D[u] + w(u, v)) from the goal's anchors.  Every value a cell ever holds
// is the left-to-right binary32 sum along some path and x -> fl(x + w) is monotone, so ANY schedule that stops only when no
// edge can lower anything ends on the same bits.  tests/test_navfield_host.py restates all of it in numpy.
//
//   nav_free_kernel    one lane a cell, the env's static walls staged through LDS a block of WG at a time.
//   nav_relax_kernel   one workgroup per field.  The field lives in LDS (a frame of blocked cells round it, so that no
//                      neighbour needs a bounds check) next to a byte a cell: bit 0 free, bits 1-4 which diagonals are
//                      open.  A pass: every lane relaxes cells tid, tid + T, ... IN PLACE from their eight neighbours -
//                      consecutive lanes read consecutive words whatever the row pitch, so no read or write meets a bank
//                      conflict; the lanes race, on purpose: a cell is written by its own lane only and only ever lowered,
//                      a stale read costs a pass, never a bit.  One barrier a pass carries the "something changed" flag;
//                      the first pass in which no lane lowered anything saw constant values throughout, so no edge can
//                      lower anything: the fixed point.  Then the field is stored once.  Three instantiations by the LDS
//                      they declare (40, 80, 160 KiB: four, two, one workgroup a CU); a field too large for the launch's
//                      one runs the same relaxation on the field in global memory - slower, the same bits.
//                      SEEDED (MsNavSeedFields): the sources are a set of cells at +0.f instead of a goal's
//                      anchors at their legs - the fill, the passes and the store are the single-goal kernel's.
//                      COST (MsNavCostFields), seeded only: the weights of a cell are c and c*1.41421356f times
//                      the cell's own multiplier k_v (nav_cost_multiplier of its cost) - only the per-cell weights differ.  Two
//                      variants of where k_v lives: NAV_COST_GLOBAL reads the cost every pass, by the cell's own lane, and
//                      keeps the seeded kernel's 5 bytes a cell and its tiers; NAV_COST_LDS keeps k_v in LDS beside the value
//                      and the byte, 9 bytes a cell (nav_cost_capacity).  Both give the same bits.
//   nav_query_kernel   one lane a point: the point's (at most four) anchors gathered from its field.
constexpr int NAV_LDS_SMALL = 40*1024, NAV_LDS_MEDIUM = 80*1024, NAV_LDS_LARGE = 160*1024;
constexpr int nav_capacity(const int lds_bytes) { return (lds_bytes - 64)/5/4*4; }      // framed cells: a float and a byte each
constexpr int nav_cost_capacity(const int lds_bytes) { return (lds_bytes - 64)/9/4*4; } // ... and the cell's multiplier, a float
constexpr float NAV_DIAGONAL = 1.41421356f;
constexpr float NAV_COST_MAX = 256.f;
constexpr int NAV_UNWEIGHTED = 0, NAV_COST_GLOBAL = 1, NAV_COST_LDS = 2;       // nav_relax_kernel's COST
constexpr float NAV_INDEX_LIMIT = 1073741824.f;      // |floorf(x/c - .5f)| at or beyond 2^30 (or a NaN): the point has no anchor

struct NavArgs {                                     // MsNavGrid, checked
    const int* geom;                                 // (N, 4) jx0, iy0, nx, ny
    const long long* starts;                         // (N + 1,) first cell of every env
    int n_envs;
    float cell, clearance;
};

// One env's grid as the per-cell pieces read it.
struct NavCells { int jx0, iy0, nx, ny; float c; };
__host__ __device__ inline NavCells nav_cells(const NavArgs& a, const int e) {
    return NavCells{a.geom[4*e], a.geom[4*e + 1], a.geom[4*e + 2], a.geom[4*e + 3], a.cell};
}
// Env e's cells, 0 without any: all that a piece which may have nothing to do reads of the grid before it knows.
__host__ __device__ inline long long nav_count(const NavArgs& a, const int e) {
    const int nx = a.geom[4*e + 2], ny = a.geom[4*e + 3];
    return nx > 0 && ny > 0 ? (long long)nx*ny : 0;
}

__host__ __device__ inline float nav_centre(const int origin, const int k, const float c) { return ((float)(origin + k) + .5f)*c; }
__host__ __device__ inline bool nav_finite(const float v) { return fabsf(v) < INFINITY; }

// The store item k of its env - a view, a draw set, a point, a request; `at` = (n, k) - reads in a layer of n_fields stores
// (MsNavLayer's rule): the one `field` names, else the env's one store or store k; -1: a bad index.
__host__ __device__ inline int nav_layer_store(const int* field, const int n_fields, const long long at, const int k) {
    const int f = field ? field[at] : (n_fields == 1 ? 0 : k);
    return ((f >= 0) & (f < n_fields)) ? f : -1;
}

// The cell (i0, j0) whose centre is the last at or below p on both axes - p's anchors are (i0 + {0, 1}, j0 + {0, 1}); false:
// p has none (NaN, or further out than any grid).
__host__ __device__ inline bool nav_anchor_corner(const float x, const float y, const float c, const int jx0, const int iy0, long long& i0, long long& j0) {
    const float fx = floorf(x/c - .5f), fy = floorf(y/c - .5f);
    if (!(fabsf(fx) < NAV_INDEX_LIMIT) || !(fabsf(fy) < NAV_INDEX_LIMIT)) return false;
    j0 = (long long)fx - jx0; i0 = (long long)fy - iy0;
    return true;
}

__host__ __device__ inline float nav_leg(const float x, const float y, const int jx0, const int iy0, const int i, const int j, const float c) {
    const float dx = x - nav_centre(jx0, j, c), dy = y - nav_centre(iy0, i, c);
    return sqrtf(dx*dx + dy*dy);
}

// Racy by design (see above): relaxed atomics are plain loads and stores that the compiler may not invent, merge or carry
// across passes.  For the fields' floats and for the labels' and successors' ints (navregion.h, navbasin.h).
template <class T>
__host__ __device__ inline T nav_load(const T* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    return *p;                                       // (the host instantiations sweep serially)
#endif
}
template <class T>
__host__ __device__ inline void nav_store(T* p, const T v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    *p = v;
#endif
}

// The settle loop of every kernel that sweeps to a fixed point (the relaxation here, navregion.h's labels, navbasin.h's jumps):
// lane tid takes items tid, tid + T, ... of n, `cell(k)` says whether it changed item k, and the sweeps end with the first that
// changed nothing; returns the passes taken.  One barrier a pass carries the "something changed" flag through three rotating
// slots - a pass sets its own, reads it behind the barrier and clears the next one's, which was last read two barriers ago - and
// makes the workgroup's stores visible to its loads.  s_flag[0..2] start zeroed, behind a barrier.
template <int THREADS, class Index, class Cell>
__device__ inline int nav_settle(int* s_flag, const Index n, const Cell cell) {
    const int tid = threadIdx.x;
    int passes = 0;
    for (;;) {
        if (tid == 0) s_flag[(passes + 1) % 3] = 0;
        bool changed = false;
        for (Index k = tid; k < n; k += THREADS)
            if (cell(k)) changed = true;
        if (changed) s_flag[passes % 3] = 1;
        __syncthreads();
        const int again = s_flag[passes % 3];
        passes++;
        if (!again) return passes;                                      // (uniform)
    }
}

__global__ __launch_bounds__(WG) void nav_free_kernel(const MsScenery sc, const NavArgs a, unsigned char* free_cells) {
    __shared__ float4 s_rows[WG];
    const int e = blockIdx.y, tid = threadIdx.x;
    const int4 g = reinterpret_cast<const int4*>(a.geom)[e];
    const long long cells = (long long)g.z*g.w;
    const long long k = (long long)blockIdx.x*WG + tid;
    if ((long long)blockIdx.x*WG >= cells) return;                      // (uniform: the grid is sized for the largest env)
    const bool live = k < cells;
    const int i = live ? (int)(k / g.z) : 0, j = live ? (int)(k - (long long)i*g.z) : 0;
    const float x = nav_centre(g.x, j, a.cell), y = nav_centre(g.y, i, a.cell);
    const float h2 = a.clearance*a.clearance;
    const int AF = sc.n_agents*sc.n_model;
    const int L = sc.lines_widths[e];
    const float4* const rows = reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[e];
    OvBest best{INFINITY, INT_MAX, 0.f};
    for (int l0 = AF; l0 < L; l0 += WG) {
        if (l0 + tid < L) s_rows[tid] = rows[l0 + tid];
        __syncthreads();
        const int count = min(WG, L - l0);
        for (int q = 0; q < count; q++) ov_fold(x, y, s_rows[q], l0 + q, h2, best);
        __syncthreads();
    }
    if (live) free_cells[a.starts[e] + k] = best.idx == INT_MAX ? 1 : 0;
}

struct NavFieldArgs {
    const float* goals;                              // (N, G, 2); NULL for seeded fields
    const unsigned char* mask;                       // (N, G) or NULL
    const unsigned char* free_cells;
    float* fields;
    int* passes;                                     // (N, G) or NULL: passes the field took (0: masked out)
    int n_goals;
    const unsigned char* marks;                      // seeded fields only: a byte a cell and field, the fields' layout
    const unsigned char* among;                      //   a byte a cell (free_cells' layout) or NULL
    int where;                                       //   0 or 1: the value of a seed's mark
    int* n_seeds;                                    //   (N, G) or NULL: the seeds of every computed field
    const float* costs;                              // cost fields only: a float a cell, free_cells' layout (n_costs 1) or the
    int n_costs;                                     //   fields' (n_costs n_goals)
};

// The per-cell pieces of the relaxation are __host__ __device__ functions over plain pointers: ms_host_nav_seed_field sweeps
// them over host arrays, so the CPU suite holds this very text to the rule (tests/test_navseed_host.py).

// The lowered value of a cell from its neighbours' (the min first, one addition per weight: x -> fl(x + w) is monotone, so
// fl(min + w) is the min of the sums).
__host__ __device__ inline float nav_relaxed(const float d, const float straight, const float diagonal, const float ws, const float wd) {
    return fminf(d, fminf(straight + ws, diagonal + wd));
}

// The multiplier of a cell from its cost (MsNavCostFields): below 1 counts as 1, above NAV_COST_MAX - +inf too - as that, and a
// NaN is the dearest, not the cheapest.
__host__ __device__ inline float nav_cost_multiplier(const float x) { return x >= 1.f ? fminf(x, NAV_COST_MAX) : (x < 1.f ? 1.f : NAV_COST_MAX); }

// The weights of a step out of a cell of multiplier k towards the seeds: fl(c k) straight, fl(fl(c 1.41421356f) k) diagonal -
// times 1.f is exact, so k = 1 gives the unweighted weights' bits.
__host__ __device__ inline void nav_cost_weights(const float c, const float k, float& ws, float& wd) { ws = c*k; wd = (c*NAV_DIAGONAL)*k; }

// Is cell k of its env a seed (MsNavSeedFields): free, among the cells that may be one, its mark's bit 0 equal to `where`.
__host__ __device__ inline bool nav_is_seed(const unsigned char* fr, const unsigned char* among, const unsigned char* marks, const long long k,
                                            const int where) {
    return (fr[k] & 1) && (!among || (among[k] & 1)) && (marks[k] & 1) == where;
}

// The framed field (row pitch P = nx + 2, a ring of blocked cells round the env's): bit 0 of framed cell k, and the cell of
// the env it stands for (-1: the frame).
__host__ __device__ inline int nav_frame_free(const unsigned char* fr, const int nx, const int ny, const int P, const int k, long long& cell) {
    const int i = k / P - 1, j = k - (i + 1)*P - 1;
    const bool inside = (i >= 0) & (i < ny) & (j >= 0) & (j < nx);
    cell = inside ? (long long)i*nx + j : -1;
    return inside ? fr[cell] & 1 : 0;
}

// Bits 0-4 of a free framed cell's byte: which diagonals are open - neither corner is cut.  Reads bit 0 of the neighbours only.
__host__ __device__ inline int nav_frame_open(const unsigned char* s_m, const int k, const int P) {
    const int N_ = s_m[k - P] & 1, S_ = s_m[k + P] & 1, W_ = s_m[k - 1] & 1, E_ = s_m[k + 1] & 1;
    return 1 | ((N_ & W_ & s_m[k - P - 1]) << 1) | ((N_ & E_ & s_m[k - P + 1]) << 2) | ((S_ & W_ & s_m[k + P - 1]) << 3) |
           ((S_ & E_ & s_m[k + P + 1]) << 4);
}

// What one relaxation makes of free cell k (value d, byte m) of the framed field, from its eight neighbours; a neighbour that
// does not count is never read as less than +inf (a blocked one holds +inf, a closed diagonal is skipped).
__host__ __device__ inline float nav_cell_framed(const float* s_d, const int m, const int k, const int P, const float d, const float ws, const float wd) {
    const float st = fminf(fminf(nav_load(s_d + k - 1), nav_load(s_d + k + 1)), fminf(nav_load(s_d + k - P), nav_load(s_d + k + P)));
    const float nw = m & 2 ? nav_load(s_d + k - P - 1) : INFINITY, ne = m & 4 ? nav_load(s_d + k - P + 1) : INFINITY;
    const float sw = m & 8 ? nav_load(s_d + k + P - 1) : INFINITY, se = m & 16 ? nav_load(s_d + k + P + 1) : INFINITY;
    return nav_relaxed(d, st, fminf(fminf(nw, ne), fminf(sw, se)), ws, wd);
}

// The same of free cell k (value d) of the field as it is stored: nx x ny, no frame, every neighbour bounds-checked.
__host__ __device__ inline float nav_cell_stored(const float* out, const unsigned char* fr, const int nx, const int ny, const long long k, const float d,
                                                 const float ws, const float wd) {
    const int i = (int)(k / nx), j = (int)(k - (long long)i*nx);
    const bool up = i > 0, down = i < ny - 1, left = j > 0, right = j < nx - 1;
    const bool N_ = up && (fr[k - nx] & 1), S_ = down && (fr[k + nx] & 1), W_ = left && (fr[k - 1] & 1), E_ = right && (fr[k + 1] & 1);
    const float st = fminf(fminf(W_ ? nav_load(out + k - 1) : INFINITY, E_ ? nav_load(out + k + 1) : INFINITY),
                           fminf(N_ ? nav_load(out + k - nx) : INFINITY, S_ ? nav_load(out + k + nx) : INFINITY));
    const float nw = N_ && W_ && (fr[k - nx - 1] & 1) ? nav_load(out + k - nx - 1) : INFINITY;
    const float ne = N_ && E_ && (fr[k - nx + 1] & 1) ? nav_load(out + k - nx + 1) : INFINITY;
    const float sw = S_ && W_ && (fr[k + nx - 1] & 1) ? nav_load(out + k + nx - 1) : INFINITY;
    const float se = S_ && E_ && (fr[k + nx + 1] & 1) ? nav_load(out + k + nx + 1) : INFINITY;
    return nav_relaxed(d, st, fminf(fminf(nw, ne), fminf(sw, se)), ws, wd);
}

// SEEDED: the field's sources are the cells nav_is_seed names (value +0.f) instead of a goal's anchors (value: their leg).  A
// seed keeps bit 5 of its byte; the seeds are counted a wave at a time - one ballot a round, one LDS atomic a wave - into
// s_flag[3].
template <int LDS_BYTES, int THREADS, bool SEEDED, int COST = NAV_UNWEIGHTED>
__global__ __launch_bounds__(THREADS) void nav_relax_kernel(const NavArgs a, const NavFieldArgs f) {
    static_assert(SEEDED || COST == NAV_UNWEIGHTED, "cost fields are seeded fields");
    constexpr int CAP = COST == NAV_COST_LDS ? nav_cost_capacity(LDS_BYTES) : nav_capacity(LDS_BYTES);
    constexpr int FLAGS = SEEDED ? 4 : 3;
    __shared__ float s_d[CAP];
    __shared__ float s_k[COST == NAV_COST_LDS ? CAP : 1];               // (NAV_COST_LDS alone touches it)
    __shared__ unsigned char s_m[CAP];
    __shared__ int s_flag[FLAGS];
    const int tid = threadIdx.x;
    const long long field = blockIdx.x;                                // (n, g): n G + g
    const int e = (int)(field / f.n_goals), gi = (int)(field - (long long)e*f.n_goals);
    if (f.mask && !f.mask[field]) return;                               // (uniform) left as it is
    const int4 g = reinterpret_cast<const int4*>(a.geom)[e];
    const int nx = g.z, ny = g.w;
    const long long cells = (long long)nx*ny;
    if (cells <= 0) {
        if (f.passes && tid == 0) f.passes[field] = 0;
        if (SEEDED && f.n_seeds && tid == 0) f.n_seeds[field] = 0;
        return;
    }
    const unsigned char* const fr = f.free_cells + a.starts[e];
    const long long first = (long long)f.n_goals*a.starts[e] + (long long)gi*cells;
    float* const out = f.fields + first;
    const unsigned char* const marks = SEEDED ? f.marks + first : nullptr;
    const unsigned char* const among = SEEDED && f.among ? f.among + a.starts[e] : nullptr;
    const float* const cost = COST != NAV_UNWEIGHTED ? f.costs + (f.n_costs == 1 ? a.starts[e] : first) : nullptr;
    const float c = a.cell, ws = c, wd = c*NAV_DIAGONAL;
    float2 p = make_float2(0.f, 0.f);
    long long i0 = 0, j0 = 0;
    bool anchored = false;
    if constexpr (!SEEDED) {
        p = reinterpret_cast<const float2*>(f.goals)[field];
        anchored = nav_anchor_corner(p.x, p.y, c, g.x, g.y, i0, j0);
    }
    const long long framed = (long long)(nx + 2)*(ny + 2);
    int passes = 0, seeds = 0;

    if (framed <= CAP) {
        const int P = nx + 2, n = (int)framed;
        for (int k = tid; k < n; k += THREADS) {
            long long cell;
            const int fb = nav_frame_free(fr, nx, ny, P, k, cell);
            bool seed = false;
            if constexpr (SEEDED) seed = fb && nav_is_seed(fr, among, marks, cell, f.where);
            s_d[k] = seed ? 0.f : INFINITY;
            s_m[k] = (unsigned char)(fb | (seed ? 32 : 0));
            if constexpr (COST == NAV_COST_LDS) s_k[k] = fb ? nav_cost_multiplier(cost[cell]) : 1.f;
        }
        if (tid < FLAGS) s_flag[tid] = 0;
        __syncthreads();
        for (int k = tid; k < n; k += THREADS) {                       // which diagonals are open: neither corner is cut
            const int m = s_m[k];
            if (m & 1) s_m[k] = (unsigned char)(nav_frame_open(s_m, k, P) | (m & 32));      // (bit 0, all a neighbour reads, does not change)
            if constexpr (SEEDED) seeds += __popcll(__ballot(m & 32)); // (lane 0 has its wave's lowest k: it is in every round its wave is)
        }
        if constexpr (SEEDED) {
            if ((tid & 63) == 0 && seeds) atomicAdd(&s_flag[3], seeds);
        } else if (anchored && tid < 4) {
            const long long i = i0 + (tid >> 1), j = j0 + (tid & 1);
            if ((i >= 0) & (i < ny) & (j >= 0) & (j < nx)) {
                const int k = ((int)i + 1)*P + (int)j + 1;
                if (s_m[k] & 1) s_d[k] = nav_leg(p.x, p.y, g.x, g.y, (int)i, (int)j, c);
            }
        }
        __syncthreads();
        passes = nav_settle<THREADS>(s_flag, n, [=](const int k) {
            const int m = s_m[k];
            if (!(m & 1)) return false;
            float w_s = ws, w_d = wd;
            if constexpr (COST == NAV_COST_LDS) nav_cost_weights(c, s_k[k], w_s, w_d);
            if constexpr (COST == NAV_COST_GLOBAL) {
                const int i = k / P - 1, j = k - (i + 1)*P - 1;         // (a free framed cell is inside)
                nav_cost_weights(c, nav_cost_multiplier(cost[(long long)i*nx + j]), w_s, w_d);
            }
            const float d = nav_load(s_d + k), v = nav_cell_framed(s_d, m, k, P, d, w_s, w_d);
            if (v < d) nav_store(s_d + k, v);
            return v < d;
        });
        for (long long k = tid; k < cells; k += THREADS) {
            const int i = (int)(k / nx), j = (int)(k - (long long)i*nx);
            out[k] = s_d[(i + 1)*P + j + 1];
        }
    } else {
        // the same relaxation on the field where it is stored
        for (long long k = tid; k < cells; k += THREADS) {
            bool seed = false;
            if constexpr (SEEDED) {
                seed = nav_is_seed(fr, among, marks, k, f.where);
                seeds += __popcll(__ballot(seed));
            }
            out[k] = seed ? 0.f : INFINITY;
        }
        if (tid < FLAGS) s_flag[tid] = 0;
        __syncthreads();
        if constexpr (SEEDED) {
            if ((tid & 63) == 0 && seeds) atomicAdd(&s_flag[3], seeds);
        } else if (anchored && tid < 4) {
            const long long i = i0 + (tid >> 1), j = j0 + (tid & 1);
            if ((i >= 0) & (i < ny) & (j >= 0) & (j < nx) && (fr[i*nx + j] & 1)) out[i*nx + j] = nav_leg(p.x, p.y, g.x, g.y, (int)i, (int)j, c);
        }
        __syncthreads();
        passes = nav_settle<THREADS>(s_flag, cells, [=](const long long k) {
            if (!(fr[k] & 1)) return false;
            float w_s = ws, w_d = wd;
            if constexpr (COST != NAV_UNWEIGHTED) nav_cost_weights(c, nav_cost_multiplier(cost[k]), w_s, w_d);
            const float d = nav_load(out + k), v = nav_cell_stored(out, fr, nx, ny, k, d, w_s, w_d);
            if (v < d) nav_store(out + k, v);
            return v < d;
        });
    }
    if (f.passes && tid == 0) f.passes[field] = passes;
    if (SEEDED && f.n_seeds && tid == 0) f.n_seeds[field] = s_flag[FLAGS - 1];
}

struct NavQueryArgs {
    const float* points;                             // (N, P, 2)
    const int* goal;                                 // (N, P) or NULL
    const float* fields;
    float* out;                                      // (N, P)
    int n_points, n_goals;
    long long total;                                 // N P
};

__global__ __launch_bounds__(WG) void nav_query_kernel(const NavArgs a, const NavQueryArgs q) {
    const long long at = (long long)blockIdx.x*WG + threadIdx.x;
    if (at >= q.total) return;
    const int e = (int)(at / q.n_points), k = (int)(at - (long long)e*q.n_points);
    const int gi = q.goal ? q.goal[at] : k;
    const int4 g = reinterpret_cast<const int4*>(a.geom)[e];
    const int nx = g.z, ny = g.w;
    const long long cells = (long long)nx*ny;
    float best = INFINITY;
    const float2 p = reinterpret_cast<const float2*>(q.points)[at];
    long long i0, j0;
    if ((gi >= 0) & (gi < q.n_goals) && cells > 0 && nav_anchor_corner(p.x, p.y, a.cell, g.x, g.y, i0, j0)) {
        const float* const D = q.fields + (long long)q.n_goals*a.starts[e] + (long long)gi*cells;
        for (int t = 0; t < 4; t++) {
            const long long i = i0 + (t >> 1), j = j0 + (t & 1);
            if ((i >= 0) & (i < ny) & (j >= 0) & (j < nx)) {
                const float d = D[i*nx + j];                            // (+inf on a blocked cell: it is no anchor)
                if (d < INFINITY) best = fminf(best, d + nav_leg(p.x, p.y, g.x, g.y, (int)i, (int)j, a.cell));
            }
        }
    }
    q.out[at] = best;
}
