// kernels/navbasin.h -- nav_basin_kernel, nav_basin_query_kernel, nav_point_mark_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navpath.h, whose NavEnv,
// nav_seeded, nav_hop and nav_start it follows the fields with; the grid, the relaxed loads and stores, the store rule and the
// settle loop are navfield.h's); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// basins: the seed each cell's path ends on                                 no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavBasins) and DESIGN.md section 3.22: succ(v) is what nav_hop does
// from v on a seeded field's values as they stand; end(v) the seed the chain v, succ(v), ... ends on; label(v) = end(v)'s row-major
// index within the env (ids[end(v)] with ids), -1 on a blocked cell, on a cell whose value is not < +inf and on a cell whose chain
// breaks.  tests/test_navbasin_host.py restates all of it in numpy (basin_rule: chains followed cell by cell).
//
//   nav_basin_kernel    one workgroup per field, nav_region_kernel's shape.  Each lane computes succ for its cells ONCE, from the
//                       field in global memory, through nav_hop itself (basin_succ), and keeps it as an int32 a cell in LDS, N:
//                       a seed names itself; a blocked, unreachable or broken cell holds BASIN_DEAD (-1), which no jump follows.
//                       Then it pointer-jumps IN PLACE, N[k] = N[N[k]] (basin_jump), through relaxed workgroup-scope atomics -
//                       the lanes race, on purpose - one barrier a pass carrying the "something changed" flag
//                       (nav_settle's three rotating slots), until a pass changes nothing.
//                       INVARIANT: read BASIN_DEAD as one more cell at the far end of every broken chain.  Every value a slot
//                       ever holds is a cell of its own chain, at or beyond its successor (succ(k): yes; N[v] for such a v: v is on
//                       k's chain, what v's slot holds is on v's chain at or beyond succ(v), so on k's beyond v, by induction -
//                       whichever of the values v's slot has held the racing load returns), and the value only ever moves DOWN
//                       the chain.  A hop needs a strictly lower D, so the successor graph has no cycle: only a seed names
//                       itself.  THEREFORE a pass that changes nothing saw N[N[k]] == N[k] on every live slot: each names a cell
//                       that names itself - its chain's end, whatever the schedule.  After t passes a slot is
//                       min(2^t, chain length) hops ahead: ceil(log2(longest chain)) + 1 passes at the most.
//                       AFTER the fixed point each cell writes its label (through ids when given), the sizes are counted into at
//                       most 256 LDS counters with integer atomics - one a wave where the wave's cells agree (region_count's
//                       idiom) - the reached cells by shuffles and one atomic a wave, and lanes 0 .. K - 1 store sizes, lane 0
//                       reached and passes: every output element has one writer.  Three instantiations by the LDS they declare
//                       (40, 80, 160 KiB); an env too large for the launch's one runs the same jumps on the `labels` store itself
//                       in global memory - slower, the same result, no scratch.
//   nav_basin_query_kernel   one lane a point: nav_start, then the label under the anchor it picks.
//   nav_point_mark_kernel    one lane a point: a byte store and an integer atomic min on the id of each free anchor cell.
constexpr int BASIN_MAX_IDS = 256;
constexpr int BASIN_DEAD = -1;
constexpr int basin_capacity(const int lds_bytes) { return (lds_bytes - 64)/4 - BASIN_MAX_IDS; }      // cells: an int each, beside the counters

// succ of cell k = (i, j) of env g as a slot's first value: k itself on a seed, the cell nav_hop moves to, BASIN_DEAD where the
// cell is blocked, its value is not < +inf (a NaN too) or no hop leads on.
__host__ __device__ inline int basin_succ(const NavEnv& g, const int k) {
    if (!(g.free[k] & 1) || !(g.D[k] < INFINITY)) return BASIN_DEAD;
    int i = k / g.nx, j = k - i*g.nx;
    const int state = nav_hop(g, nav_seeded(), i, j);
    return state == 1 ? i*g.nx + j : state == 0 ? k : BASIN_DEAD;
}

// What one pass makes of slot k, which holds v: N[v] - v when v is dead already.
__host__ __device__ inline int basin_jump(const int* N, const int v) { return v < 0 ? v : nav_load(N + v); }

// The label of a cell whose slot ended on `end`: -1 dead, the seed's index, or - with ids, the field's store - what it holds there.
__host__ __device__ inline int basin_label(const int end, const int* ids) { return end < 0 ? -1 : ids ? ids[end] : end; }

// Env e's grid with one of its fields, as navpath.h's pieces read them.
__host__ __device__ inline NavEnv basin_env(const NavArgs& a, const int e, const unsigned char* free_cells, const float* D) {
    const NavCells c = nav_cells(a, e);
    return NavEnv{c.jx0, c.iy0, c.nx, c.ny, c.c, free_cells + a.starts[e], D};
}

struct NavBasinArgs {                                // MsNavBasins, checked
    const unsigned char* free_cells;
    const float* fields;                             // the seeded fields' values
    const int* ids;                                  // an int a cell and field, or NULL
    const unsigned char* mask;                       // (N, G) or NULL
    int* labels;
    int* sizes;                                      // (N, G, K) or NULL (K == 0)
    int* reached;                                    // (N, G)
    int* passes;                                     // (N, G) or NULL
    int n_fields, n_ids;
};

// One field, serially (host instantiation only): the kernel's successors, passes, labels and counts with the same pieces - in a
// copy when the env fits `capacity` cells, else in its labels store.
inline void basin_serial_field(const NavArgs& a, const NavBasinArgs& b, const long long field, const int capacity) {
    const int e = (int)(field / b.n_fields), gi = (int)(field - (long long)e*b.n_fields);
    const long long cells = nav_count(a, e);
    int* const sizes = b.n_ids ? b.sizes + field*b.n_ids : nullptr;
    for (int k = 0; k < b.n_ids; k++) sizes[k] = 0;
    int passes = 0, reached = 0;
    if (cells > 0) {
        const long long first = (long long)b.n_fields*a.starts[e] + (long long)gi*cells;
        const NavEnv g = basin_env(a, e, b.free_cells, b.fields + first);
        const int* const ids = b.ids ? b.ids + first : nullptr;
        int* const out = b.labels + first;
        std::vector<int> copy(cells <= capacity ? (size_t)cells : 0);
        int* const N = cells <= capacity ? copy.data() : out;
        const int n = (int)cells;
        for (int k = 0; k < n; k++) N[k] = basin_succ(g, k);
        for (bool changed = true; changed; passes++) {
            changed = false;
            for (int k = 0; k < n; k++) {
                const int v = N[k], w = basin_jump(N, v);
                if (w != v) { nav_store(N + k, w); changed = true; }
            }
        }
        for (int k = 0; k < n; k++) {
            const int label = basin_label(N[k], ids);
            out[k] = label;
            reached += label >= 0;
            if ((label >= 0) & (label < b.n_ids)) sizes[label]++;
        }
    }
    b.reached[field] = reached;
    if (b.passes) b.passes[field] = passes;
}

inline void basin_serial(const NavArgs& a, const NavBasinArgs& b, const int capacity) {
    for (long long field = 0; field < (long long)a.n_envs*b.n_fields; field++)
        if (!b.mask || b.mask[field]) basin_serial_field(a, b, field, capacity);
}

// One cell's share of the sizes: a cell whose label is in 0 .. K - 1 adds one to that counter - one atomic for the wave where all
// of the wave's counting cells in this round agree (a territory), one a lane otherwise.
__device__ inline void basin_count(int* s_size, const int label, const int n_ids) {
    const bool counts = (label >= 0) & (label < n_ids);
    const unsigned long long voters = __ballot(counts);
    if (!counts) return;
    const int first = __builtin_amdgcn_readfirstlane(label);           // (of the lanes that count)
    if (__ballot(label == first) == voters) {
        if ((int)__lane_id() == __ffsll((long long)voters) - 1) __hip_atomic_fetch_add(s_size + first, __popcll(voters), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else
        __hip_atomic_fetch_add(s_size + label, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int LDS_BYTES, int THREADS>
__global__ __launch_bounds__(THREADS) void nav_basin_kernel(const NavArgs a, const NavBasinArgs b) {
    constexpr int CAP = basin_capacity(LDS_BYTES);
    __shared__ int N[CAP];
    __shared__ int s_size[BASIN_MAX_IDS];
    __shared__ int s_flag[3];
    __shared__ int s_reached;
    const int tid = threadIdx.x;
    const long long field = blockIdx.x;                                // (n, g): n G + g
    const int e = (int)(field / b.n_fields), gi = (int)(field - (long long)e*b.n_fields);
    if (b.mask && !b.mask[field]) return;                               // (uniform) left as it is
    const int4 geom = reinterpret_cast<const int4*>(a.geom)[e];
    const int nx = geom.z, ny = geom.w;
    const long long cells = nx > 0 && ny > 0 ? (long long)nx*ny : 0;
    const int K = b.n_ids;
    if (cells <= 0) {
        if (tid < K) b.sizes[field*K + tid] = 0;
        if (tid == 0) {
            b.reached[field] = 0;
            if (b.passes) b.passes[field] = 0;
        }
        return;
    }
    const long long first = (long long)b.n_fields*a.starts[e] + (long long)gi*cells;
    const NavEnv g{geom.x, geom.y, nx, ny, a.cell, b.free_cells + a.starts[e], b.fields + first};
    const int* const ids = b.ids ? b.ids + first : nullptr;
    int* const out = b.labels + first;
    const int n = (int)cells;                                           // (an env has fewer than 2^31 cells: MsNavGrid.max_framed is an int)
    if (tid < 3) s_flag[tid] = 0;
    if (tid == 0) s_reached = 0;
    if (tid < BASIN_MAX_IDS) s_size[tid] = 0;
    int* const slots = cells <= CAP ? N : out;                          // (uniform) in LDS, or where the labels are stored
    for (int k = tid; k < n; k += THREADS) nav_store(slots + k, basin_succ(g, k));
    __syncthreads();
    const int passes = nav_settle<THREADS>(s_flag, n, [=](const int k) {         // the jumps, in LDS or on the labels store
        const int v = nav_load(slots + k), w = basin_jump(slots, v);
        if (w != v) nav_store(slots + k, w);
        return w != v;
    });
    int reached = 0;
    for (int k0 = 0; k0 < n; k0 += THREADS) {                           // (whole waves go round: basin_count ballots)
        const int k = k0 + tid;
        int label = -1;
        if (k < n) {
            label = basin_label(nav_load(slots + k), ids);              // (a slot is read and written by its own lane only from here on)
            out[k] = label;
            reached += label >= 0;
        }
        basin_count(s_size, label, K);
    }
    for (int step = 32; step >= 1; step >>= 1) reached += __shfl_xor(reached, step);
    if ((tid & 63) == 0 && reached) atomicAdd(&s_reached, reached);
    __syncthreads();
    if (tid < K) b.sizes[field*K + tid] = s_size[tid];
    if (tid == 0) {
        b.reached[field] = s_reached;
        if (b.passes) b.passes[field] = passes;
    }
}

struct NavBasinQueryArgs {                           // MsNavBasinQuery, checked
    const float* points;                             // (N, P, 2)
    const int* field;                                // (N, P) or NULL
    const unsigned char* free_cells;
    const float* fields;
    const int* labels;
    int* out;                                        // (N, P)
    int n_points, n_fields;
    long long total;                                 // N P
};

// Point `at` = (e, k): the label under the anchor nav_start picks on the field it asks; -1 without one.
__host__ __device__ inline void basin_query_one(const NavArgs& a, const NavBasinQueryArgs& q, const long long at) {
    const int e = (int)(at / q.n_points), k = (int)(at - (long long)e*q.n_points);
    const long long cells = nav_count(a, e);
    const int f = nav_layer_store(q.field, q.n_fields, at, k);
    int label = -1;
    if ((f >= 0) & (cells > 0)) {
        const long long first = (long long)q.n_fields*a.starts[e] + (long long)f*cells;
        const NavEnv g = basin_env(a, e, q.free_cells, q.fields + first);
        int i = 0, j = 0;
        float leg0;
        if (nav_start(g, q.points[2*at], q.points[2*at + 1], i, j, leg0)) label = q.labels[first + (long long)i*g.nx + j];
    }
    q.out[at] = label;
}

__global__ __launch_bounds__(WG) void nav_basin_query_kernel(const NavArgs a, const NavBasinQueryArgs q) {
    const long long at = (long long)blockIdx.x*WG + threadIdx.x;
    if (at < q.total) basin_query_one(a, q, at);
}

struct NavPointMarkArgs {                            // MsNavPointMarks, checked
    const float* points;                             // (N, P, 2)
    const int* field;                                // (N, P) or NULL
    const int* point_ids;                            // (N, P) or NULL: point k has id k
    const unsigned char* free_cells;
    unsigned char* marks;
    int* ids;
    int n_points, n_fields;
    long long total;                                 // N P
};

// Point `at` = (e, k): every free cell among its four anchors gets mark byte 1 and the least of its id and the point's.
__host__ __device__ inline void point_mark_one(const NavArgs& a, const NavPointMarkArgs& q, const long long at) {
    const int e = (int)(at / q.n_points), k = (int)(at - (long long)e*q.n_points);
    const long long cells = nav_count(a, e);
    const int f = nav_layer_store(q.field, q.n_fields, at, k);
    if ((f < 0) | (cells <= 0)) return;
    const NavCells c = nav_cells(a, e);
    const int nx = c.nx, ny = c.ny;
    long long i0, j0;
    if (!nav_anchor_corner(q.points[2*at], q.points[2*at + 1], c.c, c.jx0, c.iy0, i0, j0)) return;
    const unsigned char* const fr = q.free_cells + a.starts[e];
    const long long first = (long long)q.n_fields*a.starts[e] + (long long)f*cells;
    const int id = q.point_ids ? q.point_ids[at] : k;
    for (int t = 0; t < 4; t++) {
        const long long i = i0 + (t >> 1), j = j0 + (t & 1);
        if ((i >= 0) & (i < ny) & (j >= 0) & (j < nx) && (fr[i*nx + j] & 1)) {
            const long long cell = first + i*nx + j;
            q.marks[cell] = 1;                                          // (two points that share the cell store the same byte)
#if defined(__HIP_DEVICE_COMPILE__)
            __hip_atomic_fetch_min(q.ids + cell, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
            if (id < q.ids[cell]) q.ids[cell] = id;
#endif
        }
    }
}

__global__ __launch_bounds__(WG) void nav_point_mark_kernel(const NavArgs a, const NavPointMarkArgs q) {
    const long long at = (long long)blockIdx.x*WG + threadIdx.x;
    if (at < q.total) point_mark_one(a, q, at);
}
