// kernels/navregion.h -- nav_region_kernel, nav_region_query_kernel, nav_region_mask_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navfield.h, whose
// NavArgs, NavCells, nav_is_seed, nav_anchor_corner, nav_load / nav_store, nav_layer_store and settle loop it shares); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// regions: the connected spaces of the nav grid, labelled                   no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavRegions) and DESIGN.md section 3.20: a cell is OPEN when it is
// free (or, with marks, when nav_is_seed holds on it); open cells are joined to their open 4-neighbours; a cell's label is the
// least row-major index of an open cell of its component (-1 on a closed cell), its area the component's cell count times c*c.
// tests/test_navregion_host.py restates all of it in numpy (region_rule: a flood fill).
//
//   nav_region_kernel   one workgroup per regions field, nav_relax_kernel's shape.  The labels live in LDS as int32 with a frame
//                       of closed cells round them (row pitch P = nx + 2), so that no neighbour needs a bounds check; a closed
//                       cell holds INT_MAX, which a min never takes; an open cell starts at its own framed index - framed and
//                       stored row-major orders agree, so the least framed index is the least stored one.  A pass: lane tid
//                       takes cells tid, tid + T, ... IN PLACE: v = min(own, the four neighbours), then JUMPS v = L[v] until
//                       that lowers nothing more; if v is lower it goes, by an integer atomic min, into the cell's slot AND into
//                       the slot of the cell its old value named (the root its neighbourhood had agreed on hears at once, and
//                       every cell that jumps to it with it) - consecutive lanes read consecutive words whatever the pitch (no
//                       bank conflict; the jump's reads land where they land, mostly on one word - a broadcast).  The lanes
//                       race, on purpose, through relaxed atomics.
//                       INVARIANT: every value a cell ever holds is the index of an open cell of its own component, is never
//                       larger than the cell's own index and is only ever lowered (own index: yes; a neighbour's value: the
//                       neighbour is in the component, so is what it holds, by induction; L[v] for such a v: likewise; a value
//                       written into the slot the old value `own` names is below `own`, that slot's index; a min never raises).  THEREFORE a pass that lowers nothing saw constant values throughout, each
//                       cell's at most its neighbours': every component is constant, at a value m that is one of its cells and
//                       at most the index of every cell of it - its least index, whatever the schedule.  The jump is what turns
//                       a corridor's hundreds of passes into a handful: a lowered label is handed on through L, not cell by cell.
//                       One barrier a pass carries the "something changed" flag (nav_settle's three rotating slots).
//                       AFTER the fixed point the sizes are counted IN PLACE: a root (L[k] == k) turns its slot into -1, every
//                       other open cell subtracts one from its root's slot - an integer LDS atomic, one a wave where the wave's
//                       cells share a root - so that a root's slot holds -(cells of its component) and every other slot still
//                       names its root; then each cell writes its label and area, and the lanes' region counts, open cells and
//                       largest key (cells << 32 | INT_MAX - label: most cells, then least label) meet by shuffles and one LDS
//                       atomic a wave.  Integer atomics only; every output element has one writer.  Three instantiations by
//                       the LDS they declare (40, 80, 160 KiB); a field too large for the launch's one runs the same
//                       propagation and the same count on the `labels` store itself in global memory - slower, the same bits,
//                       no scratch.
//   nav_region_query_kernel   one lane a point: the labels under the point's four anchors.
//   nav_region_mask_kernel    blockIdx.x a request (n, p), blockIdx.y a run of WG cells (nav_window_kernel's geometry, strided
//                       over y where an env has more cells than the launch has lanes): a lane a cell, a wave's loads of the
//                       labels and stores of the bytes contiguous; every byte of the store is written, the zeros too.
constexpr int region_capacity(const int lds_bytes) { return (lds_bytes - 64)/4; }      // framed cells: an int each

// Is cell k of its env open: free (marks NULL), or a seed of MsNavSeedFields' rule - nav_is_seed, the very function.
__host__ __device__ inline bool region_open(const unsigned char* fr, const unsigned char* among, const unsigned char* marks, const long long k,
                                            const int where) {
    return marks ? nav_is_seed(fr, among, marks, k, where) : (fr[k] & 1) != 0;
}

__host__ __device__ inline int region_min(const int a, const int b) { return a < b ? a : b; }

// What a cell starts at: its own index when open, INT_MAX (no min takes it) when closed.
__host__ __device__ inline int region_fill(const bool open, const int index) { return open ? index : INT_MAX; }

// v, jumped: L[v], L[L[v]], ... while that lowers (v is an open cell's index; the values only fall, so this ends).
__host__ __device__ inline int region_jump(const int* L, int v) {
    for (;;) {
        const int w = nav_load(L + v);
        if (w >= v) return v;
        v = w;
    }
}

// What one pass makes of open cell k (value own) of the framed labels: the least of its own and its four neighbours', jumped.
__host__ __device__ inline int region_lowered_framed(const int* L, const int k, const int P, const int own) {
    const int v = region_min(region_min(own, region_min(nav_load(L + k - 1), nav_load(L + k + 1))),
                             region_min(nav_load(L + k - P), nav_load(L + k + P)));
    return region_jump(L, v);
}

// The same of open cell k of the labels as they are stored: nx x ny, no frame, every neighbour bounds-checked (rows do not wrap).
__host__ __device__ inline int region_lowered_stored(const int* L, const int nx, const int ny, const long long k, const int own) {
    const int i = (int)(k / nx), j = (int)(k - (long long)i*nx);
    int v = own;
    if (j > 0) v = region_min(v, nav_load(L + k - 1));
    if (j < nx - 1) v = region_min(v, nav_load(L + k + 1));
    if (i > 0) v = region_min(v, nav_load(L + k - nx));
    if (i < ny - 1) v = region_min(v, nav_load(L + k + nx));
    return region_jump(L, v);
}

// Cell k held `own` and found v < own: k's slot is lowered to v - and so is the slot of the cell `own` names, the root k's
// neighbourhood had agreed on: without that a lower label creeps one cell a pass up a branch whose cells already share a root
// (they all jump to it, and it has not heard).  Both by an integer atomic min: two lanes may lower one slot, and neither may raise it.
__host__ __device__ inline void region_lower(int* L, const long long k, const int own, const int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_fetch_min(L + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_min(L + own, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    if (v < L[k]) L[k] = v;
    if (v < L[own]) L[own] = v;
#endif
}

// The stored index of framed cell v (pitch P = nx + 2), and back.
__host__ __device__ inline int region_unframe(const int v, const int P, const int nx) { const int i = v / P; return (i - 1)*nx + (v - i*P - 1); }

// After the fixed point and the count: the slot of cell `index` holds `held` - INT_MAX closed, -(cells) on a root, else its root,
// whose slot holds `at_root`.  Its label (an index of L's kind; -1 closed) and its component's cells (0 closed).
__host__ __device__ inline bool region_is_root(const int held, const int index) { return held == index; }
__host__ __device__ inline int region_label(const int held, const int index) { return held == INT_MAX ? -1 : held < 0 ? index : held; }
__host__ __device__ inline int region_cells(const int held, const int at_root) { return held == INT_MAX ? 0 : held < 0 ? -held : -at_root; }

__host__ __device__ inline float region_area(const int cells, const float c) { return cells > 0 ? (float)cells*(c*c) : 0.f; }

// Most cells first, then the least label: the greatest key wins; 0: no region.
__host__ __device__ inline unsigned long long region_key(const int cells, const int label) {
    return ((unsigned long long)(unsigned)cells << 32) | (unsigned)(INT_MAX - label);
}
__host__ __device__ inline int region_key_label(const unsigned long long key) { return key ? INT_MAX - (int)(unsigned)(key & 0xffffffffull) : -1; }
__host__ __device__ inline int region_key_cells(const unsigned long long key) { return (int)(key >> 32); }

// The labels under the four anchors of (x, y), in the order i0 + (t>>1), j0 + (t&1); -1 outside the grid and on a closed cell
// (which holds -1).  `labels`: the field's store, or NULL (a bad field index, an env without cells): all -1.
__host__ __device__ inline void region_anchor_labels(const int* labels, const NavCells& g, const float x, const float y, int out[4]) {
    out[0] = out[1] = out[2] = out[3] = -1;
    long long i0, j0;
    if (!labels || !nav_anchor_corner(x, y, g.c, g.jx0, g.iy0, i0, j0)) return;
    for (int t = 0; t < 4; t++) {
        const long long i = i0 + (t >> 1), j = j0 + (t & 1);
        if ((i >= 0) & (i < g.ny) & (j >= 0) & (j < g.nx)) out[t] = labels[i*g.nx + j];
    }
}

__host__ __device__ inline unsigned char region_mask_byte(const int label, const int w[4]) {
    return ((label >= 0) & ((label == w[0]) | (label == w[1]) | (label == w[2]) | (label == w[3]))) ? 1 : 0;
}

struct NavRegionArgs {                               // MsNavRegions, checked
    const unsigned char* free_cells;
    const unsigned char* marks;                      // a byte a cell and field, or NULL: the free cells
    const unsigned char* among;                      // a byte a cell, or NULL
    const unsigned char* mask;                       // (N, G) or NULL
    int* labels;
    float* areas;
    int* counts;                                     // (N, G) each
    int* open_cells;
    int* largest;
    int* largest_cells;
    int* passes;                                     // (N, G) or NULL
    int n_fields, where;
};

struct RegionSums { int regions, open; unsigned long long key; };

// What cell `index` (slot `held`, its root's slot `at_root`) adds to its lane's sums.
__host__ __device__ inline void region_sum(RegionSums& s, const int held, const int cells, const int label) {
    if (held == INT_MAX) return;
    s.open++;
    if (held < 0) {
        s.regions++;
        const unsigned long long key = region_key(cells, label);
        if (key > s.key) s.key = key;
    }
}

// One field, serially (host instantiation only): the kernel's fill, passes, count and stores with the same pieces - framed when
// the field fits `capacity` framed cells, else on the labels as they are stored.
inline void region_serial_field(const NavArgs& a, const NavRegionArgs& r, const long long field, const int capacity) {
    const int e = (int)(field / r.n_fields), gi = (int)(field - (long long)e*r.n_fields);
    const NavCells g = nav_cells(a, e);
    const int nx = g.nx, ny = g.ny;
    const long long cells = nx > 0 && ny > 0 ? (long long)nx*ny : 0;
    RegionSums s{0, 0, 0ull};
    int passes = 0;
    if (cells > 0) {
        const unsigned char* const fr = r.free_cells + a.starts[e];
        const long long first = (long long)r.n_fields*a.starts[e] + (long long)gi*cells;
        const unsigned char* const marks = r.marks ? r.marks + first : nullptr;
        const unsigned char* const among = r.marks && r.among ? r.among + a.starts[e] : nullptr;
        int* const out = r.labels + first;
        float* const areas = r.areas + first;
        const long long framed = (long long)(nx + 2)*(ny + 2);
        if (framed <= capacity) {
            const int P = nx + 2, n = (int)framed;
            std::vector<int> L(n);
            for (int k = 0; k < n; k++) {
                long long cell;
                nav_frame_free(fr, nx, ny, P, k, cell);
                L[k] = region_fill(cell >= 0 && region_open(fr, among, marks, cell, r.where), k);
            }
            for (bool changed = true; changed; passes++) {
                changed = false;
                for (int k = 0; k < n; k++) {
                    const int own = L[k];
                    if (own == INT_MAX) continue;
                    const int v = region_lowered_framed(L.data(), k, P, own);
                    if (v < own) { region_lower(L.data(), k, own, v); changed = true; }
                }
            }
            for (int k = 0; k < n; k++) if (region_is_root(L[k], k)) L[k] = -1;
            for (int k = 0; k < n; k++) if (L[k] >= 0 && L[k] != INT_MAX) L[L[k]] -= 1;
            for (long long k = 0; k < cells; k++) {
                const int f = (int)(k / nx + 1)*P + (int)(k % nx) + 1, held = L[f];
                const int at = region_label(held, f), n_cells = region_cells(held, held >= 0 && held != INT_MAX ? L[held] : 0);
                const int label = at < 0 ? -1 : region_unframe(at, P, nx);
                out[k] = label;
                areas[k] = region_area(n_cells, a.cell);
                region_sum(s, held, n_cells, label);
            }
        } else {
            for (long long k = 0; k < cells; k++) out[k] = region_fill(region_open(fr, among, marks, k, r.where), (int)k);
            for (bool changed = true; changed; passes++) {
                changed = false;
                for (long long k = 0; k < cells; k++) {
                    const int own = out[k];
                    if (own == INT_MAX) continue;
                    const int v = region_lowered_stored(out, nx, ny, k, own);
                    if (v < own) { region_lower(out, k, own, v); changed = true; }
                }
            }
            for (long long k = 0; k < cells; k++) if (region_is_root(out[k], (int)k)) out[k] = -1;
            for (long long k = 0; k < cells; k++) if (out[k] >= 0 && out[k] != INT_MAX) out[out[k]] -= 1;
            for (long long k = 0; k < cells; k++) {
                const int held = out[k];
                const int label = region_label(held, (int)k), n_cells = region_cells(held, held >= 0 && held != INT_MAX ? out[held] : 0);
                areas[k] = region_area(n_cells, a.cell);
                region_sum(s, held, n_cells, label);
            }
            for (long long k = 0; k < cells; k++) out[k] = region_label(out[k], (int)k);
        }
    }
    r.counts[field] = s.regions;
    r.open_cells[field] = s.open;
    r.largest[field] = region_key_label(s.key);
    r.largest_cells[field] = region_key_cells(s.key);
    if (r.passes) r.passes[field] = passes;
}

inline void region_serial(const NavArgs& a, const NavRegionArgs& r, const int capacity) {
    for (long long field = 0; field < (long long)a.n_envs*r.n_fields; field++)
        if (!r.mask || r.mask[field]) region_serial_field(a, r, field, capacity);
}

// One cell's share of the count: a cell that is no root takes one off its root's slot - one atomic for the wave where all of
// the wave's cells in this round share a root (a room), one a lane otherwise.
__device__ inline void region_count(int* L, const int held) {
    const bool counts = (held >= 0) & (held != INT_MAX);
    const unsigned long long voters = __ballot(counts);
    if (!counts) return;
    const int first = __builtin_amdgcn_readfirstlane(held);            // (of the lanes that count)
    if (__ballot(held == first) == voters) {
        if ((int)__lane_id() == __ffsll((long long)voters) - 1) __hip_atomic_fetch_sub(L + first, __popcll(voters), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else
        __hip_atomic_fetch_sub(L + held, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The lanes' sums into s_sum[0] (regions), s_sum[1] (open cells) and s_key: shuffles within the wave, then one atomic a wave.
__device__ inline void region_reduce(RegionSums s, int* s_sum, unsigned long long* s_key) {
    for (int step = 32; step >= 1; step >>= 1) {
        s.regions += __shfl_xor(s.regions, step);
        s.open += __shfl_xor(s.open, step);
        const unsigned long long other = __shfl_xor(s.key, step);
        if (other > s.key) s.key = other;
    }
    if ((threadIdx.x & 63) == 0) {
        if (s.regions) atomicAdd(s_sum, s.regions);
        if (s.open) atomicAdd(s_sum + 1, s.open);
        if (s.key) atomicMax(s_key, s.key);
    }
}

template <int LDS_BYTES, int THREADS>
__global__ __launch_bounds__(THREADS) void nav_region_kernel(const NavArgs a, const NavRegionArgs r) {
    constexpr int CAP = region_capacity(LDS_BYTES);
    __shared__ int L[CAP];
    __shared__ int s_flag[3];
    __shared__ int s_sum[2];
    __shared__ unsigned long long s_key;
    const int tid = threadIdx.x;
    const long long field = blockIdx.x;                                // (n, g): n G + g
    const int e = (int)(field / r.n_fields), gi = (int)(field - (long long)e*r.n_fields);
    if (r.mask && !r.mask[field]) return;                               // (uniform) left as it is
    const int4 g = reinterpret_cast<const int4*>(a.geom)[e];
    const int nx = g.z, ny = g.w;
    const long long cells = nx > 0 && ny > 0 ? (long long)nx*ny : 0;
    if (cells <= 0) {
        if (tid == 0) {
            r.counts[field] = 0; r.open_cells[field] = 0; r.largest[field] = -1; r.largest_cells[field] = 0;
            if (r.passes) r.passes[field] = 0;
        }
        return;
    }
    const unsigned char* const fr = r.free_cells + a.starts[e];
    const long long first = (long long)r.n_fields*a.starts[e] + (long long)gi*cells;
    const unsigned char* const marks = r.marks ? r.marks + first : nullptr;
    const unsigned char* const among = r.marks && r.among ? r.among + a.starts[e] : nullptr;
    int* const out = r.labels + first;
    float* const areas = r.areas + first;
    const long long framed = (long long)(nx + 2)*(ny + 2);
    if (tid < 3) s_flag[tid] = 0;
    if (tid < 2) s_sum[tid] = 0;
    if (tid == 0) s_key = 0ull;
    RegionSums s{0, 0, 0ull};
    int passes;

    if (framed <= CAP) {
        const int P = nx + 2, n = (int)framed;
        for (int k = tid; k < n; k += THREADS) {
            long long cell;
            nav_frame_free(fr, nx, ny, P, k, cell);
            L[k] = region_fill(cell >= 0 && region_open(fr, among, marks, cell, r.where), k);
        }
        __syncthreads();
        passes = nav_settle<THREADS>(s_flag, n, [=](const int k) {
            const int own = nav_load(L + k);
            if (own == INT_MAX) return false;
            const int v = region_lowered_framed(L, k, P, own);
            if (v < own) region_lower(L, k, own, v);
            return v < own;
        });
        // the count, in place: roots to -1, the others take one off their root's, behind a barrier each
        for (int k = tid; k < n; k += THREADS)
            if (region_is_root(L[k], k)) L[k] = -1;
        __syncthreads();
        for (int k = tid; k < n; k += THREADS) region_count(L, L[k]);
        __syncthreads();
        for (long long k = tid; k < cells; k += THREADS) {
            const int i = (int)(k / nx), j = (int)(k - (long long)i*nx);
            const int f = (i + 1)*P + j + 1, held = L[f];
            const int at = region_label(held, f), n_cells = region_cells(held, ((held >= 0) & (held != INT_MAX)) ? L[held] : 0);
            const int label = at < 0 ? -1 : region_unframe(at, P, nx);
            out[k] = label;
            areas[k] = region_area(n_cells, a.cell);
            region_sum(s, held, n_cells, label);
        }
    } else {
        // the same propagation and count on the labels where they are stored
        for (long long k = tid; k < cells; k += THREADS) out[k] = region_fill(region_open(fr, among, marks, k, r.where), (int)k);
        __syncthreads();
        passes = nav_settle<THREADS>(s_flag, cells, [=](const long long k) {
            const int own = nav_load(out + k);
            if (own == INT_MAX) return false;
            const int v = region_lowered_stored(out, nx, ny, k, own);
            if (v < own) region_lower(out, k, own, v);
            return v < own;
        });
        for (long long k = tid; k < cells; k += THREADS)
            if (region_is_root(out[k], (int)k)) out[k] = -1;
        __syncthreads();
        for (long long k = tid; k < cells; k += THREADS) region_count(out, nav_load(out + k));
        __syncthreads();
        for (long long k = tid; k < cells; k += THREADS) {
            const int held = nav_load(out + k);
            const int label = region_label(held, (int)k), n_cells = region_cells(held, ((held >= 0) & (held != INT_MAX)) ? nav_load(out + held) : 0);
            areas[k] = region_area(n_cells, a.cell);
            region_sum(s, held, n_cells, label);
        }
        __syncthreads();                                                // (every root's slot has been read)
        for (long long k = tid; k < cells; k += THREADS) out[k] = region_label(out[k], (int)k);
    }
    region_reduce(s, s_sum, &s_key);
    __syncthreads();
    if (tid == 0) {
        const unsigned long long key = s_key;
        r.counts[field] = s_sum[0];
        r.open_cells[field] = s_sum[1];
        r.largest[field] = region_key_label(key);
        r.largest_cells[field] = region_key_cells(key);
        if (r.passes) r.passes[field] = passes;
    }
}

struct NavRegionQueryArgs {                          // MsNavRegionQuery, checked
    const float* points;                             // (N, P, 2)
    const int* field;                                // (N, P) or NULL
    const int* labels;
    int* out;                                        // (N, P, 4)
    int n_points, n_fields;
    long long total;                                 // N P
};

// Point `at` = (e, k) of a query: the store it asks (NULL: none) and its env's grid.
__host__ __device__ inline const int* region_asked(const NavArgs& a, const int* labels, const int* field, const int n_fields, const long long at,
                                                   const int e, const int k, NavCells& g) {
    g = nav_cells(a, e);
    const long long cells = g.nx > 0 && g.ny > 0 ? (long long)g.nx*g.ny : 0;
    const int f = nav_layer_store(field, n_fields, at, k);
    return ((f >= 0) & (cells > 0)) ? labels + ((long long)n_fields*a.starts[e] + (long long)f*cells) : nullptr;
}

__host__ __device__ inline void region_query_one(const NavArgs& a, const NavRegionQueryArgs& q, const long long at) {
    const int e = (int)(at / q.n_points), k = (int)(at - (long long)e*q.n_points);
    NavCells g;
    int w[4];
    const int* const labels = region_asked(a, q.labels, q.field, q.n_fields, at, e, k, g);
    region_anchor_labels(labels, g, q.points[2*at], q.points[2*at + 1], w);
    for (int t = 0; t < 4; t++) q.out[4*at + t] = w[t];
}

__global__ __launch_bounds__(WG) void nav_region_query_kernel(const NavArgs a, const NavRegionQueryArgs q) {
    const long long at = (long long)blockIdx.x*WG + threadIdx.x;
    if (at < q.total) region_query_one(a, q, at);
}

struct NavRegionMaskArgs {                           // MsNavRegionMasks, checked
    const float* points;                             // (N, P, 2), or NULL: wanted
    const int* wanted;                               // (N, P), or NULL: points
    const int* field;                                // (N, P) or NULL
    const int* labels;
    unsigned char* out;                              // P stores per env
    int n_requests, n_fields;
};

// Request `at` = (e, p): the labels it wants (-1: none), the store it reads (NULL: none: an empty mask) and the store it writes.
__host__ __device__ inline const int* region_request(const NavArgs& a, const NavRegionMaskArgs& q, const long long at, int w[4], long long& cells,
                                                     unsigned char*& out) {
    const int e = (int)(at / q.n_requests), p = (int)(at - (long long)e*q.n_requests);
    NavCells g;
    const int* const labels = region_asked(a, q.labels, q.field, q.n_fields, at, e, p, g);
    cells = g.nx > 0 && g.ny > 0 ? (long long)g.nx*g.ny : 0;
    out = q.out + ((long long)q.n_requests*a.starts[e] + (long long)p*cells);
    if (q.points) region_anchor_labels(labels, g, q.points[2*at], q.points[2*at + 1], w);
    else { w[0] = q.wanted[at]; w[1] = w[2] = w[3] = -1; }
    return labels;
}

inline void region_mask_serial(const NavArgs& a, const NavRegionMaskArgs& q) {
    for (long long at = 0; at < (long long)a.n_envs*q.n_requests; at++) {
        int w[4];
        long long cells;
        unsigned char* out;
        const int* const labels = region_request(a, q, at, w, cells, out);
        for (long long k = 0; k < cells; k++) out[k] = labels ? region_mask_byte(labels[k], w) : 0;
    }
}

__global__ __launch_bounds__(WG) void nav_region_mask_kernel(const NavArgs a, const NavRegionMaskArgs q) {
    int w[4];
    long long cells;
    unsigned char* out;
    const int* const labels = region_request(a, q, blockIdx.x, w, cells, out);      // (uniform: the request's)
    for (long long k = (long long)blockIdx.y*WG + threadIdx.x; k < cells; k += (long long)gridDim.y*WG)
        out[k] = labels ? region_mask_byte(labels[k], w) : 0;
}
