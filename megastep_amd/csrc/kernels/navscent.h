// kernels/navscent.h -- nav_scent_kernel, nav_scent_query_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navfield.h, whose
// NavArgs, NavCells, nav_layer_store and nav_frame_free it shares); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// scent fields: a quantity that is left behind, spreads round corners and fades      no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavScent) and DESIGN.md section 3.35: a call is one tick of every
// marked store - reset, the deposits in ascending source index, T Jacobi sub-steps of a four-neighbour stencil with zero flux
// into closed cells, a decay and a floor, then the store's peak and its scented cells.  Every step is one binary32 operation in
// a FIXED ORDER, so unlike the min and pointer updates of the other LDS-resident fields nothing here may be left to the
// schedule: the kernel keeps the rule's order of every addition.  tests/scent_rule.py restates all of it in numpy.
//
// The rule's pieces - scent_cell, scent_source_cell, scent_deposits, scent_gradient - are __host__ __device__ functions over
// plain numbers: ms_host_nav_scent sweeps them serially on host arrays, so the CPU suite holds this very text to the rule.
//
//   nav_scent_kernel   one WORKGROUP a store (n, g), nav_relax_kernel's launch shape and LDS tiers.  The store lives in LDS as
//                      ONE FLOAT A FRAMED CELL (row pitch P = nx + 2): the frame and the closed cells hold SCENT_CLOSED, a
//                      negative number no open cell can hold (the rule's values are never negative, not even -0.f), so a
//                      neighbour needs neither a bounds check nor an openness bitmap - `y >= 0.f` is the whole test.
//                      THE LOAD: framed cell k takes its value from the store (0.f under a reset), or the sentinel.
//                      THE DEPOSITS, without float atomics: the cells are dealt to the workgroup's waves by cell % n_waves.
//                      Every wave walks ALL the env's sources 64 at a time, a lane a source, ballots those that deposit on
//                      one of its own cells and into this store, and lane 0 applies them one after another, lowest bit
//                      first: no two waves touch one cell, and within a wave the order is ascending k - the rule's.
//                      THE SWEEP is register-resident: lane tid owns framed cells tid, tid + THREADS, ... - at most
//                      PER = ceil(capacity / THREADS) of them, a compile-time bound (20, 20, 40), the loop unrolled.  A
//                      sub-step: the lane reads its cells and their four neighbours from LDS (consecutive lanes, consecutive
//                      words - no bank conflict at any pitch) and keeps the new values in registers; a barrier; it writes
//                      them back; a barrier.  Two barriers a sub-step at 4 bytes a cell, where ping-pong between two LDS
//                      stores would take one barrier at 8 bytes - and a tier more for most floorplans.  (Ping-pong was not
//                      built: DESIGN.md 3.35.)
//                      THE SUMMARY: the lanes' greatest value and count of positive cells meet by shuffles and one integer
//                      LDS atomic a wave each - non-negative floats order as their bit patterns, so an integer max serves.
//                      A store too large for the launch's LDS runs the same sweeps in global memory, ping-pong between
//                      `values` and the caller's `workspace`, a barrier a sub-step; an odd T starts from a copy in the
//                      workspace so that the result ends in `values` either way - the same bits.
//   nav_scent_query_kernel   one lane a point: the value under it and the central differences, zero-flux at closed sides.
constexpr int scent_capacity(const int lds_bytes) { return (lds_bytes - 64)/4; }       // framed cells: a float each
constexpr float SCENT_CLOSED = -1.f;                 // what the frame and the closed cells hold in LDS
constexpr int SCENT_MAX_SOURCES = 1024, SCENT_MAX_SUBSTEPS = 64;

// One cell's new value from its five reads: x its own, then west, east, south, north - a neighbour that is closed or outside
// the grid arrives as a negative number and adds nothing.
__host__ __device__ inline float scent_cell(const float x, const float w, const float e, const float s, const float n, const float rate,
                                            const float keep, const float floor) {
    float acc = 0.f;
    if (w >= 0.f) acc = acc + (w - x);
    if (e >= 0.f) acc = acc + (e - x);
    if (s >= 0.f) acc = acc + (s - x);
    if (n >= 0.f) acc = acc + (n - x);
    const float v = (x + rate*acc)*keep;
    return v >= floor ? v : 0.f;
}

// The same of open cell k (value x) of the store as it is stored: nx x ny, no frame, every neighbour bounds-checked (rows do
// not wrap) and asked for its free byte.
__host__ __device__ inline float scent_cell_stored(const float* V, const unsigned char* fr, const int nx, const int ny, const int k, const float x,
                                                   const float rate, const float keep, const float floor) {
    const int i = k / nx, j = k - i*nx;
    const float w = j > 0 && (fr[k - 1] & 1) ? V[k - 1] : SCENT_CLOSED, e = j < nx - 1 && (fr[k + 1] & 1) ? V[k + 1] : SCENT_CLOSED;
    const float s = i > 0 && (fr[k - nx] & 1) ? V[k - nx] : SCENT_CLOSED, n = i < ny - 1 && (fr[k + nx] & 1) ? V[k + nx] : SCENT_CLOSED;
    return scent_cell(x, w, e, s, n, rate, keep, floor);
}

// The cell under (x, y), row-major in its env's grid, as MsNavSeen finds it; -1: none.
__host__ __device__ inline int scent_source_cell(const NavCells& g, const float x, const float y) {
    const float fx = floorf(x/g.c), fy = floorf(y/g.c);
    if (!(fabsf(fx) < NAV_INDEX_LIMIT) || !(fabsf(fy) < NAV_INDEX_LIMIT)) return -1;
    const long long j = (long long)fx - g.jx0, i = (long long)fy - g.iy0;
    if ((i < 0) | (i >= g.ny) | (j < 0) | (j >= g.nx)) return -1;
    return (int)(i*g.nx + j);
}

// Does a source on `cell` with `amount` deposit (its field index is its caller's to test): an open cell, an amount > 0.f.
__host__ __device__ inline bool scent_deposits(const unsigned char* fr, const int cell, const float amount) {
    return cell >= 0 && (fr[cell] & 1) && amount > 0.f;
}

// Central differences of open cell `cell` (value x) with zero-flux sides: a side that is closed or outside stands in as x.
__host__ __device__ inline void scent_gradient(const float* V, const unsigned char* fr, const NavCells& g, const int cell, const float x,
                                               float& gx, float& gy) {
    const int nx = g.nx, ny = g.ny, i = cell / nx, j = cell - i*nx;
    const float e = j < nx - 1 && (fr[cell + 1] & 1) ? V[cell + 1] : x, w = j > 0 && (fr[cell - 1] & 1) ? V[cell - 1] : x;
    const float n = i < ny - 1 && (fr[cell + nx] & 1) ? V[cell + nx] : x, s = i > 0 && (fr[cell - nx] & 1) ? V[cell - nx] : x;
    const float span = 2.f*g.c;
    gx = (e - w)/span;
    gy = (n - s)/span;
}

struct NavScentArgs {                                // MsNavScent, checked
    const unsigned char* free_cells;
    const float* points;                             // (N, P, 2) or NULL (P = 0)
    const float* amounts;                            // (N, P)
    const int* field;                                // (N, P) or NULL
    const unsigned char* reset;                      // (N, G) or NULL
    const unsigned char* mask;                       // (N, G) or NULL
    float* values;
    float* workspace;                                // as values, or NULL
    float* peaks;                                    // (N, G)
    int* scented;                                    // (N, G)
    int n_fields, n_sources, substeps;
    float rate, keep, floor;
};

// Source k of env e: the cell it deposits `amount` on in store gi, or -1 (no cell, a closed cell, another or no store, an amount
// that is not > 0.f).
__host__ __device__ inline int scent_source(const NavScentArgs& q, const NavCells& g, const unsigned char* fr, const int e, const int gi, const int k,
                                            float& amount) {
    const long long at = (long long)e*q.n_sources + k;
    amount = q.amounts[at];
    if (nav_layer_store(q.field, q.n_fields, at, k) != gi) return -1;
    const int cell = scent_source_cell(g, q.points[2*at], q.points[2*at + 1]);
    return scent_deposits(fr, cell, amount) ? cell : -1;
}

// One store, serially (host instantiation only): the kernel's load, deposits, sweeps and summary with the same pieces - framed
// when the store fits `capacity` framed cells, else on the store itself and the workspace.
inline void scent_serial_store(const NavArgs& a, const NavScentArgs& q, const long long store, const int capacity) {
    const int e = (int)(store / q.n_fields), gi = (int)(store - (long long)e*q.n_fields);
    const NavCells g = nav_cells(a, e);
    const int nx = g.nx, ny = g.ny;
    const long long cells = nx > 0 && ny > 0 ? (long long)nx*ny : 0, framed = (long long)(nx + 2)*(ny + 2);
    float peak = 0.f;
    int count = 0;
    if (cells > 0 && (framed <= capacity || q.workspace)) {
        const unsigned char* const fr = q.free_cells + a.starts[e];
        const long long first = (long long)q.n_fields*a.starts[e] + (long long)gi*cells;
        float* const out = q.values + first;
        const bool clear = q.reset && q.reset[store];
        if (framed <= capacity) {
            const int P = nx + 2, n = (int)framed;
            std::vector<float> V(n), R(n);
            for (int k = 0; k < n; k++) {
                long long cell;
                V[k] = nav_frame_free(fr, nx, ny, P, k, cell) ? (clear ? 0.f : out[cell]) : SCENT_CLOSED;
            }
            for (int k = 0; k < q.n_sources; k++) {
                float amount;
                const int cell = scent_source(q, g, fr, e, gi, k, amount);
                if (cell >= 0) { const int f = (cell / nx + 1)*P + cell % nx + 1; V[f] = V[f] + amount; }
            }
            for (int t = 0; t < q.substeps; t++) {
                for (int k = 0; k < n; k++)
                    R[k] = V[k] >= 0.f ? scent_cell(V[k], V[k - 1], V[k + 1], V[k - P], V[k + P], q.rate, q.keep, q.floor) : SCENT_CLOSED;
                V.swap(R);
            }
            for (long long k = 0; k < cells; k++) {
                const float v = V[(k / nx + 1)*P + k % nx + 1];
                out[k] = v >= 0.f ? v : 0.f;
            }
        } else {
            float* src = q.substeps & 1 ? q.workspace + first : out;
            float* dst = q.substeps & 1 ? out : q.workspace + first;
            for (long long k = 0; k < cells; k++) src[k] = (fr[k] & 1) && !clear ? out[k] : 0.f;
            for (int k = 0; k < q.n_sources; k++) {
                float amount;
                const int cell = scent_source(q, g, fr, e, gi, k, amount);
                if (cell >= 0) src[cell] = src[cell] + amount;
            }
            for (int t = 0; t < q.substeps; t++) {
                for (long long k = 0; k < cells; k++)
                    dst[k] = fr[k] & 1 ? scent_cell_stored(src, fr, nx, ny, (int)k, src[k], q.rate, q.keep, q.floor) : 0.f;
                float* const was = src; src = dst; dst = was;
            }
        }
        for (long long k = 0; k < cells; k++) {
            if (out[k] > peak) peak = out[k];
            count += out[k] > 0.f;
        }
    }
    q.peaks[store] = peak;
    q.scented[store] = count;
}

inline void scent_serial(const NavArgs& a, const NavScentArgs& q, const int capacity) {
    for (long long store = 0; store < (long long)a.n_envs*q.n_fields; store++)
        if (!q.mask || q.mask[store]) scent_serial_store(a, q, store, capacity);
}

// The deposits of one store into V, where `slot(cell)` is the cell's place in V: every wave walks all the env's sources, a lane
// a source, and applies those on ITS cells (cell % WAVES_HERE == wave) in ascending k, through lane 0 alone - one lane's loads
// and stores of one address keep their program order, in LDS and in global memory alike.
template <int WAVES_HERE, class Slot>
__device__ inline void scent_deposit(float* V, const NavScentArgs& q, const NavCells& g, const unsigned char* fr, const int e, const int gi,
                                     const Slot slot) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int k0 = 0; k0 < q.n_sources; k0 += 64) {
        const int k = k0 + lane;
        float amount = 0.f;
        int cell = -1;
        if (k < q.n_sources) cell = scent_source(q, g, fr, e, gi, k, amount);
        unsigned long long mine = __ballot(cell >= 0 && cell % WAVES_HERE == wave);
        while (mine) {                                                  // (uniform) lowest k first
            const int l = __ffsll((long long)mine) - 1;
            mine &= mine - 1;
            const int at = slot(__shfl(cell, l));
            const float add = __shfl(amount, l);
            if (lane == 0) V[at] = V[at] + add;
        }
    }
}

template <int LDS_BYTES, int THREADS>
__global__ __launch_bounds__(THREADS) void nav_scent_kernel(const NavArgs a, const NavScentArgs q) {
    constexpr int CAP = scent_capacity(LDS_BYTES), PER = (CAP + THREADS - 1)/THREADS;
    __shared__ float V[CAP];
    __shared__ int s_sum[2];                                            // the peak's bits, the scented cells
    const int tid = threadIdx.x;
    const long long store = blockIdx.x;                                 // (n, g): n G + g
    const int e = (int)(store / q.n_fields), gi = (int)(store - (long long)e*q.n_fields);
    if (q.mask && !q.mask[store]) return;                               // (uniform) left as it is
    const int4 geom = reinterpret_cast<const int4*>(a.geom)[e];
    const int nx = geom.z, ny = geom.w;
    const long long cells = nx > 0 && ny > 0 ? (long long)nx*ny : 0, framed = (long long)(nx + 2)*(ny + 2);
    if (cells <= 0 || (framed > CAP && !q.workspace)) {                 // (uniform) no cells; or no room and nowhere to sweep
        if (tid == 0) { q.peaks[store] = 0.f; q.scented[store] = 0; }
        return;
    }
    const NavCells g{geom.x, geom.y, nx, ny, a.cell};
    const unsigned char* const fr = q.free_cells + a.starts[e];
    const long long first = (long long)q.n_fields*a.starts[e] + (long long)gi*cells;
    float* const out = q.values + first;
    const bool clear = q.reset && q.reset[store];
    const float rate = q.rate, keep = q.keep, floor = q.floor;
    if (tid < 2) s_sum[tid] = 0;
    float peak = 0.f;
    int count = 0;

    if (framed <= CAP) {
        const int P = nx + 2, n = (int)framed;
        for (int k = tid; k < n; k += THREADS) {
            long long cell;
            V[k] = nav_frame_free(fr, nx, ny, P, k, cell) ? (clear ? 0.f : out[cell]) : SCENT_CLOSED;
        }
        __syncthreads();
        if (q.n_sources > 0) {
            scent_deposit<THREADS/64>(V, q, g, fr, e, gi, [=](const int cell) { const int i = cell / nx; return (i + 1)*P + (cell - i*nx) + 1; });
            __syncthreads();
        }
        float r[PER];
        for (int t = 0; t < q.substeps; t++) {
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const int k = tid + i*THREADS;
                float v = SCENT_CLOSED;
                if (k < n) {
                    const float x = V[k];                               // (an open cell is inside the frame: k +- 1, k +- P are in V)
                    if (x >= 0.f) v = scent_cell(x, V[k - 1], V[k + 1], V[k - P], V[k + P], rate, keep, floor);
                }
                r[i] = v;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < PER; i++)
                if (r[i] >= 0.f) V[tid + i*THREADS] = r[i];
            __syncthreads();
        }
        for (int k = tid; k < (int)cells; k += THREADS) {
            const int i = k / nx;
            const float held = V[(i + 1)*P + (k - i*nx) + 1], v = held >= 0.f ? held : 0.f;
            out[k] = v;
            peak = v > peak ? v : peak;
            count += v > 0.f;
        }
    } else {
        // the same sweeps where the store is, ping-pong with the workspace; an odd T starts from the workspace
        float* src = q.substeps & 1 ? q.workspace + first : out;
        float* dst = q.substeps & 1 ? out : q.workspace + first;
        const int n = (int)cells;
        for (int k = tid; k < n; k += THREADS) src[k] = (fr[k] & 1) && !clear ? out[k] : 0.f;
        __syncthreads();
        if (q.n_sources > 0) {
            scent_deposit<THREADS/64>(src, q, g, fr, e, gi, [](const int cell) { return cell; });
            __syncthreads();
        }
        for (int t = 0; t < q.substeps; t++) {
            for (int k = tid; k < n; k += THREADS)
                dst[k] = fr[k] & 1 ? scent_cell_stored(src, fr, nx, ny, k, src[k], rate, keep, floor) : 0.f;
            __syncthreads();
            float* const was = src; src = dst; dst = was;
        }
        for (int k = tid; k < n; k += THREADS) {                        // (src is `out` by now)
            const float v = out[k];
            peak = v > peak ? v : peak;
            count += v > 0.f;
        }
    }
    for (int step = 32; step >= 1; step >>= 1) {
        const float other = __shfl_xor(peak, step);
        peak = other > peak ? other : peak;
        count += __shfl_xor(count, step);
    }
    if ((tid & 63) == 0) {
        if (peak > 0.f) atomicMax(s_sum, __float_as_int(peak));
        if (count) atomicAdd(s_sum + 1, count);
    }
    __syncthreads();
    if (tid == 0) { q.peaks[store] = __int_as_float(s_sum[0]); q.scented[store] = s_sum[1]; }
}

struct NavScentQueryArgs {                           // MsNavScentQuery, checked
    const unsigned char* free_cells;
    const float* points;                             // (N, P, 2)
    const int* field;                                // (N, P) or NULL
    const float* values;
    float* out;                                      // (N, P)
    float* gradients;                                // (N, P, 2) or NULL
    int n_points, n_fields;
    long long total;                                 // N P
};

__host__ __device__ inline void scent_query_one(const NavArgs& a, const NavScentQueryArgs& q, const long long at) {
    const int e = (int)(at / q.n_points), k = (int)(at - (long long)e*q.n_points);
    const NavCells g = nav_cells(a, e);
    const long long cells = g.nx > 0 && g.ny > 0 ? (long long)g.nx*g.ny : 0;
    const int f = nav_layer_store(q.field, q.n_fields, at, k);
    const int cell = cells > 0 ? scent_source_cell(g, q.points[2*at], q.points[2*at + 1]) : -1;
    float x = 0.f, gx = 0.f, gy = 0.f;
    if (f >= 0 && cell >= 0) {
        const unsigned char* const fr = q.free_cells + a.starts[e];
        if (fr[cell] & 1) {
            const float* const V = q.values + ((long long)q.n_fields*a.starts[e] + (long long)f*cells);
            x = V[cell];
            scent_gradient(V, fr, g, cell, x, gx, gy);
        }
    }
    q.out[at] = x;
    if (q.gradients) { q.gradients[2*at] = gx; q.gradients[2*at + 1] = gy; }
}

__global__ __launch_bounds__(WG) void nav_scent_query_kernel(const NavArgs a, const NavScentQueryArgs q) {
    const long long at = (long long)blockIdx.x*WG + threadIdx.x;
    if (at < q.total) scent_query_one(a, q, at);
}
