// kernels/navzone.h -- nav_zone_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navregion.h and navbasin.h,
// whose labels it reads and whose basin_count it counts with; the grid and a cell's centre are navfield.h's); not a header to compile
// on its own.
// ------------------------------------------------------------------------------------------------
// zones: per-label counts, least values and nearest cells                    no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavZones) and DESIGN.md section 3.28: a cell's zone is the rank of its
// label among the roots (ranked) or the label itself (direct); per zone the cells, the marked cells, the least value over the cells
// that take part, the least cell attaining it and that cell's centre.  Every output is an integer or a copied float with one
// definition, so nothing depends on the order of execution.  tests/test_navzone_host.py restates all of it in numpy (zone_rule).
//
// The rule's pieces - zone_is_root, zone_rank, zone_of, zone_marked, zone_key, zone_write - are __host__ __device__ functions over
// plain numbers and pointers: ms_host_nav_zones (zone_serial) runs them on host arrays, so the CPU suite holds this very text to
// zone_rule.
//
//   nav_zone_kernel   one WORKGROUP of 256 lanes a field (n, f); its LDS - a list of 256 roots, two counters and one 64-bit key a
//                     zone: 5 KiB - does not grow with the env, so there is one instantiation and no global-memory path.
//                     RANKED: pass 1 walks the env's cells 256 a round, ballots "labels[k] == k" per wave, and a workgroup prefix
//                     of the four waves' popcounts (navdraw.h's scan, one barrier a round: the popcounts alternate between two
//                     rows) gives every root its rank; the first K go into the list in LDS, in index order, and all are counted.
//                     Pass 2 walks the cells again - a round's label, mark byte and value are loaded together, nothing waits for
//                     a branch - and finds each cell's zone: the label itself, or a binary search of the list, 8 LDS reads (a
//                     wave's lanes mostly share a label: the reads are broadcasts).  The counters take integer atomics, one a wave
//                     where the wave's cells agree (basin_count).  Least and nearest are ONE 64-bit LDS atomic min on
//                     (value bits << 32) | cell: a non-negative binary32 below +inf orders as its bits, so the minimum of the keys
//                     is the least value and, among the cells that attain it, the least index - the rule exactly.  Where a wave's
//                     candidates agree on the zone (the common case: a zone is a room) the wave takes the minimum by shuffles
//                     first and issues one atomic.  Lanes 0 .. K - 1 store the outputs, lane 0 n_zones: every output element has
//                     one writer.
constexpr int ZONE_MAX = 256;                        // zones a call: a lane each
constexpr int ZONE_THREADS = ZONE_MAX;
constexpr int ZONE_WAVES = ZONE_THREADS/64;
constexpr unsigned long long ZONE_NONE = ~0ull;      // the key of a cell that takes no part: above every key that does
constexpr int ZONE_UNUSED = 0x7fffffff;              // a slot of the list beyond the last root: above every label of a cell

struct NavZoneArgs {                                 // MsNavZones, checked
    const int* labels;                               // n_labels stores per env
    const float* values;                             // n_values stores per env, or NULL
    const unsigned char* marks;                      // n_marks stores per env, or NULL
    const unsigned char* mask;                       // (N, F) or NULL
    int* cells;                                      // (N, F, K)
    int* marked;                                     // (N, F, K)
    float* least;                                    // (N, F, K)
    int* nearest;                                    // (N, F, K)
    float* points;                                   // (N, F, K, 2)
    int* roots;                                      // (N, F, K)
    int* n_zones;                                    // (N, F)
    int n_fields, n_labels, n_values, n_marks, where, within_marks, ranked, K;
};

// Where store f of a layer of `count` stores per env (1: the one store serves every field) begins, for an env whose cells begin at
// `start`.
__host__ __device__ inline long long zone_store(const long long start, const long long cells, const int count, const int f) {
    return (long long)count*start + (long long)(count == 1 ? 0 : f)*cells;
}

__host__ __device__ inline bool zone_is_root(const int label, const int k) { return label == k; }

// The rank of `label` in the list - ZONE_MAX slots, the roots ascending, ZONE_UNUSED beyond them; first = list[0] - or -1 when it is
// not there: a negative label, one beyond the env's cells, one that is no root, a root beyond the K-th.
__host__ __device__ inline int zone_rank(const int* list, const int first, const int label) {
    int lo = 0, held = first;
#pragma unroll
    for (int step = ZONE_MAX/2; step >= 1; step >>= 1) {
        const int v = list[lo + step];
        if (v <= label) { lo += step; held = v; }
    }
    return ((held == label) & (label != ZONE_UNUSED)) ? lo : -1;      // (a label of 2^31 - 1 is no cell: it names no unused slot)
}

__host__ __device__ inline int zone_of(const NavZoneArgs& z, const int* list, const int first, const int label) {
    if (z.ranked) return zone_rank(list, first, label);
    return ((label >= 0) & (label < z.K)) ? label : -1;
}

// Is a cell with mark byte `byte` marked?  Without marks every cell is.
__host__ __device__ inline bool zone_marked(const NavZoneArgs& z, const unsigned char byte) {
    return !z.marks || ((byte != 0) == (z.where != 0));
}

// The key of cell k with value v: (bits << 32) | k where the cell takes part - the sign bit clear and v < +inf, so that NaN,
// negatives and -0 are left out - and `allowed` (marked, under within_marks); ZONE_NONE otherwise, and without values.
__host__ __device__ inline unsigned long long zone_key(const NavZoneArgs& z, const float v, const int k, const bool allowed) {
    const unsigned bits = __builtin_bit_cast(unsigned, v);
    return ((z.values != nullptr) & allowed & (bits < 0x7f800000u)) ? ((unsigned long long)bits << 32) | (unsigned)k : ZONE_NONE;
}

// Zone k of field `field`: what its lane stores.
__host__ __device__ inline void zone_write(const NavZoneArgs& z, const NavCells& g, const long long field, const int k, const int cells,
                                           const int marked, const unsigned long long best, const int root) {
    const long long at = field*z.K + k;
    z.cells[at] = cells;
    z.marked[at] = z.marks ? marked : cells;
    z.roots[at] = root;
    if (best != ZONE_NONE) {
        const int cell = (int)(unsigned)(best & 0xffffffffull);
        const int i = cell / g.nx, j = cell - i*g.nx;
        z.least[at] = __builtin_bit_cast(float, (unsigned)(best >> 32));
        z.nearest[at] = cell;
        z.points[2*at] = nav_centre(g.jx0, j, g.c);
        z.points[2*at + 1] = nav_centre(g.iy0, i, g.c);
    } else {
        z.least[at] = INFINITY;
        z.nearest[at] = -1;
        z.points[2*at] = NAN;
        z.points[2*at + 1] = NAN;
    }
}

// One call, serially (host instantiation only): the list, the counters and the keys as the kernel keeps them, cell after cell.
inline void zone_serial(const NavArgs& a, const NavZoneArgs& z) {
    for (long long field = 0; field < (long long)a.n_envs*z.n_fields; field++) {
        if (z.mask && !z.mask[field]) continue;
        const int e = (int)(field / z.n_fields), f = (int)(field - (long long)e*z.n_fields);
        const NavCells g = nav_cells(a, e);
        const long long cells = nav_count(a, e);
        int list[ZONE_MAX], count[ZONE_MAX], marked[ZONE_MAX];
        unsigned long long best[ZONE_MAX];
        for (int k = 0; k < ZONE_MAX; k++) { list[k] = ZONE_UNUSED; count[k] = 0; marked[k] = 0; best[k] = ZONE_NONE; }
        int total = 0;
        if (cells > 0) {
            const long long start = a.starts[e];
            const int n = (int)cells;
            const int* const labels = z.labels + zone_store(start, cells, z.n_labels, f);
            const float* const values = z.values ? z.values + zone_store(start, cells, z.n_values, f) : nullptr;
            const unsigned char* const marks = z.marks ? z.marks + zone_store(start, cells, z.n_marks, f) : nullptr;
            if (z.ranked)
                for (int k = 0; k < n; k++)
                    if (zone_is_root(labels[k], k)) {
                        if (total < z.K) list[total] = k;
                        total++;
                    }
            for (int k = 0; k < n; k++) {
                const int zone = zone_of(z, list, list[0], labels[k]);
                if (zone < 0) continue;
                const bool m = zone_marked(z, marks ? marks[k] : (unsigned char)0);
                const unsigned long long key = zone_key(z, values ? values[k] : 0.f, k, m | !z.within_marks);
                count[zone]++;
                marked[zone] += m;
                if (key < best[zone]) best[zone] = key;
            }
        }
        int used = 0;
        for (int k = 0; k < z.K; k++) {
            const int root = z.ranked ? (list[k] != ZONE_UNUSED ? list[k] : -1) : (count[k] > 0 ? k : -1);
            used += count[k] > 0;
            zone_write(z, g, field, k, count[k], marked[k], best[k], root);
        }
        z.n_zones[field] = z.ranked ? total : used;
    }
}

// One cell's share of least and nearest: the 64-bit minimum of its key into its zone's slot - one atomic for the wave where all of
// the wave's candidates in this round agree on the zone (the wave's minimum by shuffles first), one a lane otherwise.  Every lane of
// the wave calls it; zone < 0 or key == ZONE_NONE: no candidate.
__device__ inline void zone_least(unsigned long long* s_best, const int zone, const unsigned long long key) {
    const bool takes = (zone >= 0) & (key != ZONE_NONE);
    const unsigned long long voters = __ballot(takes);
    if (!voters) return;                                                // (uniform)
    const int lead = __ffsll((long long)voters) - 1;
    const int first = __shfl(zone, lead);
    if (__ballot(takes & (zone == first)) == voters) {
        unsigned long long least = takes ? key : ZONE_NONE;
        for (int step = 32; step >= 1; step >>= 1) {
            const unsigned long long other = __shfl_xor(least, step);
            least = other < least ? other : least;
        }
        if ((int)__lane_id() == lead) __hip_atomic_fetch_min(s_best + first, least, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (takes)
        __hip_atomic_fetch_min(s_best + zone, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(ZONE_THREADS) void nav_zone_kernel(const NavArgs a, const NavZoneArgs z) {
    __shared__ int s_list[ZONE_MAX];                                    // the first K roots, ascending; ZONE_UNUSED beyond
    __shared__ int s_cells[ZONE_MAX], s_marked[ZONE_MAX];
    __shared__ unsigned long long s_best[ZONE_MAX];
    __shared__ int s_wave[2][ZONE_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long field = blockIdx.x;                                 // (n, f): n F + f
    if (z.mask && !z.mask[field]) return;                               // (uniform) left as it is
    const int e = (int)(field / z.n_fields), f = (int)(field - (long long)e*z.n_fields);
    const int4 geom = reinterpret_cast<const int4*>(a.geom)[e];
    const NavCells g{geom.x, geom.y, geom.z, geom.w, a.cell};
    const long long cells = geom.z > 0 && geom.w > 0 ? (long long)geom.z*geom.w : 0;
    const int K = z.K;
    s_list[tid] = ZONE_UNUSED;                                          // (a lane a slot: ZONE_THREADS == ZONE_MAX)
    s_cells[tid] = 0;
    s_marked[tid] = 0;
    s_best[tid] = ZONE_NONE;
    int total = 0;
    if (cells > 0) {                                                    // (uniform)
        const long long start = a.starts[e];
        const int* const labels = z.labels + zone_store(start, cells, z.n_labels, f);
        const float* const values = z.values ? z.values + zone_store(start, cells, z.n_values, f) : nullptr;
        const unsigned char* const marks = z.marks ? z.marks + zone_store(start, cells, z.n_marks, f) : nullptr;
        __syncthreads();
        if (z.ranked) {                                                 // (uniform) pass 1: the roots, ranked in index order
            int round = 0;
            for (long long k0 = 0; k0 < cells; k0 += ZONE_THREADS, round ^= 1) {
                const long long k = k0 + tid;
                const bool root = k < cells && zone_is_root(labels[k], (int)k);
                const unsigned long long word = __ballot(root);
                if (lane == 0) s_wave[round][wave] = __popcll(word);
                __syncthreads();
                int before = total, all = 0;
#pragma unroll
                for (int w = 0; w < ZONE_WAVES; w++) {
                    const int t = s_wave[round][w];
                    before += w < wave ? t : 0;
                    all += t;
                }
                const int rank = before + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(word >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)word, 0u));
                if (root && rank < K) s_list[rank] = (int)k;
                total += all;
            }
            __syncthreads();
        }
        const int first = s_list[0];
        for (long long k0 = 0; k0 < cells; k0 += ZONE_THREADS) {       // pass 2 (whole waves go round: the counts ballot)
            const long long k = k0 + tid;
            int zone = -1, zone_if_marked = -1;
            unsigned long long key = ZONE_NONE;
            if (k < cells) {
                const int label = labels[k];                            // (the three loads are in flight together)
                const unsigned char byte = marks ? marks[k] : (unsigned char)0;
                const float v = values ? values[k] : 0.f;
                zone = zone_of(z, s_list, first, label);
                const bool m = zone_marked(z, byte);
                zone_if_marked = m ? zone : -1;
                key = zone_key(z, v, (int)k, m | !z.within_marks);
            }
            basin_count(s_cells, zone, K);
            if (marks) basin_count(s_marked, zone_if_marked, K);        // (uniform)
            if (values) zone_least(s_best, zone, key);                  // (uniform)
        }
        __syncthreads();
    }
    const int mine = s_cells[tid];                                      // (a lane reads the slots it cleared itself: an env without cells needs no barrier)
    if (!z.ranked) {                                                    // (uniform) the zones in use
        const unsigned long long word = __ballot((tid < K) & (mine > 0));
        if (lane == 0) s_wave[0][wave] = __popcll(word);
        __syncthreads();
        for (int w = 0; w < ZONE_WAVES; w++) total += s_wave[0][w];
    }
    if (tid < K) {
        const int slot = s_list[tid];
        const int root = z.ranked ? (slot != ZONE_UNUSED ? slot : -1) : (mine > 0 ? tid : -1);
        zone_write(z, g, field, tid, mine, s_marked[tid], s_best[tid], root);
    }
    if (tid == 0) z.n_zones[field] = total;
}
