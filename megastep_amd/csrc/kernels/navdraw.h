// kernels/navdraw.h -- nav_draw_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navwindow.h; the
// store a set reads in a layer is navfield.h's nav_layer_store); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// cell draws: uniform random free cells of an env that satisfy a predicate on a layer      no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavDraws) and DESIGN.md section 3.19: a cell qualifies for draw set
// (n, p) when it is free, the source's predicate holds on it and its gate byte is set; draw k of the set picks the r-th
// qualifying cell in row-major order, r = (h*M) >> 32 with h a 32-bit hash of (seed, set, counter, k); the set's counter then
// moves on by one.  Every output element has one writer and every value is integer-derived, so nothing depends on the order
// of execution.  tests/test_navdraw_host.py restates all of it in numpy (draw_rule).
//
// The rule's pieces - draw_qualifies, draw_mix, draw_hash, draw_rank, draw_uniform, draw_select, draw_write - are
// __host__ __device__ functions over plain numbers and pointers: ms_host_nav_draws runs them on host arrays, so the CPU suite
// holds this very text to draw_rule.
//
//   nav_draw_kernel   one WORKGROUP a draw set (n, p).  Pass 1 walks the env's cells: a wave takes four 64-bit words of the
//                     bitmap a round, a lane a cell of each - the predicate is straight-line code, so the round's loads
//                     (the free bytes, the source, the gate: contiguous across the wave) are in flight together - ballots
//                     "qualifies" and its lane 0 stores the words into a bitmap in (dynamic) LDS: a bit a cell, no atomics.
//                     Pass 2: each of the 256 lanes owns a contiguous span of words - the least power of two that covers
//                     the env - and sums their popcounts; a wave scan by shuffles and a 4-wave combine through LDS turn the
//                     sums into 256 exclusive span prefixes and M.  Pass 3: lane k < K forms its rank, finds the span that
//                     holds it by a binary search of the prefixes, walks that span's words to the one holding the rank,
//                     selects the n-th set bit of it and writes the draw.  Lane 0 writes M and moves the counter on (every
//                     lane read it before the first barrier).  A span's words are one word further apart than they are long
//                     (word w sits at w + w/span): with 64 words a lane - an env of 2^20 cells - the lanes' reads in passes
//                     2 and 3 would otherwise all fall into one pair of LDS banks.
constexpr int DRAW_MAX_DRAWS = WG;                   // a lane a draw
constexpr int DRAW_ROUND = 4;                        // words of the bitmap a wave forms a round

__host__ __device__ inline unsigned draw_mix(unsigned a) {              // murmur3's 32-bit finaliser
    a ^= a >> 16; a *= 0x85ebca6bu; a ^= a >> 13; a *= 0xc2b2ae35u; a ^= a >> 16;
    return a;
}

__host__ __device__ inline unsigned draw_hash(const unsigned seed_lo, const unsigned seed_hi, const unsigned set, const unsigned counter,
                                              const unsigned k, const unsigned stream) {
    unsigned s = 0x9e3779b9u;
    s = draw_mix(s + seed_lo); s = draw_mix(s + seed_hi); s = draw_mix(s + set);
    s = draw_mix(s + counter); s = draw_mix(s + k); s = draw_mix(s + stream);
    return s;
}

__host__ __device__ inline unsigned draw_rank(const unsigned h, const unsigned M) { return (unsigned)(((unsigned long long)h*M) >> 32); }
__host__ __device__ inline float draw_uniform(const unsigned h) { return (float)(h >> 8)*5.9604644775390625e-8f; }      // (2^-24: exact)

// Does cell k of the env qualify?  `free_cells`, `source` and `gate` point at the env's (the set's) first cell; gate NULL: none.
__host__ __device__ inline bool draw_qualifies(const unsigned char* free_cells, const void* source, const int is_float, const int where,
                                               const float lo, const float hi, const unsigned char* gate, const long long k) {
    // (no early exit: the loads do not wait for one another, and a wave's unrolled rounds keep theirs in flight together)
    const bool open = (free_cells[k] != 0) & (!gate || gate[k] != 0);
    if (is_float) {
        const float D = static_cast<const float*>(source)[k];
        return open & (lo <= D) & (D <= hi);                            // (a NaN fails both)
    }
    return open & ((static_cast<const unsigned char*>(source)[k] != 0) == (where != 0));
}

// The position of the n-th (0-based) set bit of w; n is below w's popcount.
__host__ __device__ inline int draw_select(const unsigned long long w, int n) {
    int pos = 0;
#pragma unroll
    for (int width = 32; width >= 1; width >>= 1) {
        const int c = __builtin_popcountll((w >> pos) & ((1ull << width) - 1ull));
        if (n >= c) { n -= c; pos += width; }
    }
    return pos;
}

struct NavDrawArgs {                                 // MsNavDraws, checked
    const void* source;                              // bytes or floats: source_fields stores per env
    const int* source_field;                         // (N, P) or NULL
    const unsigned char* gate;                       // bytes, or NULL: no gate
    const int* gate_field;                           // (N, P) or NULL
    const unsigned char* free_cells;                 // (starts[N],)
    const unsigned char* mask;                       // (N, P) or NULL
    int* counter;                                    // (N, P)
    int* cells;                                      // (N, P, K)
    float* points;                                   // (N, P, K, 2)
    float* uniforms;                                 // (N, P, K)
    float* values;                                   // (N, P, K) or NULL
    int* counts;                                     // (N, P)
    int source_fields, gate_fields, is_float, where;
    float lo, hi;
    unsigned seed_lo, seed_hi;
    int n_sets, n_draws, max_cells;
};

// The stores set (n, p) reads, from the env's first cell on; false: a field index is bad, nothing qualifies.
__host__ __device__ inline bool draw_stores(const NavDrawArgs& q, const long long first, const long long cells, const long long set, const int p,
                                            const void*& source, const unsigned char*& gate) {
    const int fs = nav_layer_store(q.source_field, q.source_fields, set, p);
    const int fg = q.gate ? nav_layer_store(q.gate_field, q.gate_fields, set, p) : 0;
    if ((fs < 0) | (fg < 0)) return false;
    const long long at = (long long)q.source_fields*first + (long long)fs*cells;
    source = q.is_float ? static_cast<const void*>(static_cast<const float*>(q.source) + at)
                        : static_cast<const void*>(static_cast<const unsigned char*>(q.source) + at);
    gate = q.gate ? q.gate + ((long long)q.gate_fields*first + (long long)fg*cells) : nullptr;
    return true;
}

// Draw k of set `set`: cell = the chosen cell, -1 when M = 0.
__host__ __device__ inline void draw_write(const NavDrawArgs& q, const NavCells& g, const void* source, const long long set, const int k,
                                           const unsigned counter, const long long cell) {
    const long long at = set*q.n_draws + k;
    q.cells[at] = (int)cell;
    q.uniforms[at] = draw_uniform(draw_hash(q.seed_lo, q.seed_hi, (unsigned)set, counter, (unsigned)k, 1u));
    if (cell >= 0) {
        const int i = (int)(cell / g.nx), j = (int)(cell - (long long)i*g.nx);
        q.points[2*at] = nav_centre(g.jx0, j, g.c);
        q.points[2*at + 1] = nav_centre(g.iy0, i, g.c);
        if (q.values) q.values[at] = static_cast<const float*>(source)[cell];
    } else {
        q.points[2*at] = NAN;
        q.points[2*at + 1] = NAN;
        if (q.values) q.values[at] = NAN;
    }
}

// One call, serially (host instantiation only): the bitmap as the kernel builds it, walked from its first word.
inline void draw_serial(const NavArgs& a, const NavDrawArgs& q) {
    std::vector<unsigned long long> bitmap;
    for (long long set = 0; set < (long long)a.n_envs*q.n_sets; set++) {
        if (q.mask && !q.mask[set]) continue;
        const int e = (int)(set / q.n_sets), p = (int)(set - (long long)e*q.n_sets);
        const NavCells g = nav_cells(a, e);
        long long cells = g.nx > 0 && g.ny > 0 ? (long long)g.nx*g.ny : 0;
        if (cells > q.max_cells) cells = 0;
        const void* source = nullptr;
        const unsigned char* gate = nullptr;
        if (cells > 0 && !draw_stores(q, a.starts[e], cells, set, p, source, gate)) cells = 0;
        const unsigned counter = (unsigned)q.counter[set];
        bitmap.assign((size_t)((cells + 63) >> 6), 0ull);
        unsigned M = 0;
        for (long long k = 0; k < cells; k++)
            if (draw_qualifies(q.free_cells + a.starts[e], source, q.is_float, q.where, q.lo, q.hi, gate, k)) { bitmap[k >> 6] |= 1ull << (k & 63); M++; }
        for (int k = 0; k < q.n_draws; k++) {
            long long cell = -1;
            if (M > 0) {
                int rest = (int)draw_rank(draw_hash(q.seed_lo, q.seed_hi, (unsigned)set, counter, (unsigned)k, 0u), M);
                size_t w = 0;
                for (;; w++) {
                    const int c = __builtin_popcountll(bitmap[w]);
                    if (rest < c) break;
                    rest -= c;
                }
                cell = ((long long)w << 6) + draw_select(bitmap[w], rest);
            }
            draw_write(q, g, source, set, k, counter, cell);
        }
        q.counts[set] = (int)M;
        q.counter[set] = (int)(counter + 1u);
    }
}

__global__ __launch_bounds__(WG) void nav_draw_kernel(const NavArgs a, const NavDrawArgs q) {
    extern __shared__ unsigned long long s_bits[];                      // a bit a cell: word w at w + w/span
    __shared__ int s_prefix[WG];                                        // the qualifying cells before each lane's span
    __shared__ int s_wave[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long set = blockIdx.x;                                   // (n, p): n P + p
    if (q.mask && !q.mask[set]) return;                                 // (uniform) not touched at all
    const int e = (int)(set / q.n_sets), p = (int)(set - (long long)e*q.n_sets);
    const int4 geom = reinterpret_cast<const int4*>(a.geom)[e];
    const NavCells g{geom.x, geom.y, geom.z, geom.w, a.cell};
    long long cells = geom.z > 0 && geom.w > 0 ? (long long)geom.z*geom.w : 0;
    if (cells > q.max_cells) cells = 0;                                 // (uniform) more than the launch has bits for
    const unsigned counter = (unsigned)q.counter[set];                  // (read by every lane before the first barrier)
    const long long first = a.starts[e];
    const void* source = nullptr;
    const unsigned char* gate = nullptr;
    if (cells > 0 && !draw_stores(q, first, cells, set, p, source, gate)) cells = 0;

    const int words = (int)((cells + 63) >> 6);                         // (at most 2^14)
    int shift = 0;                                                      // a lane's span: 1 << shift words, 256 spans cover the env
    while ((WG << shift) < words) shift++;                              // (uniform; at most 6)
    const int span = 1 << shift;
    const unsigned char* const free_cells = q.free_cells + first;
    for (int w0 = wave*DRAW_ROUND; w0 < words; w0 += WAVES*DRAW_ROUND) {        // a wave DRAW_ROUND words, a lane a cell of each
        bool ok[DRAW_ROUND];
#pragma unroll
        for (int u = 0; u < DRAW_ROUND; u++) {
            const long long k = ((long long)(w0 + u) << 6) + lane;
            ok[u] = k < cells && draw_qualifies(free_cells, source, q.is_float, q.where, q.lo, q.hi, gate, k);
        }
#pragma unroll
        for (int u = 0; u < DRAW_ROUND; u++) {
            const unsigned long long word = __ballot(ok[u]);
            const int w = w0 + u;
            if (lane == 0 && w < words) s_bits[w + (w >> shift)] = word;
        }
    }
    __syncthreads();

    const int w_lo = tid << shift, w_hi = w_lo + span < words ? w_lo + span : words;
    int sum = 0;
    for (int w = w_lo; w < w_hi; w++) sum += __popcll(s_bits[w + tid]);
    int scan = sum;                                                     // inclusive, within the wave
    for (int step = 1; step < 64; step <<= 1) {
        const int below = __shfl_up(scan, step);
        if (lane >= step) scan += below;
    }
    if (lane == 63) s_wave[wave] = scan;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < WAVES; k++) {
        const int t = s_wave[k];
        before += k < wave ? t : 0;
        all += t;
    }
    s_prefix[tid] = before + scan - sum;
    __syncthreads();

    const unsigned M = (unsigned)all;
    if (tid < q.n_draws) {
        long long cell = -1;
        if (M > 0) {
            const int r = (int)draw_rank(draw_hash(q.seed_lo, q.seed_hi, (unsigned)set, counter, (unsigned)tid, 0u), M);
            int t = 0;                                                  // the last span whose prefix is at most r
            for (int step = WG/2; step >= 1; step >>= 1)
                if (s_prefix[t + step] <= r) t += step;
            int rest = r - s_prefix[t];
            int w = t << shift;                                         // (the span holds the rank: the walk ends inside it)
            const int end = w + span < words ? w + span : words;
            unsigned long long word = 0ull;
            for (; w < end; w++) {
                word = s_bits[w + t];
                const int c = __popcll(word);
                if (rest < c) break;
                rest -= c;
            }
            if (w < end) cell = ((long long)w << 6) + draw_select(word, rest);
        }
        draw_write(q, g, source, set, tid, counter, cell);
    }
    if (tid == 0) {
        q.counts[set] = (int)M;
        q.counter[set] = (int)(counter + 1u);
    }
}
