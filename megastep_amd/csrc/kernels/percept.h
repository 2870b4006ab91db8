// kernels/percept.h -- percept_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navview.h: the rule is
// made of the view fields' predicates); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// percepts: the points each eye sees, nearest first                          no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsPercepts) and DESIGN.md section 3.31: point p is a candidate of eye
// (n, e) when `valid` and `pairs` allow it, view_point accepts the eye and view_candidate holds; a candidate is visible when no
// static wall of the env satisfies view_wall_blocks.  Those are navview.h's functions, called, not restated: a pair of an eye
// and a point is a viewpoint and a cell centre to them.  Every output is a copied float, an integer or one correctly rounded
// sqrtf, each element with one writer: any wall order, any cull consistent with `meets` and any schedule give the same bits.
// tests/percept_rule.py restates all of it in numpy.
//
// The pieces below the kernel's schedule - percept_eye, percept_wanted, percept_point, percept_store_pair, percept_key,
// percept_store_near - are __host__ __device__: ms_host_percepts sweeps them serially over host arrays through the kernel's own
// cull, its boxes of 64 points and both wall paths, so the CPU suite holds this very text to percept_rule, bit for bit.
//
//   percept_kernel    one WORKGROUP an env.  The env's static rows are read WG at a time, a row kept when its box meets the union of
//                     the unmasked eyes' view_boxes, and the kept rows compacted into LDS by ballot and prefix count
//                     (VIEW_WALL_CAPACITY rows; more than fit: the env's rows are walked in global memory at wave-uniform addresses
//                     instead, to the same bits).  A wave takes eyes wave, wave + 4, ...; its lanes take points lane + 64 j.  For
//                     each 64 points the wave walks the walls at a uniform index (LDS broadcasts) until no lane holds an unblocked
//                     candidate, passing over - for four comparisons - a wall whose box misses the box of the eye and the wave's
//                     candidates: it fails `meets` for every one of them.  The per-pair outputs are stored, the count is a
//                     popcount of ballots, and the bits of rr of a lane's visible points go to the wave's slice of LDS (each lane
//                     reads only what it wrote).  The nearest K take K rounds: every lane offers its least unused key
//                     (bits(rr) << 32) | p, the wave's minimum goes by shuffles, the lane that owns it retires it and rescans
//                     its own sixteen; lane k keeps round k's key and stores it behind the last round.  No atomics, no scratch.
constexpr int PERCEPT_MAX_EYES = 64, PERCEPT_MAX_POINTS = 1024, PERCEPT_MAX_NEAREST = 16;
constexpr unsigned PERCEPT_HIDDEN = 0xffffffffu;     // in place of bits(rr): rr is never a NaN where visible
constexpr unsigned long long PERCEPT_NONE = ~0ull;   // the key of "no visible point left"

struct PerceptArgs {                                 // MsPercepts, checked
    const float* eyes;                               // (N, E, 2)
    const float* headings;                           // (N, E, 2) or NULL
    const float* points;                             // (N, P, 2)
    const unsigned char* valid;                      // (N, P) or NULL
    const unsigned char* pairs;                      // (E, P) or (N, E, P) or NULL
    const unsigned char* mask;                       // (N, E) or NULL
    unsigned char* visible;                          // (N, E, P) or NULL
    float* squares;                                  // (N, E, P) or NULL
    float* offsets;                                  // (N, E, P, 2) or NULL
    int* counts;                                     // (N, E) or NULL
    int* nearest;                                    // (N, E, K) or NULL
    float* near_offsets;                             // (N, E, K, 2) or NULL
    float* near_distances;                           // (N, E, K) or NULL
    int n_eyes, n_points, n_nearest, pairs_per_env, capacity;
    float R, R2, cos_half;
};

__host__ __device__ inline unsigned percept_bits(const float v) { unsigned u; memcpy(&u, &v, sizeof u); return u; }
__host__ __device__ inline float percept_float(const unsigned u) { float v; memcpy(&v, &u, sizeof v); return v; }

// Eye (n, e) - `at` = n E + e - as the points read it; false: it sees nothing (view_point's verdict).
__host__ __device__ inline bool percept_eye(const PerceptArgs& q, const long long at, ViewPoint& v) {
    return view_point(q.eyes[2*at], q.eyes[2*at + 1], q.headings != nullptr, q.headings ? q.headings[2*at] : 0.f,
                      q.headings ? q.headings[2*at + 1] : 0.f, v);
}

// Do `valid` and `pairs` allow point p of env n to eye e?
__host__ __device__ inline bool percept_wanted(const PerceptArgs& q, const int n, const int e, const int p) {
    if (q.valid && !q.valid[(long long)n*q.n_points + p]) return false;
    if (!q.pairs) return true;
    const long long row = q.pairs_per_env ? (long long)n*q.n_eyes + e : e;
    return q.pairs[row*q.n_points + p] != 0;
}

// Point p of env n against a live eye: is it a candidate?  Leaves the point, its offset from the eye and rr.
__host__ __device__ inline bool percept_point(const PerceptArgs& q, const ViewPoint& v, const int n, const int p, float& x, float& y, float& rx,
                                              float& ry, float& rr) {
    x = q.points[2*((long long)n*q.n_points + p)]; y = q.points[2*((long long)n*q.n_points + p) + 1];
    const bool candidate = view_candidate(v, x, y, q.R2, q.cos_half, rx, ry);
    rr = rx*rx + ry*ry;                                                 // (view_candidate's own rr, formed again: the same two products and sum)
    return candidate;
}

// The per-pair outputs of pair `at` = (n E + e) P + p.
__host__ __device__ inline void percept_store_pair(const PerceptArgs& q, const long long at, const bool visible, const float rx, const float ry,
                                                   const float rr) {
    if (q.visible) q.visible[at] = visible ? 1 : 0;
    if (q.squares) q.squares[at] = visible ? rr : INFINITY;
    if (q.offsets) { q.offsets[2*at] = visible ? rx : NAN; q.offsets[2*at + 1] = visible ? ry : NAN; }
}

// The order of the nearest: rr is not negative, so its bits order as its value; equal distances go to the lower index.
__host__ __device__ inline unsigned long long percept_key(const unsigned bits, const int p) {
    return bits == PERCEPT_HIDDEN ? PERCEPT_NONE : ((unsigned long long)bits << 32) | (unsigned)p;
}

// Entry k of the nearest of eye `at` = n E + e from round k's key: the point's index, its offset (the subtraction view_candidate
// made, made again) and one sqrtf; -1, NaN and +inf beyond the visible ones.
__host__ __device__ inline void percept_store_near(const PerceptArgs& q, const ViewPoint& v, const int n, const long long at, const int k,
                                                   const unsigned long long key) {
    const long long slot = at*q.n_nearest + k;
    const bool some = key != PERCEPT_NONE;
    const int p = some ? (int)(unsigned)key : -1;
    if (q.nearest) q.nearest[slot] = p;
    if (q.near_distances) q.near_distances[slot] = some ? sqrtf(percept_float((unsigned)(key >> 32))) : INFINITY;
    if (q.near_offsets) {
        float rx = NAN, ry = NAN;
        if (some) { rx = q.points[2*((long long)n*q.n_points + p)] - v.px; ry = q.points[2*((long long)n*q.n_points + p) + 1] - v.py; }
        q.near_offsets[2*slot] = rx; q.near_offsets[2*slot + 1] = ry;
    }
}

// The box of everything any unmasked, live eye of env n has in range; false: there is no such eye.
__host__ __device__ inline bool percept_box(const PerceptArgs& q, const int n, ViewBox& box) {
    bool any = false;
    for (int e = 0; e < q.n_eyes; e++) {
        const long long at = (long long)n*q.n_eyes + e;
        if (q.mask && !q.mask[at]) continue;
        ViewPoint v;
        if (!percept_eye(q, at, v)) continue;
        const ViewBox b = view_box(v, q.R, 0.f);
        if (!any) box = b;
        else box = ViewBox{b.x0 < box.x0 ? b.x0 : box.x0, b.y0 < box.y0 ? b.y0 : box.y0, b.x1 > box.x1 ? b.x1 : box.x1, b.y1 > box.y1 ? b.y1 : box.y1};
        any = true;
    }
    return any;
}

// One whole call on host arrays, serially: `walls` holds every env's STATIC rows, env n's from wall_starts[n] on.
inline void percept_serial(const PerceptArgs& q, const int n_envs, const float4* walls, const long long* wall_starts) {
    std::vector<float4> staged((size_t)(q.capacity > 0 ? q.capacity : 1));
    std::vector<unsigned> keys((size_t)PERCEPT_MAX_POINTS);
    const int E = q.n_eyes, P = q.n_points, K = q.n_nearest;
    for (int n = 0; n < n_envs; n++) {
        const float4* const rows = walls + wall_starts[n];
        const long long n_rows = wall_starts[n + 1] - wall_starts[n];
        long long kept = 0;
        ViewBox box{0.f, 0.f, 0.f, 0.f};
        if (percept_box(q, n, box))
            for (long long l = 0; l < n_rows; l++)
                if (view_keeps(box, rows[l])) {
                    if (kept < q.capacity) staged[(size_t)kept] = rows[l];
                    kept++;
                }
        const bool overflow = kept > q.capacity;
        for (int e = 0; e < E; e++) {
            const long long at = (long long)n*E + e;
            if (q.mask && !q.mask[at]) continue;
            ViewPoint v;
            const bool live = percept_eye(q, at, v);
            int count = 0;
            for (int p0 = 0; p0 < P; p0 += WAVE) {                      // a wave's 64 points
                const int p1 = p0 + WAVE < P ? p0 + WAVE : P;
                float xa = INFINITY, ya = INFINITY, xb = -INFINITY, yb = -INFINITY;
                for (int p = p0; p < p1; p++) {
                    float x, y, rx, ry, rr;
                    if (live && percept_wanted(q, n, e, p) && percept_point(q, v, n, p, x, y, rx, ry, rr)) {
                        xa = x < xa ? x : xa; ya = y < ya ? y : ya; xb = x > xb ? x : xb; yb = y > yb ? y : yb;
                    }
                }
                const ViewBox tile = view_tile_box(v, xa, ya, xb, yb);
                for (int p = p0; p < p1; p++) {
                    float x = 0.f, y = 0.f, rx = 0.f, ry = 0.f, rr = 0.f;
                    bool visible = live && percept_wanted(q, n, e, p) && percept_point(q, v, n, p, x, y, rx, ry, rr);
                    if (!overflow)
                        for (long long k = 0; k < kept && visible; k++)
                            visible = !(view_keeps(tile, staged[(size_t)k]) && view_wall_blocks(v.px, v.py, x, y, rx, ry, staged[(size_t)k]));
                    else
                        for (long long l = 0; l < n_rows && visible; l++)
                            visible = !(view_keeps(tile, rows[l]) && view_wall_blocks(v.px, v.py, x, y, rx, ry, rows[l]));
                    percept_store_pair(q, at*P + p, visible, rx, ry, rr);
                    keys[(size_t)p] = visible ? percept_bits(rr) : PERCEPT_HIDDEN;
                    count += visible;
                }
            }
            if (q.counts) q.counts[at] = count;
            if (q.nearest || q.near_offsets || q.near_distances)
                for (int k = 0; k < K; k++) {
                    unsigned long long best = PERCEPT_NONE;
                    for (int p = 0; p < P; p++) {
                        const unsigned long long key = percept_key(keys[(size_t)p], p);
                        best = key < best ? key : best;
                    }
                    if (best != PERCEPT_NONE) keys[(size_t)(unsigned)best] = PERCEPT_HIDDEN;
                    percept_store_near(q, v, n, at, k, best);
                }
        }
    }
}

// A lane's least unused key among its points lane + 64 j.
__device__ inline unsigned long long percept_lane_least(const unsigned* keys, const int lane, const int chunks) {
    unsigned long long best = PERCEPT_NONE;
    for (int j = 0; j < chunks; j++) {
        const unsigned long long key = percept_key(keys[j*WAVE + lane], j*WAVE + lane);
        best = key < best ? key : best;
    }
    return best;
}

__device__ inline float percept_wave_min(float v) {
    for (int s = 32; s > 0; s >>= 1) { const float o = __shfl_xor(v, s); v = o < v ? o : v; }
    return v;
}
__device__ inline float percept_wave_max(float v) {
    for (int s = 32; s > 0; s >>= 1) { const float o = __shfl_xor(v, s); v = o > v ? o : v; }
    return v;
}

__global__ __launch_bounds__(WG) void percept_kernel(const MsScenery sc, const PerceptArgs q) {
    __shared__ float4 s_walls[VIEW_WALL_CAPACITY];
    __shared__ unsigned s_keys[WAVES][PERCEPT_MAX_POINTS];
    __shared__ int s_kept[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.x;
    const int E = q.n_eyes, P = q.n_points, K = q.n_nearest;

    // the walls that can matter to any eye of the env, compacted into LDS in their own order
    const int AF = sc.n_agents*sc.n_model;
    const int L = sc.lines_widths[n];
    const float4* const rows = reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[n];
    int kept = 0;                                                       // (uniform)
    ViewBox box{0.f, 0.f, 0.f, 0.f};
    if (percept_box(q, n, box)) {                                       // (uniform)
        for (int l0 = AF; l0 < L; l0 += WG) {
            const int l = l0 + tid;
            float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
            bool keep = false;
            if (l < L) { row = rows[l]; keep = view_keeps(box, row); }
            const unsigned long long votes = __ballot(keep);
            if (lane == 0) s_kept[wave] = (int)__popcll(votes);
            __syncthreads();
            int at = kept, all = 0;
            for (int k = 0; k < WAVES; k++) { const int c = s_kept[k]; at += k < wave ? c : 0; all += c; }
            at += (int)__popcll(votes & ((1ull << lane) - 1ull));
            if (keep && at < q.capacity) s_walls[at] = row;
            kept += all;
            __syncthreads();
        }
    }
    const bool overflow = kept > q.capacity;                            // (uniform)

    // the eyes: a wave an eye, a lane the points lane + 64 j
    unsigned* const keys = s_keys[wave];
    const int chunks = (P + WAVE - 1)/WAVE;
    for (int e = wave; e < E; e += WAVES) {
        const long long at = (long long)n*E + e;
        if (q.mask && !q.mask[at]) continue;                            // (uniform)
        ViewPoint v;
        const bool live = percept_eye(q, at, v);
        int count = 0;                                                  // (uniform within the wave)
        for (int j = 0; j < chunks; j++) {
            const int p = j*WAVE + lane;
            const bool mine = p < P;
            float x = 0.f, y = 0.f, rx = 0.f, ry = 0.f, rr = 0.f;
            const bool candidate = mine && live && percept_wanted(q, n, e, p) && percept_point(q, v, n, p, x, y, rx, ry, rr);
            const ViewBox tile = view_tile_box(v, percept_wave_min(candidate ? x : INFINITY), percept_wave_min(candidate ? y : INFINITY),
                                               percept_wave_max(candidate ? x : -INFINITY), percept_wave_max(candidate ? y : -INFINITY));
            bool blocked = !candidate;
            // (measured: fetching the next row while this one is tested costs a third more time, not less - the walk is bound by
            // its arithmetic, not by the rows' latency)
            if (!overflow) {
                for (int l = 0; l < kept; l++) {
                    if (__ballot(!blocked) == 0ull) break;
                    const float4 row = s_walls[l];
                    if (__ballot(view_keeps(tile, row)) == 0ull) continue;  // (uniform: the wall fails `meets` for every candidate of the wave)
                    if (!blocked) blocked = view_wall_blocks(v.px, v.py, x, y, rx, ry, row);
                }
            } else {
                for (int l = AF; l < L; l++) {
                    if (__ballot(!blocked) == 0ull) break;
                    const float4 row = rows[l];
                    if (__ballot(view_keeps(tile, row)) == 0ull) continue;
                    if (!blocked) blocked = view_wall_blocks(v.px, v.py, x, y, rx, ry, row);
                }
            }
            const bool visible = candidate & !blocked;
            if (mine) percept_store_pair(q, at*P + p, visible, rx, ry, rr);
            keys[j*WAVE + lane] = visible ? percept_bits(rr) : PERCEPT_HIDDEN;      // (j*64 + lane < 1024: ms_percepts checks P)
            count += (int)__popcll(__ballot(visible));
        }
        if (lane == 0 && q.counts) q.counts[at] = count;

        // the nearest K: K rounds of the wave's least key
        if (K > 0 && (q.nearest || q.near_offsets || q.near_distances)) {
            unsigned long long offer = percept_lane_least(keys, lane, chunks), round_key = PERCEPT_NONE;
            for (int k = 0; k < K; k++) {
                unsigned lo = (unsigned)offer, hi = (unsigned)(offer >> 32);
                for (int s = 32; s > 0; s >>= 1) {
                    const unsigned olo = __shfl_xor(lo, s), ohi = __shfl_xor(hi, s);
                    const bool less = (ohi < hi) | ((ohi == hi) & (olo < lo));
                    lo = less ? olo : lo; hi = less ? ohi : hi;
                }
                const unsigned long long least = ((unsigned long long)hi << 32) | lo;
                if (least == PERCEPT_NONE) break;                       // (uniform: nothing visible is left)
                if (lane == k) round_key = least;
                if (offer == least) {                                   // (one lane: the keys differ in p)
                    keys[lo] = PERCEPT_HIDDEN;
                    offer = percept_lane_least(keys, lane, chunks);
                }
            }
            if (lane < K) percept_store_near(q, v, n, at, lane, round_key);
        }
    }
}
