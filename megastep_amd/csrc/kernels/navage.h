// kernels/navage.h -- nav_age_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navseen.h, whose
// seen_ray and seen_sample say which cells a call marks); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// age maps: the tick at which each nav-grid cell was last under a depth ray   no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavAges) and DESIGN.md section 3.25: a map keeps, per cell, the
// tick of its clock at which the cell was last marked (0: never); a call moves the clock on by one, marks the SET of cells
// under its rays' samples, and reports how many countable cells it swept, how many of them for the first time, and the sum
// of their ages; a survey then gives every cell's age, the countable cells' largest and summed age, and which are stale.
// Integers throughout, each with one definition, so nothing depends on who marks what or when.
// tests/test_navage_host.py restates all of it in numpy (age_rule).
//
// The rule's pieces - age_now, age_mark, age_survey - are __host__ __device__ functions over plain numbers: ms_host_nav_ages
// runs them (age_serial) on host arrays, so the CPU suite holds this very text to age_rule, bit for bit.
//
//   nav_age_kernel    one WORKGROUP a map (n, s), the map's only writer in the call: nav_seen_kernel's scheme.  MARK: the
//                     call's marks are a bitmask in (dynamic) LDS, a bit a cell, sized by the launch from the largest env;
//                     a wave takes rays in turn, a lane a sample, an LDS atomic OR.  MERGE, behind a barrier: a lane takes
//                     words of the bitmask in turn; a zero word costs no global traffic; per set bit one dword load and one
//                     dword store of `last`.  The two int32 counts and the int64 sum are reduced by shuffles within the wave,
//                     through LDS across the waves; one lane stores them and the clock.  SURVEY, behind a second barrier (a
//                     workgroup's own stores are visible to its loads behind one - the seen kernel's argument for its reset):
//                     a lane a cell, coalesced dword loads of `last`, dword and byte stores of `ages` and `stale` (a map's
//                     start is not 16-byte aligned: nothing wider); maximum, sum and count reduced the same way.  Whether
//                     there is a survey, and each optional store, is a wave-uniform pointer test.
constexpr int AGE_MAX_TICK = 1 << 24;                // binary32 holds every tick up to here exactly

// The tick of a call: the clock as it was (0 after a reset), moved on by one - up to the cap - when the call advances.
__host__ __device__ inline int age_now(const int clock, const bool clear, const bool advance) {
    const int before = clear ? 0 : clock;
    if (!advance) return before;
    return before + 1 < AGE_MAX_TICK ? before + 1 : AGE_MAX_TICK;
}

struct AgeSweep { int swept, gained; long long idle; };     // a call's marks, over the countable cells
struct AgeSurvey { int oldest, n_stale; long long total; }; // a call's survey, over the countable cells

// One marked cell: its tick becomes `now`; a countable one is counted with the age it had.
__host__ __device__ inline void age_mark(float* const last, const unsigned char counts, const int now, AgeSweep& w) {
    const float before = *last;
    const int age = now - (int)before;
    *last = (float)now;
    if (counts & 1) {
        w.swept += 1;
        w.gained += before == 0.f;
        w.idle += age;
    }
}

// One cell of the survey: its age and whether it is stale, stored where asked; a countable one goes into the statistics.
__host__ __device__ inline void age_survey(const float last, const unsigned char counts, const int now, const int threshold,
                                           unsigned char* const stale, float* const ages, AgeSurvey& v) {
    const int age = now - (int)last;
    const bool counted = counts & 1;
    const bool old = counted && age >= threshold;
    if (stale) *stale = old ? 1 : 0;
    if (ages) *ages = (float)age;
    if (counted) {
        v.oldest = age > v.oldest ? age : v.oldest;
        v.n_stale += old;
        v.total += age;
    }
}

struct NavAgeArgs {                                  // MsNavAges, checked
    const float* origins;                            // (N, P, 2)
    const float* dirs;                               // (N, P, R, 2)
    const float* distances;                          // (N, P, R)
    const int* slot;                                 // (N, P) or NULL
    const unsigned char* reset;                      // (N, S) or NULL
    const unsigned char* countable;                  // (starts[N],)
    float* last;
    int* clock;                                      // (N, S)
    int* swept;                                      // (N, S) or NULL, as are all below
    int* gained;
    long long* idle;
    int* oldest;
    long long* total_age;
    int* n_stale;
    unsigned char* stale;
    float* ages;
    int n_maps, n_viewers, n_rays, max_cells, advance, threshold;
    float max_range;
};

__host__ __device__ inline bool age_surveys(const NavAgeArgs& q) { return q.oldest || q.total_age || q.n_stale || q.stale || q.ages; }

// A map's numbers, stored where asked: the marks' with its clock, and the survey's.
__host__ __device__ inline void age_store(const NavAgeArgs& q, const long long map, const int now, const AgeSweep w) {
    if (q.swept) q.swept[map] = w.swept;
    if (q.gained) q.gained[map] = w.gained;
    if (q.idle) q.idle[map] = w.idle;
    q.clock[map] = now;
}
__host__ __device__ inline void age_store(const NavAgeArgs& q, const long long map, const AgeSurvey v) {
    if (q.oldest) q.oldest[map] = v.oldest;
    if (q.total_age) q.total_age[map] = v.total;
    if (q.n_stale) q.n_stale[map] = v.n_stale;
}

// One call for one env, serially (host instantiation only): q's pointers hold the one env's share.  The marks are the
// kernel's bitmask, so a cell under many samples is marked once.
inline void age_serial(const NavCells& g, const NavAgeArgs& q) {
    const long long cells = g.nx > 0 && g.ny > 0 ? (long long)g.nx*g.ny : 0;
    const bool survey = age_surveys(q);
    for (int s = 0; s < q.n_maps; s++) {
        const bool clear = q.reset && q.reset[s];
        const int now = age_now(q.clock[s], clear, q.advance != 0);
        AgeSweep w{0, 0, 0};
        AgeSurvey v{0, 0, 0};
        if (cells <= 0) {
            age_store(q, s, now, w);
            if (survey) age_store(q, s, v);
            continue;
        }
        float* const last = q.last + s*cells;
        if (clear) for (long long k = 0; k < cells; k++) last[k] = 0.f;
        if (q.advance) {
            std::vector<unsigned> marks((size_t)((cells + 31) >> 5), 0u);
            for (int p = 0; p < q.n_viewers; p++) {
                if ((q.slot ? q.slot[p] : p) != s) continue;
                for (int k = 0; k < q.n_rays; k++) {
                    SeenRay ray;
                    const long long at = (long long)p*q.n_rays + k;
                    if (!seen_ray(g.c, q.origins[2*p], q.origins[2*p + 1], q.dirs[2*at], q.dirs[2*at + 1], q.distances[at], q.max_range, ray)) continue;
                    for (int i = 0; i <= ray.K; i++) {
                        const long long cell = seen_sample(g, ray, i);
                        if (cell >= 0) marks[(size_t)(cell >> 5)] |= 1u << (cell & 31);
                    }
                }
            }
            for (long long cell = 0; cell < cells; cell++)
                if (marks[(size_t)(cell >> 5)] >> (cell & 31) & 1u) age_mark(last + cell, q.countable[cell], now, w);
        }
        if (survey)
            for (long long k = 0; k < cells; k++)
                age_survey(last[k], q.countable[k], now, q.threshold, q.stale ? q.stale + s*cells + k : nullptr,
                           q.ages ? q.ages + s*cells + k : nullptr, v);
        age_store(q, s, now, w);
        if (survey) age_store(q, s, v);
    }
}

__global__ __launch_bounds__(WG) void nav_age_kernel(const NavArgs a, const NavAgeArgs q) {
    extern __shared__ unsigned s_age_marks[];                           // a bit a cell: ceil(max_cells/32) words
    __shared__ int s_first[WAVES], s_second[WAVES];
    __shared__ long long s_sum[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long map = blockIdx.x;                                   // (n, s): n S + s
    const int e = (int)(map / q.n_maps), s = (int)(map - (long long)e*q.n_maps);
    const int4 geom = reinterpret_cast<const int4*>(a.geom)[e];
    const long long cells = geom.z > 0 && geom.w > 0 ? (long long)geom.z*geom.w : 0;
    const bool clear = q.reset && q.reset[map];
    const bool survey = age_surveys(q);                                 // (uniform)
    const int now = age_now(q.clock[map], clear, q.advance != 0);       // (read by all before the first barrier, stored behind it)
    if (cells <= 0 || cells > q.max_cells) {                            // (uniform) no cells, or more than the launch has bits for
        __syncthreads();                                                // (every lane has read the clock)
        if (tid == 0) {
            age_store(q, map, now, AgeSweep{0, 0, 0});
            if (survey) age_store(q, map, AgeSurvey{0, 0, 0});
        }
        return;
    }
    const NavCells g{geom.x, geom.y, geom.z, geom.w, a.cell};
    const int words = (int)((cells + 31) >> 5);
    const long long first = (long long)q.n_maps*a.starts[e] + (long long)s*cells;
    float* const last = q.last + first;
    const unsigned char* const counts = q.countable + a.starts[e];
    for (int k = tid; k < words; k += WG) s_age_marks[k] = 0u;
    if (clear) for (long long k = tid; k < cells; k += WG) last[k] = 0.f;
    __syncthreads();

    AgeSweep w{0, 0, 0};
    if (q.advance) {                                                    // (uniform)
        for (int p = 0; p < q.n_viewers; p++) {
            const long long viewer = (long long)e*q.n_viewers + p;
            if ((q.slot ? q.slot[viewer] : p) != s) continue;           // (uniform)
            const float2 o = reinterpret_cast<const float2*>(q.origins)[viewer];
            for (int k = wave; k < q.n_rays; k += WAVES) {              // a wave a ray
                const long long at = viewer*q.n_rays + k;
                const float2 d = reinterpret_cast<const float2*>(q.dirs)[at];
                SeenRay ray;
                if (!seen_ray(g.c, o.x, o.y, d.x, d.y, q.distances[at], q.max_range, ray)) continue;      // (uniform)
                for (int s0 = 0; s0 <= ray.K; s0 += 64) {               // a lane a sample
                    const int i = s0 + lane;
                    if (i <= ray.K) {
                        const long long cell = seen_sample(g, ray, i);
                        if (cell >= 0) atomicOr(&s_age_marks[cell >> 5], 1u << (cell & 31));
                    }
                }
            }
        }
        __syncthreads();
        for (int k = tid; k < words; k += WG) {
            unsigned m = s_age_marks[k];
            while (m) {                                                 // (a zero word: no global traffic)
                const int b = __ffs((int)m) - 1;
                m &= m - 1;
                const long long cell = ((long long)k << 5) + b;         // (< cells: only cells of the grid are marked)
                age_mark(last + cell, counts[cell], now, w);
            }
        }
    }
    for (int step = 32; step >= 1; step >>= 1) {
        w.swept += __shfl_xor(w.swept, step);
        w.gained += __shfl_xor(w.gained, step);
        w.idle += __shfl_xor(w.idle, step);
    }
    if (lane == 0) { s_first[wave] = w.swept; s_second[wave] = w.gained; s_sum[wave] = w.idle; }
    __syncthreads();
    if (tid == 0) {
        AgeSweep all{0, 0, 0};
        for (int k = 0; k < WAVES; k++) { all.swept += s_first[k]; all.gained += s_second[k]; all.idle += s_sum[k]; }
        age_store(q, map, now, all);
    }
    if (!survey) return;                                                // (uniform)
    __syncthreads();                                                    // (the merge's stores of `last`, and lane 0's reads of the sums)

    AgeSurvey v{0, 0, 0};
    unsigned char* const stale = q.stale ? q.stale + first : nullptr;
    float* const ages = q.ages ? q.ages + first : nullptr;
    for (long long k = tid; k < cells; k += WG)
        age_survey(last[k], counts[k], now, q.threshold, stale ? stale + k : nullptr, ages ? ages + k : nullptr, v);
    for (int step = 32; step >= 1; step >>= 1) {
        const int other = __shfl_xor(v.oldest, step);
        v.oldest = other > v.oldest ? other : v.oldest;
        v.n_stale += __shfl_xor(v.n_stale, step);
        v.total += __shfl_xor(v.total, step);
    }
    if (lane == 0) { s_first[wave] = v.oldest; s_second[wave] = v.n_stale; s_sum[wave] = v.total; }
    __syncthreads();
    if (tid == 0) {
        AgeSurvey all{0, 0, 0};
        for (int k = 0; k < WAVES; k++) {
            all.oldest = s_first[k] > all.oldest ? s_first[k] : all.oldest;
            all.n_stale += s_second[k];
            all.total += s_sum[k];
        }
        age_store(q, map, all);
    }
}
