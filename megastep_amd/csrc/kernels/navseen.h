// kernels/navseen.h -- nav_seen_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after navpath.h, whose
// nav_sight_samples gives a ray its samples); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// seen maps: the nav-grid cells that depth rays pass over                  no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsNavSeen) and DESIGN.md section 3.16: a ray is cut at
// min(distance, max_range) and sampled at most half a cell apart, both ends included; the cell under each sample is marked
// in the viewer's map; a call reports, per map, how many countable cells it marked for the first time.  Marks are
// idempotent and the counts are integers, so nothing depends on who marks what or when.
// tests/test_navseen_host.py restates all of it in numpy (seen_rule).
//
// The rule's pieces - seen_ray, seen_sample - are __host__ __device__ functions over plain numbers: ms_host_nav_seen runs
// them on host arrays, so the CPU suite holds this very text to seen_rule, bit for bit.
//
//   nav_seen_kernel   one WORKGROUP a map (n, s): the map's only writer in the call.  The call's marks are a bitmask in
//                     (dynamic) LDS, a bit a cell, sized by the launch from the largest env.  The workgroup zeroes it and
//                     runs the rays of every viewer whose slot is s, the mapping of nav_waypoint_kernel's sight: a wave
//                     takes rays in turn, K is wave-uniform, each lane takes one sample per round of 64 and marks with an
//                     LDS atomic OR.  After a barrier the merge: a lane takes words of the bitmask in turn; a zero word
//                     costs no global traffic; for each set bit the seen byte is read, a 1 stored where it was 0, and the
//                     countable byte counted.  The count is reduced by shuffles within the wave, through LDS across the
//                     waves; one lane stores gained and total.  A reset map is zeroed in global memory by the workgroup
//                     before the barrier (a workgroup's stores are visible to its loads behind one).
struct SeenRay { float ox, oy, ex, ey; int K; };     // the ray cut at its reach: samples o + e*(s/K), s = 0 .. K

// The ray as the samples read it; false: skipped.
__host__ __device__ inline bool seen_ray(const float c, const float ox, const float oy, const float dx, const float dy, const float dist,
                                         const float max_range, SeenRay& r) {
    if (!(nav_finite(ox) && nav_finite(oy) && nav_finite(dx) && nav_finite(dy))) return false;
    const float rlen = sqrtf(dx*dx + dy*dy);
    if (!nav_finite(rlen) || !(rlen > 0.f) || !(dist > 0.f)) return false;      // (a NaN distance is not > 0)
    const float reach = dist < max_range ? dist : max_range;
    const float ux = dx/rlen, uy = dy/rlen;
    r.ox = ox; r.oy = oy;
    r.ex = ux*reach; r.ey = uy*reach;
    const int K = nav_sight_samples(c, r.ex, r.ey);
    if (K < 0) return false;
    r.K = K > 0 ? K : 1;
    return true;
}

// The cell under sample s of the ray, row-major in its env's grid; -1: none (outside the grid, or further than any).
__host__ __device__ inline long long seen_sample(const NavCells& g, const SeenRay& r, const int s) {
    const float t = (float)s/(float)r.K;
    const float x = r.ox + r.ex*t, y = r.oy + r.ey*t;
    const float fx = floorf(x/g.c), fy = floorf(y/g.c);
    if (!(fabsf(fx) < NAV_INDEX_LIMIT) || !(fabsf(fy) < NAV_INDEX_LIMIT)) return -1;
    const long long j = (long long)fx - g.jx0, i = (long long)fy - g.iy0;
    if ((i < 0) | (i >= g.ny) | (j < 0) | (j >= g.nx)) return -1;
    return i*g.nx + j;
}

// One call for one env, serially (host instantiation only): a cell is gained when its byte goes from 0 to 1 and it counts.
inline void seen_serial(const NavCells& g, const unsigned char* countable, const int S, const int P, const int R, const float* origins,
                        const float* dirs, const float* distances, const int* slot, const float max_range, const unsigned char* reset,
                        unsigned char* maps, int* gained, int* total) {
    const long long cells = g.nx > 0 && g.ny > 0 ? (long long)g.nx*g.ny : 0;
    for (int s = 0; s < S; s++) {
        unsigned char* const m = maps + s*cells;
        const bool clear = reset && reset[s];
        int count = 0;
        if (clear) for (long long k = 0; k < cells; k++) m[k] = 0;
        for (int p = 0; p < P && cells > 0; p++) {
            if ((slot ? slot[p] : p) != s) continue;
            for (int k = 0; k < R; k++) {
                SeenRay ray;
                const long long at = (long long)p*R + k;
                if (!seen_ray(g.c, origins[2*p], origins[2*p + 1], dirs[2*at], dirs[2*at + 1], distances[at], max_range, ray)) continue;
                for (int q = 0; q <= ray.K; q++) {
                    const long long cell = seen_sample(g, ray, q);
                    if (cell >= 0 && !m[cell]) { m[cell] = 1; count += countable[cell] & 1; }
                }
            }
        }
        if (gained) gained[s] = count;
        if (total) total[s] = (clear ? 0 : total[s]) + count;
    }
}

struct NavSeenArgs {                                 // MsNavSeen, checked
    const float* origins;                            // (N, P, 2)
    const float* dirs;                               // (N, P, R, 2)
    const float* distances;                          // (N, P, R)
    const int* slot;                                 // (N, P) or NULL
    const unsigned char* reset;                      // (N, S) or NULL
    const unsigned char* countable;                  // (starts[N],)
    unsigned char* maps;
    int* gained;                                     // (N, S) or NULL
    int* total;                                      // (N, S) or NULL
    int n_maps, n_viewers, n_rays, max_cells;
    float max_range;
};

__global__ __launch_bounds__(WG) void nav_seen_kernel(const NavArgs a, const NavSeenArgs q) {
    extern __shared__ unsigned s_marks[];                               // a bit a cell: ceil(max_cells/32) words
    __shared__ int s_count[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long map = blockIdx.x;                                   // (n, s): n S + s
    const int e = (int)(map / q.n_maps), s = (int)(map - (long long)e*q.n_maps);
    const int4 geom = reinterpret_cast<const int4*>(a.geom)[e];
    const long long cells = geom.z > 0 && geom.w > 0 ? (long long)geom.z*geom.w : 0;
    const bool clear = q.reset && q.reset[map];
    if (cells <= 0 || cells > q.max_cells) {                            // (uniform) no cells, or more than the launch has bits for
        if (tid == 0) {
            if (q.gained) q.gained[map] = 0;
            if (q.total && clear) q.total[map] = 0;
        }
        return;
    }
    const NavCells g{geom.x, geom.y, geom.z, geom.w, a.cell};
    const int words = (int)((cells + 31) >> 5);
    unsigned char* const m = q.maps + (long long)q.n_maps*a.starts[e] + (long long)s*cells;
    const unsigned char* const counts = q.countable + a.starts[e];
    for (int k = tid; k < words; k += WG) s_marks[k] = 0u;
    if (clear) for (long long k = tid; k < cells; k += WG) m[k] = 0;
    __syncthreads();

    for (int p = 0; p < q.n_viewers; p++) {
        const long long viewer = (long long)e*q.n_viewers + p;
        if ((q.slot ? q.slot[viewer] : p) != s) continue;               // (uniform)
        const float2 o = reinterpret_cast<const float2*>(q.origins)[viewer];
        for (int k = wave; k < q.n_rays; k += WAVES) {                  // a wave a ray
            const long long at = viewer*q.n_rays + k;
            const float2 d = reinterpret_cast<const float2*>(q.dirs)[at];
            SeenRay ray;
            if (!seen_ray(g.c, o.x, o.y, d.x, d.y, q.distances[at], q.max_range, ray)) continue;      // (uniform)
            for (int s0 = 0; s0 <= ray.K; s0 += 64) {                   // a lane a sample
                const int i = s0 + lane;
                if (i <= ray.K) {
                    const long long cell = seen_sample(g, ray, i);
                    if (cell >= 0) atomicOr(&s_marks[cell >> 5], 1u << (cell & 31));
                }
            }
        }
    }
    __syncthreads();

    int count = 0;
    for (int k = tid; k < words; k += WG) {
        unsigned w = s_marks[k];
        while (w) {                                                     // (a zero word: no global traffic)
            const int b = __ffs((int)w) - 1;
            w &= w - 1;
            const long long cell = ((long long)k << 5) + b;             // (< cells: only cells of the grid are marked)
            if (!m[cell]) { m[cell] = 1; count += counts[cell] & 1; }
        }
    }
    for (int step = 32; step >= 1; step >>= 1) count += __shfl_xor(count, step);
    if (lane == 0) s_count[wave] = count;
    __syncthreads();
    if (tid == 0) {
        int all = 0;
        for (int k = 0; k < WAVES; k++) all += s_count[k];
        if (q.gained) q.gained[map] = all;
        if (q.total) q.total[map] = (clear ? 0 : q.total[map]) + all;
    }
}
