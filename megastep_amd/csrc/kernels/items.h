// kernels/items.h -- item_collect_kernel, item_overlay_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after percept.h: the reach
// test is made of the view fields' view_wall_blocks, the overlay of raycast.h's ray_fold); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// items: things in the world that agents see, touch and collect               no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsItemCollect, MsItemOverlay) and DESIGN.md section 3.34.  An item is
// present exactly when both its coordinates are finite; an absent one holds (NaN, NaN), which fails the reach test and gives a
// billboard the fold never hits.  Every output of the collect is an integer or a stored NaN; every output of the overlay is a
// float ray_fold made, one product or quotient of such, or an integer - each element with one writer: any schedule gives the same
// bits.  tests/item_rule.py restates all of it in numpy.
//
// The pieces below the kernels' schedules - item_present, item_reaches, item_key, item_settle; item_billboard, item_row_live,
// item_ray - are __host__ __device__: ms_host_item_collect and ms_host_item_overlay sweep them serially over host
// arrays, so the CPU suite holds this very text to item_rule, bit for bit.
//
//   item_collect_kernel   one WAVE an env, a lane the items lane + 64 j.  The A agents are read at wave-uniform addresses; for each
//                     agent the lanes whose item is in its reach are balloted, and only when some are does the wave walk the env's
//                     static rows at a uniform index, until every such lane is blocked or the rows end.  The least key
//                     (bits(rr) << 32) | a stays in a register; the item is settled - taken, ticked, due - by its own lane; the
//                     counts go through integer LDS atomics into the wave's slice and are stored whole.  No float atomics.
//   item_overlay_kernel   one WORKGROUP up to 256 rays of one origin.  A lane an item, it builds the P billboards for that origin -
//                     one sqrtf and two divisions per item and origin, not per ray - drops the rows with a NaN and compacts the
//                     rest in ascending k into LDS by ballot, popcount and a prefix over the waves (nav_draw_kernel's and
//                     percept_kernel's idiom); then every lane folds its ray over the compacted rows (LDS broadcasts).  A workgroup
//                     without a live row writes items = -1 and returns.  No cull: none is part of the rule.
constexpr int ITEM_MAX_ITEMS = 1024, ITEM_MAX_AGENTS = 64, ITEM_MAX_KINDS = 8;
constexpr unsigned long long ITEM_NONE = ~0ull;      // the key of "no candidate"

struct ItemCollectArgs {                             // MsItemCollect, checked
    float* positions;                                // (N, P, 2)
    int* timers;                                     // (N, P)
    const int* kinds;                                // (N, P)
    const unsigned char* takers;                     // (N, A) or NULL
    const unsigned char* reset;                      // (N,) or NULL
    const float* agents;                             // (N, A, 2): the agents' positions
    int* taker;                                      // (N, P) or NULL
    int* counts;                                     // (N, A, K) or NULL
    unsigned char* due;                              // (N, P) or NULL
    int n_envs, n_agents, n_items, n_kinds, delay, through_walls;
    float reach2;
};

__host__ __device__ inline bool item_present(const float x, const float y) { return nav_finite(x) && nav_finite(y); }

// May agent a of env n take at all, and where is it?  false: a masked agent or one that is nowhere.
__host__ __device__ inline bool item_agent(const ItemCollectArgs& q, const int n, const int a, float& px, float& py) {
    const long long at = (long long)n*q.n_agents + a;
    px = q.agents[2*at]; py = q.agents[2*at + 1];
    if (q.takers && !q.takers[at]) return false;
    return nav_finite(px) && nav_finite(py);
}

// Is the item at (x, y) within the reach of an agent at (px, py)?  Leaves the offset and rr.  (A NaN item fails rr <= reach2.)
__host__ __device__ inline bool item_reaches(const ItemCollectArgs& q, const float px, const float py, const float x, const float y, float& rx,
                                             float& ry, float& rr) {
    rx = x - px; ry = y - py;
    rr = rx*rx + ry*ry;
    return rr <= q.reach2;
}

// The order of the takers: rr is not negative, so its bits order as its value; equal distances go to the lower index.
__host__ __device__ inline unsigned long long item_key(const float rr, const int a) { return ((unsigned long long)percept_bits(rr) << 32) | (unsigned)a; }

// Item `at` = n P + k after its candidates are known (`key`: the least, or ITEM_NONE; `present`: as it was on entry; `reset`:
// its env is being emptied): taken, tick, due and the stores.  Returns the taker, or -1.
__host__ __device__ inline int item_settle(const ItemCollectArgs& q, const long long at, const bool reset, const bool present,
                                           const unsigned long long key) {
    const int taker = (!reset && present && key != ITEM_NONE) ? (int)(unsigned)key : -1;
    int timer = q.timers[at];
    bool absent = !present;
    if (reset) { timer = 0; absent = true; }
    else if (taker >= 0) { timer = q.delay; absent = true; }
    else if (!present) timer = timer > 0 ? timer - 1 : timer;
    if (reset || taker >= 0) { q.positions[2*at] = NAN; q.positions[2*at + 1] = NAN; }
    if (reset || taker >= 0 || !present) q.timers[at] = timer;
    if (q.taker) q.taker[at] = taker;
    if (q.due) q.due[at] = (absent && timer == 0) ? 1 : 0;
    return taker;
}

// One whole call on host arrays, serially: `walls` holds every env's STATIC rows, env n's from wall_starts[n] on.
inline void item_collect_serial(const ItemCollectArgs& q, const float4* walls, const long long* wall_starts) {
    const int A = q.n_agents, P = q.n_items, K = q.n_kinds;
    for (int n = 0; n < q.n_envs; n++) {
        const float4* const rows = walls + wall_starts[n];
        const long long n_rows = wall_starts[n + 1] - wall_starts[n];
        const bool reset = q.reset && q.reset[n];
        if (q.counts) for (int i = 0; i < A*K; i++) q.counts[(long long)n*A*K + i] = 0;
        for (int k = 0; k < P; k++) {
            const long long at = (long long)n*P + k;
            const float x = q.positions[2*at], y = q.positions[2*at + 1];
            const bool present = item_present(x, y);
            unsigned long long best = ITEM_NONE;
            if (!reset && present)
                for (int a = 0; a < A; a++) {
                    float px, py, rx, ry, rr;
                    if (!item_agent(q, n, a, px, py) || !item_reaches(q, px, py, x, y, rx, ry, rr)) continue;
                    bool blocked = false;
                    if (!q.through_walls)
                        for (long long l = 0; l < n_rows && !blocked; l++) blocked = view_wall_blocks(px, py, x, y, rx, ry, rows[l]);
                    if (blocked) continue;
                    const unsigned long long key = item_key(rr, a);
                    best = key < best ? key : best;
                }
            const int taker = item_settle(q, at, reset, present, best);
            const int kind = q.kinds[at];
            if (taker >= 0 && q.counts && kind >= 0 && kind < K) q.counts[((long long)n*A + taker)*K + kind]++;
        }
    }
}

__global__ __launch_bounds__(WG) void item_collect_kernel(const MsScenery sc, const ItemCollectArgs q) {
    __shared__ int s_counts[WAVES][ITEM_MAX_AGENTS*ITEM_MAX_KINDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.x*WAVES + wave;                              // (uniform)
    const bool live = n < q.n_envs;
    const int A = q.n_agents, P = q.n_items, K = q.n_kinds;
    int* const tally = s_counts[wave];
    for (int i = lane; i < A*K; i += WAVE) tally[i] = 0;                // (A K <= 512: ms_item_collect checks both)
    __syncthreads();
    if (live) {
        const bool reset = q.reset && q.reset[n];                       // (uniform)
        const int AF = sc.n_agents*sc.n_model;
        const int L = sc.lines_widths[n];
        const float4* const rows = reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[n];
        for (int k = lane; k - lane < P; k += WAVE) {                   // (the wave's chunks in step: the ballots below are whole)
            const bool mine = k < P;
            const long long at = (long long)n*P + (mine ? k : P - 1);   // (spare lanes of the last chunk read its last item, store nothing)
            const float2 c = reinterpret_cast<const float2*>(q.positions)[at];
            const bool present = mine && item_present(c.x, c.y);
            unsigned long long best = ITEM_NONE;
            if (!reset)
                for (int a = 0; a < A; a++) {
                    float px, py, rx = 0.f, ry = 0.f, rr = 0.f;
                    if (!item_agent(q, n, a, px, py)) continue;         // (uniform)
                    const bool reached = present && item_reaches(q, px, py, c.x, c.y, rx, ry, rr);
                    if (__ballot(reached) == 0ull) continue;            // (uniform: nobody's item is in this agent's reach)
                    bool blocked = !reached;
                    if (!q.through_walls)
                        for (int l = AF; l < L; l++) {
                            if (__ballot(!blocked) == 0ull) break;
                            const float4 row = rows[l];
                            if (!blocked) blocked = view_wall_blocks(px, py, c.x, c.y, rx, ry, row);
                        }
                    if (!blocked) { const unsigned long long key = item_key(rr, a); best = key < best ? key : best; }
                }
            if (mine) {
                const int taker = item_settle(q, at, reset, present, best);
                const int kind = q.kinds[at];
                if (taker >= 0 && kind >= 0 && kind < K) atomicAdd(&tally[taker*K + kind], 1);
            }
        }
    }
    __syncthreads();
    if (live && q.counts)
        for (int i = lane; i < A*K; i += WAVE) q.counts[(long long)n*A*K + i] = tally[i];
}

struct ItemOverlayArgs {                             // MsItemOverlay, checked
    const float* positions;                          // (N, P, 2)
    const float* colors;                             // (N, P, 3) or NULL
    const float* origins;                            // (N, Q, 2)
    const float* dirs;                               // (N, R, 2)
    const int* lines_widths;                         // (N,): MsScenery's
    float* distances;                                // (N, R)
    int* indices;                                    // (N, R) or NULL
    float* locations;                                // (N, R) or NULL
    float* dots;                                     // (N, R) or NULL
    float* screen;                                   // (N, R, 3) or NULL
    int* items;                                      // (N, R) or NULL
    int n_envs, n_items, n_rays, n_origins, per_origin, chunks;
    float radius, near_plane;
};

// Item at c as origin p sees it: a segment of length 2 radius across the line of sight.
__host__ __device__ inline float4 item_billboard(const P2 p, const float cx, const float cy, const float radius) {
    const float ux = cx - p.x, uy = cy - p.y;
    const float l = sqrtf(ux*ux + uy*uy);
    const float nx = (-uy/l)*radius, ny = (ux/l)*radius;
    return make_float4(cx - nx, cy - ny, cx + nx, cy + ny);
}

// Can the fold ever hit the row?  Not with a NaN in it (ray_fold's own test fails): an absent item, an origin on the item.
__host__ __device__ inline bool item_row_live(const float4 row) { return (row.x == row.x) & (row.y == row.y) & (row.z == row.z) & (row.w == row.w); }

// Ray i = n R + r over the `kept` live rows of its origin (their items' numbers in `ks`, ascending): the fold, then the winner
// against what the planes hold.
__host__ __device__ inline void item_ray(const ItemOverlayArgs& q, const int n, const long long i, const P2 p, const float4* rows, const int* ks,
                                         const int kept) {
    const P2 ru = p2(q.dirs[2*i], q.dirs[2*i + 1]);
    const float rlen = len(ru);
    const float near_s = q.near_plane/rlen;
    RayFold f{INFINITY, -1, NAN, 0.f, 0.f};
    for (int j = 0; j < kept; j++) ray_fold(p, ru, near_s, rows[j], ks[j], f);
    int won = -1;
    if (f.idx >= 0) {
        const float d = f.s*rlen;
        if (d < q.distances[i]) {
            won = f.idx;
            const float dtop = dot(ru, p2(f.vx, f.vy));                 // (raycast_kernel's closing lines, kernels.cu:360-364)
            const float dbot = rlen*len(p2(f.vx, f.vy));
            const float dt = dtop/(dbot + 1.e-6f);
            q.distances[i] = d;
            if (q.screen) {
                const float dn = 1.f - dt*dt;
                const float* const rgb = q.colors + 3*((long long)n*q.n_items + won);
                q.screen[3*i] = dn*rgb[0]; q.screen[3*i + 1] = dn*rgb[1]; q.screen[3*i + 2] = dn*rgb[2];
            }
            if (q.indices) q.indices[i] = q.lines_widths[n] + won;
            if (q.locations) q.locations[i] = f.t;
            if (q.dots) q.dots[i] = dt;
        }
    }
    if (q.items) q.items[i] = won;
}

// One whole call on host arrays, serially, origin by origin through the kernel's own compaction.
inline void item_overlay_serial(const ItemOverlayArgs& q) {
    std::vector<float4> rows((size_t)ITEM_MAX_ITEMS);
    std::vector<int> ks((size_t)ITEM_MAX_ITEMS);
    const int P = q.n_items, Q = q.n_origins;
    for (int n = 0; n < q.n_envs; n++)
        for (int o = 0; o < Q; o++) {
            const long long oq = (long long)n*Q + o;
            const P2 p = p2(q.origins[2*oq], q.origins[2*oq + 1]);
            int kept = 0;
            for (int k = 0; k < P; k++) {
                const long long at = (long long)n*P + k;
                const float4 row = item_billboard(p, q.positions[2*at], q.positions[2*at + 1], q.radius);
                if (item_row_live(row)) { rows[(size_t)kept] = row; ks[(size_t)kept] = k; kept++; }
            }
            for (int r = 0; r < q.per_origin; r++)
                item_ray(q, n, (long long)n*q.n_rays + (long long)o*q.per_origin + r, p, rows.data(), ks.data(), kept);
        }
}

__global__ __launch_bounds__(WG) void item_overlay_kernel(const ItemOverlayArgs q) {
    __shared__ float4 s_rows[ITEM_MAX_ITEMS];
    __shared__ int s_ks[ITEM_MAX_ITEMS];
    __shared__ int s_kept[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int oq = blockIdx.x / q.chunks, chunk = blockIdx.x - oq*q.chunks;         // (n Q + o) and the chunk of its rays
    const int n = oq / q.n_origins, o = oq - n*q.n_origins;
    const int P = q.n_items;
    const float2 origin = reinterpret_cast<const float2*>(q.origins)[oq];
    const P2 p = p2(origin.x, origin.y);

    // the billboards this origin sees, compacted into LDS in ascending k
    int kept = 0;                                                       // (uniform)
    for (int k0 = 0; k0 < P; k0 += WG) {
        const int k = k0 + tid;
        float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
        bool keep = false;
        if (k < P) {
            const float2 c = reinterpret_cast<const float2*>(q.positions)[(long long)n*P + k];
            row = item_billboard(p, c.x, c.y, q.radius);
            keep = item_row_live(row);
        }
        const unsigned long long votes = __ballot(keep);
        if (lane == 0) s_kept[wave] = (int)__popcll(votes);
        __syncthreads();
        int at = kept, all = 0;
        for (int w = 0; w < WAVES; w++) { const int c = s_kept[w]; at += w < wave ? c : 0; all += c; }
        at += (int)__popcll(votes & ((1ull << lane) - 1ull));
        if (keep) { s_rows[at] = row; s_ks[at] = k; }                   // (at < P <= 1024: ms_item_overlay checks P)
        kept += all;
        __syncthreads();
    }

    const int r = chunk*WG + tid;
    if (r >= q.per_origin) return;                                      // (behind the last barrier)
    const long long i = (long long)n*q.n_rays + (long long)o*q.per_origin + r;
    if (kept == 0) {                                                    // (uniform: nothing of this env can be seen from here)
        if (q.items) q.items[i] = -1;
        return;
    }
    item_ray(q, n, i, p, s_rows, s_ks, kept);
}
