// kernels/raycast.h -- raycast_kernel, camera_rays_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after wallgrid.h: it uses
// render.h's draw and camera-ray helpers and the wall grid's constants); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// ray queries: the reference's per-ray rule for rays the caller gives                kernels.cu:349-382
// ------------------------------------------------------------------------------------------------
// The render's rays all start at an agent and point along its camera fan.  ms_raycast casts arbitrary ones - line of
// sight, lidar rings, hit-scan - by the same rule: one ray per lane, rays of one env next to each other (a wave shares one
// env's line rows and, where origins cluster, one cell's vis list), the nearest-hit fold in line order written out as the
// reference has it.  Nothing is written but the outputs: the agents' rows are drawn in registers, never stored.

// The state of the reference's fold over one ray's lines (kernels.cu:348-377): nearest s, its line, its q.t, its line's
// direction (for the dot, which depends on the winner alone: worked out once, at the end).
struct RayFold { float s; int idx; float t, vx, vy; };

// One line of the fold, statement for statement kernels.cu:352-377 (its dot aside, see above) - behind a test that lets
// through every line the rule can take and spares the rest intersect()'s two divisions: t = nt/d lies in [0, 1] only if
// |nt| <= |d| with nt of d's sign (an exact quotient of floats above 1 exceeds 1 + 2^-24 and never rounds down to 1; one
// below 0 rounds to -0 only when it is below 2^-150, i.e. nt above -2^-150 |d|), and only if |d| >= 1e-3 (kernels.cu:77).
// NaNs fail the test and could not have hit.  (d and nt are intersect()'s own cross products, the same bits.)
// (__host__ too: kernels/items.h folds an item's billboard by it, on the device and in its host instantiation)
__host__ __device__ inline void ray_fold(const P2 p, const P2 ru, const float near_s, const float4 L, const int l, RayFold& f) {
    const P2 v = p2(L.z - L.x, L.w - L.y);
    const P2 pq = p2(L.x, L.y) - p;
    const float d = cross(ru, v), nt = cross(pq, ru);
    const float ad = fabsf(d);
    const float ntp = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, nt) ^ (__builtin_bit_cast(unsigned, d) & 0x80000000u));    // nt with d's sign taken out
    if ((ad >= 1.e-3f) & (ntp <= ad) & (ntp >= -1e-30f*ad)) {
        const Isect q = intersect(p, ru, p2(L.x, L.y), v);
        const bool hit = (0 <= q.t) & (q.t <= 1);
        const bool better = (near_s < q.s) & (q.s < f.s - 1.e-4f);
        if (hit & better) { f.s = q.s; f.idx = l; f.t = q.t; f.vx = v.x; f.vy = v.y; }
    }
}

// Ray i = n R + r of the launch: origin and direction (n, r) of MsRaycast.  with_agents: the A M agent rows come first,
// drawn from the agents' poses by the render's own arithmetic (drawn_row); else they are skipped and only static walls
// (rows A M .. L - 1) are met.  gridded: the host found the scenery's wall grid usable for this near plane; a ray may then
// walk its origin cell's vis list - ascending wall numbers, as wallgrid_fill_kernel writes them, thinned by the arc cull:
// the walls it drops are each hidden behind one it keeps (wallgrid.h), so the fold ends where the
// fold over all lines does - when the origin is in the grid and 1 <= |ru|^2 <= WG_MAX_RU2 (the proof's |U| >= 1 and its
// band's longest direction vector).  Any other ray - outside the grid, an env of 0 cells, NaNs, a short or long ru - meets
// every line of its env.
// The wave walks lists and lines in step, at addresses that are the same in every lane (scalar loads, no gathers): rays
// of one env are neighbours, so a wave nearly always holds one env, and rays cast from a few points (an agent's lidar ring,
// lines of sight) share cells.  Cell after cell of its rays the wave walks that cell's list for the rays in it - if the
// lists of all its rays' cells together are shorter than the env's walls; else those rays meet every wall, as do the rays
// that cannot take the grid and every ray of a wave that straddles two envs (per lane then).  Rays cast from everywhere at once - a wave of 64 cells - are served by the all-walls
// sweep: a list walk per ray would be 64 walks of scattered loads.
__global__ __launch_bounds__(WG) void raycast_kernel(const MsScenery sc, const AgentsK ag, const MsRaycast q, const int with_agents,
                                                     const int gridded, const int n_total) {
    const int i_raw = blockIdx.x*WG + threadIdx.x;
    const bool live = i_raw < n_total;
    const int i = live ? i_raw : n_total - 1;                           // (spare lanes of the last block redo its last ray, store nothing)
    const int n = i / q.n_rays;
    const float2 o = reinterpret_cast<const float2*>(q.origins)[i];
    const float2 d = reinterpret_cast<const float2*>(q.dirs)[i];
    const P2 p = p2(o.x, o.y), ru = p2(d.x, d.y);
    const float rlen = len(ru);                                          // kernels.cu:340
    const float near_s = q.near_plane/rlen;                              // kernels.cu:370
    const int A = sc.n_agents, M = sc.n_model, AF = A*M;
    RayFold f{INFINITY, -1, NAN, 0.f, 0.f};
    // the agents' rows of env e, at the poses the agents have now (draw_kernel, kernels.cu:297-318): first in line order
    auto fold_agents = [&](const int e) {
        for (int a = 0; a < A; a++) {
            float s, c;
            sincospi_f(ag.angles[e*A + a]/180.f, s, c);
            const float2 pa = reinterpret_cast<const float2*>(ag.positions)[e*A + a];
            for (int m = 0; m < M; m++)
                ray_fold(p, ru, near_s, drawn_row(s, c, pa.x, pa.y, reinterpret_cast<const float4*>(sc.model)[m]), a*M + m, f);
        }
    };
    const int n_w = __builtin_amdgcn_readfirstlane(n);
    const bool one_env = __ballot(n != n_w) == 0ull;                    // (uniform)

    if (one_env) {
        const int L = sc.lines_widths[n_w];
        const float4* const rows = reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[n_w];
        if (with_agents) fold_agents(n_w);
        // the static walls: cell by cell the vis lists of the rays' cells, then every wall for the rest
        bool listed = false;
        int cell = -1;
        if (gridded) {
            bool inside;
            const int c = wg_cell_at(reinterpret_cast<const float4*>(sc.wg_geom)[n_w], sc.wg_cell, p.x, p.y, inside);
            const float ru2 = len2(ru);
            listed = inside & (ru2 >= 1.f) & (ru2 <= WG_MAX_RU2);
            cell = listed ? sc.wg_starts[n_w] + c : -1;
        }
        // (first the cells' list lengths alone: the lists are walked only if all of them together are shorter than the
        // env's walls - else every listed ray joins the sweep, and a wave of scattered rays pays a few header loads for it)
        unsigned long long pending = __ballot(listed);
        int walk = 0;
        for (unsigned long long todo = pending; todo && walk <= L - AF;) {
            const int cell_w = __builtin_amdgcn_readlane(cell, __ffsll((long long)todo) - 1);
            walk += (int)reinterpret_cast<const uint4*>(sc.wg_cells)[cell_w].y;
            todo &= ~__ballot(cell == cell_w);
        }
        if (walk > L - AF) pending = 0ull;
        bool done = false;
        while (pending) {
            const int cell_w = __builtin_amdgcn_readlane(cell, __ffsll((long long)pending) - 1);
            const uint4 hdr = reinterpret_cast<const uint4*>(sc.wg_cells)[cell_w];
            const int count = (int)hdr.y;
            const bool mine = cell == cell_w;
            pending &= ~__ballot(mine);
            if (mine) {
                int wa8, wb8;
                const float pa = pseudo_angle(ru.x, ru.y);
                wg_wedge(pa, pa, wa8, wb8);
                const unsigned* const vis = sc.wg_pool + sc.wg_pool_base[n_w] + hdr.x;
                for (int k = 0; k < count; k++) {
                    const unsigned e = vis[k];
                    const int l = AF + (int)(e & 0xffffu);
                    if (wg_arcs_meet((int)((e >> 16) & 255u), (int)(e >> 24), wa8, wb8) & (l < L)) ray_fold(p, ru, near_s, rows[l], l, f);
                }
                done = true;
            }
        }
        if (__ballot(!done))
            for (int l = AF; l < L; l++) {
                const float4 row = rows[l];
                if (!done) ray_fold(p, ru, near_s, row, l, f);
            }
        if (q.grid_rays) {                                               // (tests: did the grid serve?)
            const unsigned long long took = __ballot(live & done);
            if (took && (int)threadIdx.x % WAVE == __ffsll((long long)__ballot(1)) - 1) atomicAdd(q.grid_rays, (int)__popcll(took));
        }
    } else {                                                             // a wave across two envs: lane by lane, every line
        const int L = sc.lines_widths[n];
        const float4* const rows = reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[n];
        if (with_agents) fold_agents(n);
        for (int l = AF; l < L; l++) ray_fold(p, ru, near_s, rows[l], l, f);
    }

    if (!live) return;
    float dt = NAN;
    if (f.idx >= 0) {                                                    // kernels.cu:360-364
        const float dtop = dot(ru, p2(f.vx, f.vy));
        const float dbot = rlen*len(p2(f.vx, f.vy));
        dt = dtop/(dbot + 1.e-6f);
    }
    if (q.indices) q.indices[i] = f.idx;
    if (q.locations) q.locations[i] = f.t;
    if (q.dots) q.dots[i] = dt;
    if (q.distances) q.distances[i] = f.s*rlen;                         // kernels.cu:382
    if (q.agents) q.agents[i] = (with_agents && f.idx >= 0 && f.idx < AF) ? f.idx/M : -1;
}

// ru of every camera ray of every agent, (N, A, R, 2): the heading as the render evaluates it (sincospi_f of angle/180, the
// function behind ms_physics' heading cache and render_prep_kernel) and the column's ray by camera_ray, the render's own.
__global__ __launch_bounds__(WG) void camera_rays_kernel(const float* __restrict__ angles, const int n_agents_total, const int R,
                                                         const float half_screen, const float inv_res, float2* __restrict__ dirs) {
    const long long i = (long long)blockIdx.x*WG + threadIdx.x;
    if (i >= (long long)n_agents_total*R) return;
    const int agent = (int)(i / R), r = (int)(i - (long long)agent*R);
    float s, c;
    sincospi_f(angles[agent]/180.f, s, c);
    float rx, ry;
    camera_ray(c, s, r, (float)R, half_screen, inv_res, rx, ry);
    dirs[i] = make_float2(rx, ry);
}
