// host/nav.h -- the nav grid and what follows its distance fields: ms_nav_free, ms_nav_fields, ms_nav_seed_fields,
// ms_nav_cost_fields and ms_nav_query (kernels/navfield.h), ms_nav_{,seed_,cost_}{waypoints,paths} (navpath.h), ms_nav_pulls
// (navpull.h); their host hooks; and nav_grid_ok, nav_args and the LDS tiers that every nav family's file uses.
// Every argument is checked in full before the first launch; nothing is allocated, nothing waits.
namespace {
bool nav_grid_ok(const MsNavGrid* g) {
    return g && g->n_envs > 0 && positive_finite(g->cell) && positive_finite(g->clearance) &&
           g->cell <= 1.4f*g->clearance && g->geom && g->starts && g->free_cells && g->max_framed >= 0 && aligned(g->geom, 16);
}
NavArgs nav_args(const MsNavGrid* g) { return NavArgs{g->geom, g->starts, g->n_envs, g->cell, g->clearance}; }

// The three LDS tiers of the kernels that keep an env's field in LDS (relaxation, regions, basins) and the threads of each
// tier's instantiations.  A launch takes the least tier whose capacity - by the kernel's own capacity function - holds the
// largest env's framed field: more workgroups a CU (an env that still does not fit - or is larger than max_framed says - runs in
// global memory).
constexpr int NAV_TIER_LDS[3] = {NAV_LDS_SMALL, NAV_LDS_MEDIUM, NAV_LDS_LARGE}, NAV_TIER_THREADS[3] = {512, 1024, 1024};
int nav_tier(const MsNavGrid* grid, int (*capacity)(int)) {
    return grid->max_framed <= capacity(NAV_TIER_LDS[0]) ? 0 : grid->max_framed <= capacity(NAV_TIER_LDS[1]) ? 1 : 2;
}
int nav_capacity_for(const MsNavGrid* grid, int (*capacity)(int)) { return capacity(NAV_TIER_LDS[nav_tier(grid, capacity)]); }
int nav_host_capacities(int* capacities, int (*capacity)(int)) {
    if (!capacities) return MS_EINVAL;
    for (int t = 0; t < 3; t++) capacities[t] = capacity(NAV_TIER_LDS[t]);
    return MS_OK;
}

// The launch of either relaxation.
int nav_relax_launch(const MsNavGrid* grid, const NavFieldArgs& f, long long total, bool seeded, void* stream) {
    static void (*const kernels[3][2])(NavArgs, NavFieldArgs) = {                   // [tier][seeded, single-goal]
        {nav_relax_kernel<NAV_LDS_SMALL, 512, true>, nav_relax_kernel<NAV_LDS_SMALL, 512, false>},
        {nav_relax_kernel<NAV_LDS_MEDIUM, 1024, true>, nav_relax_kernel<NAV_LDS_MEDIUM, 1024, false>},
        {nav_relax_kernel<NAV_LDS_LARGE, 1024, true>, nav_relax_kernel<NAV_LDS_LARGE, 1024, false>}};
    const int t = nav_tier(grid, nav_capacity);
    hipLaunchKernelGGL(kernels[t][seeded ? 0 : 1], dim3((unsigned)total), dim3(NAV_TIER_THREADS[t]), 0, (hipStream_t)stream, nav_args(grid), f);
    return launch_status();
}

// ... and of the weighted one (MsNavCostFields), in either variant of where a cell's multiplier lives: read from global memory
// every pass (the seeded kernel's bytes a cell and its tiers) or kept in LDS (its own capacity, its own tier).  The library's
// choice is the first (DESIGN.md 3.24 has the reasons); the other stays reachable through ms_debug_nav_cost_variant for A/B runs.
int nav_cost_launch(const MsNavGrid* grid, const NavFieldArgs& f, long long total, void* stream) {
    static void (*const kernels[3][2])(NavArgs, NavFieldArgs) = {                   // [tier][from global memory, in LDS]
        {nav_relax_kernel<NAV_LDS_SMALL, 512, true, NAV_COST_GLOBAL>, nav_relax_kernel<NAV_LDS_SMALL, 512, true, NAV_COST_LDS>},
        {nav_relax_kernel<NAV_LDS_MEDIUM, 1024, true, NAV_COST_GLOBAL>, nav_relax_kernel<NAV_LDS_MEDIUM, 1024, true, NAV_COST_LDS>},
        {nav_relax_kernel<NAV_LDS_LARGE, 1024, true, NAV_COST_GLOBAL>, nav_relax_kernel<NAV_LDS_LARGE, 1024, true, NAV_COST_LDS>}};
    const int in_lds = g_nav_cost_variant == 1 ? 1 : 0;
    const int t = in_lds ? nav_tier(grid, nav_cost_capacity) : nav_tier(grid, nav_capacity);
    hipLaunchKernelGGL(kernels[t][in_lds], dim3((unsigned)total), dim3(NAV_TIER_THREADS[t]), 0, (hipStream_t)stream, nav_args(grid), f);
    return launch_status();
}

// What the seeded and the cost fields' entries refuse alike (MsNavSeedFields, MsNavCostFields), and the costs' own rule.
template <typename F> bool nav_seed_fields_ok(const MsNavGrid* grid, const F* sf) {
    return nav_grid_ok(grid) && sf && sf->n_fields >= 1 && sf->marks && sf->fields && is_flag(sf->where) &&
           all_aligned<4>(sf->fields, sf->passes, sf->n_seeds);
}
bool nav_costs_ok(const float* costs, int n_costs, int n_fields) { return costs && aligned(costs, 4) && (n_costs == 1 || n_costs == n_fields); }

// Paths and waypoints (MsNavWaypoints, MsNavPaths, their seeded and cost kin, MsNavPulls): what every struct that follows fields
// from points has, checked alike; then the waypoints' and the paths' own members.
template <typename Q> bool nav_follow_ok(const MsNavGrid* grid, const Q* q) {
    return q && nav_grid_ok(grid) && q->n_points >= 1 && q->n_goals >= 1 && q->points && q->fields && (q->goal || q->n_points == q->n_goals) &&
           aligned(q->points, 8) && all_aligned<4>(q->fields, q->goal);
}
bool nav_goals_ok(const float* goals) { return goals && aligned(goals, 8); }
template <typename Q> bool nav_waypoints_ok(const Q* w) {
    return w->lookahead >= 1 && w->lookahead <= WAVE && w->waypoints && aligned(w->waypoints, 8) && aligned(w->hops, 4);
}
template <typename Q> bool nav_paths_ok(const Q* np) {
    return np->max_points >= 2 && np->paths && np->counts && all_aligned<4>(np->paths, np->counts);
}

// The two launches, of any of the three structs: for fields of goals and - goals NULL - for seeded fields, and - costs not NULL,
// n_costs 1 or n_goals - for cost fields (the WEIGHTED instantiations); the arguments are checked by then.
template <typename Q>
int nav_waypoints_launch(const MsNavGrid* grid, const Q* w, const float* goals, const float* costs, int n_costs, void* stream) {
    const long long total = (long long)grid->n_envs*w->n_points;
    if ((total + WAVES - 1)/WAVES > 0x7fffffffLL) return MS_EUNSUPPORTED;
    const NavPathArgs q{w->points, w->goal, w->fields, goals, grid->free_cells, w->waypoints, w->hops, nullptr, nullptr, w->n_points, w->n_goals,
                        w->lookahead, 0, total, costs, n_costs};
    hipLaunchKernelGGL(costs ? nav_waypoint_kernel<true> : nav_waypoint_kernel<false>, dim3((unsigned)((total + WAVES - 1)/WAVES)), dim3(WG), 0,
                       (hipStream_t)stream, nav_args(grid), q);
    return launch_status();
}
template <typename Q>
int nav_paths_launch(const MsNavGrid* grid, const Q* np, const float* goals, const float* costs, int n_costs, void* stream) {
    const long long total = (long long)grid->n_envs*np->n_points;
    if (total > 0x7fffff00LL) return MS_EUNSUPPORTED;
    const NavPathArgs q{np->points, np->goal, np->fields, goals, grid->free_cells, nullptr, nullptr, np->paths, np->counts, np->n_points, np->n_goals,
                        0, np->max_points, total, costs, n_costs};
    hipLaunchKernelGGL(costs ? nav_path_kernel<true> : nav_path_kernel<false>, dim3((unsigned)((total + WG - 1)/WG)), dim3(WG), 0,
                       (hipStream_t)stream, nav_args(grid), q);
    return launch_status();
}

// The env of the host hooks that take one env's loose arrays.
bool nav_host_env(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* point, NavEnv& g) {
    if (!geom || !free_cells || !D || !point || !(cell > 0.f) || geom[2] <= 0 || geom[3] <= 0) return false;
    g = NavEnv{geom[0], geom[1], geom[2], geom[3], cell, free_cells, D, nullptr};
    return true;
}

// The waypoint and the path hooks' bodies: towards `goal`, or - NULL - down a seeded field; by `costs`, or - NULL - unweighted.
// `given`: what the hook's own caller owes of the two is there.
int nav_host_waypoint(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* goal, const float* costs,
                      bool given, const float* point, int lookahead, float* waypoint) {
    if (lookahead < 1 || lookahead > WAVE || !waypoint) return -2;
    waypoint[0] = waypoint[1] = NAN;
    NavEnv g;
    if (!given || !nav_host_env(geom, cell, free_cells, D, point, g)) return -1;
    g.cost = costs;
    return nav_waypoint_serial(g, goal ? nav_goal(g, goal[0], goal[1]) : nav_seeded(), point[0], point[1], lookahead, waypoint[0], waypoint[1]);
}
int nav_host_path(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* goal, const float* costs,
                  bool given, const float* point, int max_points, float* points) {
    if (max_points < 2 || !points) return 0;
    NavEnv g;
    if (!given || !nav_host_env(geom, cell, free_cells, D, point, g)) {
        for (int k = 0; k < 2*max_points; k++) points[k] = NAN;
        return 0;
    }
    g.cost = costs;
    return nav_path(g, goal ? nav_goal(g, goal[0], goal[1]) : nav_seeded(), point[0], point[1], (long long)g.nx*g.ny, max_points, points);
}

// The seeded relaxation on host arrays, and - costs not NULL - the weighted one: the kernel's fill and per-cell functions, swept.
int nav_host_seed_field(const int* geom, float cell, const unsigned char* free_cells, const unsigned char* marks, int where,
                        const unsigned char* among, const float* costs, int framed, float* D, int* n_seeds) {
    if (!geom || !positive_finite(cell) || !is_flag(where) || geom[2] < 0 || geom[3] < 0) return -1;
    const int nx = geom[2], ny = geom[3];
    const long long cells = (long long)nx*ny;
    if (n_seeds) *n_seeds = 0;
    if (cells <= 0) return 0;
    if (!free_cells || !marks || !D || (long long)(nx + 2)*(ny + 2) > 0x7fffffffLL) return -1;
    float ws = cell, wd = cell*NAV_DIAGONAL;
    int seeds = 0, sweeps = 0;
    if (framed) {
        // as the kernel fills its LDS: the frame, the bytes, the seeds; then nav_cell_framed swept in place
        const int P = nx + 2, n = (nx + 2)*(ny + 2);
        std::vector<float> d(n);
        std::vector<unsigned char> m(n);
        std::vector<float> mult(costs ? n : 0);                         // (as NAV_COST_LDS keeps them)
        for (int k = 0; k < n; k++) {
            long long at;
            const int fb = nav_frame_free(free_cells, nx, ny, P, k, at);
            const bool seed = fb && nav_is_seed(free_cells, among, marks, at, where);
            d[k] = seed ? 0.f : INFINITY;
            m[k] = (unsigned char)(fb | (seed ? 32 : 0));
            if (costs) mult[k] = fb ? nav_cost_multiplier(costs[at]) : 1.f;
            seeds += seed;
        }
        for (int k = 0; k < n; k++)
            if (m[k] & 1) m[k] = (unsigned char)(nav_frame_open(m.data(), k, P) | (m[k] & 32));
        for (bool changed = true; changed; sweeps++) {
            changed = false;
            for (int k = 0; k < n; k++) {
                if (!(m[k] & 1)) continue;
                if (costs) nav_cost_weights(cell, mult[k], ws, wd);
                const float v = nav_cell_framed(d.data(), m[k], k, P, d[k], ws, wd);
                if (v < d[k]) { d[k] = v; changed = true; }
            }
        }
        for (long long k = 0; k < cells; k++) D[k] = d[(k / nx + 1)*P + k % nx + 1];
    } else {
        for (long long k = 0; k < cells; k++) {
            const bool seed = nav_is_seed(free_cells, among, marks, k, where);
            D[k] = seed ? 0.f : INFINITY;
            seeds += seed;
        }
        for (bool changed = true; changed; sweeps++) {
            changed = false;
            for (long long k = 0; k < cells; k++) {
                if (!(free_cells[k] & 1)) continue;
                if (costs) nav_cost_weights(cell, nav_cost_multiplier(costs[k]), ws, wd);
                const float v = nav_cell_stored(D, free_cells, nx, ny, k, D[k], ws, wd);
                if (v < D[k]) { D[k] = v; changed = true; }
            }
        }
    }
    if (n_seeds) *n_seeds = seeds;
    return sweeps;
}
}  // namespace

extern "C" {
int ms_nav_free(const MsScenery* sc, const MsNavGrid* grid, void* stream) {
    if (!scenery_ok(sc) || !nav_grid_ok(grid) || grid->n_envs != sc->n_envs) return MS_EINVAL;
    if (grid->n_envs > 65535) return MS_EUNSUPPORTED;
    if (grid->max_framed == 0) return MS_OK;
    const unsigned blocks = (unsigned)(((long long)grid->max_framed + WG - 1)/WG);        // (at least the largest env's cells)
    hipLaunchKernelGGL(nav_free_kernel, dim3(blocks, (unsigned)grid->n_envs), dim3(WG), 0, (hipStream_t)stream, *sc, nav_args(grid), grid->free_cells);
    return launch_status();
}

int ms_nav_fields(const MsNavGrid* grid, const MsNavFields* nf, void* stream) {
    if (!nav_grid_ok(grid) || !nf || nf->n_goals < 1 || !nf->goals || !nf->fields || !aligned(nf->goals, 8)) return MS_EINVAL;
    const long long total = (long long)grid->n_envs*nf->n_goals;
    if (total > 0x7fffffffLL) return MS_EUNSUPPORTED;
    const NavFieldArgs f{nf->goals, nf->mask, grid->free_cells, nf->fields, nf->passes, nf->n_goals, nullptr, nullptr, 0, nullptr, nullptr, 0};
    return nav_relax_launch(grid, f, total, false, stream);
}

int ms_nav_seed_fields(const MsNavGrid* grid, const MsNavSeedFields* sf, void* stream) {
    if (!nav_seed_fields_ok(grid, sf)) return MS_EINVAL;
    const long long total = (long long)grid->n_envs*sf->n_fields;
    if (total > 0x7fffffffLL) return MS_EUNSUPPORTED;
    const NavFieldArgs f{nullptr, sf->mask, grid->free_cells, sf->fields, sf->passes, sf->n_fields, sf->marks, sf->among, sf->where, sf->n_seeds,
                         nullptr, 0};
    return nav_relax_launch(grid, f, total, true, stream);
}

int ms_nav_cost_fields(const MsNavGrid* grid, const MsNavCostFields* cf, void* stream) {
    if (!nav_seed_fields_ok(grid, cf) || !nav_costs_ok(cf->costs, cf->n_costs, cf->n_fields)) return MS_EINVAL;
    const long long total = (long long)grid->n_envs*cf->n_fields;
    if (total > 0x7fffffffLL) return MS_EUNSUPPORTED;
    const NavFieldArgs f{nullptr, cf->mask, grid->free_cells, cf->fields, cf->passes, cf->n_fields, cf->marks, cf->among, cf->where, cf->n_seeds,
                         cf->costs, cf->n_costs};
    return nav_cost_launch(grid, f, total, stream);
}

int ms_debug_nav_cost_variant(int variant) {
    if (variant < -1 || variant > 1) return MS_EINVAL;
    g_nav_cost_variant = variant;
    return MS_OK;
}

int ms_nav_query(const MsNavGrid* grid, const MsNavQuery* nq, void* stream) {
    if (!nav_grid_ok(grid) || !nq || nq->n_points < 1 || nq->n_goals < 1 || !nq->points || !nq->fields || !nq->out ||
        (!nq->goal && nq->n_points != nq->n_goals) || !aligned(nq->points, 8)) return MS_EINVAL;
    const long long total = (long long)grid->n_envs*nq->n_points;
    if (total > 0x7fffff00LL) return MS_EUNSUPPORTED;
    const NavQueryArgs q{nq->points, nq->goal, nq->fields, nq->out, nq->n_points, nq->n_goals, total};
    hipLaunchKernelGGL(nav_query_kernel, dim3((unsigned)((total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, nav_args(grid), q);
    return launch_status();
}

int ms_nav_waypoints(const MsNavGrid* grid, const MsNavWaypoints* w, void* stream) {
    if (!nav_follow_ok(grid, w) || !nav_goals_ok(w->goals) || !nav_waypoints_ok(w)) return MS_EINVAL;
    return nav_waypoints_launch(grid, w, w->goals, nullptr, 0, stream);
}
int ms_nav_paths(const MsNavGrid* grid, const MsNavPaths* np, void* stream) {
    if (!nav_follow_ok(grid, np) || !nav_goals_ok(np->goals) || !nav_paths_ok(np)) return MS_EINVAL;
    return nav_paths_launch(grid, np, np->goals, nullptr, 0, stream);
}
int ms_nav_seed_waypoints(const MsNavGrid* grid, const MsNavSeedWaypoints* w, void* stream) {
    if (!nav_follow_ok(grid, w) || !nav_waypoints_ok(w)) return MS_EINVAL;
    return nav_waypoints_launch(grid, w, nullptr, nullptr, 0, stream);
}
int ms_nav_seed_paths(const MsNavGrid* grid, const MsNavSeedPaths* np, void* stream) {
    if (!nav_follow_ok(grid, np) || !nav_paths_ok(np)) return MS_EINVAL;
    return nav_paths_launch(grid, np, nullptr, nullptr, 0, stream);
}
int ms_nav_cost_waypoints(const MsNavGrid* grid, const MsNavCostWaypoints* w, void* stream) {
    if (!nav_follow_ok(grid, w) || !nav_waypoints_ok(w) || !nav_costs_ok(w->costs, w->n_costs, w->n_goals)) return MS_EINVAL;
    return nav_waypoints_launch(grid, w, nullptr, w->costs, w->n_costs, stream);
}
int ms_nav_cost_paths(const MsNavGrid* grid, const MsNavCostPaths* np, void* stream) {
    if (!nav_follow_ok(grid, np) || !nav_paths_ok(np) || !nav_costs_ok(np->costs, np->n_costs, np->n_goals)) return MS_EINVAL;
    return nav_paths_launch(grid, np, nullptr, np->costs, np->n_costs, stream);
}

// Pulled paths (navpull.h, MsNavPulls): one entry for fields of goals, seeded fields (goals NULL) and cost fields (costs not NULL).
// The library's scheme is a lane a candidate; the waypoint kernel's, a lane a sample, stays reachable through
// ms_debug_nav_pull_scheme for A/B runs.
int ms_nav_pulls(const MsNavGrid* grid, const MsNavPulls* np, void* stream) {
    if (!nav_follow_ok(grid, np) || !aligned(np->goals, 8) ||
        np->reach < 1 || np->reach > NAV_PULL_REACH || np->max_points < 2 || np->max_points > NAV_PULL_POINTS ||
        !np->vertices || !np->counts || !np->lengths || !all_aligned<4>(np->vertices, np->indices, np->counts, np->cells, np->lengths) ||
        (np->n_costs == 0 ? np->costs != nullptr : !nav_costs_ok(np->costs, np->n_costs, np->n_goals))) return MS_EINVAL;
    const long long total = (long long)grid->n_envs*np->n_points;
    if ((total + WAVES - 1)/WAVES > 0x7fffffffLL) return MS_EUNSUPPORTED;
    const NavPullArgs u{NavPathArgs{np->points, np->goal, np->fields, np->goals, grid->free_cells, nullptr, nullptr, np->vertices, np->counts,
                                    np->n_points, np->n_goals, 0, np->max_points, total, np->costs, np->n_costs},
                        np->mask, np->indices, np->cells, np->lengths, np->reach, nav_pull_ring(np->reach)};
    static void (*const kernels[2][2])(NavArgs, NavPullArgs) = {                    // [weighted][a lane a candidate, a lane a sample]
        {nav_pull_kernel<false, false>, nav_pull_kernel<false, true>}, {nav_pull_kernel<true, false>, nav_pull_kernel<true, true>}};
    hipLaunchKernelGGL(kernels[np->costs != nullptr][g_nav_pull_scheme == 1], dim3((unsigned)((total + WAVES - 1)/WAVES)), dim3(WG),
                       (size_t)WAVES*u.ring*sizeof(int), (hipStream_t)stream, nav_args(grid), u);
    return launch_status();
}

int ms_debug_nav_pull_scheme(int scheme) {
    if (scheme < -1 || scheme > 1) return MS_EINVAL;
    g_nav_pull_scheme = scheme;
    return MS_OK;
}

int ms_host_nav_waypoint(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* goal, const float* point,
                         int lookahead, float* waypoint) {
    return nav_host_waypoint(geom, cell, free_cells, D, goal, nullptr, goal != nullptr, point, lookahead, waypoint);
}
int ms_host_nav_path(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* goal, const float* point,
                     int max_points, float* points) {
    return nav_host_path(geom, cell, free_cells, D, goal, nullptr, goal != nullptr, point, max_points, points);
}
int ms_host_nav_seed_waypoint(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* point, int lookahead,
                              float* waypoint) {
    return nav_host_waypoint(geom, cell, free_cells, D, nullptr, nullptr, true, point, lookahead, waypoint);
}
int ms_host_nav_seed_path(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* point, int max_points,
                          float* points) {
    return nav_host_path(geom, cell, free_cells, D, nullptr, nullptr, true, point, max_points, points);
}
int ms_host_nav_cost_waypoint(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* costs, const float* point,
                              int lookahead, float* waypoint) {
    return nav_host_waypoint(geom, cell, free_cells, D, nullptr, costs, costs != nullptr, point, lookahead, waypoint);
}
int ms_host_nav_cost_path(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* costs, const float* point,
                          int max_points, float* points) {
    return nav_host_path(geom, cell, free_cells, D, nullptr, costs, costs != nullptr, point, max_points, points);
}

int ms_host_nav_pull(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* goal, const float* costs,
                     const float* point, int reach, int max_points, float* vertices, int* indices, float* length) {
    if (reach < 1 || reach > NAV_PULL_REACH) return -2;
    if (max_points < 2 || max_points > NAV_PULL_POINTS || !vertices || !length) return 0;
    NavEnv g;
    if (!nav_host_env(geom, cell, free_cells, D, point, g)) {
        for (int k = 0; k < max_points; k++) {
            vertices[2*k] = vertices[2*k + 1] = NAN;
            if (indices) indices[k] = -1;
        }
        *length = INFINITY;
        return 0;
    }
    g.cost = costs;
    return nav_pull_serial(g, goal ? nav_goal(g, goal[0], goal[1]) : nav_seeded(), point[0], point[1], reach, max_points, vertices, indices,
                           nullptr, *length);
}

int ms_host_nav_seed_field(const int* geom, float cell, const unsigned char* free_cells, const unsigned char* marks, int where,
                           const unsigned char* among, int framed, float* D, int* n_seeds) {
    return nav_host_seed_field(geom, cell, free_cells, marks, where, among, nullptr, framed, D, n_seeds);
}

int ms_host_nav_cost_field(const int* geom, float cell, const unsigned char* free_cells, const unsigned char* marks, int where,
                           const unsigned char* among, const float* costs, int framed, float* D, int* n_seeds) {
    if (!costs && geom && (long long)geom[2]*geom[3] > 0) return -1;
    return nav_host_seed_field(geom, cell, free_cells, marks, where, among, costs, framed, D, n_seeds);
}

int ms_host_nav_field_capacity(int* capacities) { return nav_host_capacities(capacities, nav_capacity); }
int ms_host_nav_cost_capacity(int* capacities) { return nav_host_capacities(capacities, nav_cost_capacity); }
}  // extern "C"
