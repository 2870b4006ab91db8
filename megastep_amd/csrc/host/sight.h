// host/sight.h -- what can be seen or reached from where: ms_nav_views (kernels/navview.h), ms_percepts (percept.h),
// ms_nav_clearance and ms_nav_clear_query (navclear.h), and the host instantiation of each.  One check serves a launch and its
// host instantiation.
namespace {
// View fields.  An env of more than 2^30 cells cannot be (MsNavGrid's geom is 32768 a side at most in cuda.nav_grid; here it is
// max_framed, an int, that bounds it).
int nav_views_check(const MsNavGrid* grid, const MsNavViews* v) {
    if (!nav_grid_ok(grid) || !v || v->n_points < 1 || !v->points || !v->countable || (!v->values && !v->counts && !v->gains) ||
        !positive_finite(v->max_range) || (v->headings && !(v->cos_half >= -1.f && v->cos_half <= 1.f)) ||
        (v->gains && !v->unseen) || (v->unseen && v->n_maps < 1) ||
        (v->unseen && !v->slot && v->n_maps != 1 && v->n_maps != v->n_points) || !all_aligned<8>(v->points, v->headings) ||
        !all_aligned<4>(v->slot, v->counts, v->gains)) return MS_EINVAL;
    return ((long long)grid->n_envs*v->n_points > 0x7fffffffLL || grid->max_framed > (1 << 30)) ? MS_EUNSUPPORTED : MS_OK;
}
NavViewArgs nav_view_args(const MsNavViews* v, const int capacity) {
    return NavViewArgs{v->points, v->headings, v->mask, v->countable, v->unseen, v->unseen ? v->slot : nullptr, v->values, v->counts, v->gains,
                       v->n_points, v->unseen ? v->n_maps : 0, capacity, v->max_range, v->max_range*v->max_range, v->headings ? v->cos_half : 0.f};
}

// Percepts.  The limits keep a lane's points within sixteen and a round's key within a lane.
int percepts_check(const MsPercepts* p) {
    if (!p || p->n_eyes < 1 || p->n_eyes > PERCEPT_MAX_EYES || p->n_points < 1 || p->n_points > PERCEPT_MAX_POINTS || p->n_nearest < 0 ||
        p->n_nearest > PERCEPT_MAX_NEAREST || !p->eyes || !p->points || !positive_finite(p->max_range) ||
        (p->headings && !(p->cos_half >= -1.f && p->cos_half <= 1.f)) || p->pairs_shape < 0 || p->pairs_shape > 2 ||
        (p->pairs != nullptr) != (p->pairs_shape != 0) ||
        (!p->visible && !p->squares && !p->offsets && !p->counts && !p->nearest && !p->near_offsets && !p->near_distances) ||
        !all_aligned<8>(p->eyes, p->headings, p->points, p->offsets, p->near_offsets) ||
        !all_aligned<4>(p->squares, p->counts, p->nearest, p->near_distances)) return MS_EINVAL;
    return MS_OK;
}
PerceptArgs percept_args(const MsPercepts* p, const int capacity) {
    return PerceptArgs{p->eyes, p->headings, p->points, p->valid, p->pairs, p->mask, p->visible, p->squares, p->offsets, p->counts, p->nearest,
                       p->near_offsets, p->near_distances, p->n_eyes, p->n_points, p->n_nearest, p->pairs_shape == 2 ? 1 : 0, capacity,
                       p->max_range, p->max_range*p->max_range, p->headings ? p->cos_half : 0.f};
}

// Clearance.  CLEAR_DEFAULT_CULL is the instantiation ms_nav_clearance launches (DESIGN.md 3.23 has the measurements that chose
// it); the other stays reachable through ms_debug_nav_clear_cull for A/B runs.
constexpr int CLEAR_DEFAULT_CULL = CLEAR_TILE_WAVE;
int nav_clearance_check(const MsNavGrid* grid, const MsNavClearance* c) {
    if (!nav_grid_ok(grid) || !c || !positive_finite(c->max_range) || c->n_radii < 0 || c->n_radii > CLEAR_MAX_RADII ||
        !c->values || (c->n_radii > 0) != (c->fits != nullptr) || !all_aligned<4>(c->values, c->nearest) ||
        (grid->max_framed > 0 && c->max_tiles < 1)) return MS_EINVAL;
    for (int k = 0; k < c->n_radii; k++)
        if (!(c->radii[k] > 0.f) || !(c->radii[k] <= c->max_range)) return MS_EINVAL;
    return grid->n_envs > 65535 ? MS_EUNSUPPORTED : MS_OK;
}
ClearArgs nav_clear_args(const MsNavClearance* c, const int cull) {
    ClearArgs q{c->mask, c->values, c->nearest, c->fits, c->n_radii, cull, c->max_range, c->max_range*c->max_range, {}};
    for (int k = 0; k < c->n_radii; k++) q.r2[k] = c->radii[k]*c->radii[k];
    return q;
}
int nav_clear_query_check(const MsNavClearQuery* q) {
    if (!q || q->n_envs < 1 || q->n_points < 1 || !q->points || (!q->distances && !q->nearest && !q->towards) ||
        !positive_finite(q->max_range) || !all_aligned<8>(q->points, q->towards) ||
        !all_aligned<4>(q->skip, q->distances, q->nearest)) return MS_EINVAL;
    return (long long)q->n_envs*q->n_points > 0x7fffffffLL ? MS_EUNSUPPORTED : MS_OK;
}
ClearQueryArgs nav_clear_query_args(const MsNavClearQuery* q, const bool with_agents) {
    return ClearQueryArgs{q->points, with_agents ? q->skip : nullptr, q->mask, q->distances, q->nearest, q->towards, q->n_points, with_agents ? 1 : 0,
                          (long long)q->n_envs*q->n_points, q->max_range*q->max_range};
}
}  // namespace

extern "C" {
int ms_nav_views(const MsScenery* sc, const MsNavGrid* grid, const MsNavViews* v, void* stream) {
    if (!scenery_ok(sc) || !nav_grid_ok(grid) || grid->n_envs != sc->n_envs) return MS_EINVAL;
    if (const int status = nav_views_check(grid, v)) return status;
    hipLaunchKernelGGL(nav_view_kernel, dim3((unsigned)((long long)grid->n_envs*v->n_points)), dim3(WG), 0, (hipStream_t)stream, *sc, nav_args(grid),
                       nav_view_args(v, VIEW_WALL_CAPACITY));
    return launch_status();
}

int ms_host_nav_views(const MsNavGrid* grid, const MsNavViews* v, const float* walls, const long long* wall_starts, int capacity) {
    if (const int status = nav_views_check(grid, v)) return status;
    if (!walls || !wall_starts || capacity > VIEW_WALL_CAPACITY) return MS_EINVAL;
    view_serial(nav_args(grid), nav_view_args(v, capacity > 0 ? capacity : VIEW_WALL_CAPACITY), reinterpret_cast<const float4*>(walls), wall_starts);
    return MS_OK;
}

int ms_host_nav_view_capacity(void) { return VIEW_WALL_CAPACITY; }

int ms_percepts(const MsScenery* sc, const MsPercepts* p, void* stream) {
    if (!scenery_ok(sc)) return MS_EINVAL;
    if (const int status = percepts_check(p)) return status;
    hipLaunchKernelGGL(percept_kernel, dim3((unsigned)sc->n_envs), dim3(WG), 0, (hipStream_t)stream, *sc, percept_args(p, VIEW_WALL_CAPACITY));
    return launch_status();
}

int ms_host_percepts(const MsPercepts* p, int n_envs, const float* walls, const long long* wall_starts, int capacity) {
    if (const int status = percepts_check(p)) return status;
    if (n_envs < 1 || !walls || !wall_starts || capacity < 0 || capacity > VIEW_WALL_CAPACITY) return MS_EINVAL;
    percept_serial(percept_args(p, capacity > 0 ? capacity : VIEW_WALL_CAPACITY), n_envs, reinterpret_cast<const float4*>(walls), wall_starts);
    return MS_OK;
}

int ms_nav_clearance(const MsScenery* sc, const MsNavGrid* grid, const MsNavClearance* c, void* stream) {
    if (!scenery_ok(sc) || !nav_grid_ok(grid) || grid->n_envs != sc->n_envs) return MS_EINVAL;
    if (const int status = nav_clearance_check(grid, c)) return status;
    if (grid->max_framed == 0) return MS_OK;
    const int cull = g_nav_clear_cull < 0 ? CLEAR_DEFAULT_CULL : g_nav_clear_cull;
    hipLaunchKernelGGL(cull == CLEAR_TILE_WAVE ? nav_clear_kernel<true> : nav_clear_kernel<false>, dim3((unsigned)c->max_tiles, (unsigned)grid->n_envs),
                       dim3(WG), 0, (hipStream_t)stream, *sc, nav_args(grid), nav_clear_args(c, cull != CLEAR_BRUTE));
    return launch_status();
}

int ms_nav_clear_query(const MsScenery* sc, const MsAgents* ag, const MsNavClearQuery* q, void* stream) {
    if (!scenery_ok(sc)) return MS_EINVAL;
    if (const int status = nav_clear_query_check(q)) return status;
    if (q->n_envs != sc->n_envs || !posed_or_none_ok(ag)) return MS_EINVAL;
    const long long total = (long long)q->n_envs*q->n_points;
    hipLaunchKernelGGL(nav_clear_query_kernel, dim3((unsigned)((total + WAVES - 1)/WAVES)), dim3(WG), 0, (hipStream_t)stream, *sc, agents_or_none(ag),
                       nav_clear_query_args(q, ag != nullptr));
    return launch_status();
}

int ms_debug_nav_clear_cull(int mode) {
    if (mode < -1 || mode > CLEAR_TILE_WAVE) return MS_EINVAL;
    g_nav_clear_cull = mode;
    return MS_OK;
}

int ms_host_nav_clearance(const MsNavGrid* grid, const MsNavClearance* c, const float* walls, const long long* wall_starts, int flags) {
    if (const int status = nav_clearance_check(grid, c)) return status;
    if (!walls || !wall_starts || flags < CLEAR_BRUTE || flags > CLEAR_TILE_WAVE) return MS_EINVAL;
    clear_serial(nav_args(grid), nav_clear_args(c, flags != CLEAR_BRUTE), reinterpret_cast<const float4*>(walls), wall_starts, 0, flags, &g_clear_folds,
                 &g_clear_pairs);
    return MS_OK;
}

long long ms_host_nav_clear_folds(long long* pairs) {
    if (pairs) *pairs = g_clear_pairs;
    return g_clear_folds;
}

int ms_host_nav_clear_chunk(void) { return OV_CHUNK; }

int ms_host_nav_clear_query(const MsNavClearQuery* q, const float* rows, const long long* row_starts, int n_agents, int n_model, int with_agents,
                            int flags) {
    if (const int status = nav_clear_query_check(q)) return status;
    if (!rows || !row_starts || n_agents < 1 || n_model < 1 || flags < 0 || flags > 1) return MS_EINVAL;
    clear_query_serial(nav_clear_query_args(q, with_agents != 0), n_agents, n_model, reinterpret_cast<const float4*>(rows), row_starts, flags != 0);
    return MS_OK;
}
}  // extern "C"
