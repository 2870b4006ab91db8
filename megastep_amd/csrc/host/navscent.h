// host/navscent.h -- scent fields on the nav grid: ms_nav_scent and ms_nav_scent_query (kernels/navscent.h) and the host
// instantiation of each.  One check serves a launch and its host instantiation.
namespace {
bool in_range(const float x, const float lo, const float hi) { return x >= lo && x <= hi; }       // (a NaN is in no range)

// The launch's LDS is chosen as the relaxation's, by the largest framed store; a grid beyond the top tier needs the workspace.
int nav_scent_check(const MsNavGrid* grid, const MsNavScent* s) {
    if (!nav_grid_ok(grid) || !s || s->n_fields < 1 || s->n_sources < 0 || s->n_sources > SCENT_MAX_SOURCES ||
        (s->n_sources > 0 && (!s->points || !s->amounts || (!s->field && s->n_fields != 1 && s->n_fields != s->n_sources))) ||
        !in_range(s->rate, 0.f, .25f) || !in_range(s->keep, 0.f, 1.f) || !(s->floor >= 0.f && s->floor < INFINITY) ||
        s->substeps < 1 || s->substeps > SCENT_MAX_SUBSTEPS || !s->values || !s->peaks || !s->scented || s->workspace == s->values ||
        (!s->workspace && grid->max_framed > scent_capacity(NAV_LDS_LARGE)) || !aligned(s->points, 8) ||
        !all_aligned<4>(s->amounts, s->field, s->values, s->workspace, s->peaks, s->scented)) return MS_EINVAL;
    return (long long)grid->n_envs*s->n_fields > 0x7fffffffLL ? MS_EUNSUPPORTED : MS_OK;
}
NavScentArgs nav_scent_args(const MsNavGrid* grid, const MsNavScent* s) {
    return NavScentArgs{grid->free_cells, s->points, s->amounts, s->field, s->reset, s->mask, s->values, s->workspace, s->peaks, s->scented,
                        s->n_fields, s->n_sources, s->substeps, s->rate, s->keep, s->floor};
}
int nav_scent_query_check(const MsNavGrid* grid, const MsNavScentQuery* q) {
    if (!nav_grid_ok(grid) || !q || q->n_points < 1 || q->n_fields < 1 || !q->points || !q->values || !q->out ||
        (!q->field && q->n_fields != 1 && q->n_fields != q->n_points) || !aligned(q->points, 8) ||
        !all_aligned<4>(q->field, q->values, q->out, q->gradients)) return MS_EINVAL;
    return (long long)grid->n_envs*q->n_points > 0x7fffff00LL/2 ? MS_EUNSUPPORTED : MS_OK;
}
NavScentQueryArgs nav_scent_query_args(const MsNavGrid* grid, const MsNavScentQuery* q) {
    return NavScentQueryArgs{grid->free_cells, q->points, q->field, q->values, q->out, q->gradients, q->n_points, q->n_fields,
                             (long long)grid->n_envs*q->n_points};
}
}  // namespace

extern "C" {
int ms_nav_scent(const MsNavGrid* grid, const MsNavScent* s, void* stream) {
    if (const int status = nav_scent_check(grid, s)) return status;
    static void (*const kernels[3])(NavArgs, NavScentArgs) = {nav_scent_kernel<NAV_LDS_SMALL, 512>, nav_scent_kernel<NAV_LDS_MEDIUM, 1024>,
                                                              nav_scent_kernel<NAV_LDS_LARGE, 1024>};
    const int t = nav_tier(grid, scent_capacity);
    hipLaunchKernelGGL(kernels[t], dim3((unsigned)((long long)grid->n_envs*s->n_fields)), dim3(NAV_TIER_THREADS[t]), 0, (hipStream_t)stream,
                       nav_args(grid), nav_scent_args(grid, s));
    return launch_status();
}

int ms_nav_scent_query(const MsNavGrid* grid, const MsNavScentQuery* q, void* stream) {
    if (const int status = nav_scent_query_check(grid, q)) return status;
    const NavScentQueryArgs a = nav_scent_query_args(grid, q);
    hipLaunchKernelGGL(nav_scent_query_kernel, dim3((unsigned)((a.total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, nav_args(grid), a);
    return launch_status();
}

int ms_host_nav_scent(const MsNavGrid* grid, const MsNavScent* s) {
    if (const int status = nav_scent_check(grid, s)) return status;
    scent_serial(nav_args(grid), nav_scent_args(grid, s), nav_capacity_for(grid, scent_capacity));
    return MS_OK;
}

int ms_host_nav_scent_query(const MsNavGrid* grid, const MsNavScentQuery* q) {
    if (const int status = nav_scent_query_check(grid, q)) return status;
    const NavScentQueryArgs a = nav_scent_query_args(grid, q);
    for (long long at = 0; at < a.total; at++) scent_query_one(nav_args(grid), a, at);
    return MS_OK;
}

int ms_host_nav_scent_capacity(int* capacities) { return nav_host_capacities(capacities, scent_capacity); }
}  // extern "C"
