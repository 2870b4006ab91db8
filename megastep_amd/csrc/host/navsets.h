// host/navsets.h -- sets of cells of the nav grid: ms_nav_regions, ms_nav_region_query, ms_nav_region_masks
// (kernels/navregion.h), ms_nav_basins, ms_nav_basin_query, ms_nav_point_marks (navbasin.h), ms_nav_zones (navzone.h), and the host
// instantiation of each.  One check serves a launch and its host instantiation.
namespace {
// Regions: the launch's LDS is chosen as the relaxation's, by the largest framed field.
int nav_regions_check(const MsNavGrid* grid, const MsNavRegions* r) {
    if (!nav_grid_ok(grid) || !r || r->n_fields < 1 || (r->marks && !is_flag(r->where)) || !r->labels || !r->areas || !r->counts ||
        !r->open_cells || !r->largest || !r->largest_cells ||
        !all_aligned<4>(r->labels, r->areas, r->counts, r->open_cells, r->largest, r->largest_cells, r->passes)) return MS_EINVAL;
    return (long long)grid->n_envs*r->n_fields > 0x7fffffffLL ? MS_EUNSUPPORTED : MS_OK;
}
NavRegionArgs nav_region_args(const MsNavGrid* grid, const MsNavRegions* r) {
    return NavRegionArgs{grid->free_cells, r->marks, r->marks ? r->among : nullptr, r->mask, r->labels, r->areas, r->counts, r->open_cells,
                         r->largest, r->largest_cells, r->passes, r->n_fields, r->marks ? r->where : 1};
}
int nav_region_query_check(const MsNavGrid* grid, const MsNavRegionQuery* q) {
    if (!nav_grid_ok(grid) || !q || q->n_points < 1 || q->n_fields < 1 || !q->points || !q->labels || !q->labels_at ||
        (!q->field && q->n_fields != 1 && q->n_fields != q->n_points) ||
        !all_aligned<4>(q->points, q->field, q->labels, q->labels_at)) return MS_EINVAL;
    return (long long)grid->n_envs*q->n_points > 0x7fffff00LL/4 ? MS_EUNSUPPORTED : MS_OK;
}
int nav_region_masks_check(const MsNavGrid* grid, const MsNavRegionMasks* m) {
    if (!nav_grid_ok(grid) || !m || m->n_requests < 1 || m->n_fields < 1 || (m->points != nullptr) == (m->wanted != nullptr) || !m->labels ||
        !m->out || (!m->field && m->n_fields != 1 && m->n_fields != m->n_requests) ||
        !all_aligned<4>(m->points, m->wanted, m->field, m->labels)) return MS_EINVAL;
    return (long long)grid->n_envs*m->n_requests > 0x7fffffffLL ? MS_EUNSUPPORTED : MS_OK;
}

// Basins: the launch's LDS is chosen by max_framed, which bounds every env's cells from above.
int nav_basins_check(const MsNavGrid* grid, const MsNavBasins* b) {
    if (!nav_grid_ok(grid) || !b || b->n_fields < 1 || !b->fields || !b->labels || !b->reached || b->n_ids < 0 || b->n_ids > BASIN_MAX_IDS ||
        (b->sizes != nullptr) != (b->n_ids > 0) || b->ids == b->labels ||
        !all_aligned<4>(b->fields, b->ids, b->labels, b->sizes, b->reached, b->passes)) return MS_EINVAL;
    return (long long)grid->n_envs*b->n_fields > 0x7fffffffLL/(b->n_ids > 0 ? b->n_ids : 1) ? MS_EUNSUPPORTED : MS_OK;
}
NavBasinArgs nav_basin_args(const MsNavGrid* grid, const MsNavBasins* b) {
    return NavBasinArgs{grid->free_cells, b->fields, b->ids, b->mask, b->labels, b->sizes, b->reached, b->passes, b->n_fields, b->n_ids};
}
int nav_basin_query_check(const MsNavGrid* grid, const MsNavBasinQuery* q) {
    if (!nav_grid_ok(grid) || !q || q->n_points < 1 || q->n_fields < 1 || !q->points || !q->fields || !q->labels || !q->out ||
        (!q->field && q->n_fields != 1 && q->n_fields != q->n_points) ||
        !all_aligned<4>(q->points, q->field, q->fields, q->labels, q->out)) return MS_EINVAL;
    return (long long)grid->n_envs*q->n_points > 0x7fffff00LL ? MS_EUNSUPPORTED : MS_OK;
}
NavBasinQueryArgs nav_basin_query_args(const MsNavGrid* grid, const MsNavBasinQuery* q) {
    return NavBasinQueryArgs{q->points, q->field, grid->free_cells, q->fields, q->labels, q->out, q->n_points, q->n_fields,
                             (long long)grid->n_envs*q->n_points};
}
int nav_point_marks_check(const MsNavGrid* grid, const MsNavPointMarks* m) {
    if (!nav_grid_ok(grid) || !m || m->n_points < 1 || m->n_fields < 1 || !m->points || !m->marks || !m->ids ||
        (!m->field && m->n_fields != 1 && m->n_fields != m->n_points) ||
        !all_aligned<4>(m->points, m->field, m->point_ids, m->ids)) return MS_EINVAL;
    return (long long)grid->n_envs*m->n_points > 0x7fffff00LL ? MS_EUNSUPPORTED : MS_OK;
}
NavPointMarkArgs nav_point_mark_args(const MsNavGrid* grid, const MsNavPointMarks* m) {
    return NavPointMarkArgs{m->points, m->field, m->point_ids, grid->free_cells, m->marks, m->ids, m->n_points, m->n_fields,
                            (long long)grid->n_envs*m->n_points};
}

// Zones: one instantiation - the kernel's LDS does not grow with the env.
int nav_zones_check(const MsNavGrid* grid, const MsNavZones* z) {
    const auto stores_ok = [&](int count) { return count == 1 || count == z->n_fields; };
    if (!nav_grid_ok(grid) || !z || z->n_fields < 1 || z->max_zones < 1 || z->max_zones > ZONE_MAX || !z->labels || !stores_ok(z->n_labels) ||
        (z->values && !stores_ok(z->n_values)) || (z->marks && (!stores_ok(z->n_marks) || !is_flag(z->where))) ||
        !is_flag(z->ranked) || !is_flag(z->within_marks) || !z->cells || !z->marked || !z->least ||
        !z->nearest || !z->points || !z->roots || !z->n_zones ||
        !all_aligned<4>(z->labels, z->values, z->cells, z->marked, z->least, z->nearest, z->points, z->roots, z->n_zones)) return MS_EINVAL;
    return (long long)grid->n_envs*z->n_fields > 0x7fffffffLL/(2*z->max_zones) ? MS_EUNSUPPORTED : MS_OK;
}
NavZoneArgs nav_zone_args(const MsNavZones* z) {
    return NavZoneArgs{z->labels, z->values, z->marks, z->mask, z->cells, z->marked, z->least, z->nearest, z->points, z->roots, z->n_zones,
                       z->n_fields, z->n_labels, z->values ? z->n_values : 1, z->marks ? z->n_marks : 1, z->marks ? z->where : 1,
                       z->within_marks, z->ranked, z->max_zones};
}
}  // namespace

extern "C" {
int ms_nav_regions(const MsNavGrid* grid, const MsNavRegions* r, void* stream) {
    if (const int status = nav_regions_check(grid, r)) return status;
    static void (*const kernels[3])(NavArgs, NavRegionArgs) = {nav_region_kernel<NAV_LDS_SMALL, 512>, nav_region_kernel<NAV_LDS_MEDIUM, 1024>,
                                                               nav_region_kernel<NAV_LDS_LARGE, 1024>};
    const int t = nav_tier(grid, region_capacity);
    hipLaunchKernelGGL(kernels[t], dim3((unsigned)((long long)grid->n_envs*r->n_fields)), dim3(NAV_TIER_THREADS[t]), 0, (hipStream_t)stream,
                       nav_args(grid), nav_region_args(grid, r));
    return launch_status();
}

int ms_nav_region_query(const MsNavGrid* grid, const MsNavRegionQuery* q, void* stream) {
    if (const int status = nav_region_query_check(grid, q)) return status;
    const long long total = (long long)grid->n_envs*q->n_points;
    const NavRegionQueryArgs a{q->points, q->field, q->labels, q->labels_at, q->n_points, q->n_fields, total};
    hipLaunchKernelGGL(nav_region_query_kernel, dim3((unsigned)((total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, nav_args(grid), a);
    return launch_status();
}

int ms_nav_region_masks(const MsNavGrid* grid, const MsNavRegionMasks* m, void* stream) {
    if (const int status = nav_region_masks_check(grid, m)) return status;
    if (grid->max_framed == 0) return MS_OK;                            // (no env has cells: nothing to write)
    const long long runs = ((long long)grid->max_framed + WG - 1)/WG;  // (at least the largest env's cells; the kernel strides beyond)
    const NavRegionMaskArgs a{m->points, m->wanted, m->field, m->labels, m->out, m->n_requests, m->n_fields};
    hipLaunchKernelGGL(nav_region_mask_kernel, dim3((unsigned)((long long)grid->n_envs*m->n_requests), (unsigned)(runs < 4096 ? runs : 4096)), dim3(WG), 0,
                       (hipStream_t)stream, nav_args(grid), a);
    return launch_status();
}

int ms_host_nav_regions(const MsNavGrid* grid, const MsNavRegions* r) {
    if (const int status = nav_regions_check(grid, r)) return status;
    region_serial(nav_args(grid), nav_region_args(grid, r), nav_capacity_for(grid, region_capacity));
    return MS_OK;
}

int ms_host_nav_region_query(const MsNavGrid* grid, const MsNavRegionQuery* q) {
    if (const int status = nav_region_query_check(grid, q)) return status;
    const long long total = (long long)grid->n_envs*q->n_points;
    const NavRegionQueryArgs a{q->points, q->field, q->labels, q->labels_at, q->n_points, q->n_fields, total};
    for (long long at = 0; at < total; at++) region_query_one(nav_args(grid), a, at);
    return MS_OK;
}

int ms_host_nav_region_masks(const MsNavGrid* grid, const MsNavRegionMasks* m) {
    if (const int status = nav_region_masks_check(grid, m)) return status;
    region_mask_serial(nav_args(grid), NavRegionMaskArgs{m->points, m->wanted, m->field, m->labels, m->out, m->n_requests, m->n_fields});
    return MS_OK;
}

int ms_host_nav_region_capacity(int* capacities) { return nav_host_capacities(capacities, region_capacity); }

int ms_nav_basins(const MsNavGrid* grid, const MsNavBasins* b, void* stream) {
    if (const int status = nav_basins_check(grid, b)) return status;
    static void (*const kernels[3])(NavArgs, NavBasinArgs) = {nav_basin_kernel<NAV_LDS_SMALL, 512>, nav_basin_kernel<NAV_LDS_MEDIUM, 1024>,
                                                              nav_basin_kernel<NAV_LDS_LARGE, 1024>};
    const int t = nav_tier(grid, basin_capacity);
    hipLaunchKernelGGL(kernels[t], dim3((unsigned)((long long)grid->n_envs*b->n_fields)), dim3(NAV_TIER_THREADS[t]), 0, (hipStream_t)stream,
                       nav_args(grid), nav_basin_args(grid, b));
    return launch_status();
}

int ms_nav_basin_query(const MsNavGrid* grid, const MsNavBasinQuery* q, void* stream) {
    if (const int status = nav_basin_query_check(grid, q)) return status;
    const NavBasinQueryArgs a = nav_basin_query_args(grid, q);
    hipLaunchKernelGGL(nav_basin_query_kernel, dim3((unsigned)((a.total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, nav_args(grid), a);
    return launch_status();
}

int ms_nav_point_marks(const MsNavGrid* grid, const MsNavPointMarks* m, void* stream) {
    if (const int status = nav_point_marks_check(grid, m)) return status;
    const NavPointMarkArgs a = nav_point_mark_args(grid, m);
    hipLaunchKernelGGL(nav_point_mark_kernel, dim3((unsigned)((a.total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, nav_args(grid), a);
    return launch_status();
}

int ms_host_nav_basins(const MsNavGrid* grid, const MsNavBasins* b) {
    if (const int status = nav_basins_check(grid, b)) return status;
    basin_serial(nav_args(grid), nav_basin_args(grid, b), nav_capacity_for(grid, basin_capacity));
    return MS_OK;
}

int ms_host_nav_basin_query(const MsNavGrid* grid, const MsNavBasinQuery* q) {
    if (const int status = nav_basin_query_check(grid, q)) return status;
    const NavBasinQueryArgs a = nav_basin_query_args(grid, q);
    for (long long at = 0; at < a.total; at++) basin_query_one(nav_args(grid), a, at);
    return MS_OK;
}

int ms_host_nav_point_marks(const MsNavGrid* grid, const MsNavPointMarks* m) {
    if (const int status = nav_point_marks_check(grid, m)) return status;
    const NavPointMarkArgs a = nav_point_mark_args(grid, m);
    for (long long at = 0; at < a.total; at++) point_mark_one(nav_args(grid), a, at);
    return MS_OK;
}

int ms_host_nav_basin_capacity(int* capacities) { return nav_host_capacities(capacities, basin_capacity); }

int ms_nav_zones(const MsNavGrid* grid, const MsNavZones* z, void* stream) {
    if (const int status = nav_zones_check(grid, z)) return status;
    hipLaunchKernelGGL(nav_zone_kernel, dim3((unsigned)((long long)grid->n_envs*z->n_fields)), dim3(ZONE_THREADS), 0, (hipStream_t)stream,
                       nav_args(grid), nav_zone_args(z));
    return launch_status();
}

int ms_host_nav_zones(const MsNavGrid* grid, const MsNavZones* z) {
    if (const int status = nav_zones_check(grid, z)) return status;
    zone_serial(nav_args(grid), nav_zone_args(z));
    return MS_OK;
}
}  // extern "C"
