// host/wallgrid.h -- ms_wallgrid_scan and ms_wallgrid_fill (kernels/wallgrid.h: wallgrid_scan_kernel, wallgrid_fill_kernel) and
// the host hooks of the grid's predicates: ms_host_wall_hidden, ms_host_wallgrid_cell, ms_host_wall_sectors, ms_host_wall_arc,
// ms_host_wedge, ms_host_wedge_meets.
namespace {
bool wallgrid_ok(const MsScenery* sc) {
    return sc->wg_starts && sc->wg_geom && sc->wg_cell > 0.f && sc->wg_reach_lo >= 0.f && sc->wg_reach >= sc->wg_reach_lo &&
           sc->wg_near > 0.f && aligned(sc->wg_geom, 16);
}
}  // namespace

extern "C" {
int ms_host_wall_hidden(float x0, float y0, float x1, float y1, const float* o, const float* w, float near_plane) {
    const WgCell k{x0, y0, x1, y1};
    const WgTarget t = wg_target(k, make_float4(w[0], w[1], w[2], w[3]));
    return wg_hides(k, t, make_float4(o[0], o[1], o[2], o[3]), near_plane) ? 1 : 0;
}

void ms_host_wallgrid_cell(const float* walls, int n_walls, float ox, float oy, int nx, int ny, float cell, int c,
                           float near_plane, float reach_lo, float reach, unsigned char* vis, unsigned char* close) {
    const float4* ln = reinterpret_cast<const float4*>(walls);
    const WgCell k = wg_cell_of(make_float4(ox, oy, (float)nx, (float)ny), cell, c);
    for (int t = 0; t < n_walls; t++) {
        const WgTarget tg = wg_target(k, ln[t]);
        bool hidden = false;
        for (int o = 0; o < n_walls && !hidden; o++) hidden = (o != t) && wg_hides(k, tg, ln[o], near_plane);
        vis[t] = hidden ? 0 : 1;
        close[t] = wg_close(k, ln[t], reach) ? (wg_close(k, ln[t], reach_lo) ? 2 : 1) : 0;
    }
}

void ms_host_wall_sectors(float x0, float y0, float x1, float y1, const float* o, int* first, int* count, const float* w, int* sector) {
    const float cx = .5f*(x0 + x1), cy = .5f*(y0 + y1);
    wg_sectors_of(cx, cy, make_float4(o[0], o[1], o[2], o[3]), *first, *count);
    *sector = wg_sector_of(cx, cy, make_float4(w[0], w[1], w[2], w[3]));
}
void ms_host_wall_arc(float x0, float y0, float x1, float y1, const float* w, int* lo8, int* hi8) {
    wg_arc(WgCell{x0, y0, x1, y1}, make_float4(w[0], w[1], w[2], w[3]), *lo8, *hi8);
}
void ms_host_wedge(float right_x, float right_y, float left_x, float left_y, int* wa8, int* wb8) {
    wg_wedge(pseudo_angle(right_x, right_y), pseudo_angle(left_x, left_y), *wa8, *wb8);
}
int ms_host_wedge_meets(float right_x, float right_y, float left_x, float left_y, int lo8, int hi8) {
    int wa8, wb8;
    ms_host_wedge(right_x, right_y, left_x, left_y, &wa8, &wb8);
    return wg_arcs_meet(lo8, hi8, wa8, wb8) ? 1 : 0;
}

int ms_wallgrid_scan(const MsScenery* sc, const MsWallGridParent* parent, const int* reps, int n_reps, int max_groups,
                     const long long* bits_starts, unsigned* bits, unsigned* counts, void* stream) {
    if (!scenery_ok(sc) || !wallgrid_ok(sc) || !reps || n_reps < 0 || max_groups < 0 || !bits_starts || !bits || !counts) return MS_EINVAL;
    WgParent par{nullptr, nullptr, nullptr, 0.f, nullptr};
    if (parent) {
        if (!parent->cells || !parent->starts || !parent->geom || !parent->pool || !(parent->cell >= sc->wg_cell) ||
            !all_aligned<16>(parent->cells, parent->geom)) return MS_EINVAL;
        par = WgParent{parent->cells, parent->starts, parent->geom, parent->cell, parent->pool};
    }
    if (n_reps == 0 || max_groups == 0) return MS_OK;
    if (n_reps > 65535) return MS_EUNSUPPORTED;
    hipLaunchKernelGGL(wallgrid_scan_kernel, dim3((unsigned)max_groups, (unsigned)n_reps), dim3(WG), 0, (hipStream_t)stream,
                       *sc, par, reps, bits_starts, bits, counts);
    return launch_status();
}

int ms_wallgrid_fill(const MsScenery* sc, const int* reps, int n_reps, int max_cells,
                     const long long* bits_starts, const unsigned* bits, unsigned short* pool, unsigned* vis_entries, float* near_rows,
                     void* stream) {
    if (!scenery_ok(sc) || !wallgrid_ok(sc) || !sc->wg_cells || !aligned(sc->wg_cells, 16) || !reps || n_reps < 0 || max_cells < 0 ||
        !bits_starts || !bits || ((vis_entries != nullptr) != (near_rows != nullptr)) || (!pool && !vis_entries) || (vis_entries && !sc->wg_pool_base) ||
        !aligned(near_rows, 16) || !aligned(vis_entries, 4)) return MS_EINVAL;
    if (n_reps == 0 || max_cells == 0) return MS_OK;
    const long long blocks = (2LL*max_cells + WAVES - 1)/WAVES;
    if (blocks > 0x7fffffffLL || n_reps > 65535) return MS_EUNSUPPORTED;
    hipLaunchKernelGGL(wallgrid_fill_kernel, dim3((unsigned)blocks, (unsigned)n_reps), dim3(WG), 0, (hipStream_t)stream,
                       *sc, reps, bits_starts, bits, pool, reinterpret_cast<float4*>(near_rows), vis_entries);
    return launch_status();
}
}  // extern "C"
