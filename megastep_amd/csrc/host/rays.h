// host/rays.h -- rays and pictures asked for as data: ms_raycast and ms_camera_rays (kernels/raycast.h), ms_shade and
// ms_camera_pose_rays (shade.h) with ms_host_shade, ms_overhead (overhead.h) with ms_host_overhead_keeps, and ms_host_fold_hits
// (render.h's three-slot fold of a ray's hits).  Every entry checks its arguments in full before anything is launched.
namespace {
// Shading of given rays: what both ms_shade and ms_host_shade refuse - a scenery without textures or baked light, lights
// announced but not given, a query that lacks a plane, R < 1, agents without poses.
int shade_status(const MsScenery* sc, const MsAgents* ag, const MsShade* q) {
    if (!scenery_ok(sc) || !q || q->n_rays < 1 || !q->indices || !q->locations || !q->dots || !q->screen || !sc->textures_vals ||
        !sc->textures_widths || !sc->textures_starts || !sc->baked_vals || !sc->lights_widths || !sc->lights_starts ||
        (sc->n_lights_total > 0 && !sc->lights_vals) || !all_aligned<4>(q->indices, q->locations, q->dots, q->screen) ||
        !posed_or_none_ok(ag)) return MS_EINVAL;
    return (long long)sc->n_envs*q->n_rays > 0x7fffff00LL/3 ? MS_EUNSUPPORTED : MS_OK;
}
}  // namespace

extern "C" {
int ms_raycast(const MsScenery* sc, const MsAgents* ag, const MsRaycast* rq, const MsConfig* cfg, void* stream) {
    (void)cfg;
    if (!scenery_ok(sc) || !rq || rq->n_rays < 1 || !rq->origins || !rq->dirs || !(rq->near_plane >= 0.f) ||
        !all_aligned<8>(rq->origins, rq->dirs) || !posed_or_none_ok(ag)) return MS_EINVAL;
    const long long total = (long long)sc->n_envs*rq->n_rays;
    if (total > 0x7fffff00LL) return MS_EUNSUPPORTED;
    const bool gridded = vis_lists_serve(sc, rq->near_plane);
    if (gridded && !all_aligned<16>(sc->wg_cells, sc->wg_geom)) return MS_EINVAL;
    const unsigned blocks = (unsigned)((total + WG - 1)/WG);
    hipLaunchKernelGGL(raycast_kernel, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, *sc, agents_or_none(ag), *rq, ag ? 1 : 0,
                       gridded ? 1 : 0, (int)total);
    return launch_status();
}

int ms_camera_rays(const MsAgents* ag, int n_envs, int n_agents, const MsConfig* cfg, float* dirs, void* stream) {
    if (!ag || !ag->angles || n_envs < 1 || n_agents < 1 || !config_ok(cfg) || !dirs || !aligned(dirs, 8)) return MS_EINVAL;
    const long long total = (long long)n_envs*n_agents*cfg->res;
    if ((long long)n_envs*n_agents > 0x7fffffffLL || total > 0x7fffff00LL*(long long)WG) return MS_EUNSUPPORTED;
    const float half_screen = half_screen_of(cfg->fov);
    hipLaunchKernelGGL(camera_rays_kernel, dim3((unsigned)((total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, ag->angles,
                       n_envs*n_agents, cfg->res, half_screen, camera_inv_res(cfg->res, half_screen), reinterpret_cast<float2*>(dirs));
    return launch_status();
}

int ms_shade(const MsScenery* sc, const MsAgents* ag, const MsShade* q, const MsConfig* cfg, void* stream) {
    (void)cfg;
    if (const int status = shade_status(sc, ag, q); status != MS_OK) return status;
    // a light grid is used whole or refused: verdict rows are read 16 bytes at a time, list headers 8, the candidates' rows 16
    const bool gridded = sc->lg_vals != nullptr;
    if (gridded && (!light_grid_in(sc) || !all_aligned<16>(sc->lg_vals, sc->lg_geom, sc->lg_pool_rows) || !aligned(sc->lg_list, 8) ||
                    (sc->lg_list && !sc->lg_pool))) return MS_EINVAL;
    const long long total = (long long)sc->n_envs*q->n_rays;
    hipLaunchKernelGGL(shade_kernel, dim3((unsigned)((total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, *sc, agents_or_none(ag), *q,
                       ag ? 1 : 0, gridded ? 1 : 0, divisor_of((unsigned)sc->n_model), (int)total);
    return launch_status();
}
int ms_host_shade(const MsScenery* sc, const MsAgents* ag, const MsShade* q) {
    if (const int status = shade_status(sc, ag, q); status != MS_OK) return status;
    shade_serial(*sc, ag, *q);
    return MS_OK;
}

int ms_camera_pose_rays(const MsCameraPoses* cams, void* stream) {
    if (!cams || cams->n_envs < 1 || cams->n_cameras < 1 || cams->res < 1 || !cams->poses || !cams->origins || !cams->dirs ||
        !aligned(cams->poses, 4) || !all_aligned<8>(cams->origins, cams->dirs) || !(cams->fov > 0.f)) return MS_EINVAL;
    if (cams->projection == MS_CAMERA_PLANE ? !(cams->fov < 180.f) : (cams->projection != MS_CAMERA_RING || !(cams->fov <= 360.f))) return MS_EINVAL;
    const long long total = (long long)cams->n_envs*cams->n_cameras*cams->res;
    if (total > 0x7fffff00LL) return MS_EUNSUPPORTED;
    const bool plane = cams->projection == MS_CAMERA_PLANE;
    const float half_screen = plane ? half_screen_of(cams->fov) : 0.f;
    hipLaunchKernelGGL(camera_pose_rays_kernel, dim3((unsigned)((total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, *cams, half_screen,
                       plane ? camera_inv_res(cams->res, half_screen) : 0.f, total);
    return launch_status();
}

// Top-down pictures: the env ids are the kernel's to check.
int ms_overhead(const MsScenery* sc, const MsAgents* ag, const MsOverhead* ov, void* stream) {
    if (!scenery_ok(sc) || !ov || ov->n_images < 1 || ov->n_views < 1 || ov->height < 1 || ov->width < 1 || !ov->views ||
        (!ov->rgb && !ov->indices) || !(ov->half_width >= 0.f) || !(ov->half_width < INFINITY)) return MS_EINVAL;
    if (ov->rgb && (!sc->textures_vals || !sc->textures_widths || !sc->textures_starts || (ov->lit && !sc->baked_vals))) return MS_EINVAL;
    if (!posed_or_none_ok(ag)) return MS_EINVAL;
    if (ov->height > (1 << 15) || ov->width > (1 << 15)) return MS_EUNSUPPORTED;
    OvArgs a;
    a.envs = ov->envs; a.views = ov->views; a.rgb = ov->rgb; a.indices = ov->indices;
    a.n_views = ov->n_views; a.height = ov->height; a.width = ov->width;
    a.tiles_x = (ov->width + OV_TILE - 1)/OV_TILE; a.tiles_y = (ov->height + OV_TILE - 1)/OV_TILE;
    a.half_width = ov->half_width; a.h2 = ov->half_width*ov->half_width;
    a.bg_r = ov->background[0]; a.bg_g = ov->background[1]; a.bg_b = ov->background[2];
    a.lit = ov->lit ? 1 : 0; a.with_agents = ag ? 1 : 0; a.cull = g_overhead_cull ? 1 : 0;
    // (a launch of at most 2^22 blocks - 2^30 lanes - at a time: the (image, view, tile) number is 64-bit, the grid's is not)
    const long long total = (long long)ov->n_images*ov->n_views*a.tiles_x*a.tiles_y;
    const long long per_launch = 1LL << 22;
    for (long long b0 = 0; b0 < total; b0 += per_launch) {
        a.block0 = b0;
        const unsigned blocks = (unsigned)(total - b0 < per_launch ? total - b0 : per_launch);
        hipLaunchKernelGGL(overhead_kernel, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, *sc, agents_or_none(ag), a);
        if (const int status = launch_status(); status != MS_OK) return status;
    }
    return MS_OK;
}

int ms_debug_overhead_cull(int on) { g_overhead_cull = on; return MS_OK; }

int ms_host_overhead_keeps(const float* g, int height, int width, int tile_row, int tile_col, float half_width, const float* line) {
    const int i0 = tile_row*OV_TILE, j0 = tile_col*OV_TILE;
    const OvBox box = ov_footprint(g[0], g[1], g[2], g[3], g[4], g[5], i0, j0, i0 + OV_TILE - 1 < height - 1 ? i0 + OV_TILE - 1 : height - 1,
                                   j0 + OV_TILE - 1 < width - 1 ? j0 + OV_TILE - 1 : width - 1);
    return ov_keeps(box, half_width, make_float4(line[0], line[1], line[2], line[3])) ? 1 : 0;
}

int ms_host_fold_hits(const float* s, const int* line, int n_hits, const int* order, float* nearest_s, int* nearest_line) {
    // one ray's hits through the three slots the way a wave plays them: windows of 64 in the given order, and within a
    // window in lockstep - every hit's first merge, then the second merges of those that go on, then the third
    unsigned long long best = ~0ull, second = ~0ull, third = ~0ull;
    for (int w0 = 0; w0 < n_hits; w0 += WAVE) {
        const int nw = (n_hits - w0 < WAVE) ? n_hits - w0 : WAVE;
        unsigned long long lose1[WAVE], lose2[WAVE];
        bool on[WAVE];
        for (int k = 0; k < nw; k++) {
            const int h = order[w0 + k];
            const unsigned long long key = hit_key(s[h], line[h]);
            on[k] = hit_loser_matters(key, s[h], slot_min(&best, key), lose1[k]);
        }
        for (int k = 0; k < nw; k++) if (on[k]) {
            const unsigned long long old2 = slot_min(&second, lose1[k]);
            lose2[k] = old2 > lose1[k] ? old2 : lose1[k];
        }
        for (int k = 0; k < nw; k++) if (on[k] && lose2[k] != ~0ull) slot_min(&third, lose2[k]);
    }
    *nearest_s = INFINITY; *nearest_line = -1;
    return hit_resolve(best, second, third, *nearest_s, *nearest_line) ? 1 : 0;
}
}  // extern "C"
