// host/bake.h -- ms_bake (kernels/bake.h: visibility_kernel and bake_sum_kernel, or bake_kernel; kernels/lighting.h:
// lightgrid_kernel, lightlist_kernel) and the host hooks of their predicates: ms_host_bake_*, ms_host_lightgrid_cell.
extern "C" {
int ms_host_bake_point_bin(float light_x, float light_y, float x, float y) { return bake_point_bin(p2(light_x, light_y), p2(x, y)); }
void ms_host_bake_wall_bins(float light_x, float light_y, float ax, float ay, float bx, float by, int* first, int* count) {
    bake_wall_bins(p2(light_x, light_y), ax, ay, bx, by, *first, *count);
}

int ms_host_lightgrid_cell(const float* walls, int n_walls, const float* lights, int n_lights, float ox, float oy, int nx, int ny,
                           float cell, int c, unsigned* words, unsigned* candidates, int max_candidates) {
    // lightgrid_kernel's verdicts and lightlist_kernel's candidates for one cell, from the predicates those are compiled from
    const LgCell k = lg_cell_of(make_float4(ox, oy, (float)nx, (float)ny), cell, c);
    const int num_i = n_lights < LG_LIGHTS ? n_lights : LG_LIGHTS;
    words[0] = words[1] = words[2] = words[3] = 0u;
    int count = 0;
    for (int i = 0; i < num_i; i++) {
        const LgView v = lg_view_of(k, p2(lights[3*i], lights[3*i + 1]));
        bool touched = false, dark = false;
        for (int j = 0; j < n_walls && !dark; j++) {
            const float4 w = make_float4(walls[4*j], walls[4*j + 1], walls[4*j + 2] - walls[4*j], walls[4*j + 3] - walls[4*j + 1]);
            if (!lg_touches(k, v, w)) continue;
            touched = true;
            dark = lg_shadows(v, w);
        }
        const unsigned st = dark ? 2u : (touched ? 0u : 1u);
        words[i >> 4] |= st << (2*(i & 15));
        if (st == 0u) {
            for (int j = 0; j < n_walls; j++) {
                const float4 w = make_float4(walls[4*j], walls[4*j + 1], walls[4*j + 2] - walls[4*j], walls[4*j + 3] - walls[4*j + 1]);
                if (!lg_touches(k, v, w)) continue;
                if (count < max_candidates) candidates[count] = 0x80000000u | ((unsigned)i << 24) | (unsigned)j;
                count++;
            }
        }
    }
    return count;
}

int ms_bake(const MsScenery* sc, const MsConfig* cfg, void* stream) {
    (void)cfg;
    if (!scenery_ok(sc) || !sc->textures_widths || !sc->textures_starts || !sc->textures_inverse ||
        !sc->baked_vals || !sc->lights_widths || !sc->lights_starts) return MS_EINVAL;
    if (sc->n_lights_total > 0 && !sc->lights_vals) return MS_EINVAL;
    if (sc->n_texels_total > 0 && sc->bake_vis &&
        (!sc->bake_vis_starts || sc->bake_vis_words < 0 || !sc->lines_inverse || !aligned(sc->bake_vis, 8))) return MS_EINVAL;
    if (sc->lg_vals && (!sc->lg_starts || !sc->lg_geom || !(sc->lg_cell > 0.f) || sc->lg_max_cells <= 0 ||
                        !all_aligned<16>(sc->lg_vals, sc->lg_geom) || (sc->lg_list != nullptr) != (sc->lg_pool != nullptr) ||
                        (sc->lg_pool && sc->lg_pool_size < 1) || (sc->lg_pool_rows && (!sc->lg_pool || !aligned(sc->lg_pool_rows, 16))) ||
                        !aligned(sc->lg_list, 8))) return MS_EINVAL;
    if (sc->n_texels_total > 0 && sc->bake_vis) {
        // two phases: visibility once per representative env and light, then the per-env sums
        const char* be = getenv("MEGASTEP_BAKE_BINS");                 // =0: every texel meets every wall (A/B runs)
        const bool bins = !(be && be[0] == '0');
        if (sc->n_lights_total > 0)
            hipLaunchKernelGGL(visibility_kernel, dim3(sc->n_lights_total), dim3(WG), 0, (hipStream_t)stream, *sc, bins ? 1 : 0);
        const long long blocks = ((long long)sc->n_texels_total + WG - 1)/WG;
        hipLaunchKernelGGL(bake_sum_kernel, dim3((unsigned)blocks), dim3(WG), 0, (hipStream_t)stream, *sc);
    } else if (sc->n_texels_total > 0) {
        hipLaunchKernelGGL(bake_kernel, dim3(sc->n_envs), dim3(WG), 0, (hipStream_t)stream, *sc);
    }
    if (sc->lg_vals) {
        const dim3 cells((sc->lg_max_cells + WG - 1)/WG, sc->n_envs);
        hipLaunchKernelGGL(lightgrid_kernel, cells, dim3(WG), 0, (hipStream_t)stream, *sc);
        if (sc->lg_list) {
            if (hipMemsetAsync(sc->lg_pool, 0, sizeof(unsigned), (hipStream_t)stream) != hipSuccess) return hip_fail(hipGetLastError());
            hipLaunchKernelGGL(lightlist_kernel, cells, dim3(WG), 0, (hipStream_t)stream, *sc);
        }
    }
    return launch_status();
}
}  // extern "C"
