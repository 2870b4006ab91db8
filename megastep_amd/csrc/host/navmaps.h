// host/navmaps.h -- per-cell maps on the nav grid: ms_nav_seen (kernels/navseen.h), ms_nav_ages (navage.h), ms_nav_windows
// (navwindow.h), ms_nav_draws (navdraw.h), and the host instantiation of each: ms_host_nav_seen, ms_host_nav_ages,
// ms_host_nav_windows, ms_host_nav_draws.  An env of more than 2^20 cells is refused, and nothing is enqueued.
namespace {
constexpr int NAV_SEEN_MAX_CELLS = 1 << 20;
bool nav_seen_ok(const MsNavSeen* v) {
    return v && v->n_maps >= 1 && v->n_viewers >= 1 && v->n_rays >= 1 && v->origins && v->dirs && v->distances && v->maps &&
           (v->slot || v->n_viewers == v->n_maps) && positive_finite(v->max_range) && v->max_cells >= 0 &&
           all_aligned<8>(v->origins, v->dirs) && all_aligned<4>(v->distances, v->slot, v->gained, v->total);
}

// Age maps: the seen maps' limit; one check serves the launch and the host instantiation.
int nav_ages_check(const MsNavAges* v) {
    if (!v || v->n_maps < 1 || !v->last || !v->clock || v->threshold < 1 || !is_flag(v->advance) ||
        !positive_finite(v->max_range) || v->max_cells < 0 ||
        !all_aligned<4>(v->last, v->clock, v->swept, v->gained, v->oldest, v->n_stale, v->ages) ||
        !all_aligned<8>(v->idle, v->total_age)) return MS_EINVAL;
    if (v->advance && (v->n_viewers < 1 || v->n_rays < 1 || !v->origins || !v->dirs || !v->distances ||
                       !(v->slot || v->n_viewers == v->n_maps) || !all_aligned<8>(v->origins, v->dirs) ||
                       !all_aligned<4>(v->distances, v->slot))) return MS_EINVAL;
    return v->max_cells > NAV_SEEN_MAX_CELLS ? MS_EUNSUPPORTED : MS_OK;
}
NavAgeArgs nav_age_args(const MsNavAges* v, const unsigned char* countable) {
    return NavAgeArgs{v->origins, v->dirs, v->distances, v->slot, v->reset, countable, v->last, v->clock, v->swept, v->gained, v->idle,
                      v->oldest, v->total_age, v->n_stale, v->stale, v->ages, v->n_maps, v->advance ? v->n_viewers : 0,
                      v->advance ? v->n_rays : 0, v->max_cells, v->advance, v->threshold, v->max_range};
}

// Map windows: the channels go into the kernel's arguments by value.
bool nav_layer_ok(const MsNavLayer& l, const int n_views) {
    return l.values && is_flag(l.is_float) && l.n_fields >= 1 && (l.field || l.n_fields == 1 || l.n_fields == n_views) &&
           aligned(l.field, 4) && (!l.is_float || aligned(l.values, 4));
}
bool nav_windows_ok(const MsNavWindows* w) {
    if (!w || w->n_views < 1 || w->height < 1 || w->height > WIN_MAX_SIDE || w->width < 1 || w->width > WIN_MAX_SIDE ||
        w->samples < 1 || w->samples > WIN_MAX_SAMPLES || w->n_channels < 1 || w->n_channels > WIN_MAX_CHANNELS || !w->views ||
        !w->channels || !w->out || !all_aligned<4>(w->views, w->out)) return false;
    for (int c = 0; c < w->n_channels; c++) {
        const MsNavChannel& ch = w->channels[c];
        if (!nav_layer_ok(ch.source, w->n_views) || !is_flag(ch.where)) return false;
        if (ch.gate.values && (!nav_layer_ok(ch.gate, w->n_views) || ch.gate.is_float)) return false;
    }
    return true;
}
NavWindowArgs nav_window_args(const MsNavWindows* w) {
    NavWindowArgs q{w->views, w->out, w->n_views, w->height, w->width, w->n_channels, {}};
    for (int c = 0; c < w->n_channels; c++) {
        const MsNavChannel& ch = w->channels[c];
        const bool gated = ch.gate.values != nullptr;
        q.ch[c] = WinChannel{ch.source.values, ch.source.field, static_cast<const unsigned char*>(ch.gate.values), gated ? ch.gate.field : nullptr,
                             ch.source.n_fields, gated ? ch.gate.n_fields : 1, ch.source.is_float, ch.where, ch.scale, ch.outside, ch.hidden};
    }
    return q;
}

// Cell draws: the bitmap's size is the seen maps'.
int nav_draws_check(const MsNavGrid* grid, const MsNavDraws* d) {
    if (!nav_grid_ok(grid) || !d || d->n_sets < 1 || d->n_draws < 1 || d->n_draws > DRAW_MAX_DRAWS || !nav_layer_ok(d->source, d->n_sets) ||
        !is_flag(d->where) || (d->gate.values && (!nav_layer_ok(d->gate, d->n_sets) || d->gate.is_float)) ||
        (d->source.is_float && (d->lo != d->lo || d->hi != d->hi)) || (d->values && !d->source.is_float) ||
        !d->counter || !d->cells || !d->points || !d->uniforms || !d->counts || d->max_cells < 0 ||
        !all_aligned<4>(d->counter, d->cells, d->points, d->uniforms, d->values, d->counts)) return MS_EINVAL;
    return (d->max_cells > NAV_SEEN_MAX_CELLS || (long long)grid->n_envs*d->n_sets > 0x7fffffffLL/d->n_draws) ? MS_EUNSUPPORTED : MS_OK;
}
NavDrawArgs nav_draw_args(const MsNavGrid* grid, const MsNavDraws* d) {
    const bool gated = d->gate.values != nullptr;
    return NavDrawArgs{d->source.values, d->source.field, static_cast<const unsigned char*>(d->gate.values), gated ? d->gate.field : nullptr,
                       grid->free_cells, d->mask, d->counter, d->cells, d->points, d->uniforms, d->values, d->counts,
                       d->source.n_fields, gated ? d->gate.n_fields : 1, d->source.is_float, d->where, d->lo, d->hi,
                       (unsigned)(d->seed & 0xffffffffull), (unsigned)(d->seed >> 32), d->n_sets, d->n_draws, d->max_cells};
}
}  // namespace

extern "C" {
int ms_nav_seen(const MsNavGrid* grid, const MsNavSeen* v, void* stream) {
    if (!nav_grid_ok(grid) || !nav_seen_ok(v)) return MS_EINVAL;
    const long long total = (long long)grid->n_envs*v->n_maps;
    if (v->max_cells > NAV_SEEN_MAX_CELLS || total > 0x7fffffffLL || (long long)grid->n_envs*v->n_viewers > 0x7fffffffLL/v->n_rays)
        return MS_EUNSUPPORTED;
    const NavSeenArgs q{v->origins, v->dirs, v->distances, v->slot, v->reset, v->countable ? v->countable : grid->free_cells, v->maps,
                        v->gained, v->total, v->n_maps, v->n_viewers, v->n_rays, v->max_cells, v->max_range};
    const size_t lds = (size_t)((v->max_cells + 31)/32)*sizeof(unsigned);                   // (at most 128 KiB of the CU's 160)
    if (const int status = allow_dynamic_lds(nav_seen_kernel, lds, 64*1024)) return status;
    hipLaunchKernelGGL(nav_seen_kernel, dim3((unsigned)total), dim3(WG), lds, (hipStream_t)stream, nav_args(grid), q);
    return launch_status();
}

int ms_host_nav_seen(const int* geom, float cell, const unsigned char* countable, int n_maps, int n_viewers, int n_rays,
                     const float* origins, const float* dirs, const float* distances, const int* slot, float max_range,
                     const unsigned char* reset, unsigned char* maps, int* gained, int* total) {
    if (!geom || !positive_finite(cell) || n_maps < 1 || n_viewers < 1 || n_rays < 1 || !origins || !dirs || !distances ||
        !maps || !countable || !(slot || n_viewers == n_maps) || !positive_finite(max_range)) return -1;
    seen_serial(NavCells{geom[0], geom[1], geom[2], geom[3], cell}, countable, n_maps, n_viewers, n_rays, origins, dirs, distances, slot,
                max_range, reset, maps, gained, total);
    return 0;
}

int ms_nav_ages(const MsNavGrid* grid, const MsNavAges* v, void* stream) {
    if (!nav_grid_ok(grid)) return MS_EINVAL;
    if (const int status = nav_ages_check(v)) return status;
    const long long total = (long long)grid->n_envs*v->n_maps;
    if (total > 0x7fffffffLL || (v->advance && (long long)grid->n_envs*v->n_viewers > 0x7fffffffLL/v->n_rays)) return MS_EUNSUPPORTED;
    const size_t lds = (size_t)((v->max_cells + 31)/32)*sizeof(unsigned);                   // (at most 128 KiB of the CU's 160)
    if (const int status = allow_dynamic_lds(nav_age_kernel, lds, 64*1024 - 256)) return status;
    hipLaunchKernelGGL(nav_age_kernel, dim3((unsigned)total), dim3(WG), lds, (hipStream_t)stream, nav_args(grid),
                       nav_age_args(v, v->countable ? v->countable : grid->free_cells));
    return launch_status();
}

int ms_host_nav_ages(const int* geom, float cell, const MsNavAges* v) {
    if (!geom || !positive_finite(cell)) return MS_EINVAL;
    if (const int status = nav_ages_check(v)) return status;
    if (!v->countable) return MS_EINVAL;
    if (geom[2] > 0 && geom[3] > 0 && (long long)geom[2]*geom[3] > NAV_SEEN_MAX_CELLS) return MS_EUNSUPPORTED;
    age_serial(NavCells{geom[0], geom[1], geom[2], geom[3], cell}, nav_age_args(v, v->countable));
    return MS_OK;
}

int ms_nav_windows(const MsNavGrid* grid, const MsNavWindows* w, void* stream) {
    if (!nav_grid_ok(grid) || !nav_windows_ok(w)) return MS_EINVAL;
    const long long images = (long long)grid->n_envs*w->n_views;
    if (images > 0x7fffffffLL) return MS_EUNSUPPORTED;
    const dim3 blocks((unsigned)images, (unsigned)((w->height*w->width + WG - 1)/WG));      // (y: at most 4096)
    static void (*const kernels[WIN_MAX_SAMPLES])(NavArgs, NavWindowArgs) = {nav_window_kernel<1>, nav_window_kernel<2>, nav_window_kernel<3>,
                                                                             nav_window_kernel<4>};   // [samples - 1]
    hipLaunchKernelGGL(kernels[w->samples - 1], blocks, dim3(WG), 0, (hipStream_t)stream, nav_args(grid), nav_window_args(w));
    return launch_status();
}

int ms_host_nav_windows(const MsNavGrid* grid, const MsNavWindows* w) {
    if (!nav_grid_ok(grid) || !nav_windows_ok(w)) return MS_EINVAL;
    static void (*const serial[WIN_MAX_SAMPLES])(const NavArgs&, const NavWindowArgs&) = {win_serial<1>, win_serial<2>, win_serial<3>, win_serial<4>};
    serial[w->samples - 1](nav_args(grid), nav_window_args(w));
    return MS_OK;
}

int ms_nav_draws(const MsNavGrid* grid, const MsNavDraws* d, void* stream) {
    if (const int status = nav_draws_check(grid, d)) return status;
    const size_t lds = (size_t)((d->max_cells + 63)/64 + WG)*sizeof(unsigned long long);      // (at most 130 KiB of the CU's 160)
    if (const int status = allow_dynamic_lds(nav_draw_kernel, lds, 64*1024)) return status;
    hipLaunchKernelGGL(nav_draw_kernel, dim3((unsigned)((long long)grid->n_envs*d->n_sets)), dim3(WG), lds, (hipStream_t)stream,
                       nav_args(grid), nav_draw_args(grid, d));
    return launch_status();
}

int ms_host_nav_draws(const MsNavGrid* grid, const MsNavDraws* d) {
    if (const int status = nav_draws_check(grid, d)) return status;
    draw_serial(nav_args(grid), nav_draw_args(grid, d));
    return MS_OK;
}
}  // extern "C"
