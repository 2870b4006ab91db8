// host/items.h -- items: ms_item_collect and ms_item_overlay (kernels/items.h), and the host instantiation of each.  One check
// serves a launch and its host instantiation.
namespace {
// Collect.  The limits keep a wave's tally of counts within its slice of LDS and a lane's items within sixteen.
int item_collect_check(const MsItemCollect* c, const int n_agents, const float* agent_positions) {
    if (!c || !agent_positions || n_agents < 1 || n_agents > ITEM_MAX_AGENTS || c->n_items < 1 || c->n_items > ITEM_MAX_ITEMS ||
        c->n_kinds < 1 || c->n_kinds > ITEM_MAX_KINDS || !c->positions || !c->timers || !c->kinds || !positive_finite(c->reach) ||
        !is_flag(c->through_walls) || !all_aligned<8>(agent_positions, c->positions) ||
        !all_aligned<4>(c->timers, c->kinds, c->taker, c->counts)) return MS_EINVAL;
    return MS_OK;
}
ItemCollectArgs item_collect_args(const MsItemCollect* c, const int n_envs, const int n_agents, const float* agent_positions) {
    return ItemCollectArgs{c->positions, c->timers, c->kinds, c->takers, c->reset, agent_positions, c->taker, c->counts, c->due,
                           n_envs, n_agents, c->n_items, c->n_kinds, c->delay, c->through_walls, c->reach*c->reach};
}

// Overlay.  A workgroup takes up to WG rays of one origin.
int item_overlay_check(const MsItemOverlay* o, const int n_envs) {
    if (!o || n_envs < 1 || o->n_items < 1 || o->n_items > ITEM_MAX_ITEMS || o->n_rays < 1 || o->n_origins < 1 ||
        o->n_rays % o->n_origins != 0 || !o->positions || !o->origins || !o->dirs || !o->distances || (o->screen && !o->colors) ||
        !positive_finite(o->radius) || !(o->near_plane >= 0.f) || !all_aligned<8>(o->positions, o->origins, o->dirs) ||
        !all_aligned<4>(o->colors, o->distances, o->indices, o->locations, o->dots, o->screen, o->items)) return MS_EINVAL;
    if ((long long)n_envs*o->n_rays > 0x7fffffffLL) return MS_EUNSUPPORTED;
    const int per_origin = o->n_rays/o->n_origins;
    return (long long)n_envs*o->n_origins*((per_origin + WG - 1)/WG) > 0x7fffffffLL ? MS_EUNSUPPORTED : MS_OK;
}
ItemOverlayArgs item_overlay_args(const MsItemOverlay* o, const int n_envs, const int* lines_widths) {
    const int per_origin = o->n_rays/o->n_origins;
    return ItemOverlayArgs{o->positions, o->colors, o->origins, o->dirs, lines_widths, o->distances, o->indices, o->locations, o->dots,
                           o->screen, o->items, n_envs, o->n_items, o->n_rays, o->n_origins, per_origin, (per_origin + WG - 1)/WG,
                           o->radius, o->near_plane};
}
}  // namespace

extern "C" {
int ms_item_collect(const MsScenery* sc, const MsAgents* ag, const MsItemCollect* c, void* stream) {
    if (!scenery_ok(sc) || !ag) return MS_EINVAL;
    if (const int status = item_collect_check(c, sc->n_agents, ag->positions)) return status;
    hipLaunchKernelGGL(item_collect_kernel, dim3((unsigned)((sc->n_envs + WAVES - 1)/WAVES)), dim3(WG), 0, (hipStream_t)stream, *sc,
                       item_collect_args(c, sc->n_envs, sc->n_agents, ag->positions));
    return launch_status();
}

int ms_host_item_collect(const MsItemCollect* c, int n_envs, int n_agents, const float* agent_positions, const float* walls,
                         const long long* wall_starts) {
    if (const int status = item_collect_check(c, n_agents, agent_positions)) return status;
    if (n_envs < 1 || !walls || !wall_starts) return MS_EINVAL;
    item_collect_serial(item_collect_args(c, n_envs, n_agents, agent_positions), reinterpret_cast<const float4*>(walls), wall_starts);
    return MS_OK;
}

int ms_item_overlay(const MsScenery* sc, const MsItemOverlay* o, void* stream) {
    if (!scenery_ok(sc)) return MS_EINVAL;
    if (const int status = item_overlay_check(o, sc->n_envs)) return status;
    const ItemOverlayArgs q = item_overlay_args(o, sc->n_envs, sc->lines_widths);
    hipLaunchKernelGGL(item_overlay_kernel, dim3((unsigned)((long long)sc->n_envs*q.n_origins*q.chunks)), dim3(WG), 0, (hipStream_t)stream, q);
    return launch_status();
}

int ms_host_item_overlay(const MsItemOverlay* o, int n_envs, const int* lines_widths) {
    if (const int status = item_overlay_check(o, n_envs)) return status;
    if (o->indices && !lines_widths) return MS_EINVAL;
    item_overlay_serial(item_overlay_args(o, n_envs, lines_widths));
    return MS_OK;
}
}  // extern "C"
