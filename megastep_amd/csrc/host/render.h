// host/render.h -- the render family: ms_render, ms_move_step_render and ms_step_render (kernels/render.h: render_kernel,
// render_prep_kernel; lighting.h: dynlight_kernel), decided in full by render_prepare and launched by render_enqueue; the launch
// geometry behind ms_host_render_plan / ms_host_render_block; and the render's debug switches.
namespace {
// Launch geometry (host): what ms_render decides before a launch - also behind ms_host_render_plan, so that tests walk whole
// launches on the CPU (tests/test_launch_geometry.py).
// Ray groups per wave (render_kernel's NG): an agent's groups of 64 rays share the wave's list of walls instead of each wave
// building its own.  Measured: four groups pay from 256 rays up - a quarter of the vector instructions saved
// without colour, a sixth with - IF the launch has two and a half rounds of such waves to fill the machine with and every XCD's
// last envs are left to waves of one group (render_block): 4096 x 4 x 512 rays 157.5 -> 139.0 us (colourless 127.4 -> 104.7),
// C5's share 216.7 -> 196.7; with a round or less of them - 4096 x 1 x 256 rays - a quarter is LOST.  Two groups never pay.
// `pinned`: ms_debug_ray_groups (1, 2, 4; else the rule above).  The one-group waves' share: `tail_rounds` rounds of the
// machine's wave slots' worth of the wide waves' work (< 0: half a round), or `tail_envs` envs exactly if >= 0.
struct RenderPlan { int ng; long long n_blocks; };
RenderPlan render_plan(const int n_envs, const int n_agents, const int R, const int slots, const int pinned, const float tail_rounds,
                       const int tail_envs_exact, RenderConsts& rc) {
    int ng = 1;
    if (R >= 4*WAVE && 2LL*n_envs*n_agents*((R + 4*WAVE - 1)/(4*WAVE)) >= 5LL*slots) ng = 4;   // (2.5 rounds, the one-group waves' half included)
    if (pinned == 1 || pinned == 2 || pinned == 4) ng = pinned;
    int tail = 0;
    const int G1 = (R + WAVE - 1)/WAVE;
    const int envs_lo = n_envs/8, envs_rem = n_envs % 8, envs_hi = envs_lo + (envs_rem ? 1 : 0);
    if (ng > 1) {
        const double rounds = tail_rounds >= 0.f ? (double)tail_rounds : 0.5;
        const long long tail_envs = tail_envs_exact >= 0 ? tail_envs_exact : (long long)ceil(rounds*slots*ng/((double)n_agents*G1));
        tail = (int)std::min<long long>((tail_envs + 7)/8, envs_hi);                        // per XCD
        if (tail >= envs_hi && !(pinned > 1)) ng = 1;                 // nothing left for the wide waves: the plain kernel
    }
    const int G = (R + ng*WAVE - 1)/(ng*WAVE);
    rc.by_f = divisor_of((unsigned)(n_agents*G));
    rc.by_g = divisor_of((unsigned)G);
    rc.by_f1 = divisor_of((unsigned)(n_agents*G1));
    rc.by_g1 = divisor_of((unsigned)G1);
    rc.envs_lo = envs_lo; rc.envs_rem = envs_rem; rc.tail = tail;
    // (NG > 1: every XCD as many blocks as the one with the most envs needs)
    const long long n_blocks = ng > 1 ? 8LL*((long long)(envs_hi - std::min(tail, envs_hi))*n_agents*G + (long long)std::min(tail, envs_hi)*n_agents*G1)
                                      : (long long)n_envs*n_agents*G;
    return RenderPlan{ng, n_blocks};
}

// The render call, decided in full before anything is launched: render_prepare makes every check and choice, render_enqueue
// launches what they came to.  A call refused has enqueued nothing; and given `progress` (ms_move_step_render's step),
// render_prepare tells whether the step is one launch (L.fused) - if not, L is the plain render that follows ms_step_physics.
struct RenderLaunch {
    RenderPlan plan;                                  // render_kernel's NG and blocks
    RenderConstsStep rc;                              // (the STEP = 1 part is set only where the step is fused)
    int* schedule;                                    // the fan schedule, where the launch follows it (else NULL): RenderConstsOrder's
    MsScenery scn; AgentsK agn; MsRender outn;        // the copies render_kernel gets
    const MsAgents* ag; const MsRender* out;          // the caller's, as render_prep_kernel and dynlight_kernel get them
    float agent_radius, half_screen; int R;
    bool colour, obs, no_planes;                      // which instantiation of render_kernel
    bool light_grid, walls_listed;
    bool prep;        // headings from render_prep_kernel (else from the cache, from render_kernel itself, or from the fused wave)
    bool dynlight;    // dynlight_kernel afterwards: it lights the rays that landed on an agent
    bool fused;       // the physics step in the render's waves (render_kernel<..., STEP = 1>)
};

int render_prepare(const MsScenery* sc, const MsAgents* ag, const MsRender* out, const MsConfig* cfg, float* progress,
                   const MsMovement* mv, const MsStepExtras* ex, RenderLaunch& L) {
    if (!scenery_ok(sc) || !agents_ok(ag) || !config_ok(cfg) || !out || !sc->textures_vals || !sc->textures_widths ||
        !sc->textures_starts || !sc->baked_vals || !sc->lights_widths || !sc->lights_starts) return MS_EINVAL;
    if ((out->seen_stamp != nullptr) != (out->seen_epoch != nullptr) || (out->seen_stamp != nullptr) != (out->seen_count != nullptr)) return MS_EINVAL;
    if (out->obs_rgb || out->obs_depth || out->obs_centre) {
        const int sub = out->obs_subsample;
        if (sub < 1 || (sub & (sub - 1)) || sub > WAVE || cfg->res % sub) return MS_EINVAL;
        if (out->obs_depth && !(out->obs_max_depth > 0.f)) return MS_EINVAL;
        if (out->obs_centre && cfg->res/sub < 2) return MS_EINVAL;
    }
    if (sc->n_lights_total > 0 && !sc->lights_vals) return MS_EINVAL;
    const int R = cfg->res;
    L.R = R; L.agent_radius = cfg->agent_radius; L.ag = ag; L.out = out;
    L.light_grid = light_grid_in(sc);
    L.colour = out->screen || out->obs_rgb;                              // else: render_kernel<1,0>, which has no pass 3
    // Without a light grid the rays that land on an agent are lit by dynlight_kernel, which takes them by groups of 64.  With
    // one agent per env no ray can land on an agent line (own lines sit inside the near plane), so there is nothing to light.
    L.dynlight = !L.light_grid && sc->n_agents > 1 && L.colour;
    L.plan = render_plan(sc->n_envs, sc->n_agents, R, wave_slots_here(), L.dynlight ? 1 : g_ray_groups, g_tail_rounds, g_tail_envs, L.rc);
    // the workspace's layout (MS_RENDER_WORKSPACE_INTS): 16 counters, a queue of one entry per (env, agent, 64 rays), the headings
    const long long ws_queue = (long long)sc->n_envs*sc->n_agents*((R + WAVE - 1)/WAVE);
    if (L.plan.n_blocks > 0x7fffffffLL || ws_queue > 0x7fffff00LL) return MS_EUNSUPPORTED;
    L.rc.ws_headings = 16 + (int)((ws_queue + 1) & ~1LL);
    const float half_screen = L.half_screen = half_screen_of(cfg->fov);
    // the light grid is all or nothing (light_grid_in) ...
    L.scn = *sc;
    if (!L.light_grid) L.scn.lg_vals = nullptr;
    // ... and so is the wall grid: its vis lists were built for near planes below wg_near and ray direction vectors no
    // longer than sqrt(WG_MAX_RU2) (wallgrid_scan_kernel); a call outside that meets every wall instead
    L.walls_listed = vis_lists_serve(sc, cfg->agent_radius) && 1.f + half_screen*half_screen <= WG_MAX_RU2;
    if (L.walls_listed && !all_aligned<16>(sc->wg_cells, sc->wg_geom)) return MS_EINVAL;
    if (!L.walls_listed) {                                               // (the kernel reads a row of each whatever happens: see there)
        L.scn.wg_cells = nullptr;
        L.scn.wg_geom = sc->lines_vals;                                  // at least 16 bytes per env: every env has its agents' lines
        L.scn.wg_starts = sc->lines_starts;
        L.scn.wg_pool_base = reinterpret_cast<const long long*>(sc->lines_vals);   // (16 bytes of lines per env at least: 8 are there)
    }
    // dynlight_kernel reads the per-ray outputs back and patches `screen`: only the one-kernel path can do without some of them
    const bool all_planes = out->indices && out->locations && out->dots && out->distances && out->screen;
    const bool pooled = out->obs_rgb || out->obs_depth || out->obs_centre || out->seen_stamp;
    if (L.dynlight && (!all_planes || pooled)) return MS_EUNSUPPORTED;
    if (!pooled && !out->indices && !out->locations && !out->dots && !out->distances && !out->screen) return MS_EINVAL;
    L.obs = pooled || !all_planes;
    // (colour, and not one per-ray plane wanted - the demo envs' request: the instantiation that has no plane stores in it)
    L.no_planes = L.colour && !out->indices && !out->locations && !out->dots && !out->distances && !out->screen;
    // The fused step: one agent per env and at most 64 rays - the agent is ONE wave, which runs the env's physics first and
    // renders from the pose it ends on; and a wall grid that serves both halves of the step or neither (ms_render goes without
    // it when the call's near plane or field of view is outside what its vis lists were built for, ms_step_physics never does).
    const bool physics_listed = sc->wg_cells != nullptr;
    L.fused = progress && sc->n_agents == 1 && R <= WAVE && L.plan.ng == 1 && physics_listed == L.walls_listed &&
              (!physics_listed || (sc->wg_near_rows && aligned(sc->wg_near_rows, 16)));
    // Headings: from ms_physics' cache when the agents carry one and a single kernel does the whole job (then the workspace is
    // not needed at all); the fused wave works them out itself (and leaves them in the cache, if there is one); otherwise
    // render_prep_kernel, which also resets the workspace's counters - or, without a workspace, render_kernel - works them out.
    const bool cached = ag->headings && !L.dynlight;
    L.prep = !cached && !L.fused && out->workspace;
    if ((cached && !aligned(ag->headings, 16)) || (L.prep && !aligned(out->workspace, 8))) return MS_EINVAL;
    L.agn = agents_k(*ag);
    L.outn = *out;
    // the fan schedule: every agent one fan, one launch of one-group waves behind a physics launch of its own
    L.schedule = (schedule_serves(ag, sc, R) && L.plan.ng == 1 && !L.fused) ? ag->schedule : nullptr;
    if (!aligned(L.schedule, 4)) return MS_EINVAL;
    if (!cached && !L.fused) L.agn.headings = nullptr;
    if (!L.prep) L.outn.workspace = nullptr;
    if (out->obs_depth) L.outn.obs_max_depth = 1.f/out->obs_max_depth;  // (the kernel multiplies: see the pooled depth in render.h)
    L.rc.x_clip = 0.5f*cfg->agent_radius/sqrtf(1.f + half_screen*half_screen);
    L.rc.c_b = 0.5f*(float)R/half_screen;
    L.rc.by_m = divisor_of((unsigned)sc->n_model);
    L.rc.skip_own = (sc->model_radius > 0.f && sc->model_radius*1.01f < cfg->agent_radius) ? 1 : 0;
    L.rc.inv_res = camera_inv_res(R, half_screen);
    L.rc.telemetry = g_pair_telemetry;
    // (the instantiations with optional outputs - every colourless one, and the colour one of pooled observations at one ray
    // group a wave - read which are wanted from here: see OUT_* in render.h)
    if (!L.colour || (L.obs && L.plan.ng == 1))
        L.outn.obs_subsample = (out->obs_subsample & 0xff) | (((out->indices ? OUT_INDICES : 0) | (out->locations ? OUT_LOCATIONS : 0) |
                                (out->dots ? OUT_DOTS : 0) | (out->distances ? OUT_DISTANCES : 0) | (out->obs_depth ? OUT_DEPTH : 0) |
                                (out->obs_centre ? OUT_CENTRE : 0) | (out->seen_stamp ? OUT_SEEN : 0) | (out->screen ? OUT_SCREEN : 0) |
                                (out->obs_rgb ? OUT_RGB : 0)) << 8);
    if (L.fused) {
        L.rc.progress = progress; L.rc.fps = cfg->fps; L.rc.wg_cells_physics = sc->wg_cells;
        step_options_of(mv, ex, L.rc.mv, L.rc.ex);
    }
    return MS_OK;
}

int render_enqueue(const RenderLaunch& L, const hipStream_t hs) {
    g_last_render_groups = L.plan.ng;
    const int na = L.scn.n_envs*L.scn.n_agents;
    if (L.prep) hipLaunchKernelGGL(render_prep_kernel, dim3((na + WG - 1)/WG), dim3(WG), 0, hs, agents_k(*L.ag), L.out->workspace, na, L.rc.ws_headings);
    // (the STEP = 0 instantiations take the RenderConsts part of L.rc - those of one ray group a wave with the schedule behind it)
    RenderConstsOrder rco;
    static_cast<RenderConsts&>(rco) = L.rc; rco.schedule = L.schedule;
#define MS_LAUNCH_RENDER(O, S, NG_, STEP_) hipLaunchKernelGGL((render_kernel<O, S, NG_, STEP_>), dim3((int)L.plan.n_blocks), dim3(WAVE), 0, hs, \
                                                              L.scn, L.agn, L.outn, L.agent_radius, L.half_screen, L.R, (int)L.plan.n_blocks, L.rc)
#define MS_LAUNCH_RENDER_OS(NG_) { if (!L.colour) MS_LAUNCH_RENDER(1, 0, NG_, 0); else if (L.no_planes) MS_LAUNCH_RENDER(2, 1, NG_, 0); \
                                   else if (L.obs) MS_LAUNCH_RENDER(1, 1, NG_, 0); else MS_LAUNCH_RENDER(0, 1, NG_, 0); }
    if (L.fused) { if (!L.colour) MS_LAUNCH_RENDER(1, 0, 1, 1); else if (L.obs) MS_LAUNCH_RENDER(1, 1, 1, 1); else MS_LAUNCH_RENDER(0, 1, 1, 1); }
    else if (L.plan.ng == 4) MS_LAUNCH_RENDER_OS(4)
    else if (L.plan.ng == 2) MS_LAUNCH_RENDER_OS(2)
    else {
#define MS_LAUNCH_RENDER_1(O, S) hipLaunchKernelGGL((render_kernel<O, S, 1, 0>), dim3((int)L.plan.n_blocks), dim3(WAVE), 0, hs, \
                                                    L.scn, L.agn, L.outn, L.agent_radius, L.half_screen, L.R, (int)L.plan.n_blocks, rco)
        if (!L.colour) MS_LAUNCH_RENDER_1(1, 0); else if (L.no_planes) MS_LAUNCH_RENDER_1(2, 1);
        else if (L.obs) MS_LAUNCH_RENDER_1(1, 1); else MS_LAUNCH_RENDER_1(0, 1);
#undef MS_LAUNCH_RENDER_1
    }
#undef MS_LAUNCH_RENDER_OS
#undef MS_LAUNCH_RENDER
    if (L.dynlight) hipLaunchKernelGGL(dynlight_kernel, dim3((int)L.plan.n_blocks), dim3(WG), 0, hs, L.scn, agents_k(*L.ag), *L.out, L.R);
    return launch_status();
}
}  // namespace

extern "C" {
int ms_debug_ray_groups(int groups) { g_ray_groups = groups; return MS_OK; }
int ms_debug_last_render_groups(void) { return g_last_render_groups; }
int ms_debug_ray_group_tail(float rounds, int envs) { g_tail_rounds = rounds; g_tail_envs = envs; return MS_OK; }
int ms_debug_pair_telemetry(int on) { g_pair_telemetry = on ? 1 : 0; return MS_OK; }
int ms_debug_last_step_fused(void) { return g_last_step_fused; }

long long ms_host_render_plan(int n_envs, int n_agents, int res, int slots, int pinned_groups, float tail_rounds, int tail_envs, int* groups) {
    RenderConsts rc;
    const RenderPlan plan = render_plan(n_envs, n_agents, res, slots, pinned_groups, tail_rounds, tail_envs, rc);
    if (groups) *groups = plan.ng;
    return plan.n_blocks;
}
int ms_host_render_block(int n_envs, int n_agents, int res, int slots, int pinned_groups, float tail_rounds, int tail_envs, long long block, int* out4) {
    RenderConsts rc;
    const RenderPlan plan = render_plan(n_envs, n_agents, res, slots, pinned_groups, tail_rounds, tail_envs, rc);
    int fan = 0;
    if (block < 0 || block >= plan.n_blocks) return -1;
    return render_block((int)block, (int)plan.n_blocks, n_agents, res, plan.ng, rc, out4[0], out4[1], out4[2], out4[3], fan) ? 1 : 0;
}

int ms_render(const MsScenery* sc, const MsAgents* ag, const MsRender* out, const MsConfig* cfg, void* stream) {
    RenderLaunch L;
    const int planned = render_prepare(sc, ag, out, cfg, nullptr, nullptr, nullptr, L);
    return planned != MS_OK ? planned : render_enqueue(L, (hipStream_t)stream);
}

int ms_move_step_render(const MsScenery* sc, const MsAgents* ag, const MsMovement* mv, const MsStepExtras* ex, float* progress,
                        const MsRender* out, const MsConfig* cfg, void* stream) {
    if (!progress || !step_options_ok(mv, ex)) return MS_EINVAL;
    RenderLaunch L;
    const int planned = render_prepare(sc, ag, out, cfg, progress, mv, ex, L);
    g_last_step_fused = 0;
    if (planned != MS_OK) return planned;
    const int p = L.fused ? MS_OK : ms_step_physics(sc, ag, mv, ex, progress, cfg, stream);
    const int r = p != MS_OK ? p : render_enqueue(L, (hipStream_t)stream);
    g_last_step_fused = L.fused && r == MS_OK;
    return r;
}
int ms_step_render(const MsScenery* sc, const MsAgents* ag, float* progress, const MsRender* out, const MsConfig* cfg, void* stream) {
    return ms_move_step_render(sc, ag, nullptr, nullptr, progress, out, cfg, stream);
}
}  // extern "C"
