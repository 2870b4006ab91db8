// host/step.h -- the step family: ms_step_physics with ms_move_physics and ms_physics (kernels/physics.h), ms_slide_physics
// (slide.h), ms_rollouts (rollout.h), ms_scenarios (scenario.h); their host instantiations ms_host_slide, ms_host_rollouts,
// ms_host_scenarios; the hooks ms_host_physics_pack, ms_host_move_velocity, ms_host_order_fans; and the step's debug switches.
namespace {
// Envs per wave (physics_kernel's PACK), with a wall grid (without one an env's walls are streamed, and there is nothing to put
// side by side) and while a wave's agents stay within half its lanes: as many as bring the launch down to about 4096 waves -
// 32768 envs of one agent are 5.3 rounds of waves with a lane or two at work each: 30.2 us; eight to a wave 9.7 (four 13.6,
// sixteen 10.2); 16384 x 4 agents 22.2 -> 13.3 (eight: 17.8), 8192 x 4 13.4 -> 10.2 - and two even at 4096 envs, where one round
// of short waves becomes half a round of waves twice as busy (8.7 -> 8.2 us; three 8.7, four 9.5; one agent per env 7.1 -> 6.4).
// `pinned`: ms_debug_physics_pack (>= 1; else the rule).  Also behind ms_host_physics_pack, so that tests walk whole launches on
// the CPU (tests/test_launch_geometry.py).
int physics_pack_of(const int n_envs, const int n_agents, const bool gridded, const int pinned) {
    int pack = 1;
    if (gridded && n_agents <= 16) {
        pack = n_envs > 6144 ? std::min((n_envs + 4095)/4096, 16) : n_envs >= 3072 ? 2 : 1;
        pack = std::max(std::min(pack, WAVE/2/n_agents), 1);
    }
    if (pinned >= 1) pack = (gridded && (long long)pinned*n_agents <= WAVE) ? pinned : 1;
    return pack;
}

// (the optional structs of ms_step_physics / ms_move_step_render, checked alike)
bool step_options_ok(const MsMovement* mv, const MsStepExtras* ex) {
    if (mv && (!mv->actions || !mv->table || mv->n_actions < 1 || !(mv->keep == mv->keep))) return false;
    if (ex) {
        if (ex->spawn_positions && (!ex->spawn_angles || !ex->respawn_mask || !ex->respawn_choice || ex->n_spawns < 1 ||
                                    !aligned(ex->spawn_positions, 8))) return false;
        if (ex->lifespans && (!ex->max_lifespans || !ex->fresh_max)) return false;
        if (ex->imu && !(ex->imu_ang_scale == ex->imu_ang_scale && ex->imu_speed_scale == ex->imu_speed_scale)) return false;
    }
    return true;
}
// ... and as the kernels take them: all-NULL structs for none, the IMU scales inverted (the kernels multiply: see their IMU reading)
void step_options_of(const MsMovement* mv, const MsStepExtras* ex, MsMovement& mvv, MsStepExtras& exv) {
    mvv = mv ? *mv : MsMovement{nullptr, nullptr, 0, 0.f};
    exv = ex ? *ex : MsStepExtras{nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 1.f, 1.f};
    exv.imu_ang_scale = 1.f/exv.imu_ang_scale; exv.imu_speed_scale = 1.f/exv.imu_speed_scale;
}

// A scenery whose wall grid carries near lists carries all of them, rows the kernels read 16 bytes at a time (wg_cells % 16,
// wg_geom % 16, wg_near_rows % 16): what every entry of the step family holds a gridded scenery to.
bool near_lists_ok(const MsScenery* sc) {
    return !sc->wg_cells || (sc->wg_starts && sc->wg_geom && sc->wg_near_rows && sc->wg_cell > 0.f &&
                             all_aligned<16>(sc->wg_cells, sc->wg_geom, sc->wg_near_rows));
}

// The fan schedule serves launches in which every agent is ONE wave of the render: at most 64 rays (ms_step_physics sorts on this
// alone - it cannot know what the render behind it will be asked for; a table nobody follows costs it a few dozen short waves).
bool schedule_serves(const MsAgents* a, const MsScenery* sc, const int R) {
    return g_render_order && a->schedule && R <= WAVE && (long long)sc->n_envs*sc->n_agents <= 0x3fffffffLL;
}
// The fan schedule's sort waves, in front of a physics launch's own (physics.h): last frame's render costs into this frame's order
// (none where the schedule does not serve).
FanSort fan_sort_for(const MsAgents* ag, const MsScenery* sc, const int R) {
    FanSort fs{nullptr, 0, 1, 0};
    if (schedule_serves(ag, sc, R)) {
        fs.schedule = ag->schedule; fs.n_fans = sc->n_envs*sc->n_agents;
        fs.per_run = fan_sort_per_run(fs.n_fans); fs.n_blocks = 8*fs.per_run;
    }
    return fs;
}

// what ms_slide_physics and ms_host_slide refuse alike of an MsSlide and the shape it is for
int slide_status(const MsSlide* sl, const int n_agents) {
    if (!sl || !(sl->bounce >= 0.f && sl->bounce <= 1.f)) return MS_EINVAL;
    return n_agents > WAVE ? MS_EUNSUPPORTED : MS_OK;                    // (a lane an agent)
}

// what ms_rollouts and ms_host_rollouts refuse alike: the limits and the pointers of an MsRollouts
int rollouts_status(const MsRollouts* r) {
    if (!r || r->n_candidates < 1 || r->n_candidates > 256 || r->horizon < 1 || r->horizon > 64 || r->n_actions < 1 ||
        !is_flag(r->others) || !(r->keep == r->keep) || !r->actions || !r->table || !r->positions || !r->angles ||
        !r->velocity || !r->angvelocity || !r->progress || !r->stops || !r->first_stop) return MS_EINVAL;
    return (!is_flag(r->slide) || (r->slide && !(r->bounce >= 0.f && r->bounce <= 1.f))) ? MS_EINVAL : MS_OK;
}

// what ms_scenarios and ms_host_scenarios refuse alike: the limits and the pointers of an MsScenarios, and the agents an env
int scenarios_status(const MsScenarios* q, const int n_agents) {
    if (!q || q->n_scenarios < 1 || q->n_scenarios > 256 || q->horizon < 1 || q->horizon > 64 || q->n_actions < 1 ||
        !is_flag(q->focal) || !is_flag(q->shared) || !(q->keep == q->keep) || !q->actions ||
        (q->focal && !q->base) || !q->table || !q->positions || !q->angles || !q->velocity || !q->angvelocity || !q->progress ||
        !q->stops || !q->first_stop || n_agents < 1) return MS_EINVAL;
    return n_agents > WAVE ? MS_EUNSUPPORTED : MS_OK;                    // (a lane an agent, as ms_slide_physics)
}
}  // namespace

extern "C" {
int ms_debug_physics_pack(int envs) { g_physics_pack = envs; return MS_OK; }
int ms_host_physics_pack(int n_envs, int n_agents, int gridded, int pinned) { return physics_pack_of(n_envs, n_agents, gridded != 0, pinned); }
int ms_debug_render_order(int on) { g_render_order = on ? 1 : 0; return MS_OK; }
int ms_host_order_fans(int n_fans, const int* costs, int* order) {
    // fan_sort_wave, sort wave after sort wave: the classes' first ranks, slowest class first, then every fan its class's next rank
    if (n_fans < 1 || !costs || !order) return -1;
    const int K = fan_sort_per_run(n_fans);
    for (int block = 0; block < 8*K; block++) {
        int first_fan, count, first_slot, next[FAN_CLASSES] = {0};
        fan_sort_part(n_fans, K, block, first_fan, count, first_slot);
        for (int i = 0; i < count; i++) next[fan_class(costs[first_fan + i])]++;
        for (int c = FAN_CLASSES - 1, rank = 0; c >= 0; c--) { const int m = next[c]; next[c] = rank; rank += m; }
        for (int i = 0; i < count; i++) order[first_slot + K*next[fan_class(costs[first_fan + i])]++] = first_fan + i;
    }
    return 8*K;
}

int ms_step_physics(const MsScenery* sc, const MsAgents* ag, const MsMovement* mv, const MsStepExtras* ex, float* progress,
                    const MsConfig* cfg, void* stream) {
    if (!scenery_ok(sc) || !agents_ok(ag) || !progress || !config_ok(cfg)) return MS_EINVAL;
    if (!step_options_ok(mv, ex) || !aligned(ag->schedule, 4) || !near_lists_ok(sc)) return MS_EINVAL;
    const int pack = physics_pack_of(sc->n_envs, sc->n_agents, sc->wg_cells != nullptr, g_physics_pack);
    // per wave: 2 float4 + a float + an unsigned per agent, rounded up to whole float4s
    const size_t slice = ((sizeof(float)*8 + sizeof(float) + sizeof(unsigned))*(size_t)sc->n_agents*pack + 15)/16;
    if (slice*16 > 56*1024) return MS_EUNSUPPORTED;
    MsMovement mvv; MsStepExtras exv;
    step_options_of(mv, ex, mvv, exv);
    MsScenery scn = *sc;
    if (!sc->wg_cells) { scn.wg_geom = sc->lines_vals; scn.wg_starts = sc->lines_starts; }   // (rows the kernel may read: see there)
    const FanSort fs = fan_sort_for(ag, sc, cfg->res);
    // one wavefront per env (several envs per wave, one AFTER the other: 2 -> +25 %, 4 -> +85 % at 4096 envs; side by side: PACK)
    // (the table [no extras][no movement][one env a wave]: named in this order the instantiations keep their places in the code object)
    static void (*const kernels[2][2][2])(MsScenery, AgentsK, float*, float, float, MsMovement, MsStepExtras, int, Divisor, FanSort) = {
        {{physics_kernel<1, 1, 1>, physics_kernel<1, 1, 0>}, {physics_kernel<0, 1, 1>, physics_kernel<0, 1, 0>}},
        {{physics_kernel<1, 0, 1>, physics_kernel<1, 0, 0>}, {physics_kernel<0, 0, 1>, physics_kernel<0, 0, 0>}}};
    hipLaunchKernelGGL(kernels[ex == nullptr][mv == nullptr][pack <= 1], dim3(fs.n_blocks + (sc->n_envs + pack - 1)/pack), dim3(WAVE), slice*16,
                       (hipStream_t)stream, scn, agents_k(*ag), progress, cfg->agent_radius, cfg->fps, mvv, exv, pack,
                       divisor_of((unsigned)sc->n_agents), fs);
    return launch_status();
}

int ms_move_physics(const MsScenery* sc, const MsAgents* ag, const MsMovement* mv, float* progress, const MsConfig* cfg,
                    void* stream) {
    return ms_step_physics(sc, ag, mv, nullptr, progress, cfg, stream);
}

int ms_physics(const MsScenery* sc, const MsAgents* ag, float* progress, const MsConfig* cfg, void* stream) {
    return ms_step_physics(sc, ag, nullptr, nullptr, progress, cfg, stream);
}

void ms_host_move_velocity(float keep, float ang, const float* delta, float* v, float* w) {
    float2 vv = make_float2(v[0], v[1]);
    move_velocity(keep, ang, delta[0], delta[1], delta[2], vv, *w);
    v[0] = vv.x; v[1] = vv.y;
}

int ms_slide_physics(const MsScenery* sc, const MsAgents* ag, const MsMovement* mv, const MsStepExtras* ex, const MsSlide* sl,
                     float* progress, const MsConfig* cfg, void* stream) {
    if (!scenery_ok(sc) || !agents_ok(ag) || !progress || !config_ok(cfg)) return MS_EINVAL;
    if (!step_options_ok(mv, ex) || !aligned(ag->schedule, 4) || !near_lists_ok(sc)) return MS_EINVAL;
    if (!all_aligned<8>(ag->positions, ag->velocity) || !aligned(ag->headings, 16)) return MS_EINVAL;
    if (const int st = slide_status(sl, sc->n_agents)) return st;
    g_last_step_fused = 0;                                               // (a sliding step is never the one-launch step)
    MsMovement mvv; MsStepExtras exv;
    step_options_of(mv, ex, mvv, exv);
    const FanSort fs = fan_sort_for(ag, sc, cfg->res);
    static void (*const kernels[2][2])(MsScenery, AgentsK, float*, float, float, MsMovement, MsStepExtras, MsSlide, Divisor, FanSort) = {
        {physics_slide_kernel<1, 1>, physics_slide_kernel<0, 1>}, {physics_slide_kernel<1, 0>, physics_slide_kernel<0, 0>}};   // [no extras][no movement], as above
    hipLaunchKernelGGL(kernels[ex == nullptr][mv == nullptr], dim3(fs.n_blocks + sc->n_envs), dim3(WAVE), 0, (hipStream_t)stream, *sc,
                       agents_k(*ag), progress, cfg->agent_radius, cfg->fps, mvv, exv, *sl, divisor_of((unsigned)sc->n_agents), fs);
    return launch_status();
}

int ms_host_slide(const float* walls, const long long* wall_starts, int n_envs, int n_agents, const MsAgents* ag, const MsMovement* mv,
                  const MsStepExtras* ex, const MsSlide* sl, float* progress, const MsConfig* cfg) {
    if (!walls || !wall_starts || n_envs < 1 || n_agents < 1 || !agents_ok(ag) || !progress || !config_ok(cfg)) return MS_EINVAL;
    if (!step_options_ok(mv, ex)) return MS_EINVAL;
    if (const int st = slide_status(sl, n_agents)) return st;
    MsMovement mvv; MsStepExtras exv;
    step_options_of(mv, ex, mvv, exv);
    slide_serial(walls, wall_starts, n_envs, n_agents, *ag, mv ? &mvv : nullptr, exv, ex != nullptr, *sl, progress, cfg->agent_radius, cfg->fps);
    return MS_OK;
}

int ms_rollouts(const MsScenery* sc, const MsAgents* ag, const MsRollouts* r, const MsConfig* cfg, void* stream) {
    if (!scenery_ok(sc) || !agents_ok(ag) || !config_ok(cfg) || rollouts_status(r) != MS_OK) return MS_EINVAL;
    if (!all_aligned<8>(r->actions, r->positions, r->velocity, r->trail, ag->positions, ag->velocity) || !aligned(r->slides, 4) ||
        !near_lists_ok(sc)) return MS_EINVAL;
    const int groups = (r->n_candidates + WAVE - 1)/WAVE;
    const long long blocks = (long long)sc->n_envs*sc->n_agents*groups;
    if (blocks > 0x7fffffffLL) return MS_EUNSUPPORTED;
    // Which scheme: a lane a candidate pays a wall's whole exact test however few of its lanes are candidates - measured (DESIGN
    // 3.27; 4096 envs, H = 8) 117.7 us at K = 7 against 51.9 us for a lane a wall, 151.6 against 124.9 at 24, 153.4 against 163.1 at
    // 32, 164.3 against 301.2 at 64: few candidates go candidate by candidate, a wave's worth and more a lane each.
    // (The sliding step is stated for a lane a candidate only: pinning the other scheme with it is refused, not ignored.)
    if (r->slide && g_rollout_scheme == 1) return MS_EINVAL;
    const int scheme = r->slide ? 0 : g_rollout_scheme >= 0 ? g_rollout_scheme : (r->n_candidates <= ROLL_FEW ? 1 : 0);
    const auto kernel = scheme == 1 ? rollout_walls_kernel : r->slide ? rollout_kernel<1> : rollout_kernel<0>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(WAVE), 0, (hipStream_t)stream, *sc, agents_k(*ag), *r, cfg->agent_radius,
                       cfg->fps, groups, divisor_of((unsigned)groups), divisor_of((unsigned)sc->n_agents));
    return launch_status();
}

int ms_debug_rollout_scheme(int scheme) {
    if (scheme < -1 || scheme > 1) return MS_EINVAL;
    g_rollout_scheme = scheme;
    return MS_OK;
}

int ms_host_rollouts(const float* walls, int n_walls, const MsAgents* ag, int n_agents, const MsRollouts* r, const MsConfig* cfg) {
    if (!agents_ok(ag) || !config_ok(cfg) || rollouts_status(r) != MS_OK || n_agents < 1 || n_walls < 0 || (n_walls > 0 && !walls)) return MS_EINVAL;
    rollout_serial(walls, n_walls, *ag, n_agents, *r, cfg->agent_radius, cfg->fps);
    return MS_OK;
}

int ms_scenarios(const MsScenery* sc, const MsAgents* ag, const MsScenarios* q, const MsConfig* cfg, void* stream) {
    if (!scenery_ok(sc) || !agents_ok(ag) || !config_ok(cfg)) return MS_EINVAL;
    if (const int st = scenarios_status(q, sc->n_agents)) return st;
    if (!all_aligned<8>(q->actions, q->base, q->positions, q->velocity, q->trail, ag->positions, ag->velocity) ||
        !all_aligned<4>(q->table, q->angles, q->angvelocity, q->progress, q->stops, q->first_stop) || !near_lists_ok(sc)) return MS_EINVAL;
    const int G = WAVE/sc->n_agents;                                     // whole scenarios a wave
    const int S = scenario_count(*q, sc->n_agents);
    const int groups = (S + G - 1)/G;
    const long long blocks = (long long)sc->n_envs*groups;
    if (blocks > 0x7fffffffLL) return MS_EUNSUPPORTED;
    hipLaunchKernelGGL(scenario_kernel, dim3((unsigned)blocks), dim3(WAVE), 0, (hipStream_t)stream, *sc, agents_k(*ag), *q,
                       cfg->agent_radius, cfg->fps, groups, G, divisor_of((unsigned)groups), divisor_of((unsigned)sc->n_agents));
    return launch_status();
}

int ms_host_scenarios(const float* walls, int n_walls, const MsAgents* ag, int n_agents, const MsScenarios* q, const MsConfig* cfg) {
    if (!agents_ok(ag) || !config_ok(cfg) || n_walls < 0 || (n_walls > 0 && !walls)) return MS_EINVAL;
    if (const int st = scenarios_status(q, n_agents)) return st;
    scenario_serial(walls, n_walls, *ag, n_agents, *q, cfg->agent_radius, cfg->fps);
    return MS_OK;
}
}  // extern "C"
