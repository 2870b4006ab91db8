// host/walker.h -- walkers: ms_walkers (kernels/walker.h) and its host instantiation.  One check serves the launch and the host
// instantiation.
namespace {
// The limits keep an env's bodies and counts within a workgroup's LDS and a lane's slots within four.
int walkers_check(const MsWalkers* w, const int n_agents, const float* agent_positions) {
    if (!w || !agent_positions || n_agents < 1 || n_agents > WALK_MAX_AGENTS || w->n_slots < 1 || w->n_slots > WALK_MAX_SLOTS ||
        !w->positions || !w->velocities || !w->speeds || !w->towards || !positive_finite(w->personal) ||
        !(w->push >= 0.f && w->push < INFINITY) || !(w->keep >= 0.f && w->keep < 1.f) || !is_flag(w->agents_push) ||
        !positive_finite(w->fps) || !positive_finite(w->agent_radius) ||
        !all_aligned<8>(agent_positions, w->positions, w->velocities, w->towards) ||
        !all_aligned<4>(w->speeds, w->progress, w->bumps, w->close)) return MS_EINVAL;
    // the second contact phase: its fields are read only with it (MsSlide's range for bounce)
    if (!is_flag(w->slide) || (w->slide && (!(w->bounce >= 0.f && w->bounce <= 1.f) || !all_aligned<4>(w->slid)))) return MS_EINVAL;
    return MS_OK;
}
WalkArgs walkers_args(const MsWalkers* w, const int n_envs, const int n_agents, const float* agent_positions) {
    return WalkArgs{w->positions, w->velocities, w->speeds, w->towards, w->reset, agent_positions, w->progress, w->blocked, w->bumps,
                    w->close, n_envs, n_agents, w->n_slots, w->agents_push, w->personal, w->push, w->keep, w->fps, w->agent_radius,
                    w->slide, w->slide ? w->bounce : 0.f, w->slide ? w->slid : nullptr, w->slide ? w->stopped : nullptr};
}
}  // namespace

extern "C" {
int ms_walkers(const MsScenery* sc, const MsAgents* ag, const MsWalkers* w, void* stream) {
    if (!scenery_ok(sc) || !ag) return MS_EINVAL;
    if (const int status = walkers_check(w, sc->n_agents, ag->positions)) return status;
    const WalkArgs q = walkers_args(w, sc->n_envs, sc->n_agents, ag->positions);
    // a wavefront an env while a lane a walker covers the store; a workgroup an env beyond - the plain tick's kernel or the sliding one's
    const bool wide = w->n_slots > WAVE;
    const dim3 blocks(wide ? (unsigned)sc->n_envs : (unsigned)((sc->n_envs + WAVES - 1)/WAVES));
    const auto kernel = w->slide ? (wide ? walker_slide_kernel<true> : walker_slide_kernel<false>) : (wide ? walker_kernel<true> : walker_kernel<false>);
    hipLaunchKernelGGL(kernel, blocks, dim3(WG), 0, (hipStream_t)stream, *sc, q);
    return launch_status();
}

int ms_host_walkers(const MsWalkers* w, int n_envs, int n_agents, const float* agent_positions, const float* walls, const long long* wall_starts) {
    if (const int status = walkers_check(w, n_agents, agent_positions)) return status;
    if (n_envs < 1 || !walls || !wall_starts || !aligned(walls, 16)) return MS_EINVAL;
    walkers_serial(walkers_args(w, n_envs, n_agents, agent_positions), reinterpret_cast<const float4*>(walls), wall_starts);
    return MS_OK;
}
}  // extern "C"
