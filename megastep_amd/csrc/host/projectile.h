// host/projectile.h -- projectiles: ms_projectiles (kernels/projectile.h) and its host instantiation.  One check serves the launch
// and the host instantiation.
namespace {
// The limits keep a workgroup's bodies, shots and records within its LDS and a lane's slots within four.
int projectiles_check(const MsProjectiles* p, const int n_agents, const int n_model, const float* agent_positions, const float* agent_angles) {
    if (!p || !agent_positions || !agent_angles || n_agents < 1 || n_agents > PROJ_MAX_AGENTS || n_model < 1 || p->per_agent < 1 ||
        p->per_agent > PROJ_MAX_PER_AGENT || p->n_slots < 1 || p->n_slots > PROJ_MAX_SLOTS || p->n_slots != n_agents*p->per_agent ||
        !p->positions || !p->velocities || !p->owners || !p->timers || !p->bounces || !positive_finite(p->speed) ||
        !positive_finite(p->muzzle) || !positive_finite(p->fps) || !(p->restitution >= 0.f && p->restitution <= 1.f) || p->life < 1 ||
        p->n_bounces < 0 || !all_aligned<8>(agent_positions, p->positions, p->velocities) ||
        !all_aligned<4>(agent_angles, p->owners, p->timers, p->bounces, p->struck, p->hits, p->scored)) return MS_EINVAL;
    return n_agents*n_model > PROJ_MAX_BODY_ROWS ? MS_EUNSUPPORTED : MS_OK;
}
ProjArgs projectiles_args(const MsProjectiles* p, const int n_envs, const int n_agents, const int n_model, const float* agent_positions,
                          const float* agent_angles) {
    return ProjArgs{p->positions, p->velocities, p->owners, p->timers, p->bounces, p->fire, p->reset, agent_positions, agent_angles,
                    p->struck, p->ended, p->hits, p->scored, p->misfires, n_envs, n_agents, n_model, p->per_agent, p->n_slots, p->life,
                    p->n_bounces, p->speed, p->muzzle, p->restitution, p->fps};
}
}  // namespace

extern "C" {
int ms_projectiles(const MsScenery* sc, const MsAgents* ag, const MsProjectiles* p, void* stream) {
    if (!scenery_ok(sc) || !ag) return MS_EINVAL;
    if (const int status = projectiles_check(p, sc->n_agents, sc->n_model, ag->positions, ag->angles)) return status;
    hipLaunchKernelGGL(projectile_kernel, dim3((unsigned)sc->n_envs), dim3(WG), 0, (hipStream_t)stream, *sc,
                       projectiles_args(p, sc->n_envs, sc->n_agents, sc->n_model, ag->positions, ag->angles));
    return launch_status();
}

int ms_host_projectiles(const MsProjectiles* p, int n_envs, int n_agents, const float* agent_positions, const float* agent_angles,
                        const float* model, int n_model, const float* walls, const long long* wall_starts) {
    if (const int status = projectiles_check(p, n_agents, n_model, agent_positions, agent_angles)) return status;
    if (n_envs < 1 || !model || !walls || !wall_starts || !all_aligned<16>(model, walls)) return MS_EINVAL;
    projectiles_serial(projectiles_args(p, n_envs, n_agents, n_model, agent_positions, agent_angles), reinterpret_cast<const float4*>(model),
                       reinterpret_cast<const float4*>(walls), wall_starts);
    return MS_OK;
}
}  // extern "C"
