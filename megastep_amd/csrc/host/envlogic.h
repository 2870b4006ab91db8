// host/envlogic.h -- the demo envs' logic between frames: ms_deathmatch_shoot and ms_explorer_books (kernels/envlogic.h:
// deathmatch_kernel, explorer_kernel), an element-wise launch each.
extern "C" {
int ms_deathmatch_shoot(int n_envs, int n_agents, const MsDeathmatch* dm, void* stream) {
    if (n_envs <= 0 || n_agents <= 0 || !dm || !dm->centre || !dm->positions || !dm->upper || !dm->health || !dm->damage || !dm->dead ||
        !all_aligned<8>(dm->centre, dm->positions, dm->upper) ||
        !(dm->clearance == dm->clearance) || !(dm->hit_damage == dm->hit_damage) || !(dm->tick_damage == dm->tick_damage)) return MS_EINVAL;
    const long long rows = (long long)n_envs*n_agents, blocks = (rows + WG - 1)/WG;
    if (blocks > 0x7fffffffLL) return MS_EUNSUPPORTED;
    hipLaunchKernelGGL(deathmatch_kernel, dim3((unsigned)blocks), dim3(WG), 0, (hipStream_t)stream, *dm, n_envs, n_agents);
    return launch_status();
}

int ms_explorer_books(int n_envs, const MsExplorer* ex, void* stream) {
    if (n_envs <= 0 || !ex || !ex->tally || !ex->before || !ex->lengths || !ex->epoch || !ex->over || !ex->reward || ex->pixels <= 0 ||
        !all_aligned<4>(ex->tally, ex->before, ex->lengths, ex->epoch)) return MS_EINVAL;
    hipLaunchKernelGGL(explorer_kernel, dim3((unsigned)((n_envs + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, *ex, n_envs);
    return launch_status();
}
}  // extern "C"
