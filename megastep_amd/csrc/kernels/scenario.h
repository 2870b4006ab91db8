// kernels/scenario.h -- scenario_kernel: whole envs forked S ways, every agent on its own plan, a lane an agent of a scenario.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, behind step.h, whose rules,
// pieces and rolled-step functions it calls); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// scenarios                                                  (MsScenarios; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// A WAVEFRONT HOLDS G = 64 / A WHOLE SCENARIOS, lane g A + a agent a of the wave's scenario g: the agent's state, its least
// progress and its two counts stay in registers for the whole horizon.  Each step a lane moves, forms its task (p, v/fps), shows
// it to the other lanes of its scenario - a float4 a lane in LDS, 1 KiB a wave, behind a wave barrier - meets the A - 1 others
// (a uniform loop of A trips, meet_agent with both agents' moved velocities: physics_kernel's ordered-pair test), walks the near list of its own cell as rollout_kernel's lanes do, and integrates.  Every collision_* value lies in
// [+0, 1] and the fold is a minimum: the same bits as physics_kernel's atomicMin on the float's bits, in any order.

// the scenarios an env is forked into: S, or in focal mode A K - scenario f K + k puts agent f on its plan k
__host__ __device__ inline int scenario_count(const MsScenarios& q, const int A) { return q.focal ? A*q.n_scenarios : q.n_scenarios; }
// where agent a of env n reads its H actions in scenario s (the host statement's one env is n = 0)
__host__ __device__ inline const long long* scenario_plan(const MsScenarios& q, const int n, const int A, const int s, const int a) {
    const size_t H = (size_t)q.horizon, S = (size_t)q.n_scenarios;
    if (!q.focal) return q.actions + (((q.shared ? (size_t)0 : (size_t)n*S) + (size_t)s)*A + a)*H;
    const int f = s/q.n_scenarios, k = s - f*q.n_scenarios;
    if (a == f) return q.actions + ((q.shared ? (size_t)0 : ((size_t)n*A + f)*S) + (size_t)k)*H;
    return q.base + ((size_t)n*A + a)*H;
}
// the row of the outputs agent a of scenario s writes, and whether it writes one: every agent of a joint scenario of an env the
// mask (N,) marks; the focal agent alone, where the mask (N, A) marks it
__host__ __device__ inline bool scenario_row(const MsScenarios& q, const int n, const int A, const int s, const int a, size_t& row) {
    if (!q.focal) {
        row = ((size_t)n*q.n_scenarios + s)*A + a;
        return !q.mask || q.mask[n];
    }
    const int f = s/q.n_scenarios, k = s - f*q.n_scenarios;
    row = ((size_t)n*A + f)*q.n_scenarios + k;
    return a == f && (!q.mask || q.mask[(size_t)n*A + f]);
}

// block = n*groups + group; the wave's scenarios are group*G .. group*G + G - 1, G = 64 / A (by_g divides by groups, by_a by A)
__global__ __launch_bounds__(WAVE) void scenario_kernel(
        const MsScenery sc, const AgentsK ag, const MsScenarios q, const float agent_radius, const float fps, const int groups,
        const int G, const Divisor by_g, const Divisor by_a) {
    __shared__ float4 s_task[WAVE];              // per lane: (p, v/fps) of its agent, this step
    const int lane = threadIdx.x;
    const int n = div_by((int)blockIdx.x, by_g), group = (int)blockIdx.x - n*groups;
    const int A = sc.n_agents, AF = sc.n_agents*sc.n_model;
    const int S = scenario_count(q, A), H = q.horizon;
    // (the lanes past G A, and those of scenarios past the last, roll a live lane's agent again and store nothing: the table
    // rides in the lanes, which must all be there)
    const int ll = min(lane, G*A - 1);
    const int g = div_by(ll, by_a), a = ll - g*A;
    const int s = min(group*G + g, S - 1);
    size_t row;
    const bool writes = scenario_row(q, n, A, s, a, row) && lane < G*A && group*G + g < S;
    if (__ballot(writes) == 0ull) return;                                // (uniform: nothing of this wave is asked for)
    const EnvRows env = env_rows(sc, n);                                 // (gridded: the same for every wave of the launch)
    RolloutState st = rollout_start(ag, (size_t)(n*A + a), H);
    const long long* __restrict__ plan = scenario_plan(q, n, A, s, a);
    const ActionTable table(q.table, q.n_actions, lane);
    float2* __restrict__ trail = reinterpret_cast<float2*>(q.trail);
    const float4* others = s_task + g*A;                                 // the tasks of this lane's scenario, agent after agent
    long long act = plan[0];
    for (int h = 0; h < H; h++) {
        const long long next = plan[min(h + 1, H - 1)];                  // (asked for a step ahead)
        float dx, dy, dw;
        table.delta(action_row(act, q.n_actions), dx, dy, dw);
        move_velocity(q.keep, st.ang, dx, dy, dw, st.v, st.w);
        const StepTask t = rollout_task(st, agent_radius, fps);
        // the cell's header is asked for before the others are met: nothing of it depends on them
        const NearList nl = near_list(sc, env, st.p, t.reach);
        // (through LDS, one ds_read_b128 a trip; four __shfl a trip instead measured the same within the spread, 0.4-0.8 % slower
        // at 4 and at 16 agents an env: DESIGN 3.32 - the step's time is the lanes' wall walks, not the exchange)
        s_task[lane] = t.tk;
        wave_sync();
        float x = 1.f;
        for (int b = 0; b < A; b++) {                                    // (uniform: every lane meets agent b of its own scenario)
            const float4 o = others[b];
            if (b != a) x = meet_agent(x, t, o, agent_radius);
        }
        wave_sync();                                                     // (the tasks are read before the next step's are written)
        walk_rows(nl, env, AF, [&](const float4 u) { x = meet_wall(x, t, u, agent_radius); });
        rollout_advance(st, x, fps, h);
        if (trail && writes) trail[row*H + h] = st.p;
        act = next;
    }
    if (writes) rollout_store(q, row, st);
}

// The rule for ONE env, serially (ms_host_scenarios): the same functions in the same order - every agent moves, every agent
// meets every other agent and every wall, every agent advances.  (Plain float accesses: host arrays promise no more than a
// float's alignment.)
inline void scenario_serial(const float* walls, const int n_walls, const MsAgents& ag, const int A, const MsScenarios& q,
                            const float agent_radius, const float fps) {
    const int S = scenario_count(q, A), H = q.horizon;
    RolloutState st[WAVE];
    StepTask task[WAVE];
    float xs[WAVE];
    for (int s = 0; s < S; s++) {
        bool any = false;
        size_t row;
        for (int a = 0; a < A; a++) any |= scenario_row(q, 0, A, s, a, row);
        if (!any) continue;
        for (int a = 0; a < A; a++) st[a] = rollout_start(ag, a, H);
        for (int h = 0; h < H; h++) {
            for (int a = 0; a < A; a++) {
                const int c = action_row(scenario_plan(q, 0, A, s, a)[h], q.n_actions);
                move_velocity(q.keep, st[a].ang, q.table[3*c], q.table[3*c + 1], q.table[3*c + 2], st[a].v, st[a].w);
                task[a] = rollout_task(st[a], agent_radius, fps);
            }
            for (int a = 0; a < A; a++) {
                float x = 1.f;
                for (int b = 0; b < A; b++) {
                    if (b != a) x = meet_agent(x, task[a], task[b].tk, agent_radius);
                }
                for (int l = 0; l < n_walls; l++)
                    x = meet_wall(x, task[a], make_float4(walls[4*l], walls[4*l + 1], walls[4*l + 2], walls[4*l + 3]), agent_radius);
                xs[a] = x;
            }
            for (int a = 0; a < A; a++) {
                rollout_advance(st[a], xs[a], fps, h);
                if (q.trail && scenario_row(q, 0, A, s, a, row)) store2(q.trail, row*H + h, st[a].p);
            }
        }
        for (int a = 0; a < A; a++) {
            if (scenario_row(q, 0, A, s, a, row)) rollout_store(q, row, st[a]);
        }
    }
}
