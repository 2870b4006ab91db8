// kernels/scenario.h -- scenario_kernel: whole envs forked S ways, every agent on its own plan, a lane an agent of a scenario.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, behind rollout.h, whose
// per-step functions it calls); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// scenarios                                                  (MsScenarios; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// A WAVEFRONT HOLDS G = 64 / A WHOLE SCENARIOS, lane g A + a agent a of the wave's scenario g: the agent's state, its least
// progress and its two counts stay in registers for the whole horizon.  Each step a lane moves, forms its task (p, v/fps), shows
// it to the other lanes of its scenario - a float4 a lane in LDS, 1 KiB a wave, behind a wave barrier - meets the A - 1 others
// (a uniform loop of A trips, agents_apart in front of collision_cc, both agents' moved velocities: physics_kernel's ordered-pair
// test), walks the near list of its own cell as rollout_kernel's lanes do, and integrates.  Every collision_* value lies in
// [+0, 1] and the fold is a minimum: the same bits as physics_kernel's atomicMin on the float's bits, in any order.

// the moving-other test: physics_kernel's agent-agent test against (p_b, v_b/fps) as the other's task has them
__host__ __device__ inline float scenario_meet_agent(const float x, const RolloutTask& t, const float4 o, const float agent_radius) {
    if (agents_apart(t.tk, o, agent_radius)) return x;
    const float c = collision_cc(p2(t.tk.x, t.tk.y), p2(t.tk.z, t.tk.w), p2(o.x, o.y), p2(o.z, o.w), agent_radius);
    return c < x ? c : x;
}
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
    const int L = sc.lines_widths[n];
    const float4* __restrict__ ln = reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[n];
    const bool gridded = sc.wg_cells != nullptr;                         // (the same for every wave of the launch)
    float4 geom = make_float4(0.f, 0.f, 0.f, 0.f);
    int wg_start = 0;
    if (gridded) { geom = reinterpret_cast<const float4*>(sc.wg_geom)[n]; wg_start = sc.wg_starts[n]; }
    const int me = n*A + a;
    RolloutState st = rollout_start(reinterpret_cast<const float2*>(ag.positions)[me], ag.angles[me],
                                    reinterpret_cast<const float2*>(ag.velocity)[me], ag.angvelocity[me], H);
    const long long* __restrict__ plan = scenario_plan(q, n, A, s, a);
    const bool small_table = 3*q.n_actions <= WAVE;
    const float tab = q.table[min(lane, 3*q.n_actions - 1)];
    float2* __restrict__ trail = reinterpret_cast<float2*>(q.trail);
    const float4* others = s_task + g*A;                                 // the tasks of this lane's scenario, agent after agent
    auto wave_sync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    long long act = plan[0];
    for (int h = 0; h < H; h++) {
        const long long next = plan[min(h + 1, H - 1)];                  // (asked for a step ahead)
        const int c = rollout_action(act, q.n_actions);
        float dx, dy, dw;
        if (small_table) { dx = __shfl(tab, 3*c, WAVE); dy = __shfl(tab, 3*c + 1, WAVE); dw = __shfl(tab, 3*c + 2, WAVE); }
        else { dx = q.table[3*c]; dy = q.table[3*c + 1]; dw = q.table[3*c + 2]; }
        move_velocity(q.keep, st.ang, dx, dy, dw, st.v, st.w);
        const RolloutTask t = rollout_task(st, agent_radius, fps);
        // the cell's header is asked for before the others are met: nothing of it depends on them
        bool covered = false;
        int count = 0;
        const float4* __restrict__ near = nullptr;
        if (gridded) {
            bool inside;
            const int cell = wg_cell_at(geom, sc.wg_cell, st.p.x, st.p.y, inside);
            const uint4 hdr = reinterpret_cast<const uint4*>(sc.wg_cells)[wg_start + cell];
            covered = inside & (t.reach <= sc.wg_reach);
            count = covered ? near_count(hdr, t.reach, sc.wg_reach_lo) : 0;
            near = reinterpret_cast<const float4*>(sc.wg_near_rows) + hdr.z;
        }
        // (through LDS, one ds_read_b128 a trip; four __shfl a trip instead measured the same within the spread, 0.4-0.8 % slower
        // at 4 and at 16 agents an env: DESIGN 3.32 - the step's time is the lanes' wall walks, not the exchange)
        s_task[lane] = t.tk;
        wave_sync();
        float x = 1.f;
        for (int b = 0; b < A; b++) {                                    // (uniform: every lane meets agent b of its own scenario)
            const float4 o = others[b];
            if (b != a) x = scenario_meet_agent(x, t, o, agent_radius);
        }
        wave_sync();                                                     // (the tasks are read before the next step's are written)
        for (int j0 = 0; __ballot(j0 < count) != 0ull; j0 += ROLL_AHEAD) {
            float4 u[ROLL_AHEAD];
            #pragma unroll
            for (int i = 0; i < ROLL_AHEAD; i++) u[i] = (j0 + i < count) ? near[j0 + i] : make_float4(0.f, 0.f, 0.f, 0.f);
            #pragma unroll
            for (int i = 0; i < ROLL_AHEAD; i++) {
                if (j0 + i < count) x = rollout_meet_wall(x, t, u[i], agent_radius);
            }
        }
        if (__ballot(!covered) != 0ull) {
            // (rare with a grid, and plain: every static row of the env to the lanes no list covers - the rows' addresses are the wave's)
            for (int l = AF; l < L; l++) {
                const float4 u = ln[l];
                if (!covered) x = rollout_meet_wall(x, t, u, agent_radius);
            }
        }
        rollout_advance(st, x, fps, h);
        if (trail && writes) trail[row*H + h] = st.p;
        act = next;
    }
    if (writes) {
        reinterpret_cast<float2*>(q.positions)[row] = st.p;
        q.angles[row] = st.ang;
        reinterpret_cast<float2*>(q.velocity)[row] = st.v;
        q.angvelocity[row] = st.w;
        q.progress[row] = st.least;
        q.stops[row] = st.stops;
        q.first_stop[row] = st.first;
    }
}

// The rule for ONE env, serially (ms_host_scenarios): the same functions in the same order - every agent moves, every agent
// meets every other agent and every wall, every agent advances.  (Plain float accesses: host arrays promise no more than a
// float's alignment.)
inline void scenario_serial(const float* walls, const int n_walls, const MsAgents& ag, const int A, const MsScenarios& q,
                            const float agent_radius, const float fps) {
    const int S = scenario_count(q, A), H = q.horizon;
    RolloutState st[WAVE];
    RolloutTask task[WAVE];
    float xs[WAVE];
    for (int s = 0; s < S; s++) {
        bool any = false;
        size_t row;
        for (int a = 0; a < A; a++) any |= scenario_row(q, 0, A, s, a, row);
        if (!any) continue;
        for (int a = 0; a < A; a++)
            st[a] = rollout_start(make_float2(ag.positions[2*a], ag.positions[2*a + 1]), ag.angles[a],
                                  make_float2(ag.velocity[2*a], ag.velocity[2*a + 1]), ag.angvelocity[a], H);
        for (int h = 0; h < H; h++) {
            for (int a = 0; a < A; a++) {
                const int c = rollout_action(scenario_plan(q, 0, A, s, a)[h], q.n_actions);
                move_velocity(q.keep, st[a].ang, q.table[3*c], q.table[3*c + 1], q.table[3*c + 2], st[a].v, st[a].w);
                task[a] = rollout_task(st[a], agent_radius, fps);
            }
            for (int a = 0; a < A; a++) {
                float x = 1.f;
                for (int b = 0; b < A; b++) {
                    if (b != a) x = scenario_meet_agent(x, task[a], task[b].tk, agent_radius);
                }
                for (int l = 0; l < n_walls; l++)
                    x = rollout_meet_wall(x, task[a], make_float4(walls[4*l], walls[4*l + 1], walls[4*l + 2], walls[4*l + 3]), agent_radius);
                xs[a] = x;
            }
            for (int a = 0; a < A; a++) {
                rollout_advance(st[a], xs[a], fps, h);
                if (q.trail && scenario_row(q, 0, A, s, a, row)) {
                    q.trail[2*(row*H + h)] = st[a].p.x; q.trail[2*(row*H + h) + 1] = st[a].p.y;
                }
            }
        }
        for (int a = 0; a < A; a++) {
            if (!scenario_row(q, 0, A, s, a, row)) continue;
            q.positions[2*row] = st[a].p.x; q.positions[2*row + 1] = st[a].p.y;
            q.angles[row] = st[a].ang;
            q.velocity[2*row] = st[a].v.x; q.velocity[2*row + 1] = st[a].v.y;
            q.angvelocity[row] = st[a].w;
            q.progress[row] = st[a].least;
            q.stops[row] = st[a].stops;
            q.first_stop[row] = st[a].first;
        }
    }
}
