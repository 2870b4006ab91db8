// kernels/rollout.h -- rollout_kernel: candidate action plans rolled through the agent step, a lane a plan.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, behind step.h, whose rules and
// pieces it calls, and slide.h, whose rule it chains); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// rollouts                                                   (MsRollouts; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// ONE WAVEFRONT PER (AGENT, 64 CANDIDATES), a lane a candidate: the state (p, ang, v, w), the least progress and the two counts
// stay in registers for the whole horizon; no LDS, no atomics.  Each step a lane moves (move_velocity), finds the cell of the wall
// grid it stands in and walks that cell's near list - meet_wall, as every step kernel - the wave
// looping to the largest count among its lanes, four rows in flight; then integrates.  In the first steps every lane of a wave
// stands in the same cell and the loads are the same address.  A lane the lists do not cover - outside the grid, a reach beyond
// wg_reach (too fast, or crawling: wall_reach's k), a NaN pose - walks its env's static rows instead while the covered lanes
// wait, and a scenery without a wall grid does so for every lane.  Every collision_* value lies in [+0, 1] and the fold is a
// minimum: the same bits as physics_kernel's atomicMin on the float's bits, in any order.
//
// The step as values, shared with ms_host_rollouts (the serial host statement): what differs between the two is only where a
// candidate's walls come from.  RolloutState, rollout_start, rollout_task, rollout_advance and rollout_store: kernels/step.h.

// Under MsRollouts.slide a step is the sliding step (kernels/slide.h), the others at rest in both phases.
// the sliding step's end and the rollout's books for step h: a stop is a step whose velocity was zeroed
__host__ __device__ inline void rollout_advance_slide(RolloutState& st, int& slides, const SlideContact& c, const float x1, const float x2,
                                                      const float fps, const int h) {
    float slid;
    const bool stopped = slide_finish(c, x2, fps, st.p, st.ang, st.v, st.w, slid);
    st.least = x1 < st.least ? x1 : st.least;
    if (stopped) { st.stops++; st.first = h < st.first ? h : st.first; }
    else if (c.slides) slides++;
}
// another agent of the env, at rest at pb, as a task's (p, u)
__host__ __device__ inline float4 at_rest(const float2 pb) { return make_float4(pb.x, pb.y, 0.f, 0.f); }

// r.n_candidates candidates in groups of 64: block = (n A + a)*groups + group (by_g divides by groups, by_a by n_agents)
// SLIDE = 1: the sliding step - a lane's obstacles are met by one walk, called for phase A, then (only in a wave with a blocked
// candidate, and for those) for the contact, then (only with one that slides) for phase B from the cell the candidate stands in then
template <int SLIDE>
__global__ __launch_bounds__(WAVE) void rollout_kernel(
        const MsScenery sc, const AgentsK ag, const MsRollouts r, const float agent_radius, const float fps, const int groups,
        const Divisor by_g, const Divisor by_a) {
    const int lane = threadIdx.x;
    const RolloutLane b = rollout_bind(r, sc.n_agents, blockIdx.x, lane, groups, by_g, by_a);
    if (r.mask && !r.mask[b.row]) return;                                // (uniform: the agent is not rolled, its rows stay)
    const int A = sc.n_agents, AF = sc.n_agents*sc.n_model, H = r.horizon;
    const EnvRows env = env_rows(sc, b.n);                               // (gridded: the same for every wave of the launch)
    const float2* __restrict__ pos2 = reinterpret_cast<const float2*>(ag.positions);
    RolloutState st = rollout_start(ag, b.row, H);
    const ActionTable table(r.table, r.n_actions, lane);
    float2* __restrict__ trail = reinterpret_cast<float2*>(r.trail);
    [[maybe_unused]] int slides = 0;
    long long act = b.plan[0];
    for (int h = 0; h < H; h++) {
        const long long next = b.plan[min(h + 1, H - 1)];                // (asked for a step ahead)
        float dx, dy, dw;
        table.delta(action_row(act, r.n_actions), dx, dy, dw);
        move_velocity(r.keep, st.ang, dx, dy, dw, st.v, st.w);
        const StepTask t = rollout_task(st, agent_radius, fps);
        // a candidate's obstacles - the others at rest, then the near list of the cell `at` lies in, or the env's static rows -
        // met for `mode` (0: the fold of the least value; 1, SLIDE: the contact's offers) by the lanes that are `on`
        SlideBest best{0.f, 0.f, 0.f, 0};
        float2 p1 = st.p;
        float x1 = 1.f;
        auto walk = [&](const StepTask& t, const float2 at, const bool on, const int mode) -> float {
            float x = 1.f, nx, ny;
            if (r.others && on) {
                for (int o = 0; o < A; o++) {
                    if (o == b.a) continue;
                    if (SLIDE == 0 || mode != 1) x = meet_agent(x, t, at_rest(pos2[b.n*A + o]), agent_radius);
                    else if (offer_agent(t, at_rest(pos2[b.n*A + o]), x1, p1, agent_radius, nx, ny)) slide_offer(best, st.v, nx, ny);
                }
            }
            NearList nl = near_list(sc, env, at, t.reach);
            if (!on) nl = NearList{true, 0, 0u, nullptr};                        // (the lanes that are off wait)
            walk_rows(nl, env, AF, [&](const float4 u) {
                if (SLIDE == 0 || mode != 1) x = meet_wall(x, t, u, agent_radius);
                else if (offer_wall(t, u, x1, p1, agent_radius, nx, ny)) slide_offer(best, st.v, nx, ny);
            });
            return x;
        };
        if constexpr (SLIDE == 0) {
            rollout_advance(st, walk(t, st.p, true, 0), fps, h);
        } else {
            x1 = walk(t, st.p, true, 0);
            const bool blocked = x1 < 1;
            p1 = make_float2(st.p.x + x1*st.v.x/fps, st.p.y + x1*st.v.y/fps);
            if (__ballot(blocked) != 0ull) walk(t, st.p, blocked, 1);
            const SlideContact con = slide_contact(st.p, st.ang, st.v, st.w, x1, fps, best, r.bounce);
            float x2 = 1.f;
            if (__ballot(con.slides) != 0ull) x2 = walk(step_task(con.p1, p2(con.u2.x, con.u2.y), agent_radius), con.p1, con.slides, 2);
            rollout_advance_slide(st, slides, con, x1, x2, fps, h);
        }
        if (trail && b.live) trail[b.cand*H + h] = st.p;
        act = next;
    }
    if (b.live) {
        rollout_store(r, b.cand, st);
        if constexpr (SLIDE == 1) { if (r.slides) r.slides[b.cand] = slides; }
    }
}

// The other scheme (the library's for few candidates, ROLL_FEW; ms_debug_rollout_scheme pins either; the same bits): physics_kernel's own - a lane a WALL, the wave's candidates one after
// another.  The state still lives in the lanes (a lane a candidate: the movement, the other agents and the integration are as
// above), but a step's walls are met candidate by candidate: the lanes take the rows of that candidate's near list (or, where no
// list covers it, of its env) one each, cull them by wall_beyond against the candidate's task in LDS, and the surviving (row,
// candidate) pairs are laid end to end in an LDS list, so that the ten divides and five square roots of the exact test run over
// full lanes; the results are folded with atomicMin on the float's bits, as physics_kernel folds them.
constexpr int ROLL_FEW = 24;           // up to this many candidates an agent ms_rollouts takes this scheme (megastep_hip.hip: measured)
constexpr int ROLL_PAIRS = 4*WAVE;     // capacity of a wave's (row, candidate) pair list: a flush's worth and three chunks' worth

__global__ __launch_bounds__(WAVE) void rollout_walls_kernel(
        const MsScenery sc, const AgentsK ag, const MsRollouts r, const float agent_radius, const float fps, const int groups,
        const Divisor by_g, const Divisor by_a) {
    __shared__ float4 s_task[WAVE];              // per candidate: (p, v/fps) ...
    __shared__ float s_reach2[WAVE];             // ... its squared reach ...
    __shared__ unsigned s_prog[WAVE];            // ... and its progress, as bits
    __shared__ float4 s_wall[ROLL_PAIRS];        // rows near ...
    __shared__ int s_tag[ROLL_PAIRS];            // ... this candidate
    const int lane = threadIdx.x;
    const RolloutLane b = rollout_bind(r, sc.n_agents, blockIdx.x, lane, groups, by_g, by_a);
    if (r.mask && !r.mask[b.row]) return;
    const int A = sc.n_agents, AF = sc.n_agents*sc.n_model, H = r.horizon;
    const int n_live = min(WAVE, r.n_candidates - (b.k - lane));         // the wave's candidates: lanes 0 .. n_live - 1
    const EnvRows env = env_rows(sc, b.n);
    const float2* __restrict__ pos2 = reinterpret_cast<const float2*>(ag.positions);
    RolloutState st = rollout_start(ag, b.row, H);
    const ActionTable table(r.table, r.n_actions, lane);
    float2* __restrict__ trail = reinterpret_cast<float2*>(r.trail);
    PairList pairs{s_wall, s_tag, ROLL_PAIRS, 0};
    auto flush = [&]() {
        pairs.drain(lane, [&](const bool has, const float4 u, const int c) {
            // (a reach of +inf: the pairs were culled before they were appended, and nothing is beyond it - no second cull)
            if (has) fold_least(&s_prog[c], meet_wall(1.f, StepTask{s_task[c], INFINITY, INFINITY}, u, agent_radius));
        });
    };
    long long act = b.plan[0];
    for (int h = 0; h < H; h++) {
        const long long next = b.plan[min(h + 1, H - 1)];
        float dx, dy, dw;
        table.delta(action_row(act, r.n_actions), dx, dy, dw);
        move_velocity(r.keep, st.ang, dx, dy, dw, st.v, st.w);
        const StepTask t = rollout_task(st, agent_radius, fps);
        float x = 1.f;
        if (r.others) {
            for (int o = 0; o < A; o++) {
                if (o != b.a) x = meet_agent(x, t, at_rest(pos2[b.n*A + o]), agent_radius);
            }
        }
        const NearList nl = near_list(sc, env, st.p, t.reach);
        const int covered = nl.covered ? 1 : 0, first = (int)nl.first;
        s_task[lane] = t.tk;
        s_reach2[lane] = t.reach2;
        s_prog[lane] = f_bits(x);
        wave_sync();
        for (int c = 0; c < n_live; c++) {                               // (uniform: candidate after candidate)
            // candidate c's rows - its near list's, or its env's - one a lane: the cull, then the survivors appended as (row, c) pairs
            const bool listed = __builtin_amdgcn_readlane(covered, c);
            const float4* __restrict__ rows = listed ? reinterpret_cast<const float4*>(sc.wg_near_rows) + (unsigned)__builtin_amdgcn_readlane(first, c)
                                                     : env.ln + AF;
            const int n_rows = listed ? __builtin_amdgcn_readlane(nl.count, c) : env.L - AF;
            for (int j0 = 0; j0 < n_rows; j0 += WAVE) {
                const bool has = j0 + lane < n_rows;
                const float4 u = has ? rows[j0 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
                pairs.append(lane, has && !wall_beyond(s_task[c], u, s_reach2[c]), u, c, flush);
            }
        }
        if (pairs.cnt) flush();
        wave_sync();
        x = bits_f(s_prog[lane]);
        rollout_advance(st, x, fps, h);
        if (trail && b.live) trail[b.cand*H + h] = st.p;
        act = next;
    }
    if (b.live) rollout_store(r, b.cand, st);
}

// The rule for ONE env, serially (ms_host_rollouts): the same functions in the same order; every candidate meets every wall.
// (Plain float accesses: host arrays promise no more than a float's alignment.)
inline void rollout_serial(const float* walls, const int n_walls, const MsAgents& ag, const int A, const MsRollouts& r,
                           const float agent_radius, const float fps) {
    const int K = r.n_candidates, H = r.horizon;
    const auto row_of = [&](const int l) { return make_float4(walls[4*l], walls[4*l + 1], walls[4*l + 2], walls[4*l + 3]); };
    for (int a = 0; a < A; a++) {
        if (r.mask && !r.mask[a]) continue;
        // the fold of the least value over a task's obstacles: the others at rest, then every wall
        const auto least = [&](const StepTask& t) {
            float x = 1.f;
            for (int b = 0; r.others && b < A; b++) {
                if (b != a) x = meet_agent(x, t, at_rest(load2(ag.positions, b)), agent_radius);
            }
            for (int l = 0; l < n_walls; l++) x = meet_wall(x, t, row_of(l), agent_radius);
            return x;
        };
        for (int k = 0; k < K; k++) {
            RolloutState st = rollout_start(ag, a, H);
            const long long* plan = r.actions + ((r.shared_plans ? (size_t)0 : (size_t)a*K) + k)*H;
            const size_t cand = (size_t)a*K + k;
            int slides = 0;
            for (int h = 0; h < H; h++) {
                const int c = action_row(plan[h], r.n_actions);
                move_velocity(r.keep, st.ang, r.table[3*c], r.table[3*c + 1], r.table[3*c + 2], st.v, st.w);
                const StepTask t = rollout_task(st, agent_radius, fps);
                const float x = least(t);
                if (!r.slide) rollout_advance(st, x, fps, h);
                else {
                    SlideBest best{0.f, 0.f, 0.f, 0};
                    SlideContact con = slide_contact(st.p, st.ang, st.v, st.w, x, fps, best, r.bounce);
                    if (con.blocked) {
                        float nx, ny;
                        for (int b = 0; r.others && b < A; b++) {
                            if (b != a && offer_agent(t, at_rest(load2(ag.positions, b)), x, con.p1, agent_radius, nx, ny)) slide_offer(best, st.v, nx, ny);
                        }
                        for (int l = 0; l < n_walls; l++) {
                            if (offer_wall(t, row_of(l), x, con.p1, agent_radius, nx, ny)) slide_offer(best, st.v, nx, ny);
                        }
                        con = slide_contact(st.p, st.ang, st.v, st.w, x, fps, best, r.bounce);
                    }
                    const float x2 = con.slides ? least(step_task(con.p1, p2(con.u2.x, con.u2.y), agent_radius)) : 1.f;
                    rollout_advance_slide(st, slides, con, x, x2, fps, h);
                }
                if (r.trail) store2(r.trail, cand*H + h, st.p);
            }
            rollout_store(r, cand, st);
            if (r.slide && r.slides) r.slides[cand] = slides;
        }
    }
}
