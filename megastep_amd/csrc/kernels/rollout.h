// kernels/rollout.h -- rollout_kernel: candidate action plans rolled through the agent step, a lane a plan.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, behind math.h and physics.h,
// whose per-agent rules it chains); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// rollouts                                                   (MsRollouts; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// ONE WAVEFRONT PER (AGENT, 64 CANDIDATES), a lane a candidate: the state (p, ang, v, w), the least progress and the two counts
// stay in registers for the whole horizon; no LDS, no atomics.  Each step a lane moves (move_velocity), finds the cell of the wall
// grid it stands in and walks that cell's near list - wall_beyond in front of collision_cs, as physics_kernel's meet() - the wave
// looping to the largest count among its lanes, four rows in flight; then integrates.  In the first steps every lane of a wave
// stands in the same cell and the loads are the same address.  A lane the lists do not cover - outside the grid, a reach beyond
// wg_reach (too fast, or crawling: wall_reach's k), a NaN pose - walks its env's static rows instead while the covered lanes
// wait, and a scenery without a wall grid does so for every lane.  Every collision_* value lies in [+0, 1] and the fold is a
// minimum: the same bits as physics_kernel's atomicMin on the float's bits, in any order.
//
// The step as values, shared with ms_host_rollouts (the serial host statement): what differs between the two is only where a
// candidate's walls come from.
struct RolloutState { float2 p, v; float ang, w, least; int stops, first; };
// what a step's tests need of the moved state: (p, v/fps), the reach (NaN: +inf - every tier and the grid refuse it) and its square
struct RolloutTask { float4 tk; float reach, reach2; };

__host__ __device__ inline RolloutState rollout_start(const float2 p, const float ang, const float2 v, const float w, const int horizon) {
    return RolloutState{p, v, ang, w, 1.f, 0, horizon};
}
// the row of the table an action means: clamped, as physics_kernel's prologue clamps it
__host__ __device__ inline int rollout_action(const long long act, const int n_actions) {
    return (int)(act < 0 ? 0 : act > (long long)n_actions - 1 ? (long long)n_actions - 1 : act);
}
__host__ __device__ inline RolloutTask rollout_task(const RolloutState& st, const float agent_radius, const float fps) {
    const P2 p0 = p2(st.p.x, st.p.y);
    const P2 v0 = p2(st.v.x, st.v.y)/fps;
    const float reach = wall_reach(p0, v0, agent_radius);
    return RolloutTask{make_float4(p0.x, p0.y, v0.x, v0.y), (reach == reach) ? reach : INFINITY, reach_squared(reach)};
}
// one static row u = (ax, ay, bx, by): physics_kernel's meet()
__host__ __device__ inline float rollout_meet_wall(const float x, const RolloutTask& t, const float4 u, const float agent_radius) {
    if (wall_beyond(t.tk, u, t.reach2)) return x;
    const float c = collision_cs(p2(t.tk.x, t.tk.y), p2(t.tk.z, t.tk.w), p2(u.x, u.y), p2(u.z, u.w), agent_radius);
    return c < x ? c : x;
}
// another agent of the env, at rest at pb: physics_kernel's agent-agent test against (pb, (0, 0))
__host__ __device__ inline float rollout_meet_agent(const float x, const RolloutTask& t, const float2 pb, const float agent_radius) {
    const float4 o = make_float4(pb.x, pb.y, 0.f, 0.f);
    if (agents_apart(t.tk, o, agent_radius)) return x;
    const float c = collision_cc(p2(t.tk.x, t.tk.y), p2(t.tk.z, t.tk.w), p2(o.x, o.y), p2(o.z, o.w), agent_radius);
    return c < x ? c : x;
}
// the integration epilogue and the rollout's books for step h
__host__ __device__ inline void rollout_advance(RolloutState& st, const float x, const float fps, const int h) {
    const bool stopped = integrate(x, fps, st.p, st.ang, st.v, st.w);
    st.least = x < st.least ? x : st.least;
    if (stopped) { st.stops++; st.first = h < st.first ? h : st.first; }
}

// Under MsRollouts.slide a step is the sliding step (kernels/slide.h), the others at rest in both phases.  The contact's pass:
// a row, or an agent at rest at pb, whose own collision value is x1 offers its normal at p1, weighed by v
__host__ __device__ inline void rollout_offer_wall(SlideBest& best, const RolloutTask& t, const float4 u, const float x1, const float2 p1,
                                                   const float2 v, const float agent_radius) {
    if (wall_beyond(t.tk, u, t.reach2)) return;
    const float c = collision_cs(p2(t.tk.x, t.tk.y), p2(t.tk.z, t.tk.w), p2(u.x, u.y), p2(u.z, u.w), agent_radius);
    float nx, ny;
    if (c == x1 && slide_normal_wall(p2(p1.x, p1.y), u, nx, ny)) slide_offer(best, v, nx, ny);
}
__host__ __device__ inline void rollout_offer_agent(SlideBest& best, const RolloutTask& t, const float2 pb, const float x1, const float2 p1,
                                                    const float2 v, const float agent_radius) {
    const float4 o = make_float4(pb.x, pb.y, 0.f, 0.f);
    if (agents_apart(t.tk, o, agent_radius)) return;
    const float c = collision_cc(p2(t.tk.x, t.tk.y), p2(t.tk.z, t.tk.w), p2(o.x, o.y), p2(o.z, o.w), agent_radius);
    float nx, ny;
    if (c == x1 && slide_normal_agent(p2(p1.x, p1.y), p2(o.x, o.y), p2(0.f, 0.f), x1, nx, ny)) slide_offer(best, v, nx, ny);
}
// phase B's task: from where phase A left the candidate, the displacement it tries
__host__ __device__ inline RolloutTask rollout_task_b(const SlideContact& c, const float agent_radius) {
    const P2 p0 = p2(c.p1.x, c.p1.y), v0 = p2(c.u2.x, c.u2.y);
    const float reach = wall_reach(p0, v0, agent_radius);
    return RolloutTask{make_float4(p0.x, p0.y, v0.x, v0.y), (reach == reach) ? reach : INFINITY, reach_squared(reach)};
}
// the sliding step's end and the rollout's books for step h: a stop is a step whose velocity was zeroed
__host__ __device__ inline void rollout_advance_slide(RolloutState& st, int& slides, const SlideContact& c, const float x1, const float x2,
                                                      const float fps, const int h) {
    float slid;
    const bool stopped = slide_finish(c, x2, fps, st.p, st.ang, st.v, st.w, slid);
    st.least = x1 < st.least ? x1 : st.least;
    if (stopped) { st.stops++; st.first = h < st.first ? h : st.first; }
    else if (c.slides) slides++;
}

constexpr int ROLL_AHEAD = 4;          // rows of a near list a lane has in flight

// r.n_candidates candidates in groups of 64: block = (n A + a)*groups + group (by_g divides by groups, by_a by n_agents)
// SLIDE = 1: the sliding step - a lane's obstacles are met by one walk, called for phase A, then (only in a wave with a blocked
// candidate, and for those) for the contact, then (only with one that slides) for phase B from the cell the candidate stands in then
template <int SLIDE>
__global__ __launch_bounds__(WAVE) void rollout_kernel(
        const MsScenery sc, const AgentsK ag, const MsRollouts r, const float agent_radius, const float fps, const int groups,
        const Divisor by_g, const Divisor by_a) {
    const int lane = threadIdx.x;
    const int row = div_by((int)blockIdx.x, by_g), group = (int)blockIdx.x - row*groups;
    if (r.mask && !r.mask[row]) return;                                  // (uniform: the agent is not rolled, its rows stay)
    const int A = sc.n_agents, AF = sc.n_agents*sc.n_model;
    const int n = div_by(row, by_a), a = row - n*A;
    const int K = r.n_candidates, H = r.horizon;
    const int k = group*WAVE + lane;
    const bool live = k < K;                                             // (idle lanes roll the last candidate again and store nothing:
    const int kk = live ? k : K - 1;                                     //  the table rides in the lanes, which must all be there)
    const int L = sc.lines_widths[n];
    const float4* __restrict__ ln = reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[n];
    const bool gridded = sc.wg_cells != nullptr;                         // (the same for every wave of the launch)
    float4 geom = make_float4(0.f, 0.f, 0.f, 0.f);
    int wg_start = 0;
    if (gridded) { geom = reinterpret_cast<const float4*>(sc.wg_geom)[n]; wg_start = sc.wg_starts[n]; }
    const float2* __restrict__ pos2 = reinterpret_cast<const float2*>(ag.positions);
    RolloutState st = rollout_start(pos2[row], ag.angles[row], reinterpret_cast<const float2*>(ag.velocity)[row], ag.angvelocity[row], H);
    const long long* __restrict__ plan = r.actions + ((r.shared_plans ? (size_t)0 : (size_t)row*K) + kk)*H;
    // (the table rides in the lanes of one register, as in physics_kernel's prologue: looked up in memory it is a round trip
    // behind the action's own, every step)
    const bool small_table = 3*r.n_actions <= WAVE;
    const float tab = r.table[min(lane, 3*r.n_actions - 1)];
    float2* __restrict__ trail = reinterpret_cast<float2*>(r.trail);
    const size_t cand = (size_t)row*K + kk;
    [[maybe_unused]] int slides = 0;
    long long act = plan[0];
    for (int h = 0; h < H; h++) {
        const long long next = plan[min(h + 1, H - 1)];                  // (asked for a step ahead)
        const int c = rollout_action(act, r.n_actions);
        float dx, dy, dw;
        if (small_table) { dx = __shfl(tab, 3*c, WAVE); dy = __shfl(tab, 3*c + 1, WAVE); dw = __shfl(tab, 3*c + 2, WAVE); }
        else { dx = r.table[3*c]; dy = r.table[3*c + 1]; dw = r.table[3*c + 2]; }
        move_velocity(r.keep, st.ang, dx, dy, dw, st.v, st.w);
        const RolloutTask t = rollout_task(st, agent_radius, fps);
        // a candidate's obstacles - the others at rest, then the near list of the cell `at` lies in, or the env's static rows -
        // met for `mode` (0: the fold of the least value; 1, SLIDE: the contact's offers) by the lanes that are `on`
        SlideBest best{0.f, 0.f, 0.f, 0};
        float2 p1 = st.p;
        float x1 = 1.f;
        auto walk = [&](const RolloutTask& t, const float2 at, const bool on, const int mode) -> float {
            float x = 1.f;
            auto wall = [&](const float4 u) {
                if (SLIDE == 0 || mode != 1) x = rollout_meet_wall(x, t, u, agent_radius);
                else rollout_offer_wall(best, t, u, x1, p1, st.v, agent_radius);
            };
            if (r.others && on) {
                for (int b = 0; b < A; b++) {
                    if (b == a) continue;
                    if (SLIDE == 0 || mode != 1) x = rollout_meet_agent(x, t, pos2[n*A + b], agent_radius);
                    else rollout_offer_agent(best, t, pos2[n*A + b], x1, p1, st.v, agent_radius);
                }
            }
            bool covered = !on;
            if (gridded) {
                bool inside;
                const int cell = wg_cell_at(geom, sc.wg_cell, at.x, at.y, inside);
                const uint4 hdr = reinterpret_cast<const uint4*>(sc.wg_cells)[wg_start + cell];
                covered = !on | (inside & (t.reach <= sc.wg_reach));
                const int count = (on && covered) ? near_count(hdr, t.reach, sc.wg_reach_lo) : 0;
                const float4* __restrict__ near = reinterpret_cast<const float4*>(sc.wg_near_rows) + hdr.z;
                for (int j0 = 0; __ballot(j0 < count) != 0ull; j0 += ROLL_AHEAD) {
                    float4 u[ROLL_AHEAD];
                    #pragma unroll
                    for (int q = 0; q < ROLL_AHEAD; q++) u[q] = (j0 + q < count) ? near[j0 + q] : make_float4(0.f, 0.f, 0.f, 0.f);
                    #pragma unroll
                    for (int q = 0; q < ROLL_AHEAD; q++) {
                        if (j0 + q < count) wall(u[q]);
                    }
                }
            }
            if (__ballot(!covered) != 0ull) {
                // (rare with a grid, and plain: every static row of the env to the lanes no list covers - the rows' addresses are the wave's)
                for (int l = AF; l < L; l++) {
                    const float4 u = ln[l];
                    if (!covered) wall(u);
                }
            }
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
            if (__ballot(con.slides) != 0ull) x2 = walk(rollout_task_b(con, agent_radius), con.p1, con.slides, 2);
            rollout_advance_slide(st, slides, con, x1, x2, fps, h);
        }
        if (trail && live) trail[cand*H + h] = st.p;
        act = next;
    }
    if (live) {
        reinterpret_cast<float2*>(r.positions)[cand] = st.p;
        r.angles[cand] = st.ang;
        reinterpret_cast<float2*>(r.velocity)[cand] = st.v;
        r.angvelocity[cand] = st.w;
        r.progress[cand] = st.least;
        r.stops[cand] = st.stops;
        r.first_stop[cand] = st.first;
        if constexpr (SLIDE == 1) { if (r.slides) r.slides[cand] = slides; }
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
    const int row = div_by((int)blockIdx.x, by_g), group = (int)blockIdx.x - row*groups;
    if (r.mask && !r.mask[row]) return;
    const int A = sc.n_agents, AF = sc.n_agents*sc.n_model;
    const int n = div_by(row, by_a), a = row - n*A;
    const int K = r.n_candidates, H = r.horizon;
    const int k = group*WAVE + lane;
    const bool live = k < K;
    const int kk = live ? k : K - 1;
    const int n_live = min(WAVE, K - group*WAVE);                        // the wave's candidates: lanes 0 .. n_live - 1
    const int L = sc.lines_widths[n];
    const float4* __restrict__ ln = reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[n];
    const bool gridded = sc.wg_cells != nullptr;
    float4 geom = make_float4(0.f, 0.f, 0.f, 0.f);
    int wg_start = 0;
    if (gridded) { geom = reinterpret_cast<const float4*>(sc.wg_geom)[n]; wg_start = sc.wg_starts[n]; }
    const float2* __restrict__ pos2 = reinterpret_cast<const float2*>(ag.positions);
    RolloutState st = rollout_start(pos2[row], ag.angles[row], reinterpret_cast<const float2*>(ag.velocity)[row], ag.angvelocity[row], H);
    const long long* __restrict__ plan = r.actions + ((r.shared_plans ? (size_t)0 : (size_t)row*K) + kk)*H;
    const bool small_table = 3*r.n_actions <= WAVE;
    const float tab = r.table[min(lane, 3*r.n_actions - 1)];
    float2* __restrict__ trail = reinterpret_cast<float2*>(r.trail);
    const size_t cand = (size_t)row*K + kk;
    auto wave_sync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    int cnt = 0;
    auto flush = [&]() {
        wave_sync();
        #pragma unroll 1
        for (int p0 = 0; p0 < cnt; p0 += WAVE) {
            if (p0 + lane < cnt) {
                const float4 u = s_wall[p0 + lane];
                const int c = s_tag[p0 + lane];
                const float4 tk = s_task[c];
                const float x = collision_cs(p2(tk.x, tk.y), p2(tk.z, tk.w), p2(u.x, u.y), p2(u.z, u.w), agent_radius);
                if (x < 1.f) atomicMin(&s_prog[c], f_bits(x));
            }
        }
        wave_sync();
        cnt = 0;
    };
    // candidate c's rows, one a lane (`has`: this lane holds one): the cull, then the survivors appended as (row, c) pairs
    auto take = [&](const int c, const float4 u, const bool has) {
        const bool in_reach = has && !wall_beyond(s_task[c], u, s_reach2[c]);
        const unsigned long long m = __ballot(in_reach);
        if (cnt > ROLL_PAIRS - WAVE) flush();
        if (in_reach) {
            const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
            s_wall[pos] = u;
            s_tag[pos] = c;
        }
        cnt += __popcll(m);
    };
    long long act = plan[0];
    for (int h = 0; h < H; h++) {
        const long long next = plan[min(h + 1, H - 1)];
        const int c_ = rollout_action(act, r.n_actions);
        float dx, dy, dw;
        if (small_table) { dx = __shfl(tab, 3*c_, WAVE); dy = __shfl(tab, 3*c_ + 1, WAVE); dw = __shfl(tab, 3*c_ + 2, WAVE); }
        else { dx = r.table[3*c_]; dy = r.table[3*c_ + 1]; dw = r.table[3*c_ + 2]; }
        move_velocity(r.keep, st.ang, dx, dy, dw, st.v, st.w);
        const RolloutTask t = rollout_task(st, agent_radius, fps);
        float x = 1.f;
        if (r.others) {
            for (int b = 0; b < A; b++) {
                if (b != a) x = rollout_meet_agent(x, t, pos2[n*A + b], agent_radius);
            }
        }
        int count = 0, first = 0, covered = 0;
        if (gridded) {
            bool inside;
            const int cell = wg_cell_at(geom, sc.wg_cell, st.p.x, st.p.y, inside);
            const uint4 hdr = reinterpret_cast<const uint4*>(sc.wg_cells)[wg_start + cell];
            covered = (inside & (t.reach <= sc.wg_reach)) ? 1 : 0;
            count = covered ? near_count(hdr, t.reach, sc.wg_reach_lo) : 0;
            first = (int)hdr.z;
        }
        s_task[lane] = t.tk;
        s_reach2[lane] = t.reach2;
        s_prog[lane] = f_bits(x);
        wave_sync();
        for (int c = 0; c < n_live; c++) {                               // (uniform: candidate after candidate)
            if (__builtin_amdgcn_readlane(covered, c)) {
                const int count_c = __builtin_amdgcn_readlane(count, c);
                const float4* __restrict__ near = reinterpret_cast<const float4*>(sc.wg_near_rows) + (unsigned)__builtin_amdgcn_readlane(first, c);
                for (int j0 = 0; j0 < count_c; j0 += WAVE) {
                    const bool has = j0 + lane < count_c;
                    take(c, has ? near[j0 + lane] : make_float4(0.f, 0.f, 0.f, 0.f), has);
                }
            } else {
                for (int l0 = AF; l0 < L; l0 += WAVE) {
                    const bool has = l0 + lane < L;
                    take(c, has ? ln[l0 + lane] : make_float4(0.f, 0.f, 0.f, 0.f), has);
                }
            }
        }
        if (cnt) flush();
        wave_sync();
        x = bits_f(s_prog[lane]);
        rollout_advance(st, x, fps, h);
        if (trail && live) trail[cand*H + h] = st.p;
        act = next;
    }
    if (live) {
        reinterpret_cast<float2*>(r.positions)[cand] = st.p;
        r.angles[cand] = st.ang;
        reinterpret_cast<float2*>(r.velocity)[cand] = st.v;
        r.angvelocity[cand] = st.w;
        r.progress[cand] = st.least;
        r.stops[cand] = st.stops;
        r.first_stop[cand] = st.first;
    }
}

// The rule for ONE env, serially (ms_host_rollouts): the same functions in the same order; every candidate meets every wall.
// (Plain float accesses: host arrays promise no more than a float's alignment.)
inline void rollout_serial(const float* walls, const int n_walls, const MsAgents& ag, const int A, const MsRollouts& r,
                           const float agent_radius, const float fps) {
    const int K = r.n_candidates, H = r.horizon;
    for (int a = 0; a < A; a++) {
        if (r.mask && !r.mask[a]) continue;
        for (int k = 0; k < K; k++) {
            RolloutState st = rollout_start(make_float2(ag.positions[2*a], ag.positions[2*a + 1]), ag.angles[a],
                                            make_float2(ag.velocity[2*a], ag.velocity[2*a + 1]), ag.angvelocity[a], H);
            const long long* plan = r.actions + ((r.shared_plans ? (size_t)0 : (size_t)a*K) + k)*H;
            const size_t cand = (size_t)a*K + k;
            int slides = 0;
            for (int h = 0; h < H; h++) {
                const int c = rollout_action(plan[h], r.n_actions);
                move_velocity(r.keep, st.ang, r.table[3*c], r.table[3*c + 1], r.table[3*c + 2], st.v, st.w);
                const RolloutTask t = rollout_task(st, agent_radius, fps);
                float x = 1.f;
                if (r.others) {
                    for (int b = 0; b < A; b++) {
                        if (b != a) x = rollout_meet_agent(x, t, make_float2(ag.positions[2*b], ag.positions[2*b + 1]), agent_radius);
                    }
                }
                for (int l = 0; l < n_walls; l++)
                    x = rollout_meet_wall(x, t, make_float4(walls[4*l], walls[4*l + 1], walls[4*l + 2], walls[4*l + 3]), agent_radius);
                if (!r.slide) rollout_advance(st, x, fps, h);
                else {
                    SlideBest best{0.f, 0.f, 0.f, 0};
                    SlideContact con = slide_contact(st.p, st.ang, st.v, st.w, x, fps, best, r.bounce);
                    if (con.blocked) {
                        if (r.others) {
                            for (int b = 0; b < A; b++) {
                                if (b != a) rollout_offer_agent(best, t, make_float2(ag.positions[2*b], ag.positions[2*b + 1]), x, con.p1, st.v, agent_radius);
                            }
                        }
                        for (int l = 0; l < n_walls; l++)
                            rollout_offer_wall(best, t, make_float4(walls[4*l], walls[4*l + 1], walls[4*l + 2], walls[4*l + 3]), x, con.p1, st.v, agent_radius);
                        con = slide_contact(st.p, st.ang, st.v, st.w, x, fps, best, r.bounce);
                    }
                    float x2 = 1.f;
                    if (con.slides) {
                        const RolloutTask t2 = rollout_task_b(con, agent_radius);
                        if (r.others) {
                            for (int b = 0; b < A; b++) {
                                if (b != a) x2 = rollout_meet_agent(x2, t2, make_float2(ag.positions[2*b], ag.positions[2*b + 1]), agent_radius);
                            }
                        }
                        for (int l = 0; l < n_walls; l++)
                            x2 = rollout_meet_wall(x2, t2, make_float4(walls[4*l], walls[4*l + 1], walls[4*l + 2], walls[4*l + 3]), agent_radius);
                    }
                    rollout_advance_slide(st, slides, con, x, x2, fps, h);
                }
                if (r.trail) { r.trail[2*(cand*H + h)] = st.p.x; r.trail[2*(cand*H + h) + 1] = st.p.y; }
            }
            r.positions[2*cand] = st.p.x; r.positions[2*cand + 1] = st.p.y;
            r.angles[cand] = st.ang;
            r.velocity[2*cand] = st.v.x; r.velocity[2*cand + 1] = st.v.y;
            r.angvelocity[cand] = st.w;
            r.progress[cand] = st.least;
            r.stops[cand] = st.stops;
            r.first_stop[cand] = st.first;
            if (r.slide && r.slides) r.slides[cand] = slides;
        }
    }
}
