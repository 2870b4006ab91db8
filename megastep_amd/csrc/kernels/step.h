// kernels/step.h -- what the agent step's kernels share: the per-agent rules, and the scaffolding round them, each stated once.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, behind math.h and in front of
// physics.h, slide.h, rollout.h and scenario.h, which call it); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// The per-agent rules of a step, on values: physics_kernel, physics_slide_kernel, the rollout and scenario kernels, the serial host
// statements and the one-launch step (render.h) call them with loads, stores and lanes of their own.
// ------------------------------------------------------------------------------------------------
// the spawn pose of agent i, if it is to be respawned (modules.py:321-326)
__host__ __device__ inline void spawn_pose(const MsStepExtras& ex, const int i, float2& p, float& ang) {
    const long long c = min(max(ex.respawn_choice[i], 0ll), (long long)ex.n_spawns - 1);
    p = reinterpret_cast<const float2*>(ex.spawn_positions)[(size_t)i*ex.n_spawns + c];
    ang = ex.spawn_angles[(size_t)i*ex.n_spawns + c];
}
// agent i's new age (modules.py:361-366): 0 if `reset` (its respawn mask) is set or comes out set because it has lived its span
__host__ __device__ inline int lifespan_tick(const MsStepExtras& ex, const int i, bool& reset) {
    const int life = ex.lifespans[i] + 1;
    reset = reset | (life >= ex.max_lifespans[i]);
    return reset ? 0 : life;
}
// the movement modules' velocity update (modules.py:57-66,106-118): the action's delta turned into the global frame, blended in
__host__ __device__ inline void move_velocity(const float keep, const float ang, const float dx, const float dy, const float dw, float2& v, float& w) {
    const float a_ = 0.017453292519943295f*ang;                         // np.pi/180*angles, in binary32 like torch
    const float s_ = sinf(a_), c_ = cosf(a_);
    const float gx = c_*dx - s_*dy, gy = s_*dx + c_*dy;
    if (keep == 0.f) { w = dw; v = make_float2(gx, gy); }
    else { w = keep*w + dw; v = make_float2(keep*v.x + gx, keep*v.y + gy); }
}
// how many of a cell's near walls (its header hdr) an agent of this reach meets: the short tier if the reach is within wg_reach_lo
__host__ __device__ inline int near_count(const uint4 hdr, const float reach, const float reach_lo) {
    return (int)((reach <= reach_lo) ? (hdr.w & 0xffffu) : (hdr.w >> 16));
}
// the integration epilogue (kernels.cu:224-227): the fraction x of the step the agent can take; stopped (x < 1): at rest
__host__ __device__ inline bool integrate(const float x, const float fps, float2& p, float& ang, float2& v, float& w) {
    p.x = p.x + x*v.x/fps;
    p.y = p.y + x*v.y/fps;
    ang = normalize_degrees(ang + x*w/fps);
    const bool stopped = x < 1;
    if (stopped) { v = make_float2(0.f, 0.f); w = 0.f; }
    return stopped;
}
// the IMU reading (modules.py:263-270, to_local_frame :24-31); the scales are reciprocals: ATen's `a * (1.f/b)` for tensor / scalar
__host__ __device__ inline float3 imu_reading(const MsStepExtras& ex, const float ang, const float2 v, const float w) {
    const float a_ = 0.017453292519943295f*ang;                         // (as move_velocity)
    const float s_ = sinf(a_), c_ = cosf(a_);
    return make_float3(w*ex.imu_ang_scale, (c_*v.x + s_*v.y)*ex.imu_speed_scale, (-s_*v.x + c_*v.y)*ex.imu_speed_scale);
}

// ------------------------------------------------------------------------------------------------
// The scaffolding round the rules.  (physics_kernel keeps its own text where a piece of this changes an instruction of it: its
// comments name the statement here that they mirror.)
// ------------------------------------------------------------------------------------------------
// a pair of floats of a (.., 2) array: one 8-byte access on the device; plain floats on the host, whose arrays promise no more
// than a float's alignment
__host__ __device__ inline float2 load2(const float* a, const size_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return reinterpret_cast<const float2*>(a)[i];
#else
    return make_float2(a[2*i], a[2*i + 1]);
#endif
}
__host__ __device__ inline void store2(float* a, const size_t i, const float2 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    reinterpret_cast<float2*>(a)[i] = v;
#else
    a[2*i] = v.x; a[2*i + 1] = v.y;
#endif
}

// the bookkeeping prologue for agent i (MsStepExtras): its age, its span, its respawn mask written back; true: it is to be
// respawned BEFORE the step (spawn_pose, at rest - the caller's stores)
__host__ __device__ inline bool step_books(const MsStepExtras& ex, const int i) {
    bool reset = ex.respawn_mask && ex.respawn_mask[i];
    if (ex.lifespans) {
        ex.lifespans[i] = lifespan_tick(ex, i, reset);
        if (reset) ex.max_lifespans[i] = ex.fresh_max[i];
        if (ex.respawn_mask) ex.respawn_mask[i] = reset ? 1 : 0;
    }
    return reset && ex.spawn_positions && !ex.respawn_after;
}
// ... and whether it is to be respawned AFTER it
__host__ __device__ inline bool respawns_after(const MsStepExtras& ex, const int i) {
    return ex.spawn_positions && ex.respawn_after && ex.respawn_mask && ex.respawn_mask[i];
}
__host__ __device__ inline void imu_store(const MsStepExtras& ex, const int i, const float ang, const float2 v, const float w) {
    if (ex.imu) {
        const float3 m = imu_reading(ex, ang, v, w);
        ex.imu[3*i] = m.x;
        ex.imu[3*i + 1] = m.y;
        ex.imu[3*i + 2] = m.z;
    }
}
// the epilogue's stores for agent i: the pose, the headings cache, the velocity only where it `changed`, the IMU (`extras`)
__device__ inline void step_store(const AgentsK& ag, const MsStepExtras& ex, const int i, const float2 p, const float ang, const float2 v,
                                  const float w, const bool changed, const bool extras) {
    reinterpret_cast<float2*>(ag.positions)[i] = p;
    ag.angles[i] = ang;
    if (ag.headings) {                                                   // what render_prep_kernel would compute, one launch earlier
        float hs, hc;
        sincospi_f(ang/180.f, hs, hc);
        reinterpret_cast<float4*>(ag.headings)[i] = make_float4(ang, hs, hc, 0.f);
    }
    if (changed) {
        reinterpret_cast<float2*>(ag.velocity)[i] = v;
        ag.angvelocity[i] = w;
    }
    if (extras) imu_store(ex, i, ang, v, w);
}

// the row of the table an action means: clamped
__host__ __device__ inline int action_row(const long long act, const int n_actions) {
    return (int)(act < 0 ? 0 : act > (long long)n_actions - 1 ? (long long)n_actions - 1 : act);
}
// The table - seven actions, three floats each - rides in the lanes of one register, asked for up front: looked up in memory by
// the action it is a round trip behind the action's own, every step.  (The lanes exchange entries, which only works among lanes
// that are all there: idle lanes look an action up as well.)  A table of more than 64 floats is read where it lies.
struct ActionTable {
    const float* table; float tab; bool small;
    __device__ ActionTable(const float* table_, const int n_actions, const int lane)
        : table(table_), tab(table_[min(lane, 3*n_actions - 1)]), small(3*n_actions <= WAVE) {}
    __device__ void delta(const int c, float& dx, float& dy, float& dw) const {
        if (small) { dx = __shfl(tab, 3*c, WAVE); dy = __shfl(tab, 3*c + 1, WAVE); dw = __shfl(tab, 3*c + 2, WAVE); }
        else { dx = table[3*c]; dy = table[3*c + 1]; dw = table[3*c + 2]; }
    }
};

// what a step's tests need of an agent at p that tries the displacement u (v/fps; phase B of a slide: u2): (p, u), the reach
// (NaN: +inf - every tier and the grid refuse it) and its square
struct StepTask { float4 tk; float reach, reach2; };
__host__ __device__ inline StepTask step_task(const float2 p, const P2 u, const float agent_radius) {
    const float reach = wall_reach(p2(p.x, p.y), u, agent_radius);
    return StepTask{make_float4(p.x, p.y, u.x, u.y), (reach == reach) ? reach : INFINITY, reach_squared(reach)};
}
// one (row, task) pair: the reach cull on the true distance, then the reference's test (kernels.cu:135-171,202-205), folded into x
__host__ __device__ inline float meet_wall(const float x, const StepTask& t, const float4 u, const float agent_radius) {
    if (wall_beyond(t.tk, u, t.reach2)) return x;
    const float c = collision_cs(p2(t.tk.x, t.tk.y), p2(t.tk.z, t.tk.w), p2(u.x, u.y), p2(u.z, u.w), agent_radius);
    return c < x ? c : x;
}
// one (agent, agent) pair (kernels.cu:193-200): the other as its own task has it, o = (p_b, u_b) - at rest: (p_b, 0, 0)
__host__ __device__ inline float meet_agent(const float x, const StepTask& t, const float4 o, const float agent_radius) {
    if (agents_apart(t.tk, o, agent_radius)) return x;
    const float c = collision_cc(p2(t.tk.x, t.tk.y), p2(t.tk.z, t.tk.w), p2(o.x, o.y), p2(o.z, o.w), agent_radius);
    return c < x ? c : x;
}
// the fold where a task's pairs are spread over the lanes: atomicMin on the float's bits - every value is in [+0, 1], where the
// unsigned order is the float order, so the fold is exact in any order
__device__ inline void fold_least(unsigned* prog, const float x) {
    if (x < 1.f) atomicMin(prog, f_bits(x));
}

// Is an agent at (x, y) with this reach covered by the near list of its cell (inside the grid's box, a reach the lists allow -
// which a crawling agent's and a NaN's are not), and the list: `count` rows from row `first` of wg_near_rows, at `rows` (not
// covered: none).  geom, start: the env's rows of wg_geom and wg_starts.  This decides whether a wave may skip an env's walls.
struct NearList { bool covered; int count; unsigned first; const float4* rows; };
__device__ inline NearList near_list(const MsScenery& sc, const float4 geom, const int start, const float x, const float y, const float reach) {
    bool inside;
    const uint4 hdr = reinterpret_cast<const uint4*>(sc.wg_cells)[start + wg_cell_at(geom, sc.wg_cell, x, y, inside)];
    const bool covered = inside & (reach <= sc.wg_reach);
    return NearList{covered, covered ? near_count(hdr, reach, sc.wg_reach_lo) : 0, hdr.z, reinterpret_cast<const float4*>(sc.wg_near_rows) + hdr.z};
}
// an env's static rows, and its rows of the wall grid (no grid: none, and no agent is covered)
struct EnvRows { int L; const float4* ln; bool gridded; float4 geom; int wg_start; };
__device__ inline EnvRows env_rows(const MsScenery& sc, const int n) {
    EnvRows e{sc.lines_widths[n], reinterpret_cast<const float4*>(sc.lines_vals) + sc.lines_starts[n], sc.wg_cells != nullptr,
              make_float4(0.f, 0.f, 0.f, 0.f), 0};
    if (e.gridded) { e.geom = reinterpret_cast<const float4*>(sc.wg_geom)[n]; e.wg_start = sc.wg_starts[n]; }
    return e;
}
__device__ inline NearList near_list(const MsScenery& sc, const EnvRows& e, const float2 at, const float reach) {
    return e.gridded ? near_list(sc, e.geom, e.wg_start, at.x, at.y, reach) : NearList{false, 0, 0u, nullptr};
}

// A lane walks its list's rows, ROLL_AHEAD in flight, the wave looping to the largest count among its lanes; then the lanes no
// list covers walk the env's static rows AF .. L - 1 while the others wait (rare with a grid, and plain: the rows' addresses are
// the wave's).  fn(u): one row met.
constexpr int ROLL_AHEAD = 4;          // rows of a near list a lane has in flight
template <class F>
__device__ inline void walk_rows(const NearList nl, const EnvRows& e, const int AF, F&& fn) {
    const float4* __restrict__ near = nl.rows;
    for (int j0 = 0; __ballot(j0 < nl.count) != 0ull; j0 += ROLL_AHEAD) {
        float4 u[ROLL_AHEAD];
        #pragma unroll
        for (int q = 0; q < ROLL_AHEAD; q++) u[q] = (j0 + q < nl.count) ? near[j0 + q] : make_float4(0.f, 0.f, 0.f, 0.f);
        #pragma unroll
        for (int q = 0; q < ROLL_AHEAD; q++) {
            if (j0 + q < nl.count) fn(u[q]);
        }
    }
    if (__ballot(!nl.covered) != 0ull) {
        const float4* __restrict__ ln = e.ln;
        for (int l = AF; l < e.L; l++) {
            const float4 u = ln[l];
            if (!nl.covered) fn(u);
        }
    }
}

// Agents' near lists laid end to end, a pair a lane (incl: the wave's inclusive scan of the lists' counts, excl = incl - count,
// a lane an agent, A of them): whose list is pair q in - t - and which row of wg_near_rows is it - at?
__device__ inline void deal_pair(const int incl, const int excl, const unsigned first, const int A, const int q, int& t, unsigned& at) {
    t = 0;
    for (int j = 0; j < A - 1; j++) t += (__builtin_amdgcn_readlane(incl, j) <= q) ? 1 : 0;
    at = (unsigned)__shfl((int)first, t, WAVE) + (unsigned)(q - __shfl(excl, t, WAVE));
}

// The LDS pair list: the lanes' (row, tag) pairs that pass a cheap cull are laid end to end, so that the ten divides and five
// square roots of the exact test run over full lanes.  The caller owns s_wall and s_tag (`cap` of each, at least 2 x 64).
struct PairList {
    float4* s_wall; int* s_tag; int cap; int cnt;
    // the lanes that `keep` append (u, tag); flush() first - a drain - when a chunk more could overflow
    template <class F>
    __device__ void append(const int lane, const bool keep, const float4 u, const int tag, F&& flush) {
        const unsigned long long m = __ballot(keep);
        if (cnt > cap - WAVE) flush();
        if (keep) {
            const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
            s_wall[pos] = u;
            s_tag[pos] = tag;
        }
        cnt += __popcll(m);
    }
    // 64 pairs at a time, every lane of the wave in fn(has, u, tag) (has: the lane holds a pair - else zeros), and the list is empty
    template <class F>
    __device__ void drain(const int lane, F&& fn) {
        wave_sync();
        #pragma unroll 1
        for (int p0 = 0; p0 < cnt; p0 += WAVE) {
            const bool has = p0 + lane < cnt;
            fn(has, has ? s_wall[p0 + lane] : make_float4(0.f, 0.f, 0.f, 0.f), has ? s_tag[p0 + lane] : 0);
        }
        wave_sync();
        cnt = 0;
    }
};

// ------------------------------------------------------------------------------------------------
// Rolled steps (MsRollouts, MsScenarios): a lane's - or the serial statement's - state over the horizon, and its results.
// ------------------------------------------------------------------------------------------------
struct RolloutState { float2 p, v; float ang, w, least; int stops, first; };
// the state agent `row` of the (N, A) arrays starts from
template <class Agents>
__host__ __device__ inline RolloutState rollout_start(const Agents& ag, const size_t row, const int horizon) {
    return RolloutState{load2(ag.positions, row), load2(ag.velocity, row), ag.angles[row], ag.angvelocity[row], 1.f, 0, horizon};
}
__host__ __device__ inline StepTask rollout_task(const RolloutState& st, const float agent_radius, const float fps) {
    return step_task(st.p, p2(st.v.x, st.v.y)/fps, agent_radius);
}
// the integration epilogue and the rollout's books for step h
__host__ __device__ inline void rollout_advance(RolloutState& st, const float x, const float fps, const int h) {
    const bool stopped = integrate(x, fps, st.p, st.ang, st.v, st.w);
    st.least = x < st.least ? x : st.least;
    if (stopped) { st.stops++; st.first = h < st.first ? h : st.first; }
}
// the seven results of row `cand` of the outputs (MsRollouts or MsScenarios: the same members)
template <class Out>
__host__ __device__ inline void rollout_store(const Out& out, const size_t cand, const RolloutState& st) {
    store2(out.positions, cand, st.p);
    out.angles[cand] = st.ang;
    store2(out.velocity, cand, st.v);
    out.angvelocity[cand] = st.w;
    out.progress[cand] = st.least;
    out.stops[cand] = st.stops;
    out.first_stop[cand] = st.first;
}
// A rollout lane's binding: block = (n A + a)*groups + group, lane = candidate k of its group of 64.  Idle lanes (not `live`) roll
// the last candidate again and store nothing: the table rides in the lanes, which must all be there.
struct RolloutLane { int row, n, a, k, kk; bool live; const long long* plan; size_t cand; };
__device__ inline RolloutLane rollout_bind(const MsRollouts& r, const int A, const int block, const int lane, const int groups,
                                           const Divisor by_g, const Divisor by_a) {
    RolloutLane b;
    b.row = div_by(block, by_g);
    b.n = div_by(b.row, by_a); b.a = b.row - b.n*A;
    b.k = (block - b.row*groups)*WAVE + lane;
    b.live = b.k < r.n_candidates;
    b.kk = b.live ? b.k : r.n_candidates - 1;
    b.plan = r.actions + ((r.shared_plans ? (size_t)0 : (size_t)b.row*r.n_candidates) + b.kk)*r.horizon;
    b.cand = (size_t)b.row*r.n_candidates + b.kk;
    return b;
}
