// kernels/slide.h -- physics_slide_kernel<MOVE, EXTRA>: the physics step with a second contact phase (MsSlide).
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, behind step.h, whose rules and
// pieces it calls, and physics.h, and in front of rollout.h, which chains its rule); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// sliding contacts                                             (MsSlide; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// The reference's step stops an agent dead, velocity and spin, at whatever its disc touches.  Under MsSlide a blocked agent gets
// a second move in the same launch: phase A is the reference's step as it stands (x1 = its `progress`, bit for bit); the CONTACT
// picks, among the obstacles whose own collision value IS x1, the normal the velocity runs into hardest; phase B deflects the
// velocity off that normal (with a small outward part, `bounce`: without one the side test of collision_cs turns a purely
// tangential move at dp = 1.001 R into x = 0) and spends the rest of the step, 1 - x1, along it - granted, like phase A, by
// collision_cs and collision_cc themselves, so that a slide moves no agent where two plain steps from the same poses could not.
//
// The rule as values, shared with ms_host_slide (the serial host statement): what differs between the two is only where an
// agent's obstacles come from and in which order they are met - and the rule is written so that the order cannot matter: the
// folds of phases A and B are minima over values in [+0, 1], and the contact's choice is the least key by VALUE, (vn, n.x, n.y)
// under float <, so that copies of a row (the near lists hold rows, not indices) and any lane order agree: equal keys are equal
// normals.  (A velocity that is not finite is outside the rule, as it is outside the plain step's: its keys need not order.)
struct SlideBest { float vn, nx, ny; int any; };                        // the least key met so far (any = 0: none yet)

// d = p1 - (the obstacle's nearest point) as a unit normal without -0; false: no length to speak of, the blocker is passed over
__host__ __device__ inline bool slide_unit(const P2 d, float& nx, float& ny) {
    const float l = len(d);
    if (!(l > 0.f) || !(l < INFINITY)) return false;
    nx = d.x/l + 0.f;
    ny = d.y/l + 0.f;
    return true;
}
// a static row u = (a, b): the normal from the row's nearest point to p1 (a NaN foot counts as the row's first end)
__host__ __device__ inline bool slide_normal_wall(const P2 p1, const float4 u, float& nx, float& ny) {
    const P2 a = p2(u.x, u.y), ab = p2(u.z, u.w) - a;
    float t = dot(p1 - a, ab)/dot(ab, ab);
    t = (t == t) ? ((t < 0.f) ? 0.f : (t > 1.f) ? 1.f : t) : 0.f;
    const P2 q = p2(a.x + t*ab.x, a.y + t*ab.y);
    return slide_unit(p1 - q, nx, ny);
}
// another agent, which phase A met at (pb, ub = v_b/fps): the normal from where it is at x1 of ITS step to p1
__host__ __device__ inline bool slide_normal_agent(const P2 p1, const P2 pb, const P2 ub, const float x1, float& nx, float& ny) {
    const P2 q = p2(pb.x + x1*ub.x, pb.y + x1*ub.y);
    return slide_unit(p1 - q, nx, ny);
}
// is the key (vn, nx, ny) lexicographically below the best so far?
__host__ __device__ inline bool slide_key_less(const float vn, const float nx, const float ny, const SlideBest& b) {
    if (!b.any) return true;
    if (vn < b.vn) return true;
    if (b.vn < vn) return false;
    if (nx < b.nx) return true;
    if (b.nx < nx) return false;
    return ny < b.ny;
}
__host__ __device__ inline void slide_offer(SlideBest& b, const float2 v, const float nx, const float ny) {
    const float vn = v.x*nx + v.y*ny;
    if (slide_key_less(vn, nx, ny, b)) b = SlideBest{vn, nx, ny, 1};
}
// v' = v - ((1 + bounce) vn) n
__host__ __device__ inline float2 slide_deflect(const float2 v, const SlideBest& b, const float bounce) {
    const float k = (1.f + bounce)*b.vn;
    return make_float2(v.x - k*b.nx, v.y - k*b.ny);
}
// What phase A leaves of an agent: where it stands (integrate's own statements with x1) and, if it was blocked by something it
// moves into, the deflected velocity v2 and the displacement u2 phase B tries (else u2 = 0: at rest for the others' phase B).
struct SlideContact { float2 p1, v2, u2; float ang1, r1; bool blocked, slides; };
__host__ __device__ inline SlideContact slide_contact(const float2 p, const float ang, const float2 v, const float w, const float x1,
                                                      const float fps, const SlideBest& best, const float bounce) {
    SlideContact c;
    c.p1 = make_float2(p.x + x1*v.x/fps, p.y + x1*v.y/fps);
    c.ang1 = normalize_degrees(ang + x1*w/fps);
    c.blocked = x1 < 1;
    c.slides = c.blocked && best.any && (best.vn < 0.f);
    c.v2 = v; c.u2 = make_float2(0.f, 0.f); c.r1 = 0.f;
    if (c.slides) {
        c.v2 = slide_deflect(v, best, bounce);
        c.r1 = 1.f - x1;
        c.u2 = make_float2((c.v2.x*c.r1)/fps, (c.v2.y*c.r1)/fps);
    }
    return c;
}
// The step's end: an agent nothing blocked is integrate()'s, one that was blocked and does not slide is its dead stop at p1,
// one that slides goes x2 of u2 further and keeps v2 - unless phase B blocked it as well (x2 < 1: a dead stop as ever).
// Returns `stopped` (the velocity was zeroed); slid = x2 r1, the share of the whole step spent sliding.
__host__ __device__ inline bool slide_finish(const SlideContact& c, const float x2, const float fps, float2& p, float& ang, float2& v,
                                             float& w, float& slid) {
    p = c.p1; ang = c.ang1; slid = 0.f;
    if (!c.blocked) return false;
    if (!c.slides) { v = make_float2(0.f, 0.f); w = 0.f; return true; }
    p = make_float2(c.p1.x + x2*c.u2.x, c.p1.y + x2*c.u2.y);
    ang = normalize_degrees(c.ang1 + x2*(c.r1*w)/fps);
    slid = x2*c.r1;
    if (x2 < 1) { v = make_float2(0.f, 0.f); w = 0.f; return true; }
    v = c.v2;
    return false;
}

// The contact's pass over one obstacle of task t - a static row u, or another agent as its own task has it, o = (p_b, u_b): is it a
// blocker - its own collision value IS x1 - and then its normal at p1 (meet_wall's and meet_agent's culls and tests, kernels/step.h)
__host__ __device__ inline bool offer_wall(const StepTask& t, const float4 u, const float x1, const float2 p1, const float agent_radius,
                                           float& nx, float& ny) {
    if (wall_beyond(t.tk, u, t.reach2)) return false;
    const float c = collision_cs(p2(t.tk.x, t.tk.y), p2(t.tk.z, t.tk.w), p2(u.x, u.y), p2(u.z, u.w), agent_radius);
    return c == x1 && slide_normal_wall(p2(p1.x, p1.y), u, nx, ny);
}
__host__ __device__ inline bool offer_agent(const StepTask& t, const float4 o, const float x1, const float2 p1, const float agent_radius,
                                            float& nx, float& ny) {
    if (agents_apart(t.tk, o, agent_radius)) return false;
    const float c = collision_cc(p2(t.tk.x, t.tk.y), p2(t.tk.z, t.tk.w), p2(o.x, o.y), p2(o.z, o.w), agent_radius);
    return c == x1 && slide_normal_agent(p2(p1.x, p1.y), p2(o.x, o.y), p2(o.z, o.w), c, nx, ny);
}

// ONE WAVEFRONT PER ENV, a lane an agent (n_agents <= 64), as physics_kernel without PACK - and up to three passes over the env's
// obstacles instead of one, by the same walk: pass 0 folds x1 (physics_kernel's atomicMin on the float's bits), pass 1 - only
// in a wave with a blocked agent, and only for those - meets the same obstacles again and offers the ones whose value is x1 as
// blockers, pass 2 - only with an agent that slides - folds x2 from the poses phase A left.  With a wall grid the agents' near
// lists are laid end to end and dealt a (row, agent) pair to a lane, more than 64 pairs culled first and compacted in LDS
// (physics_kernel's scheme); an env with an agent no list covers (outside the grid, a reach beyond wg_reach, crawling, a NaN
// pose), and every env of a scenery without a grid, meets all its static rows, plainly.
// The blockers' least key: the lanes that hold one are taken one after another (a ballot's bits: wave-uniform), lane 0 keeping
// the least in LDS - serial, but there is a blocker or two an agent, and the least of a set does not depend on the order.
template <int MOVE, int EXTRA>
__global__ __launch_bounds__(WAVE) void physics_slide_kernel(
        const MsScenery sc, const AgentsK ag, float* __restrict__ progress, const float agent_radius, const float fps,
        const MsMovement mv, const MsStepExtras ex, const MsSlide sl, const Divisor by_a, const FanSort fs) {
    __shared__ float4 s_task[WAVE];              // per agent: (p, v/fps) of the pass - (p1, u2) in pass 2
    __shared__ float s_reach2[WAVE];
    __shared__ unsigned s_prog[WAVE];            // the pass's fold, as bits
    __shared__ float2 s_vel[WAVE];               // v: what a normal is weighed by
    __shared__ float2 s_p1[WAVE];                // where phase A leaves the agent
    __shared__ float4 s_best[WAVE];              // (vn, n.x, n.y, any)
    __shared__ float4 s_wall[PHYS_PAIRS];
    __shared__ int s_tag[PHYS_PAIRS];
    // (the fan schedule's sort waves: the launch's first blocks, as physics_kernel's)
    if ((int)blockIdx.x < fs.n_blocks) {
        fan_sort_wave(fs, blockIdx.x, threadIdx.x, s_tag);
        return;
    }
    const int A = sc.n_agents, AF = sc.n_agents*sc.n_model;              // A <= WAVE (ms_slide_physics)
    const int lane = threadIdx.x;
    const int n = blockIdx.x - fs.n_blocks;
    const int nA = n*A;
    const bool mine = lane < A;
    const int i = nA + (mine ? lane : 0);
    const float2* pos2 = reinterpret_cast<const float2*>(ag.positions);
    const float2* vel2 = reinterpret_cast<const float2*>(ag.velocity);
    const EnvRows env = env_rows(sc, n);

    float2 my_p = make_float2(0.f, 0.f), my_v = make_float2(0.f, 0.f);
    float my_w = 0.f, my_ang = 0.f;
    if (mine) { my_p = pos2[i]; my_v = vel2[i]; my_w = ag.angvelocity[i]; my_ang = ag.angles[i]; }
    if constexpr (EXTRA == 1) {
        if (mine && step_books(ex, i)) {
            spawn_pose(ex, i, my_p, my_ang);
            my_v = make_float2(0.f, 0.f); my_w = 0.f;
            reinterpret_cast<float2*>(ag.velocity)[i] = my_v;           // (the epilogue writes velocities only where they change)
            ag.angvelocity[i] = 0.f;
        }
    }
    if constexpr (MOVE == 1) {
        if (mine) {
            const int c = action_row(mv.actions[i], mv.n_actions);
            move_velocity(mv.keep, my_ang, mv.table[3*c], mv.table[3*c + 1], mv.table[3*c + 2], my_v, my_w);
            ag.angvelocity[i] = my_w;
            reinterpret_cast<float2*>(ag.velocity)[i] = my_v;
        }
    }
    // a pass's tasks: lane = agent
    float my_reach = 0.f;
    auto task = [&](const float2 p, const P2 u) {
        const StepTask t = step_task(p, u, agent_radius);
        my_reach = t.reach;
        s_reach2[lane] = t.reach2;
        s_task[lane] = t.tk;
        s_prog[lane] = f_bits(1.f);
    };
    auto task_of = [&](const int t) { return StepTask{s_task[t], 0.f, s_reach2[t]}; };
    if (mine) {
        task(my_p, p2(my_v.x, my_v.y)/fps);
        s_vel[lane] = my_v;
    }
    int mode = 0;                                                        // the pass: 0 = x1, 1 = the blockers, 2 = x2
    unsigned long long active = __ballot(mine);                          // the agents the pass is for
    // the lanes that hold a blocker's normal for agent t, one after another
    auto offer = [&](const bool has, const int t, const float nx, const float ny) {
        unsigned long long m = __ballot(has);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1ull;
            const int tt = __builtin_amdgcn_readlane(t, l);
            const float cx = readlane_f(nx, l), cy = readlane_f(ny, l);
            if (lane == 0) {
                const float4 b4 = s_best[tt];
                SlideBest b{b4.x, b4.y, b4.z, b4.w != 0.f ? 1 : 0};
                slide_offer(b, s_vel[tt], cx, cy);
                s_best[tt] = make_float4(b.vn, b.nx, b.ny, 1.f);
            }
        }
    };
    // one (row, agent) pair of the lanes that have one (every lane of the wave comes here): passes 0 and 2 fold its value; pass 1:
    // is it a blocker, and its normal
    auto meet = [&](const bool has, const float4 u, const int t) {
        float nx = 0.f, ny = 0.f;
        bool blocker = false;
        if (has) {
            if (mode != 1) fold_least(&s_prog[t], meet_wall(1.f, task_of(t), u, agent_radius));
            else blocker = offer_wall(task_of(t), u, bits_f(s_prog[t]), s_p1[t], agent_radius, nx, ny);
        }
        if (mode == 1) offer(blocker, t, nx, ny);
    };
    PairList pairs{s_wall, s_tag, PHYS_PAIRS, 0};
    auto flush = [&]() { pairs.drain(lane, meet); };
    SlideContact con;
    float my_x1 = 1.f;
    for (; mode < 3; mode++) {
        if (mode == 1) {
            // phase A is folded: who was blocked?
            wave_sync();
            my_x1 = mine ? bits_f(s_prog[lane]) : 1.f;
            active = __ballot(mine && (my_x1 < 1.f));
            if (!active) break;
            if (mine) {
                s_p1[lane] = make_float2(my_p.x + my_x1*my_v.x/fps, my_p.y + my_x1*my_v.y/fps);
                s_best[lane] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            wave_sync();
        }
        if (mode == 2) {
            // the contact is settled: the poses phase A leaves, and who slides
            wave_sync();
            bool slides = false;
            if (mine) {
                const float4 b4 = s_best[lane];
                con = slide_contact(my_p, my_ang, my_v, my_w, my_x1, fps, SlideBest{b4.x, b4.y, b4.z, b4.w != 0.f ? 1 : 0}, sl.bounce);
                slides = con.slides;
            }
            active = __ballot(slides);
            if (!active) break;
            wave_sync();
            if (mine) task(con.p1, p2(con.u2.x, con.u2.y));
        }
        wave_sync();
        // the env's other agents (kernels.cu:193-200), one ordered pair per lane: at their start-of-step (p, u) in passes 0 and 1,
        // as phase A left them, (p1, u2), in pass 2
        for (int i0 = 0; i0 < A*A; i0 += WAVE) {
            const int q = i0 + lane;
            const int t = min(div_by(q, by_a), A - 1), d1 = q - t*A;
            float nx = 0.f, ny = 0.f;
            bool has = false;
            if (q < A*A && d1 != t && ((active >> t) & 1ull)) {
                if (mode != 1) fold_least(&s_prog[t], meet_agent(1.f, task_of(t), s_task[d1], agent_radius));
                else has = offer_agent(task_of(t), s_task[d1], bits_f(s_prog[t]), s_p1[t], agent_radius, nx, ny);
            }
            if (mode == 1) offer(has, t, nx, ny);
        }
        // the static rows: the agents' near lists laid end to end, if every agent of the pass is covered by its own
        bool swept = true;
        if (env.gridded) {
            NearList nl{true, 0, 0u, nullptr};
            if ((active >> lane) & 1ull) nl = near_list(sc, env.geom, env.wg_start, s_task[lane].x, s_task[lane].y, my_reach);
            if (!__ballot(!nl.covered)) {
                swept = false;
                const int incl = wave_scan_add(nl.count);
                const int excl = incl - nl.count;
                const int P = __builtin_amdgcn_readlane(incl, 63);
                for (int p0 = 0; p0 < P; p0 += WAVE) {
                    const int q = p0 + lane;
                    int t;
                    unsigned at;
                    deal_pair(incl, excl, nl.first, A, q, t, at);
                    const float4 u = (q < P) ? reinterpret_cast<const float4*>(sc.wg_near_rows)[at] : make_float4(0.f, 0.f, 0.f, 0.f);
                    // (up to 64 pairs: one each, cull and test; more: the cull alone first, its survivors compacted - physics_kernel's scheme)
                    if (P <= WAVE) meet(q < P, u, t);
                    else pairs.append(lane, q < P && !wall_beyond(s_task[t], u, s_reach2[t]), u, t, flush);
                }
                if (pairs.cnt) flush();
            }
        }
        if (swept) {
            // (plain: every static row of the env, a lane a row, to every agent of the pass - meet() has the cull)
            for (int l0 = AF; l0 < env.L; l0 += WAVE) {
                const bool row = l0 + lane < env.L;
                const float4 u = row ? env.ln[l0 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
                unsigned long long todo = active;
                while (todo) {
                    const int t = __ffsll((long long)todo) - 1;
                    todo &= todo - 1ull;
                    meet(row, u, t);
                }
            }
        }
    }
    wave_sync();
    if (mine) {
        // (mode: the pass the loop left at - 1: nobody was blocked, 2: nobody slides, 3: x2 is folded)
        if (mode == 1) con = slide_contact(my_p, my_ang, my_v, my_w, my_x1, fps, SlideBest{0.f, 0.f, 0.f, 0}, sl.bounce);
        const float x2 = (mode == 3) ? bits_f(s_prog[lane]) : 1.f;
        float2 p, v = my_v;
        float w_ = my_w, ang, slid;
        const bool stopped = slide_finish(con, x2, fps, p, ang, v, w_, slid);
        bool changed = con.blocked;                                      // (a velocity only changes on a collision)
        if constexpr (EXTRA == 1) {
            if (respawns_after(ex, i)) {
                spawn_pose(ex, i, p, ang);
                v = make_float2(0.f, 0.f); w_ = 0.f;
                changed = true;
            }
        }
        step_store(ag, ex, i, p, ang, v, w_, changed, EXTRA == 1);
        progress[i] = my_x1;
        if (sl.slid) sl.slid[i] = slid;
        if (sl.stopped) sl.stopped[i] = stopped ? 1 : 0;
    }
}

// The rule for whole envs, serially (ms_host_slide): the same functions; every agent meets every static row of its env, behind
// the reach cull.  `walls`: the static rows of all envs, env n's rows wall_starts[n] .. wall_starts[n + 1] - 1; every other
// pointer as the device call's, host memory.  (Plain float accesses: host arrays promise no more than a float's alignment.)
inline void slide_serial(const float* walls, const long long* wall_starts, const int N, const int A, const MsAgents& ag,
                         const MsMovement* mv, const MsStepExtras& ex, const bool extras, const MsSlide& sl, float* progress,
                         const float agent_radius, const float fps) {
    struct Agent { float2 p, v; float ang, w, x1; StepTask t; SlideContact con; };
    Agent* as = new Agent[A];
    const auto row_of = [&](const long long l) { return make_float4(walls[4*l], walls[4*l + 1], walls[4*l + 2], walls[4*l + 3]); };
    for (int n = 0; n < N; n++) {
        const long long l0 = wall_starts[n], l1 = wall_starts[n + 1];
        for (int a = 0; a < A; a++) {
            const int i = n*A + a;
            Agent& me = as[a];
            me.p = load2(ag.positions, i); me.v = load2(ag.velocity, i);
            me.ang = ag.angles[i]; me.w = ag.angvelocity[i];
            if (extras && step_books(ex, i)) {
                spawn_pose(ex, i, me.p, me.ang);
                me.v = make_float2(0.f, 0.f); me.w = 0.f;
            }
            if (mv) {
                const int c = action_row(mv->actions[i], mv->n_actions);
                move_velocity(mv->keep, me.ang, mv->table[3*c], mv->table[3*c + 1], mv->table[3*c + 2], me.v, me.w);
            }
        }
        // a pass: pass 0 and 2 fold the least collision value of agent a's task, pass 1 offers the obstacles whose value is x1
        const auto pass = [&](const int a, const int mode, SlideBest& best) {
            const Agent& me = as[a];
            float least = 1.f, nx, ny;
            for (int b = 0; b < A; b++) {
                if (b == a) continue;
                if (mode != 1) least = meet_agent(least, me.t, as[b].t.tk, agent_radius);
                else if (offer_agent(me.t, as[b].t.tk, me.x1, me.con.p1, agent_radius, nx, ny)) slide_offer(best, me.v, nx, ny);
            }
            for (long long l = l0; l < l1; l++) {
                if (mode != 1) least = meet_wall(least, me.t, row_of(l), agent_radius);
                else if (offer_wall(me.t, row_of(l), me.x1, me.con.p1, agent_radius, nx, ny)) slide_offer(best, me.v, nx, ny);
            }
            return least;
        };
        SlideBest none{0.f, 0.f, 0.f, 0};
        for (int a = 0; a < A; a++) as[a].t = step_task(as[a].p, p2(as[a].v.x, as[a].v.y)/fps, agent_radius);
        for (int a = 0; a < A; a++) as[a].x1 = pass(a, 0, none);
        for (int a = 0; a < A; a++) {
            Agent& me = as[a];
            SlideBest best{0.f, 0.f, 0.f, 0};
            me.con = slide_contact(me.p, me.ang, me.v, me.w, me.x1, fps, best, sl.bounce);   // (p1: what the normals are taken at)
            if (me.con.blocked) {
                pass(a, 1, best);
                me.con = slide_contact(me.p, me.ang, me.v, me.w, me.x1, fps, best, sl.bounce);
            }
        }
        for (int a = 0; a < A; a++) as[a].t = step_task(as[a].con.p1, p2(as[a].con.u2.x, as[a].con.u2.y), agent_radius);
        for (int a = 0; a < A; a++) {
            const int i = n*A + a;
            Agent& me = as[a];
            const float x2 = me.con.slides ? pass(a, 2, none) : 1.f;
            float2 p, v = me.v;
            float w = me.w, ang, slid;
            const bool stopped = slide_finish(me.con, x2, fps, p, ang, v, w, slid);
            if (extras && respawns_after(ex, i)) {
                spawn_pose(ex, i, p, ang);
                v = make_float2(0.f, 0.f); w = 0.f;
            }
            store2(ag.positions, i, p);
            ag.angles[i] = ang;
            store2(ag.velocity, i, v);
            ag.angvelocity[i] = w;
            progress[i] = me.x1;
            if (sl.slid) sl.slid[i] = slid;
            if (sl.stopped) sl.stopped[i] = stopped ? 1 : 0;
            if (extras) imu_store(ex, i, ang, v, w);
        }
    }
    delete[] as;
}
