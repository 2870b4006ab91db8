// kernels/bodies.h -- physics_bodies_kernel<MOVE, EXTRA>: the physics step with a store of bodies in the agents' way (MsBodies,
// DESIGN 3.39).  Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, behind step.h,
// whose rules and pieces it calls, physics.h and slide.h, whose frame it takes); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// solid bodies                                                 (MsBodies; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// The plain step knows the env's agents and its static rows.  Under MsBodies the slots of an Items-shaped store - walkers, crates,
// pillars - are discs of agent_radius that stop an agent as another agent would: every present body k is folded into the agent's x
// by meet_agent against o_k = (p_k, u_k), u_k = v_k/fps or (0, 0).  The fold is a least value over [+0, 1], so x is the same in any
// order and on any path; next to it the kernel keeps, per agent, the least (bits(c_k), k) as ONE unsigned 64-bit key - `blocker`
// is its low half where its high half is the final x - and counts the bodies with c_k < 1.
//
// The per-pair statements, shared with ms_host_bodies (bodies_serial below):
constexpr int BODY_MAX_SLOTS = 1024;
constexpr int BODY_TAG = 1 << 16;                    // a pair-list tag of a (body, agent) pair: BODY_TAG | k << 6 | t (t < 64, k < 1024)
constexpr unsigned long long BODY_NO_KEY = ~0ull;

// is slot k of the store there: both coordinates finite
__host__ __device__ inline bool body_present(const float2 p) { return fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY; }
// body k as the other of a pair, o_k = (p_k, u_k): its velocity a step, (0, 0) without velocities or where one is not finite
__host__ __device__ inline float4 body_other(const float2 p, const float* velocities, const size_t at, const float fps) {
    P2 u = p2(0.f, 0.f);
    if (velocities) {
        const float2 v = load2(velocities, at);
        if (fabsf(v.x) < INFINITY && fabsf(v.y) < INFINITY) u = p2(v.x, v.y)/fps;
    }
    return make_float4(p.x, p.y, u.x, u.y);
}
// one (body, agent) pair behind the reach cull: c_k, and whether it is a contact (c_k < 1) - then folded into the agent's key
__host__ __device__ inline float body_meet(const float4 tk, const float4 o, const float agent_radius) {
    return collision_cc(p2(tk.x, tk.y), p2(tk.z, tk.w), p2(o.x, o.y), p2(o.z, o.w), agent_radius);
}
__host__ __device__ inline unsigned long long body_key(const float c, const int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ((unsigned long long)__float_as_uint(c) << 32) | (unsigned)k;
#else
    unsigned b;
    memcpy(&b, &c, sizeof b);
    return ((unsigned long long)b << 32) | (unsigned)k;
#endif
}
// the blocker of an agent whose step ended at x with the least key `key`: the body whose own fraction IS x, else -1
__host__ __device__ inline int body_blocker(const unsigned long long key, const float x) {
    return (x < 1.f && key != BODY_NO_KEY && (key >> 32) == (body_key(x, 0) >> 32)) ? (int)(key & 0xffffffffull) : -1;
}

// THE BOX CULL, for bodies AT REST.  agents_apart(me, o) with o = (q, 0, 0) culls the pair when 0.9998 |q - p|^2 > reach^2,
// reach = B + 1e-4 (|p.x| + |p.y| + |q.x| + |q.y|), where B - the 1.02 (kq^2 (1.0102 v_up + r2) + kq r2) + 1e-3 of its text -
// depends on the agent alone once the other stands still.  With |q.x| <= |p.x| + |dx| and |q.y| <= |p.y| + |dy|:
//     reach <= B + 2e-4 (|p.x| + |p.y|) + 1e-4 (|dx| + |dy|) = H + 1e-4 (|dx| + |dy|) <= H + 2e-4 d,      d = |q - p| >= max(|dx|, |dy|)
// so max(|dx|, |dy|) > 1.01 H gives 0.9999 d - 2e-4 d > 0.9997*1.01 H > H: the pair is apart.  The margin of 1 % is five orders
// of magnitude above the rounding of the dozen operations involved (p +- h included: h >= 2e-4 |p.x|, an ulp of p.x is 6e-8 |p.x|).
// A body outside [p - h, p + h], h = 1.01 H, in either coordinate is one agents_apart would have culled: the box culls nothing
// that the rule folds.  An agent at rest is apart from every body at rest (agents_apart's last term): an empty box.  An h that is
// NaN (a NaN pose or velocity) makes the box the whole plane; an infinite one does by itself.  The union of the agents' boxes is
// taken with < alone, which rounds nothing: a body outside the union is outside every agent's own box.
// A MOVING body is not put to the box - agents_apart's reach then depends on the pair's relative velocity - but to agents_apart itself.
struct BodyBox { float x0, y0, x1, y1; };
__host__ __device__ inline BodyBox body_box(const float4 tk, const float agent_radius) {
    const float ax = fabsf(tk.z), ay = fabsf(tk.w);
    if ((ax == 0.f) & (ay == 0.f)) return BodyBox{INFINITY, INFINITY, -INFINITY, -INFINITY};
    const float v_up = ax + ay, v_lo = fmaxf(ax, ay);
    const float r2 = 1.001f*2.002f*agent_radius;
    const float kq = 1.f + 1.0001e-6f/v_lo;
    const float B = 1.02f*(kq*kq*(1.0102f*v_up + r2) + kq*r2) + 1e-3f;
    const float h = 1.01f*(B + 2e-4f*(fabsf(tk.x) + fabsf(tk.y)));
    BodyBox b{tk.x - h, tk.y - h, tk.x + h, tk.y + h};
    if (!(h == h) || !(b.x0 == b.x0) || !(b.y0 == b.y0) || !(b.x1 == b.x1) || !(b.y1 == b.y1)) b = BodyBox{-INFINITY, -INFINITY, INFINITY, INFINITY};
    return b;
}
__host__ __device__ inline bool body_outside(const BodyBox& b, const float2 q) {
    return (q.x < b.x0) | (q.x > b.x1) | (q.y < b.y0) | (q.y > b.y1);
}

// ONE WAVEFRONT PER ENV, a lane an agent (n_agents <= 64): physics_slide_kernel's frame with one pass.  The other agents one
// ordered pair a lane; the walls from the agents' near lists, laid end to end and dealt a (row, agent) pair to a lane - more than
// 64 of them culled first and compacted in the LDS pair list - or, where a list does not cover an agent, every static row of the env.
// THE BODIES' PASS: the lanes stride the slots lane + 64 j with one 8-byte load each (and the velocity's).  A stride without a
// present body costs a ballot.  A present body at rest is put to the union of the agents' reach boxes - made once a wave, on
// the first stride that has a body, by six rounds of shuffles - one compare a body; what is left is tested against each agent
// by agents_apart, the agents at uniform LDS addresses, and the surviving (body, agent) pairs go into the SAME pair list as the
// walls, BODY_TAG in the tag, so that collision_cc's divides and square roots run over full lanes; meet() dispatches by the tag.
// The list drains when a chunk more could overflow, and once at the end.  A contact folds x by fold_least, the agent's key by a
// 64-bit LDS atomicMin, and its count by an integer LDS atomic - one for the wave where all its lanes' pairs are one agent's.
template <int MOVE, int EXTRA>
__global__ __launch_bounds__(WAVE) void physics_bodies_kernel(
        const MsScenery sc, const AgentsK ag, float* __restrict__ progress, const float agent_radius, const float fps,
        const MsMovement mv, const MsStepExtras ex, const MsBodies bd, const Divisor by_a, const FanSort fs) {
    __shared__ float4 s_task[WAVE];              // per agent: (p, v/fps)
    __shared__ float s_reach2[WAVE];
    __shared__ unsigned s_prog[WAVE];            // the fold of x, as bits
    __shared__ unsigned long long s_key[WAVE];   // the least (bits(c_k), k) over the agent's bodies
    __shared__ int s_contacts[WAVE];
    __shared__ float4 s_wall[PHYS_PAIRS];        // a row, or a body's (p, u)
    __shared__ int s_tag[PHYS_PAIRS];
    // (the fan schedule's sort waves: the launch's first blocks, as physics_kernel's)
    if ((int)blockIdx.x < fs.n_blocks) {
        fan_sort_wave(fs, blockIdx.x, threadIdx.x, s_tag);
        return;
    }
    const int A = sc.n_agents, AF = sc.n_agents*sc.n_model;              // A <= WAVE (ms_bodies_physics)
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
    float my_reach = 0.f;
    if (mine) {
        const StepTask t = step_task(my_p, p2(my_v.x, my_v.y)/fps, agent_radius);
        my_reach = t.reach;
        s_reach2[lane] = t.reach2;
        s_task[lane] = t.tk;
        s_prog[lane] = f_bits(1.f);
        s_key[lane] = BODY_NO_KEY;
        s_contacts[lane] = 0;
    }
    auto task_of = [&](const int t) { return StepTask{s_task[t], 0.f, s_reach2[t]}; };
    // one pair of the lanes that have one (every lane of the wave comes here): a static row against agent `tag`, or - BODY_TAG -
    // body (tag >> 6) & 1023 against agent tag & 63, behind the culls both
    auto meet = [&](const bool has, const float4 u, const int tag) {
        const int t = tag & (WAVE - 1);
        bool hit = false;
        if (has) {
            if (tag & BODY_TAG) {
                const float c = body_meet(s_task[t], u, agent_radius);
                hit = c < 1.f;
                if (hit) {
                    atomicMin(&s_prog[t], f_bits(c));
                    atomicMin(&s_key[t], body_key(c, (tag >> 6) & (BODY_MAX_SLOTS - 1)));
                }
            } else fold_least(&s_prog[t], meet_wall(1.f, task_of(t), u, agent_radius));
        }
        if (bd.contacts) {
            const unsigned long long m = __ballot(hit);
            if (m) {
                // (one agent: every hit of the wave is agent 0's - one add for the wave)
                if (A == 1) { if (lane == 0) s_contacts[0] += __popcll(m); }
                else if (hit) atomicAdd(&s_contacts[t], 1);
            }
        }
    };
    PairList pairs{s_wall, s_tag, PHYS_PAIRS, 0};
    auto flush = [&]() { pairs.drain(lane, meet); };
    wave_sync();
    // the env's other agents (kernels.cu:193-200), one ordered pair per lane, at their start-of-step (p, u)
    for (int i0 = 0; i0 < A*A; i0 += WAVE) {
        const int q = i0 + lane;
        const int t = min(div_by(q, by_a), A - 1), d1 = q - t*A;
        if (q < A*A && d1 != t) fold_least(&s_prog[t], meet_agent(1.f, task_of(t), s_task[d1], agent_radius));
    }
    // the static rows: the agents' near lists laid end to end, if every agent is covered by its own (physics_slide_kernel's walk)
    bool swept = true;
    if (env.gridded) {
        NearList nl{true, 0, 0u, nullptr};
        if (mine) nl = near_list(sc, env.geom, env.wg_start, s_task[lane].x, s_task[lane].y, my_reach);
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
                if (P <= WAVE) meet(q < P, u, t);
                else pairs.append(lane, q < P && !wall_beyond(s_task[t], u, s_reach2[t]), u, t, flush);
            }
        }
    }
    if (swept) {
        // (plain: every static row of the env, a lane a row, to every agent - meet() has the cull)
        for (int l0 = AF; l0 < env.L; l0 += WAVE) {
            const bool row = l0 + lane < env.L;
            const float4 u = row ? env.ln[l0 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
            for (int t = 0; t < A; t++) meet(row, u, t);
        }
    }
    // the bodies (the walls' pairs still listed wait in the list for the first drain)
    {
        const int P = bd.n_slots;
        const float2* __restrict__ slots = reinterpret_cast<const float2*>(bd.positions) + (size_t)n*P;
        BodyBox all{INFINITY, INFINITY, -INFINITY, -INFINITY};
        bool boxed = false;
        for (int k0 = 0; k0 < P; k0 += WAVE) {
            const int k = k0 + lane;
            const float2 q = (k < P) ? slots[k] : make_float2(NAN, NAN);
            bool near = body_present(q);
            if (!__ballot(near)) continue;                               // (an empty stride - an empty store: a ballot)
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (near) o = body_other(q, bd.velocities, (size_t)n*P + k, fps);
            if (!boxed) {
                // the union of the agents' reach boxes, once a wave: lane = agent, then six rounds of shuffles
                if (mine) all = body_box(s_task[lane], agent_radius);
                #pragma unroll
                for (int s = 1; s < WAVE; s <<= 1) {
                    const float x0 = __shfl_xor(all.x0, s, WAVE), y0 = __shfl_xor(all.y0, s, WAVE);
                    const float x1 = __shfl_xor(all.x1, s, WAVE), y1 = __shfl_xor(all.y1, s, WAVE);
                    all.x0 = x0 < all.x0 ? x0 : all.x0; all.y0 = y0 < all.y0 ? y0 : all.y0;
                    all.x1 = x1 > all.x1 ? x1 : all.x1; all.y1 = y1 > all.y1 ? y1 : all.y1;
                }
                boxed = true;
            }
            near = near && !(((o.z == 0.f) & (o.w == 0.f)) && body_outside(all, q));
            if (!__ballot(near)) continue;
            for (int t = 0; t < A; t++)
                pairs.append(lane, near && !agents_apart(s_task[t], o, agent_radius), o, BODY_TAG | (k << 6) | t, flush);
        }
    }
    if (pairs.cnt) flush();
    wave_sync();
    if (mine) {
        const float x = bits_f(s_prog[lane]);
        float2 p = my_p, v = my_v;
        float w_ = my_w, ang = my_ang;
        bool changed = integrate(x, fps, p, ang, v, w_);                 // (a velocity only changes on a collision)
        if constexpr (EXTRA == 1) {
            if (respawns_after(ex, i)) {
                spawn_pose(ex, i, p, ang);
                v = make_float2(0.f, 0.f); w_ = 0.f;
                changed = true;
            }
        }
        step_store(ag, ex, i, p, ang, v, w_, changed, EXTRA == 1);
        progress[i] = x;
        if (bd.blocker) bd.blocker[i] = body_blocker(s_key[lane], x);
        if (bd.contacts) bd.contacts[i] = s_contacts[lane];
    }
}

// The rule for whole envs, serially (ms_host_bodies): the same functions; every agent meets every other agent, every static row
// of its env and every present body, each behind its own reach cull and nothing else - no grid, no box.  `walls`, `wall_starts`
// and the other pointers: as slide_serial's.
inline void bodies_serial(const float* walls, const long long* wall_starts, const int N, const int A, const MsAgents& ag,
                          const MsMovement* mv, const MsStepExtras& ex, const bool extras, const MsBodies& bd, float* progress,
                          const float agent_radius, const float fps) {
    struct Agent { float2 p, v; float ang, w; StepTask t; };
    Agent* as = new Agent[A];
    const int P = bd.n_slots;
    for (int n = 0; n < N; n++) {
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
            me.t = step_task(me.p, p2(me.v.x, me.v.y)/fps, agent_radius);
        }
        for (int a = 0; a < A; a++) {
            const int i = n*A + a;
            Agent& me = as[a];
            float x = 1.f;
            for (int b = 0; b < A; b++)
                if (b != a) x = meet_agent(x, me.t, as[b].t.tk, agent_radius);
            for (long long l = wall_starts[n]; l < wall_starts[n + 1]; l++)
                x = meet_wall(x, me.t, make_float4(walls[4*l], walls[4*l + 1], walls[4*l + 2], walls[4*l + 3]), agent_radius);
            unsigned long long key = BODY_NO_KEY;
            int contacts = 0;
            for (int k = 0; k < P; k++) {
                const size_t at = (size_t)n*P + k;
                const float2 q = load2(bd.positions, at);
                if (!body_present(q)) continue;
                const float4 o = body_other(q, bd.velocities, at, fps);
                if (agents_apart(me.t.tk, o, agent_radius)) continue;
                const float c = body_meet(me.t.tk, o, agent_radius);
                if (c < 1.f) {
                    contacts++;
                    x = c < x ? c : x;
                    const unsigned long long mine = body_key(c, k);
                    key = mine < key ? mine : key;
                }
            }
            float2 p = me.p, v = me.v;
            float w = me.w, ang = me.ang;
            integrate(x, fps, p, ang, v, w);
            if (extras && respawns_after(ex, i)) {
                spawn_pose(ex, i, p, ang);
                v = make_float2(0.f, 0.f); w = 0.f;
            }
            store2(ag.positions, i, p);
            ag.angles[i] = ang;
            store2(ag.velocity, i, v);
            ag.angvelocity[i] = w;
            progress[i] = x;
            if (bd.blocker) bd.blocker[i] = body_blocker(key, x);
            if (bd.contacts) bd.contacts[i] = contacts;
            if (extras) imu_store(ex, i, ang, v, w);
        }
    }
    delete[] as;
}
