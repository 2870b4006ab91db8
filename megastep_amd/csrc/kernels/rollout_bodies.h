// kernels/rollout_bodies.h -- rollout_bodies_kernel: candidate action plans rolled through the step among bodies, a lane a plan.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, behind rollout.h, whose frame it
// keeps, and bodies.h, whose per-pair functions it calls); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// rollouts among bodies                                (MsRolloutBodies; no counterpart in the reference)
// ------------------------------------------------------------------------------------------------
// The rule is MsRollouts' with others 0 or 1 and no slide, plus a store read as MsBodies reads it.  Body k is, at step h of every
// candidate, at q_k^h: q_k^0 its stored position, q_k^{h+1} = q_k^h + u_k - one binary32 addition a component a step - with
// u_k = body_other's velocity a step (v_k/fps, or (0, 0) without velocities or where v_k is not finite).  A BODY IS EXTRAPOLATED
// IN A STRAIGHT LINE AND IS STOPPED BY NOTHING - not walls, not agents, not other bodies: a forecast, as others = 'rest' is.
// Step h folds, after the other agents at rest and the static rows and from the same x, every present body: o = (q_k^h, u_k),
// passed over when agents_apart(task, o), else x = min(x, body_meet(task, o)) where that is < 1.  The rest is rollout_advance.
// body_stops counts the steps whose body_blocker(key, x) is not -1 - stopped by a body and by nothing nearer - and first_blocker
// is that blocker at the first of them.  Every c lies in [+0, 1] and the fold is a least value: the same bits on any path.

// a step's fold over the bodies as a candidate keeps it: the least x so far and the least (bits(c), k) of the contacts
struct BodyFold { float x; unsigned long long key; };
__host__ __device__ inline void body_fold(BodyFold& f, const float4 tk, const float4 o, const int k, const float agent_radius) {
    if (agents_apart(tk, o, agent_radius)) return;
    const float c = body_meet(tk, o, agent_radius);
    if (c < 1.f) {
        f.x = c < f.x ? c : f.x;
        const unsigned long long mine = body_key(c, k);
        f.key = mine < f.key ? mine : f.key;
    }
}
// the two books of the bodies for step h, from the step's final x and its least key
struct BodyBooks { int stops, first; };
__host__ __device__ inline void body_books(BodyBooks& bk, const BodyFold& f) {
    const int blocker = body_blocker(f.key, f.x);
    if (blocker >= 0) {
        if (bk.stops == 0) bk.first = blocker;
        bk.stops++;
    }
}

// ONE WAVEFRONT PER (AGENT, 64 CANDIDATES), a lane a candidate - rollout_kernel<0>'s frame: the state in registers for the whole
// horizon, the walls through near_list / walk_rows, the others at rest.  THE BODIES' SIDE:
//   stage    once: the wave strides the env's P slots and compacts the present ones, ascending, by ballot and prefix, into
//            dynamic LDS - (q, u) as a float4 and the slot index beside it, 20 bytes a slot.  A wave with no present body skips
//            everything below: its cost is the ballots.
//   box      per step, where a staged body is at rest: every lane makes body_box of its own task and the wave takes the union
//            by six rounds of shuffles, min and max by < alone.  The exactness argument above body_box holds word for word - a
//            lane here is an agent there; a dead lane rolls the last candidate again and adds a box that is already in.
//   walk     the wave strides the staged list a lane a body; a body at rest outside the union is dropped, a moving one never
//            (its reach depends on the pair's relative velocity).  The ballot of survivors is walked at a uniform index, the
//            body read from LDS as a broadcast, and every lane runs agents_apart and body_meet against its own task, keeping x
//            and its least key in registers: a lane is the only writer of its candidate - no atomics.
//   advance  with velocities: every lane adds u to the q of the staged bodies lane + 64 j, a wave_sync on either side.
// No scratch, no per-lane array, no global atomics, nothing allocated.  Dynamic LDS: 20 n_slots bytes (ms_rollouts_bodies).
__global__ __launch_bounds__(WAVE) void rollout_bodies_kernel(
        const MsScenery sc, const AgentsK ag, const MsRollouts r, const MsRolloutBodies rb, const float agent_radius, const float fps,
        const int groups, const Divisor by_g, const Divisor by_a) {
    extern __shared__ float4 s_body[];                                   // n_slots (q, u), then n_slots slot indices
    const int lane = threadIdx.x;
    const RolloutLane b = rollout_bind(r, sc.n_agents, blockIdx.x, lane, groups, by_g, by_a);
    if (r.mask && !r.mask[b.row]) return;                                // (uniform: the agent is not rolled, its rows stay)
    const int A = sc.n_agents, AF = sc.n_agents*sc.n_model, H = r.horizon, P = rb.n_slots;
    int* const s_slot = reinterpret_cast<int*>(s_body + P);
    const EnvRows env = env_rows(sc, b.n);
    const float2* __restrict__ pos2 = reinterpret_cast<const float2*>(ag.positions);

    // stage: the env's present bodies, ascending; M of them, `resting` where one of them stands still
    int M = 0;
    bool resting = false;
    {
        const float2* __restrict__ slots = reinterpret_cast<const float2*>(rb.positions) + (size_t)b.n*P;
        for (int k0 = 0; k0 < P; k0 += WAVE) {
            const int k = k0 + lane;
            const float2 q = (k < P) ? slots[k] : make_float2(NAN, NAN);
            const bool present = body_present(q);
            const unsigned long long m = __ballot(present);
            if (!m) continue;
            bool still = false;
            if (present) {
                const float4 o = body_other(q, rb.velocities, (size_t)b.n*P + k, fps);
                const int at = M + __popcll(m & ((1ull << lane) - 1ull));     // (at <= k < P)
                s_body[at] = o;
                s_slot[at] = k;
                still = (o.z == 0.f) & (o.w == 0.f);
            }
            resting = resting || __ballot(still) != 0ull;
            M += __popcll(m);
        }
        wave_sync();
    }

    RolloutState st = rollout_start(ag, b.row, H);
    BodyBooks books{0, -1};
    const ActionTable table(r.table, r.n_actions, lane);
    float2* __restrict__ trail = reinterpret_cast<float2*>(r.trail);
    long long act = b.plan[0];
    for (int h = 0; h < H; h++) {
        const long long next = b.plan[min(h + 1, H - 1)];                // (asked for a step ahead)
        float dx, dy, dw;
        table.delta(action_row(act, r.n_actions), dx, dy, dw);
        move_velocity(r.keep, st.ang, dx, dy, dw, st.v, st.w);
        const StepTask t = rollout_task(st, agent_radius, fps);
        // the others at rest, then the near list of the cell the candidate stands in, or the env's static rows: rollout_kernel<0>'s
        BodyFold f{1.f, BODY_NO_KEY};
        if (r.others) {
            for (int o = 0; o < A; o++) {
                if (o != b.a) f.x = meet_agent(f.x, t, at_rest(pos2[b.n*A + o]), agent_radius);
            }
        }
        walk_rows(near_list(sc, env, st.p, t.reach), env, AF, [&](const float4 u) { f.x = meet_wall(f.x, t, u, agent_radius); });
        if (M) {
            BodyBox all{INFINITY, INFINITY, -INFINITY, -INFINITY};
            if (resting) {
                all = body_box(t.tk, agent_radius);
                #pragma unroll
                for (int s = 1; s < WAVE; s <<= 1) {
                    const float x0 = __shfl_xor(all.x0, s, WAVE), y0 = __shfl_xor(all.y0, s, WAVE);
                    const float x1 = __shfl_xor(all.x1, s, WAVE), y1 = __shfl_xor(all.y1, s, WAVE);
                    all.x0 = x0 < all.x0 ? x0 : all.x0; all.y0 = y0 < all.y0 ? y0 : all.y0;
                    all.x1 = x1 > all.x1 ? x1 : all.x1; all.y1 = y1 > all.y1 ? y1 : all.y1;
                }
            }
            for (int j0 = 0; j0 < M; j0 += WAVE) {
                const int j = j0 + lane;
                bool near = j < M;
                if (near) {
                    const float4 o = s_body[j];
                    near = !(((o.z == 0.f) & (o.w == 0.f)) && body_outside(all, make_float2(o.x, o.y)));
                }
                for (unsigned long long m = __ballot(near); m; m &= m - 1ull) {
                    const int at = j0 + __builtin_ctzll(m);              // (uniform: a broadcast read; at < M <= P)
                    body_fold(f, t.tk, s_body[at], s_slot[at], agent_radius);
                }
            }
        }
        rollout_advance(st, f.x, fps, h);
        body_books(books, f);
        if (trail && b.live) trail[b.cand*H + h] = st.p;
        if (rb.velocities && M && h + 1 < H) {
            wave_sync();
            for (int j = lane; j < M; j += WAVE) {
                float4 o = s_body[j];
                o.x = o.x + o.z; o.y = o.y + o.w;
                s_body[j] = o;
            }
            wave_sync();
        }
        act = next;
    }
    if (b.live) {
        rollout_store(r, b.cand, st);
        if (rb.body_stops) rb.body_stops[b.cand] = books.stops;
        if (rb.first_blocker) rb.first_blocker[b.cand] = books.first;
    }
}

// The rule for ONE env, serially (ms_host_rollouts_bodies): rollout_serial's statement of a plain step plus the body loop, the
// same functions in the same order; every candidate meets every wall and every present body, each behind its own cull - no box.
inline void rollout_bodies_serial(const float* walls, const int n_walls, const MsAgents& ag, const int A, const MsRollouts& r,
                                  const MsRolloutBodies& rb, const float agent_radius, const float fps) {
    const int K = r.n_candidates, H = r.horizon, P = rb.n_slots;
    std::vector<float4> bodies(P);                                        // (q_k^h, u_k) of the present slots ...
    std::vector<int> slot(P);                                             // ... and which they are
    for (int a = 0; a < A; a++) {
        if (r.mask && !r.mask[a]) continue;
        for (int k = 0; k < K; k++) {
            int M = 0;
            for (int s = 0; s < P; s++) {
                const float2 q = load2(rb.positions, s);
                if (!body_present(q)) continue;
                bodies[M] = body_other(q, rb.velocities, s, fps);
                slot[M++] = s;
            }
            RolloutState st = rollout_start(ag, a, H);
            BodyBooks books{0, -1};
            const long long* plan = r.actions + ((r.shared_plans ? (size_t)0 : (size_t)a*K) + k)*H;
            const size_t cand = (size_t)a*K + k;
            for (int h = 0; h < H; h++) {
                const int c = action_row(plan[h], r.n_actions);
                move_velocity(r.keep, st.ang, r.table[3*c], r.table[3*c + 1], r.table[3*c + 2], st.v, st.w);
                const StepTask t = rollout_task(st, agent_radius, fps);
                BodyFold f{1.f, BODY_NO_KEY};
                for (int o = 0; r.others && o < A; o++) {
                    if (o != a) f.x = meet_agent(f.x, t, at_rest(load2(ag.positions, o)), agent_radius);
                }
                for (int l = 0; l < n_walls; l++)
                    f.x = meet_wall(f.x, t, make_float4(walls[4*l], walls[4*l + 1], walls[4*l + 2], walls[4*l + 3]), agent_radius);
                for (int j = 0; j < M; j++) body_fold(f, t.tk, bodies[j], slot[j], agent_radius);
                rollout_advance(st, f.x, fps, h);
                body_books(books, f);
                if (r.trail) store2(r.trail, cand*H + h, st.p);
                for (int j = 0; rb.velocities && j < M; j++) { bodies[j].x = bodies[j].x + bodies[j].z; bodies[j].y = bodies[j].y + bodies[j].w; }
            }
            rollout_store(r, cand, st);
            if (rb.body_stops) rb.body_stops[cand] = books.stops;
            if (rb.first_blocker) rb.first_blocker[cand] = books.first;
        }
    }
}
