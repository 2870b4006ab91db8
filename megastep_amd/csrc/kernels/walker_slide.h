// kernels/walker_slide.h -- walker_slide_kernel<WIDE>: the walker tick with a second contact phase (MsWalkers' slide).
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, behind slide.h, whose contact
// rule it applies as it stands - slide_normal_wall, slide_normal_agent, slide_offer, slide_contact, slide_finish - and walker.h,
// whose steps 1 to 4 and whose frame it keeps); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// sliding walkers                                                             no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// A walker whose disc grazes a wall is stopped dead for the tick by walker_kernel, as an agent is by the plain step.  Here it gets
// the agents' cure (kernels/slide.h): phase A is walker_kernel's meet as it stands (x1 = `progress`, its class = `blocked`, bit for
// bit); the CONTACT picks, among the obstacles of any class whose own collision value IS x1, the normal the velocity runs into
// hardest; phase B deflects the velocity off it and spends the rest of the tick, 1 - x1, along it, stopped by the agents at rest,
// by the other walkers AS PHASE A LEFT THEM - (p1_j, u2_j), u2_j = 0 for one that does not slide - and by the walls.
//
// The agents' kernel folds x1 across lanes by atomics, knows it only afterwards and so walks the obstacles a second time for the
// blockers.  A walker's lane owns its walker and folds in registers, so ONE WALK serves phase A and the contact (WalkFold below): an
// obstacle whose value c is below the running x drops the best normal and offers its own, one with c == x offers its own, and a
// normal offered at value c is taken at p + c v/fps - slide_contact's own expression for p1 - so what is left at the end is
// exactly the offers of the obstacles with c == x1, each taken at p1.  The sqrtf and the divisions of a normal are paid on an
// improving or tying obstacle only.  offer_wall and offer_agent, the second walk's pieces, are not needed for it.
//
// Every piece below the kernel's schedule is __host__ __device__: ms_host_walkers sweeps them serially (walk_slide_env), so the CPU
// suite holds this very text to tests/walker_slide_rule.py, bit for bit.
//
//   walker_slide_kernel<false|true>   walker_kernel's frame: P <= 64 a wavefront an env, four envs a block, wave_sync only; beyond,
//                                     a workgroup an env, the slots tid + 256 j in registers.
//     snapshot, steer   walker_kernel's, statement for statement.
//     phase A           the uniform walk over the bodies' rows, then near_list / walk_rows, folding (key, best normal) in registers;
//                       slide_contact at once - what crosses the barrier is (p1, v', u2, r1) and the key, (p, v) die here.
//     anybody?          __syncthreads_or / a ballot: an env where nobody slides settles and leaves - the plain tick's outputs and
//                       slid = 0.  The same barrier is the one the overwrite needs: everyone has read (p, u).
//     second snapshot   a lane overwrites its own rows with (p1, u2); the agents' rows stay.  No new LDS.  A barrier / wave_sync.
//     phase B           the lanes that slide walk the rows again - meet_agent from (p1, u2) - and a FRESH near list taken at p1
//                       with the reach of u2; the others pass an empty covered list, walk_rows is called by every lane.
//     settle            slide_finish: the move, the velocity, slid, stopped.  No float atomics, no scratch.
struct WalkFold { unsigned key; SlideBest best; };                      // phase A's key, and the least normal among the obstacles AT its x

// where the walker of `t` stands at the fraction c of its step: slide_contact's p1, by slide_contact
__host__ __device__ inline P2 walk_at(const StepTask& t, const float2 v, const float c, const float fps) {
    const SlideContact at = slide_contact(make_float2(t.tk.x, t.tk.y), 0.f, v, 0.f, c, fps, SlideBest{0.f, 0.f, 0.f, 0}, 0.f);
    return p2(at.p1.x, at.p1.y);
}
// one obstacle's value c and class into the fold; normal(nx, ny): its normal (false: none to speak of), asked for only if it counts
template <class Normal>
__host__ __device__ inline void walk_slide_fold(WalkFold& f, const float c, const int cls, const float2 v, Normal&& normal) {
    const float x = walk_float(f.key >> 2);
    if (!(c < 1.f) || c > x) return;
    if (c < x) f.best.any = 0;
    float nx, ny;
    if (normal(nx, ny)) slide_offer(f.best, v, nx, ny);
    f.key = walk_fold(f.key, c, cls);
}
// walk_meet_bodies with the contact beside it: body(i) is the row (p, u) of body i, bump(a) as there
template <class Body, class Bump>
__host__ __device__ inline WalkFold walk_slide_bodies(const WalkArgs& q, const int k, const StepTask& task, const float2 v, Body&& body, Bump&& bump) {
    const int A = q.n_agents, B = A + q.n_slots;
    WalkFold f{walk_key(1.f, 0), SlideBest{0.f, 0.f, 0.f, 0}};
    for (int i = 0; i < B; i++) {
        const float4 o = body(i);
        if (i == A + k || !item_present(o.x, o.y)) continue;
        const float c = meet_agent(1.f, task, o, q.agent_radius);
        walk_slide_fold(f, c, i < A ? 1 : 2, v, [&](float& nx, float& ny) {
            return slide_normal_agent(walk_at(task, v, c, q.fps), p2(o.x, o.y), p2(o.z, o.w), c, nx, ny); });
        if (i < A && c < 1.f) bump(i);
    }
    return f;
}
__host__ __device__ inline void walk_slide_wall(WalkFold& f, const WalkArgs& q, const StepTask& task, const float2 v, const float4 row) {
    const float c = meet_wall(1.f, task, row, q.agent_radius);
    walk_slide_fold(f, c, 3, v, [&](float& nx, float& ny) { return slide_normal_wall(walk_at(task, v, c, q.fps), row, nx, ny); });
}
__host__ __device__ inline SlideContact walk_slide_contact(const WalkArgs& q, const P2 p, const float2 v, const WalkFold& f) {
    return slide_contact(make_float2(p.x, p.y), 0.f, v, 0.f, walk_float(f.key >> 2), q.fps, f.best, q.bounce);
}
// phase B's pair tests of walker k: body(i) is the row phase A left, (p1, u2) - an agent's, and a walker's that does not slide: u2 = 0
template <class Body>
__host__ __device__ inline float walk_slide_meet(const WalkArgs& q, const int k, const StepTask& task, Body&& body) {
    const int A = q.n_agents, B = A + q.n_slots;
    float x = 1.f;
    for (int i = 0; i < B; i++) {
        const float4 o = body(i);
        if (i == A + k || !item_present(o.x, o.y)) continue;
        x = meet_agent(x, task, o, q.agent_radius);
    }
    return x;
}
// slid and stopped of slot `at`
__host__ __device__ inline void walk_slide_records(const WalkArgs& q, const long long at, const bool present, const float slid, const bool stopped) {
    if (q.slid) q.slid[at] = present ? slid : NAN;
    if (q.stopped) q.stopped[at] = present ? (unsigned char)(stopped ? 1 : 0) : (unsigned char)4;
}
// Slot `at` after its tick: slide_finish - the move, the velocity - the stores, every record (an absent slot: the records alone).
__host__ __device__ inline void walk_slide_settle(const WalkArgs& q, const long long at, const bool present, const SlideContact& con,
                                                  const float x2, const unsigned key) {
    float slid = 0.f;
    bool stopped = false;
    if (present) {
        float2 p, v = con.v2;                                           // (nothing blocked it: slide_contact left v here)
        float ang, w = 0.f;
        stopped = slide_finish(con, x2, q.fps, p, ang, v, w, slid);
        store2(q.positions, (size_t)at, p);
        store2(q.velocities, (size_t)at, v);
    }
    if (q.progress) q.progress[at] = present ? walk_float(key >> 2) : NAN;
    if (q.blocked) q.blocked[at] = present ? (unsigned char)(key & 3u) : (unsigned char)4;
    walk_slide_records(q, at, present, slid, stopped);
}

// Steps 5 on of one env on host arrays, serially, behind walkers_serial's steps 1 to 4: `body` holds the rows (p, u), v the tick's
// velocities; rows: the env's static rows.
inline void walk_slide_env(const WalkArgs& q, const int n, std::vector<float4>& body, const std::vector<P2>& v, const float4* rows,
                           const long long n_rows) {
    const int A = q.n_agents, P = q.n_slots;
    std::vector<SlideContact> con((size_t)P);
    std::vector<unsigned> key((size_t)P, 0u);
    const auto present = [&](const int k) { return item_present(body[(size_t)(A + k)].x, body[(size_t)(A + k)].y); };
    for (int k = 0; k < P; k++) {
        if (!present(k)) continue;
        const float4 me = body[(size_t)(A + k)];
        const float2 vk = make_float2(v[(size_t)k].x, v[(size_t)k].y);
        const StepTask task = step_task(make_float2(me.x, me.y), p2(me.z, me.w), q.agent_radius);
        WalkFold f = walk_slide_bodies(q, k, task, vk, [&](const int i) { return body[(size_t)i]; },
                                       [&](const int a) { if (q.bumps) q.bumps[(long long)n*A + a]++; });
        for (long long l = 0; l < n_rows; l++) walk_slide_wall(f, q, task, vk, rows[l]);
        key[(size_t)k] = f.key;
        con[(size_t)k] = walk_slide_contact(q, p2(me.x, me.y), vk, f);
    }
    for (int k = 0; k < P; k++) {                                       // (phase A read the rows as the tick found them)
        if (present(k)) body[(size_t)(A + k)] = make_float4(con[(size_t)k].p1.x, con[(size_t)k].p1.y, con[(size_t)k].u2.x, con[(size_t)k].u2.y);
    }
    for (int k = 0; k < P; k++) {
        const SlideContact& c = con[(size_t)k];
        float x2 = 1.f;
        if (present(k) && c.slides) {
            const StepTask task = step_task(c.p1, p2(c.u2.x, c.u2.y), q.agent_radius);
            x2 = walk_slide_meet(q, k, task, [&](const int i) { return body[(size_t)i]; });
            for (long long l = 0; l < n_rows; l++) x2 = meet_wall(x2, task, rows[l], q.agent_radius);
        }
        walk_slide_settle(q, (long long)n*P + k, present(k), c, x2, key[(size_t)k]);
    }
}

template <bool WIDE>
__global__ __launch_bounds__(WG) void walker_slide_kernel(const MsScenery sc, const WalkArgs q) {
    constexpr int PER = WIDE ? WALK_PER : 1, ENVS = WIDE ? 1 : WAVES, STRIDE = WIDE ? WG : WAVE;
    constexpr int ROWS = WALK_MAX_AGENTS + (WIDE ? WALK_MAX_SLOTS : WAVE);
    __shared__ float4 s_bodies[ENVS][ROWS];                             // (p, u) in phase A, (p1, u2) in phase B: the agents, then the slots
    __shared__ int s_counts[ENVS][2][WALK_MAX_AGENTS];                  // bumps, close
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int part = WIDE ? 0 : wave;
    const int n = WIDE ? (int)blockIdx.x : (int)blockIdx.x*WAVES + wave;
    if (!WIDE && n >= q.n_envs) return;                                 // (a whole wave, and this instantiation has no workgroup barrier)
    const int t0 = WIDE ? tid : lane;
    const int A = q.n_agents, P = q.n_slots, AF = A*sc.n_model;
    float4* const s_body = s_bodies[part];
    int* const s_bumps = s_counts[part][0];
    int* const s_close = s_counts[part][1];
    auto sync = [] { if constexpr (WIDE) __syncthreads(); else wave_sync(); };
    auto anybody = [](const bool mine) {                                // (uniform, and a barrier / wave_sync)
        if constexpr (WIDE) return __syncthreads_or(mine) != 0;
        else { const bool some = __ballot(mine) != 0ull; wave_sync(); return some; }
    };
    auto counts = [&](const bool zero) {
        if (t0 < A) {
            if (q.bumps) q.bumps[(long long)n*A + t0] = zero ? 0 : s_bumps[t0];
            if (q.close) q.close[(long long)n*A + t0] = zero ? 0 : s_close[t0];
        }
    };
    const SlideContact nobody{make_float2(0.f, 0.f), make_float2(0.f, 0.f), make_float2(0.f, 0.f), 0.f, 0.f, false, false};

    if (q.reset && q.reset[n]) {                                        // (uniform over the env's lanes, before any barrier)
        for (int k = t0; k < P; k += STRIDE) {
            walk_wipe(q, (long long)n*P + k);
            walk_slide_records(q, (long long)n*P + k, false, 0.f, false);
        }
        counts(true);
        return;
    }

    // snapshot: the agents at rest, the slots as the store holds them; a lane keeps its slots' state
    P2 p[PER], v[PER];
    bool here[PER], any = false;
    #pragma unroll
    for (int j = 0; j < PER; j++) {
        const int k = t0 + j*STRIDE;
        p[j] = v[j] = p2(0.f, 0.f);
        here[j] = false;
        if (k < P) {
            const size_t at = (size_t)n*P + k;
            const float2 pp = load2(q.positions, at);
            here[j] = item_present(pp.x, pp.y);
            p[j] = p2(pp.x, pp.y);
            if (here[j]) { const float2 vv = load2(q.velocities, at); v[j] = p2(vv.x, vv.y); }
            s_body[A + k] = make_float4(pp.x, pp.y, 0.f, 0.f);
        }
        any |= here[j];
    }
    if (t0 < A) {
        const float2 pa = load2(q.agent_positions, (size_t)n*A + t0);
        s_body[t0] = make_float4(pa.x, pa.y, 0.f, 0.f);
        s_bumps[t0] = 0; s_close[t0] = 0;
    }
    if (!anybody(any)) {                                                // nobody walks here: the records, and done
        for (int k = t0; k < P; k += STRIDE) walk_slide_settle(q, (long long)n*P + k, false, nobody, 1.f, 0u);
        counts(true);
        return;
    }

    // steer, keep apart, blend: the positions' halves of the rows, at a uniform index
    #pragma unroll
    for (int j = 0; j < PER; j++) {
        const int k = t0 + j*STRIDE;
        if (here[j]) {
            const size_t at = (size_t)n*P + k;
            const float2 t = load2(q.towards, at);
            v[j] = walk_velocity(q, k, p[j], p2(t.x, t.y), q.speeds[at], v[j],
                                 [&](const int i) { return reinterpret_cast<const float2*>(s_body + i)[0]; },
                                 [&](const int a) { atomicAdd(&s_close[a], 1); });
            const P2 u = v[j]/q.fps;
            reinterpret_cast<float2*>(s_body + A + k)[1] = make_float2(u.x, u.y);
        }
    }
    sync();

    // phase A and the contact in one walk: the bodies' whole rows, then the walls
    const EnvRows e = env_rows(sc, n);
    SlideContact con[PER];
    unsigned key[PER];
    bool slides = false;
    #pragma unroll
    for (int j = 0; j < PER; j++) {
        const int k = t0 + j*STRIDE;
        const float2 vj = make_float2(v[j].x, v[j].y);
        WalkFold f{walk_key(1.f, 0), SlideBest{0.f, 0.f, 0.f, 0}};
        StepTask task{make_float4(0.f, 0.f, 0.f, 0.f), 0.f, 0.f};
        NearList nl{true, 0, 0u, nullptr};                              // (no walker: covered, by an empty list)
        if (here[j]) {
            const float4 me = s_body[A + k];
            task = step_task(make_float2(me.x, me.y), p2(me.z, me.w), q.agent_radius);
            f = walk_slide_bodies(q, k, task, vj, [&](const int i) { return s_body[i]; }, [&](const int a) { atomicAdd(&s_bumps[a], 1); });
            nl = near_list(sc, e, make_float2(me.x, me.y), task.reach);
        }
        walk_rows(nl, e, AF, [&](const float4 row) { walk_slide_wall(f, q, task, vj, row); });
        key[j] = f.key;
        con[j] = here[j] ? walk_slide_contact(q, p[j], vj, f) : nobody;
        slides |= con[j].slides;
    }
    if (!anybody(slides)) {                                             // the plain tick's outputs, and slid = 0
        #pragma unroll
        for (int j = 0; j < PER; j++) {
            const int k = t0 + j*STRIDE;
            if (k < P) walk_slide_settle(q, (long long)n*P + k, here[j], con[j], 1.f, key[j]);
        }
        counts(false);
        return;
    }

    // the second snapshot: everyone has read (p, u); a lane's own rows become (p1, u2)
    #pragma unroll
    for (int j = 0; j < PER; j++) {
        const int k = t0 + j*STRIDE;
        if (here[j]) s_body[A + k] = make_float4(con[j].p1.x, con[j].p1.y, con[j].u2.x, con[j].u2.y);
    }
    sync();

    // phase B: the rows again and a fresh near list at p1, for the lanes that slide; settle
    #pragma unroll
    for (int j = 0; j < PER; j++) {
        const int k = t0 + j*STRIDE;
        float x2 = 1.f;
        StepTask task{make_float4(0.f, 0.f, 0.f, 0.f), 0.f, 0.f};
        NearList nl{true, 0, 0u, nullptr};                              // (no slide: covered, by an empty list)
        if (con[j].slides) {
            task = step_task(con[j].p1, p2(con[j].u2.x, con[j].u2.y), q.agent_radius);
            x2 = walk_slide_meet(q, k, task, [&](const int i) { return s_body[i]; });
            nl = near_list(sc, e, con[j].p1, task.reach);
        }
        walk_rows(nl, e, AF, [&](const float4 row) { x2 = meet_wall(x2, task, row, q.agent_radius); });
        if (k < P) walk_slide_settle(q, (long long)n*P + k, here[j], con[j], x2, key[j]);
    }
    counts(false);
}
