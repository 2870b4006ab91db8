// kernels/walker.h -- walker_kernel<WIDE>.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after projectile.h: a walker is
// moved by step.h's step_task, meet_agent, meet_wall, near_list, walk_rows and integrate - the agents' own contact rule - and
// presence is items.h's item_present); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// walkers: bodies that steer, keep apart and stop at walls                    no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsWalkers) and DESIGN.md section 3.37.  A walker is a slot of an
// Items-shaped store - present exactly when both coordinates are finite - with a velocity and a preferred speed; its body is a disc
// of the agents' radius.  A call is one tick: steer towards a point, keep apart from the bodies near, meet the agents, the other
// walkers and the walls, move.  Everything a walker reads of another body is that body's state at the start of the tick (its
// position) or a function of such state alone (its displacement u of this tick): every output element has one writer, every sum
// has a stated order, and any schedule gives the same bits.  tests/walker_rule.py restates all of it in numpy.
//
// The pieces below the kernel's schedule - walk_steer, walk_apart, walk_blend, walk_velocity, walk_key, walk_meet_bodies,
// walk_wall, walk_settle, walk_wipe - are __host__ __device__: ms_host_walkers sweeps them serially over host arrays, so the CPU
// suite holds this very text to the rule, bit for bit.
//
//   walker_kernel<false>   P <= 64: one WAVEFRONT an env, a lane a walker, four envs a block of 256 - and no workgroup barrier
//                          anywhere: a wave's rows of LDS are its own, ordered by wave_sync.  (The common shape is 8 to 32
//                          walkers an env; a workgroup an env would idle three waves in four.)
//   walker_kernel<true>    P > 64: one WORKGROUP an env, a lane the slots tid + 256 j, their state in registers across the barriers.
//     snapshot  the bodies' (p.x, p.y, u.x, u.y) go into LDS as float4, the agents first (at rest: u = 0), then the slots.
//     steer     every lane walks the bodies at a UNIFORM index - the LDS reads are broadcasts, of the position's 8 bytes only - and
//               skips its own row by index; the sqrtf stays behind the range test.  It leaves its u in the other 8 bytes of its own
//               row (nobody reads those before the barrier / wave_sync that follows: the next phase needs everyone's u).
//     pairs     the same uniform walk over whole rows, agents_apart in front of collision_cc (meet_agent).
//     walls     near_list / walk_rows: the near list of the walker's cell where its reach is covered, the env's static rows
//               otherwise and always without a wall grid - physics' own exact cull, so both give the same bits.
//     fold      x and `blocked` are ONE unsigned key, bits(x) << 2 | class: x lies in [+0, 1], where the unsigned order is the
//               float order and the bits stay below 2^30, so a lane's running minimum of the key is the rule's tie-break.
//     counts    bumps and close through integer LDS atomics, stored whole.  An env with no present walker returns behind the
//               snapshot, its records written.  No float atomics, no scratch.
constexpr int WALK_MAX_SLOTS = 1024, WALK_MAX_AGENTS = 64;
constexpr int WALK_PER = WALK_MAX_SLOTS/WG;          // the slots a lane of the workgroup instantiation takes

struct WalkArgs {                                    // MsWalkers, checked
    float* positions;                                // (N, P, 2)
    float* velocities;                               // (N, P, 2)
    const float* speeds;                             // (N, P)
    const float* towards;                            // (N, P, 2)
    const unsigned char* reset;                      // (N,) or NULL
    const float* agent_positions;                    // (N, A, 2)
    float* progress;                                 // (N, P) or NULL
    unsigned char* blocked;                          // (N, P) or NULL
    int* bumps;                                      // (N, A) or NULL
    int* close;                                      // (N, A) or NULL
    int n_envs, n_agents, n_slots, agents_push;
    float personal, push, keep, fps, agent_radius;
    int slide;                                       // 1: walker_slide_kernel's tick (kernels/walker_slide.h) - the rest are its own
    float bounce;
    float* slid;                                     // (N, P) or NULL
    unsigned char* stopped;                          // (N, P) or NULL
};

__host__ __device__ inline unsigned walk_bits(const float x) { return __builtin_bit_cast(unsigned, x); }
__host__ __device__ inline float walk_float(const unsigned b) { return __builtin_bit_cast(float, b); }

// The preferred velocity: towards t at the preferred speed, no further than t within one tick.  A NaN in t: stand.  A NaN
// speed: NaN - walk_blend has the walker stand.
__host__ __device__ inline P2 walk_steer(const P2 p, const P2 t, const float speed, const float fps) {
    const P2 d = t - p;
    const float l = len(d);
    if (!(l > 0.f)) return p2(0.f, 0.f);
    const float s = l*fps;
    return d*(((s < speed) ? s : speed)/l);
}

// Is the body at o within `personal` of the walker at p (and not exactly on it)?  `add`: its push joins sep.
__host__ __device__ inline bool walk_apart(const P2 p, const P2 o, const float personal, const float push, const bool add, P2& sep) {
    const P2 r = p - o;
    const float l2 = len2(r);
    if (!((0.f < l2) & (l2 < personal*personal))) return false;
    if (add) {
        const float l = sqrtf(l2);
        sep = sep + r*((push*(personal - l))/(personal*l));
    }
    return true;
}

// The tick's velocity: pref + sep no longer than the preferred speed, blended into the stored one.  A velocity that does not come
// out finite - a stored NaN or infinity, a NaN speed, an infinite target - is (0, 0): the walker stands this tick.
__host__ __device__ inline P2 walk_blend(const P2 pref, const P2 sep, const float speed, const float keep, const P2 v_old) {
    P2 want = pref + sep;
    const float wl = len(want);
    if (wl > speed) want = want*(speed/wl);
    const float rest = 1.f - keep;
    const P2 v = p2(keep*v_old.x + rest*want.x, keep*v_old.y + rest*want.y);
    return (nav_finite(v.x) && nav_finite(v.y)) ? v : p2(0.f, 0.f);
}

// Steer, keep apart, blend for walker k at p: body(i) is the position of body i - the A agents, then the P slots - as the tick
// found it; close(a): agent a is within `personal`.  The order of the sum is the order of the bodies.
template <class Body, class Close>
__host__ __device__ inline P2 walk_velocity(const WalkArgs& q, const int k, const P2 p, const P2 t, const float speed, const P2 v_old,
                                            Body&& body, Close&& close) {
    const int A = q.n_agents, B = A + q.n_slots;
    P2 sep = p2(0.f, 0.f);
    for (int i = 0; i < B; i++) {
        const float2 o = body(i);
        if (i == A + k || !item_present(o.x, o.y)) continue;
        if (walk_apart(p, p2(o.x, o.y), q.personal, q.push, i >= A || q.agents_push, sep) && i < A) close(i);
    }
    return walk_blend(walk_steer(p, t, speed, q.fps), sep, speed, q.keep, v_old);
}

// x and the class of what gave it as one key; the least key is the least x, and among equal x the lowest class.
__host__ __device__ inline unsigned walk_key(const float x, const int cls) { return (walk_bits(x) << 2) | (unsigned)cls; }
__host__ __device__ inline unsigned walk_fold(const unsigned key, const float c, const int cls) {
    const unsigned mine = walk_key(c, cls);
    return (c < 1.f && mine < key) ? mine : key;
}

// The pair tests of walker k: body(i) is the whole row (p, u) of body i - an agent's u is 0, the call follows the agents' own
// step - and bump(a): the test with agent a gave a fraction below 1.
template <class Body, class Bump>
__host__ __device__ inline unsigned walk_meet_bodies(const WalkArgs& q, const int k, const StepTask& task, Body&& body, Bump&& bump) {
    const int A = q.n_agents, B = A + q.n_slots;
    unsigned key = walk_key(1.f, 0);
    for (int i = 0; i < B; i++) {
        const float4 o = body(i);
        if (i == A + k || !item_present(o.x, o.y)) continue;
        const float c = meet_agent(1.f, task, o, q.agent_radius);
        key = walk_fold(key, c, i < A ? 1 : 2);
        if (i < A && c < 1.f) bump(i);
    }
    return key;
}
__host__ __device__ inline unsigned walk_wall(const unsigned key, const StepTask& task, const float4 row, const float agent_radius) {
    return walk_fold(key, meet_wall(1.f, task, row, agent_radius), 3);
}

// Slot `at` = n P + k after its tick: the move - integrate's own expressions - the stores, the records.
__host__ __device__ inline void walk_settle(const WalkArgs& q, const long long at, const bool present, const P2 p, const P2 v, const unsigned key) {
    if (present) {
        float2 p_ = make_float2(p.x, p.y), v_ = make_float2(v.x, v.y);
        float ang = 0.f, w = 0.f;
        integrate(walk_float(key >> 2), q.fps, p_, ang, v_, w);
        store2(q.positions, (size_t)at, p_);
        store2(q.velocities, (size_t)at, v_);
    }
    if (q.progress) q.progress[at] = present ? walk_float(key >> 2) : NAN;
    if (q.blocked) q.blocked[at] = present ? (unsigned char)(key & 3u) : (unsigned char)4;
}

// An env being emptied: slot `at`.
__host__ __device__ inline void walk_wipe(const WalkArgs& q, const long long at) {
    store2(q.positions, (size_t)at, make_float2(NAN, NAN));
    if (q.progress) q.progress[at] = NAN;
    if (q.blocked) q.blocked[at] = 4;
}

// One whole call on host arrays, serially: `walls` holds every env's STATIC rows, env n's from wall_starts[n] on.  With q.slide the
// meet and the move are kernels/walker_slide.h's, which adds its records to an emptied env's and an absent slot's.
__host__ __device__ inline void walk_slide_records(const WalkArgs& q, long long at, bool present, float slid, bool stopped);
inline void walk_slide_env(const WalkArgs& q, int n, std::vector<float4>& body, const std::vector<P2>& v, const float4* rows, long long n_rows);
inline void walkers_serial(const WalkArgs& q, const float4* walls, const long long* wall_starts) {
    const int A = q.n_agents, P = q.n_slots;
    std::vector<float4> body((size_t)(A + P));
    std::vector<P2> v((size_t)P);
    for (int n = 0; n < q.n_envs; n++) {
        for (int a = 0; a < A; a++) {
            if (q.bumps) q.bumps[(long long)n*A + a] = 0;
            if (q.close) q.close[(long long)n*A + a] = 0;
        }
        if (q.reset && q.reset[n]) {
            for (int k = 0; k < P; k++) {
                walk_wipe(q, (long long)n*P + k);
                if (q.slide) walk_slide_records(q, (long long)n*P + k, false, 0.f, false);
            }
            continue;
        }
        for (int a = 0; a < A; a++) {
            const float2 pa = load2(q.agent_positions, (size_t)n*A + a);
            body[(size_t)a] = make_float4(pa.x, pa.y, 0.f, 0.f);
        }
        for (int k = 0; k < P; k++) {
            const float2 p = load2(q.positions, (size_t)n*P + k);
            body[(size_t)(A + k)] = make_float4(p.x, p.y, 0.f, 0.f);
        }
        for (int k = 0; k < P; k++) {
            const size_t at = (size_t)n*P + k;
            const float4 me = body[(size_t)(A + k)];
            if (!item_present(me.x, me.y)) continue;
            const float2 t = load2(q.towards, at), vo = load2(q.velocities, at);
            v[(size_t)k] = walk_velocity(q, k, p2(me.x, me.y), p2(t.x, t.y), q.speeds[at], p2(vo.x, vo.y),
                                         [&](const int i) { return make_float2(body[(size_t)i].x, body[(size_t)i].y); },
                                         [&](const int a) { if (q.close) q.close[(long long)n*A + a]++; });
        }
        for (int k = 0; k < P; k++) {                                   // (the steer step read positions only)
            float4& me = body[(size_t)(A + k)];
            if (!item_present(me.x, me.y)) continue;
            const P2 u = v[(size_t)k]/q.fps;
            me.z = u.x; me.w = u.y;
        }
        const float4* const rows = walls + wall_starts[n];
        const long long n_rows = wall_starts[n + 1] - wall_starts[n];
        if (q.slide) {
            walk_slide_env(q, n, body, v, rows, n_rows);
            continue;
        }
        for (int k = 0; k < P; k++) {
            const float4 me = body[(size_t)(A + k)];
            const bool present = item_present(me.x, me.y);
            unsigned key = walk_key(1.f, 0);
            if (present) {
                const StepTask task = step_task(make_float2(me.x, me.y), p2(me.z, me.w), q.agent_radius);
                key = walk_meet_bodies(q, k, task, [&](const int i) { return body[(size_t)i]; },
                                       [&](const int a) { if (q.bumps) q.bumps[(long long)n*A + a]++; });
                for (long long l = 0; l < n_rows; l++) key = walk_wall(key, task, rows[l], q.agent_radius);
            }
            walk_settle(q, (long long)n*P + k, present, p2(me.x, me.y), v[(size_t)k], key);
        }
    }
}

template <bool WIDE>
__global__ __launch_bounds__(WG) void walker_kernel(const MsScenery sc, const WalkArgs q) {
    constexpr int PER = WIDE ? WALK_PER : 1, ENVS = WIDE ? 1 : WAVES, STRIDE = WIDE ? WG : WAVE;
    constexpr int ROWS = WALK_MAX_AGENTS + (WIDE ? WALK_MAX_SLOTS : WAVE);
    __shared__ float4 s_bodies[ENVS][ROWS];                             // (p, u): the agents, then the slots
    __shared__ int s_counts[ENVS][2][WALK_MAX_AGENTS];                  // bumps, close
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int part = WIDE ? 0 : wave;
    const int n = WIDE ? (int)blockIdx.x : (int)blockIdx.x*WAVES + wave;
    if (!WIDE && n >= q.n_envs) return;                                 // (a whole wave, and this instantiation has no workgroup barrier)
    const int t0 = WIDE ? tid : lane;                                   // the lane's agent, and the first of its slots
    const int A = q.n_agents, P = q.n_slots, AF = A*sc.n_model;
    float4* const s_body = s_bodies[part];
    int* const s_bumps = s_counts[part][0];
    int* const s_close = s_counts[part][1];
    auto sync = [] { if constexpr (WIDE) __syncthreads(); else wave_sync(); };
    auto counts = [&](const bool zero) {
        if (t0 < A) {
            if (q.bumps) q.bumps[(long long)n*A + t0] = zero ? 0 : s_bumps[t0];
            if (q.close) q.close[(long long)n*A + t0] = zero ? 0 : s_close[t0];
        }
    };

    if (q.reset && q.reset[n]) {                                        // (uniform over the env's lanes, before any barrier)
        for (int k = t0; k < P; k += STRIDE) walk_wipe(q, (long long)n*P + k);
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
    bool some;
    if constexpr (WIDE) some = __syncthreads_or(any);
    else { some = __ballot(any) != 0ull; wave_sync(); }
    if (!some) {                                                        // (uniform) nobody walks here: the records, and done
        for (int k = t0; k < P; k += STRIDE) walk_settle(q, (long long)n*P + k, false, p2(0.f, 0.f), p2(0.f, 0.f), 0u);
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

    // meet: the bodies' whole rows, then the walls; move
    const EnvRows e = env_rows(sc, n);
    #pragma unroll
    for (int j = 0; j < PER; j++) {
        const int k = t0 + j*STRIDE;
        unsigned key = walk_key(1.f, 0);
        StepTask task{make_float4(0.f, 0.f, 0.f, 0.f), 0.f, 0.f};
        NearList nl{true, 0, 0u, nullptr};                              // (no walker: covered, by an empty list)
        if (here[j]) {
            const float4 me = s_body[A + k];
            task = step_task(make_float2(me.x, me.y), p2(me.z, me.w), q.agent_radius);
            key = walk_meet_bodies(q, k, task, [&](const int i) { return s_body[i]; }, [&](const int a) { atomicAdd(&s_bumps[a], 1); });
            nl = near_list(sc, e, make_float2(me.x, me.y), task.reach);
        }
        walk_rows(nl, e, AF, [&](const float4 row) { key = walk_wall(key, task, row, q.agent_radius); });
        if (k < P) walk_settle(q, (long long)n*P + k, here[j], p[j], v[j], key);
    }
    sync();
    counts(false);
}
