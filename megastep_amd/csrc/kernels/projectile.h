// kernels/projectile.h -- projectile_kernel.
// Part of megastep_hip.hip's one translation unit (included there, inside its anonymous namespace, after items.h: a leg is folded by
// raycast.h's ray_fold, an agent's row drawn by shade.h's shade_row - render.h's drawn_row on the device, its arithmetic on the
// host - presence is items.h's item_present, the wave-wide min and max and the compaction math.h's); not a header to compile on its own.
// ------------------------------------------------------------------------------------------------
// projectiles: things that fly, bounce off walls and strike agents           no counterpart in the reference
// ------------------------------------------------------------------------------------------------
// The contract is written out in include/megastep_hip.h (MsProjectiles) and DESIGN.md section 3.36.  A projectile is a slot of an
// Items-shaped store - present exactly when both coordinates are finite - with a velocity, an owner, a timer and a budget of
// bounces; a call is one tick: reset, fire, fly.  Every output is an integer, a stored NaN, or a float made by the rule's own
// operations in the rule's own order, each element with one writer, and no projectile reads another: any schedule gives the same
// bits.  tests/projectile_rule.py restates all of it in numpy.
//
// The pieces below the kernel's schedule - proj_pose, proj_free_slot, proj_fired, proj_reach, proj_row_meets, proj_leg_begin,
// proj_reflect, proj_leg_end, proj_settle - are __host__ __device__: ms_host_projectiles sweeps them serially over host arrays, so
// the CPU suite holds this very text to the rule, bit for bit.
//
//   projectile_kernel   one WORKGROUP an env, a lane the slots tid + 256 j.
//     fire     lanes a < A read their agent's pose (the sincospi_f the body rows need anyway), scan their own S slots for the least
//              absent one and leave the fired state in LDS; the barrier behind it is what makes it visible to the lanes that own
//              the slots (LDS writes before a workgroup barrier are seen by every read after it), which take it in place of what
//              the store holds.  Nothing of a fired projectile reaches global memory before it has flown.
//     bodies   the A M agent rows are drawn once per workgroup into LDS, not once per lane.
//     cull     every lane forms its slots' reach boxes; their union goes through shuffles, then across the waves through LDS.  The
//              static rows whose box meets the union are compacted into LDS in ascending order (math.h's block_compact),
//              PROJ_LIST_ROWS of them; an env that keeps more
//              walks its rows in global memory, to the same bits.  THE CULL IS EXACT BY CONSTRUCTION: min and max of floats are
//              exact, so the union box contains every projectile's own box, and a row that fails proj_row_meets against the
//              union fails the very same comparisons against each box in it - the rule would not have folded it for anyone.
//     legs     a wave-level loop: while a ballot finds a lane with a leg to fly, the wave walks the body rows and the listed rows
//              at a uniform index (LDS broadcasts); a lane folds a row only when its leg is live and - for a static row - its
//              own box test passes.  Lanes on their first leg and lanes on their fourth share a walk.
//     records  hits and scored go through integer LDS atomics and are stored whole.  No float atomics, no scratch.
constexpr int PROJ_MAX_SLOTS = 1024, PROJ_MAX_AGENTS = 64, PROJ_MAX_PER_AGENT = 16, PROJ_LEGS = 4;
constexpr int PROJ_LIST_ROWS = 512;                  // the static rows the kernel's LDS list holds
constexpr int PROJ_MAX_BODY_ROWS = 1024;             // A*M, the agents' rows the kernel draws into LDS

struct ProjArgs {                                    // MsProjectiles, checked
    float* positions;                                // (N, P, 2)
    float* velocities;                               // (N, P, 2)
    int* owners;                                     // (N, P)
    int* timers;                                     // (N, P)
    int* bounces;                                    // (N, P)
    const unsigned char* fire;                       // (N, A) or NULL
    const unsigned char* reset;                      // (N,) or NULL
    const float* agent_positions;                    // (N, A, 2)
    const float* agent_angles;                       // (N, A)
    int* struck;                                     // (N, P) or NULL
    unsigned char* ended;                            // (N, P) or NULL
    int* hits;                                       // (N, A) or NULL
    int* scored;                                     // (N, A) or NULL
    unsigned char* misfires;                         // (N, A) or NULL
    int n_envs, n_agents, n_model, per_agent, n_slots, life, n_bounces;
    float speed, muzzle, restitution, fps;
};

struct ProjBox { float x0, y0, x1, y1; };
// One projectile through one tick: where it is, how it moves, what is left of the tick, and what became of it.
struct ProjFlight {
    P2 p, v;
    float left;
    int owner, timer, bounces, prev, legs, struck, ended;
    bool live;                                       // a leg is still to fly
};

// Agent a of env n: heading (s, c) = sincospi_f(angle/180) - raycast_kernel's - and position.  false: no finite pose, no shot.
__host__ __device__ inline bool proj_pose(const ProjArgs& q, const int n, const int a, float& s, float& c, P2& pa) {
    const long long at = (long long)n*q.n_agents + a;
    const float angle = q.agent_angles[at];
    pa = p2(q.agent_positions[2*at], q.agent_positions[2*at + 1]);
    s = c = NAN;                                                        // (no heading: rows with a NaN, which nothing hits)
    if (nav_finite(angle)) sincospi_f(angle/180.f, s, c);
    return nav_finite(angle) && nav_finite(pa.x) && nav_finite(pa.y);
}

// The least-numbered absent slot among agent a's S, as the store stands; -1: none.
__host__ __device__ inline int proj_free_slot(const ProjArgs& q, const int n, const int a) {
    for (int j = 0; j < q.per_agent; j++) {
        const int k = a*q.per_agent + j;
        const long long at = (long long)n*q.n_slots + k;
        if (!item_present(q.positions[2*at], q.positions[2*at + 1])) return k;
    }
    return -1;
}

// What a shot of agent a starts as.
__host__ __device__ inline void proj_fired(const ProjArgs& q, const int a, const float s, const float c, const P2 pa, ProjFlight& F) {
    F.p = p2(pa.x + q.muzzle*c, pa.y + q.muzzle*s);
    F.v = p2(q.speed*c, q.speed*s);
    F.owner = a; F.timer = q.life; F.bounces = q.n_bounces;
}

// The reach box of a projectile at p moving at v: fixed at the start of the tick.  false: a NaN in it - it meets no row.
__host__ __device__ inline bool proj_reach(const P2 p, const P2 v, const float fps, ProjBox& b) {
    const P2 u = v/fps;
    const float r = (fabsf(u.x) + fabsf(u.y))*1.01f + 1e-3f;
    b = ProjBox{p.x - r, p.y - r, p.x + r, p.y + r};
    return (b.x0 == b.x0) & (b.y0 == b.y0) & (b.x1 == b.x1) & (b.y1 == b.y1);
}

// Does the static row L meet the box?  A row with a NaN does not.
__host__ __device__ inline bool proj_row_meets(const ProjBox& b, const float4 L) {
    return item_row_live(L) && fminf(L.x, L.z) <= b.x1 && fmaxf(L.x, L.z) >= b.x0 && fminf(L.y, L.w) <= b.y1 && fmaxf(L.y, L.w) >= b.y0;
}

__host__ __device__ inline void proj_start(ProjFlight& F, const bool present) {
    F.left = 1.f; F.prev = -1; F.legs = 0; F.struck = -1; F.ended = present ? 0 : 4; F.live = present;
}

// The next leg's ray.  false: there is none to fly - no length left, or a NaN - and the flight ends where it is.
__host__ __device__ inline bool proj_leg_begin(ProjFlight& F, const float fps, P2& ru, float& rlen) {
    ru = (F.v/fps)*F.left;
    rlen = len(ru);
    if (!(rlen > 0.f)) { F.live = false; return false; }
    return true;
}

// v off a wall of direction w.
__host__ __device__ inline P2 proj_reflect(const P2 v, const P2 w, const float restitution) {
    const P2 n = p2(-w.y, w.x);
    const float k = ((1.f + restitution)*(v.x*n.x + v.y*n.y))/(n.x*n.x + n.y*n.y);
    return p2(v.x - k*n.x, v.y - k*n.y);
}

// The leg (ru, rlen) has been folded into f (rows below AF = A M are bodies): move, strike, stop or bounce.
__host__ __device__ inline void proj_leg_end(ProjFlight& F, const RayFold& f, const P2 ru, const float rlen, const int AF, const int M,
                                             const float restitution) {
    F.legs++;
    if (f.idx < 0) { F.p = p2(F.p.x + ru.x, F.p.y + ru.y); F.live = false; return; }
    if (f.idx < AF) { F.struck = f.idx/M; F.ended = 1; F.live = false; return; }
    if (F.bounces == 0) { F.ended = 2; F.live = false; return; }
    const float s1 = fminf(f.s, 1.f);
    const float go = fmaxf(s1 - 1e-3f/rlen, 0.f);                       // (a millimetre short, never ahead of where it was)
    F.p = p2(F.p.x + ru.x*go, F.p.y + ru.y*go);
    F.bounces -= 1;
    F.left = F.left*(1.f - s1);
    F.v = proj_reflect(F.v, p2(f.vx, f.vy), restitution);
    F.prev = f.idx;
    if (F.legs == PROJ_LEGS) F.live = false;                            // (what is left of the tick is dropped)
}

// Slot `at` = n P + k after its flight: the timer, the stores, the records.  `flew`: it was present going into the fly step.
__host__ __device__ inline void proj_settle(const ProjArgs& q, const long long at, const bool flew, ProjFlight& F) {
    if (flew) {
        if (F.ended == 0) { F.timer -= 1; if (F.timer == 0) F.ended = 3; }
        const bool gone = F.ended != 0;
        q.positions[2*at] = gone ? NAN : F.p.x; q.positions[2*at + 1] = gone ? NAN : F.p.y;
        q.velocities[2*at] = F.v.x; q.velocities[2*at + 1] = F.v.y;
        q.owners[at] = F.owner; q.timers[at] = F.timer; q.bounces[at] = F.bounces;
    }
    if (q.struck) q.struck[at] = F.struck;
    if (q.ended) q.ended[at] = (unsigned char)F.ended;
}

// An env being emptied: slot `at`.
__host__ __device__ inline void proj_wipe(const ProjArgs& q, const long long at) {
    q.positions[2*at] = NAN; q.positions[2*at + 1] = NAN;
    q.timers[at] = 0; q.bounces[at] = 0;
    if (q.struck) q.struck[at] = -1;
    if (q.ended) q.ended[at] = 4;
}

// One whole call on host arrays, serially: `walls` holds every env's STATIC rows, env n's from wall_starts[n] on; `model` the M
// rows of an agent's body in its own frame.
inline void projectiles_serial(const ProjArgs& q, const float4* model, const float4* walls, const long long* wall_starts) {
    const int A = q.n_agents, M = q.n_model, AF = A*M, P = q.n_slots;
    std::vector<float4> bodies((size_t)AF);
    for (int n = 0; n < q.n_envs; n++) {
        const float4* const rows = walls + wall_starts[n];
        const long long n_rows = wall_starts[n + 1] - wall_starts[n];
        for (int a = 0; a < A; a++) {
            const long long at = (long long)n*A + a;
            if (q.hits) q.hits[at] = 0;
            if (q.scored) q.scored[at] = 0;
            if (q.misfires) q.misfires[at] = 0;
        }
        if (q.reset && q.reset[n]) {
            for (int k = 0; k < P; k++) proj_wipe(q, (long long)n*P + k);
            continue;
        }
        for (int a = 0; a < A; a++) {
            float s, c;
            P2 pa;
            const bool posed = proj_pose(q, n, a, s, c, pa);
            for (int m = 0; m < M; m++) bodies[(size_t)(a*M + m)] = shade_row(s, c, pa.x, pa.y, model[m]);
            if (!posed || !q.fire || !q.fire[(long long)n*A + a]) continue;
            const int k = proj_free_slot(q, n, a);
            if (k < 0) { if (q.misfires) q.misfires[(long long)n*A + a] = 1; continue; }
            ProjFlight F{};
            proj_fired(q, a, s, c, pa, F);
            const long long at = (long long)n*P + k;
            q.positions[2*at] = F.p.x; q.positions[2*at + 1] = F.p.y; q.velocities[2*at] = F.v.x; q.velocities[2*at + 1] = F.v.y;
            q.owners[at] = F.owner; q.timers[at] = F.timer; q.bounces[at] = F.bounces;
        }
        for (int k = 0; k < P; k++) {
            const long long at = (long long)n*P + k;
            ProjFlight F{};
            F.p = p2(q.positions[2*at], q.positions[2*at + 1]); F.v = p2(q.velocities[2*at], q.velocities[2*at + 1]);
            F.owner = q.owners[at]; F.timer = q.timers[at]; F.bounces = q.bounces[at];
            const bool flew = item_present(F.p.x, F.p.y);
            proj_start(F, flew);
            ProjBox box{};
            const bool boxed = flew && proj_reach(F.p, F.v, q.fps, box);
            P2 ru;
            float rlen;
            while (F.live && proj_leg_begin(F, q.fps, ru, rlen)) {
                RayFold f{1.001f, -1, NAN, 0.f, 0.f};
                for (int i = 0; i < AF; i++)
                    if (i/M != F.owner) ray_fold(F.p, ru, 0.f, bodies[(size_t)i], i, f);
                for (long long l = 0; l < n_rows; l++)
                    if (boxed && AF + (int)l != F.prev && proj_row_meets(box, rows[l])) ray_fold(F.p, ru, 0.f, rows[l], AF + (int)l, f);
                proj_leg_end(F, f, ru, rlen, AF, M, q.restitution);
            }
            proj_settle(q, at, flew, F);
            if (F.struck >= 0) {
                if (q.hits) q.hits[(long long)n*A + F.struck]++;
                if (q.scored && F.owner >= 0 && F.owner < A) q.scored[(long long)n*A + F.owner]++;
            }
        }
    }
}

__global__ __launch_bounds__(WG) void projectile_kernel(const MsScenery sc, const ProjArgs q) {
    __shared__ float4 s_bodies[PROJ_MAX_BODY_ROWS];
    __shared__ float4 s_rows[PROJ_LIST_ROWS];
    __shared__ int s_ls[PROJ_LIST_ROWS];
    __shared__ float4 s_pose[PROJ_MAX_AGENTS];                          // (s, c, px, py)
    __shared__ float4 s_shot[PROJ_MAX_AGENTS];                          // a fired projectile's (p, v)
    __shared__ int s_slot[PROJ_MAX_AGENTS];                             // ... and its slot, -1: the agent fired nothing
    __shared__ int s_hits[PROJ_MAX_AGENTS], s_scored[PROJ_MAX_AGENTS];
    __shared__ float s_union[WAVES][4];
    __shared__ int s_kept[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.x;
    const int A = q.n_agents, M = q.n_model, AF = A*M, P = q.n_slots, S = q.per_agent;

    if (q.reset && q.reset[n]) {                                        // (uniform, before any barrier)
        for (int k = tid; k < P; k += WG) proj_wipe(q, (long long)n*P + k);
        if (tid < A) {
            const long long at = (long long)n*A + tid;
            if (q.hits) q.hits[at] = 0;
            if (q.scored) q.scored[at] = 0;
            if (q.misfires) q.misfires[at] = 0;
        }
        return;
    }

    // fire: a lane an agent.  The shot stays in LDS; the barrier below shows it to the lanes that own the slots.
    bool busy = false;                                                  // a shot of this lane's agent, or one of its slots in flight
    for (int k = tid; k < P; k += WG) {
        const float2 p = reinterpret_cast<const float2*>(q.positions)[(long long)n*P + k];
        busy |= item_present(p.x, p.y);
    }
    if (tid < A) {
        const int a = tid;
        float s, c;
        P2 pa;
        const bool posed = proj_pose(q, n, a, s, c, pa);
        s_pose[a] = make_float4(s, c, pa.x, pa.y);
        int slot = -1;
        bool misfire = false;
        if (posed && q.fire && q.fire[(long long)n*A + a]) {
            slot = proj_free_slot(q, n, a);
            misfire = slot < 0;
            if (slot >= 0) {
                ProjFlight F{};
                proj_fired(q, a, s, c, pa, F);
                s_shot[a] = make_float4(F.p.x, F.p.y, F.v.x, F.v.y);
            }
        }
        s_slot[a] = slot;
        s_hits[a] = 0; s_scored[a] = 0;
        busy |= slot >= 0;
        if (q.misfires) q.misfires[(long long)n*A + a] = misfire ? 1 : 0;
    }
    if (!__syncthreads_or(busy)) {                                      // (uniform) nothing in flight, nobody fired: the records, and done
        ProjFlight F{};
        proj_start(F, false);
        for (int k = tid; k < P; k += WG) proj_settle(q, (long long)n*P + k, false, F);
        if (tid < A) {
            if (q.hits) q.hits[(long long)n*A + tid] = 0;
            if (q.scored) q.scored[(long long)n*A + tid] = 0;
        }
        return;
    }

    // the bodies, drawn once for the workgroup (not vectorised: the loop vectoriser pairs two rows' arithmetic into packed f32
    // instructions, SLP or not - the only ones the kernel would hold)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int i = tid; i < AF; i += WG) {
        const int a = i/M;
        const float4 pose = s_pose[a];
        s_bodies[i] = shade_row(pose.x, pose.y, pose.z, pose.w, reinterpret_cast<const float4*>(sc.model)[i - a*M]);
    }

    // slot k as it goes into the fly step: the shot fired into it, else what the store holds
    auto load = [&](const int k, ProjFlight& F) {
        const long long at = (long long)n*P + k;
        const int a = k/S;
        if (s_slot[a] == k) {
            const float4 shot = s_shot[a];
            F.p = p2(shot.x, shot.y); F.v = p2(shot.z, shot.w);
            F.owner = a; F.timer = q.life; F.bounces = q.n_bounces;
        } else {
            const float2 p = reinterpret_cast<const float2*>(q.positions)[at], v = reinterpret_cast<const float2*>(q.velocities)[at];
            F.p = p2(p.x, p.y); F.v = p2(v.x, v.y);
            F.owner = q.owners[at]; F.timer = q.timers[at]; F.bounces = q.bounces[at];
        }
        return item_present(F.p.x, F.p.y);
    };

    // the union of the env's reach boxes: the lane's slots, the wave by shuffles, the waves through LDS
    ProjBox all{INFINITY, INFINITY, -INFINITY, -INFINITY};
    for (int k = tid; k < P; k += WG) {
        ProjFlight F{};
        ProjBox b{};
        if (load(k, F) && proj_reach(F.p, F.v, q.fps, b)) {
            all.x0 = b.x0 < all.x0 ? b.x0 : all.x0; all.y0 = b.y0 < all.y0 ? b.y0 : all.y0;
            all.x1 = b.x1 > all.x1 ? b.x1 : all.x1; all.y1 = b.y1 > all.y1 ? b.y1 : all.y1;
        }
    }
    all.x0 = wave_min_f(all.x0); all.y0 = wave_min_f(all.y0);
    all.x1 = wave_max_any_f(all.x1); all.y1 = wave_max_any_f(all.y1);
    if (lane == 0) { s_union[wave][0] = all.x0; s_union[wave][1] = all.y0; s_union[wave][2] = all.x1; s_union[wave][3] = all.y1; }
    __syncthreads();                                                    // (also: the bodies are drawn)
    for (int w = 0; w < WAVES; w++) {
        all.x0 = s_union[w][0] < all.x0 ? s_union[w][0] : all.x0; all.y0 = s_union[w][1] < all.y0 ? s_union[w][1] : all.y0;
        all.x1 = s_union[w][2] > all.x1 ? s_union[w][2] : all.x1; all.y1 = s_union[w][3] > all.y1 ? s_union[w][3] : all.y1;
    }
    const bool boxed = all.x0 <= all.x1;                                // (uniform: some projectile has a box)

    // the static rows that meet the union, compacted into LDS in ascending order.  Exact: a row that misses the union misses
    // every box in it by proj_row_meets' own comparisons (min and max of floats round nothing).
    const EnvLines ln = env_lines(sc, n);                               // (its AF is the arguments' A M: ms_projectiles fills them from sc)
    const int L = ln.L;
    const float4* const rows = ln.rows;
    int kept = 0;                                                       // (uniform)
    if (boxed)
        for (int l0 = AF; l0 < L; l0 += WG) {
            const int l = l0 + tid;
            float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
            bool keep = false;
            if (l < L) { row = rows[l]; keep = proj_row_meets(all, row); }
            // (kept counts on past the list: that is !listed)
            block_compact(keep, lane, wave, s_kept, kept, [&](const int at) { if (at < PROJ_LIST_ROWS) { s_rows[at] = row; s_ls[at] = l; } });
        }
    const bool listed = kept <= PROJ_LIST_ROWS;                         // (uniform; else: the env's rows in global memory)

    // the flights: the wave's 64 slots of each chunk of 256 in step (the ballots below are whole)
    for (int k0 = 0; k0 < P; k0 += WG) {
        const int k = k0 + tid;
        const bool mine = k < P;
        ProjFlight F{};
        ProjBox box{};
        const bool flew = mine && load(k, F);
        proj_start(F, flew);
        const bool own = flew && proj_reach(F.p, F.v, q.fps, box);      // (no box: the flight meets the bodies only)
        for (;;) {
            P2 ru = p2(0.f, 0.f);
            float rlen = 0.f;
            const bool go = F.live && proj_leg_begin(F, q.fps, ru, rlen);
            if (__ballot(go) == 0ull) break;                            // (uniform: no lane of the wave has a leg to fly)
            RayFold f{1.001f, -1, NAN, 0.f, 0.f};
            for (int a = 0; a < A; a++)
                for (int m = 0; m < M; m++) {
                    const float4 row = s_bodies[a*M + m];
                    if (go && a != F.owner) ray_fold(F.p, ru, 0.f, row, a*M + m, f);
                }
            if (listed) {
                for (int j = 0; j < kept; j++) {
                    const float4 row = s_rows[j];
                    const int l = s_ls[j];
                    if (go && own && l != F.prev && proj_row_meets(box, row)) ray_fold(F.p, ru, 0.f, row, l, f);
                }
            } else {
                for (int l = AF; l < L; l++) {
                    const float4 row = rows[l];
                    if (go && own && l != F.prev && proj_row_meets(box, row)) ray_fold(F.p, ru, 0.f, row, l, f);
                }
            }
            if (go) proj_leg_end(F, f, ru, rlen, AF, M, q.restitution);
        }
        if (mine) {
            proj_settle(q, (long long)n*P + k, flew, F);
            if (F.struck >= 0) {
                atomicAdd(&s_hits[F.struck], 1);
                if (F.owner >= 0 && F.owner < A) atomicAdd(&s_scored[F.owner], 1);
            }
        }
    }
    __syncthreads();
    if (tid < A) {
        if (q.hits) q.hits[(long long)n*A + tid] = s_hits[tid];
        if (q.scored) q.scored[(long long)n*A + tid] = s_scored[tid];
    }
}
