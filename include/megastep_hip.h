/*
 * megastep_hip.h -- C-ABI of the MI355X (gfx950) simulation core.
 *
 * This is the drop-in boundary for the reference's native extension `megastepcuda`
 * (surfaced in Python as `megastep.cuda`, /root/reference/megastep/__init__.py:7-20,
 * bound in /root/reference/megastep/src/wrappers.cpp:30-173).  Every entry point below
 * names the reference interface it replaces.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers + sizes, no torch / ATen types.
 *   - the library never allocates, frees or synchronises: the caller owns every buffer
 *     and all work is enqueued asynchronously on the hipStream_t it passes
 *     (the reference enqueues on at::cuda::getCurrentCUDAStream(), kernels.cu:30-32).
 *   - configuration travels by value with each call (the reference keeps it in
 *     process-global __constant__ memory, kernels.cu:12-27), so one process can drive
 *     several devices / configurations.
 *   - every function returns MS_OK (0) or a negative MS_E* code; ms_strerror() explains it.
 *     (The reference raises c10::Error through pybind, common.h:12-14,33-37.)
 *   - all float data is IEEE binary32, all index data int32, as in the reference
 *     (rebar/arrdict.py:79-88, common.h:122).
 */
#ifndef MEGASTEP_HIP_H
#define MEGASTEP_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MS_ABI_VERSION 17

#define MS_OK            0
#define MS_EINVAL       -1   /* bad argument (null pointer, non-positive size, ...) */
#define MS_EHIP         -2   /* a HIP runtime call failed; see ms_last_hip_error()  */
#define MS_EUNSUPPORTED -3   /* shape outside what the kernels support              */
#define MS_ENODEVICE    -4   /* no usable gfx950 device                             */
/* An entry point that returns MS_EINVAL or MS_EUNSUPPORTED has enqueued nothing: every argument is checked, and every
 * choice of launch made, before the first launch. */

/* Replaces `initialize(agent_radius, res, fov, fps)` (wrappers.cpp:53, kernels.cu:18-27). */
typedef struct MsConfig {
    float agent_radius;   /* collision radius and near plane, metres (core.py:14)  */
    int   res;            /* rays per agent, R                                      */
    float fov;            /* field of view, degrees (< 180)                         */
    float fps;            /* simulation steps per second                            */
} MsConfig;

/* Replaces `Scenery` + its three `Ragged`s (common.h:102-155,179-214). Device pointers. */
typedef struct MsScenery {
    int n_envs, n_agents, n_model;   /* N, A, M = model.size(0)                                */
    const float* lights_vals;        /* (sum I, 3)  x, y, intensity                            */
    const int*   lights_widths;      /* (N,)                                                   */
    const int*   lights_starts;      /* (N,)                                                   */
    float*       lines_vals;         /* (sum L, 2, 2) [endpoint][xy]; rows [0, A*M) of each env
                                        are the agents' models and are REWRITTEN by ms_render
                                        (kernels.cu:316-317). Must be 16-byte aligned.         */
    const int*   lines_widths;       /* (N,)                                                   */
    const int*   lines_starts;       /* (N,)                                                   */
    const int*   lines_inverse;      /* (sum L,) global line -> env                            */
    const float* textures_vals;      /* (sum T, 3) linear RGB, ragged per GLOBAL line          */
    const int*   textures_widths;    /* (sum L,) texels per line                               */
    const int*   textures_starts;    /* (sum L,)                                               */
    const int*   textures_inverse;   /* (sum T,) texel -> global line                          */
    const float* model;              /* (M, 2, 2) agent outline in the agent frame             */
    float*       baked_vals;         /* (sum T,) written by ms_bake, read by ms_render         */
    int n_lines_total, n_lights_total, n_texels_total;
    /* Optional light grid (lg_vals NULL = none; no counterpart in the reference): a per-env uniform grid over the
     * floorplan that caches, for every cell and each of the env's first 64 lights, whether the light reaches the
     * cell.  Written by ms_bake, read by ms_render's dynamic lighting, exact by construction: a cell is only ever
     * marked when EVERY point in it provably has that status; anything else stays 0 (unknown) and is worked out
     * per ray - against the cell's candidate list (the walls that could not be ruled out for the cell and that
     * light) when it has one, against every wall otherwise.
     *   lg_vals   (sum cells, 4) uint32, 2 bits per light: 0 unknown, 1 lit, 2 dark; must start zeroed
     *   lg_starts (N,)   first cell of env n
     *   lg_geom   (N, 4) float: x and y of the grid's origin, cells along x, cells along y
     *   lg_cell   cell size in metres;  lg_max_cells  max over envs of cells (launch bound for ms_bake)
     *   lg_list   (sum cells, 2) uint32, optional (NULL together with lg_pool), must start zeroed:
     *             [first pool word of the cell's candidates, 0x80000000 | how many]; second word 0 = no list
     *   lg_pool   (lg_pool_size,) uint32: word 0 is ms_bake's allocation cursor, then candidates
     *             0x80000000 | light << 24 | wall (index among the env's static lines).  A pool that runs out
     *             only costs speed: the cells that did not fit go without a list.
     * Only for sceneries with at most 64 lights in every env: pass lg_vals = NULL otherwise. */
    unsigned*    lg_vals;
    const int*   lg_starts;
    const float* lg_geom;
    float        lg_cell;
    int          lg_max_cells;
    unsigned*    lg_list;
    unsigned*    lg_pool;
    int          lg_pool_size;
    /* Optional, with lg_pool: (lg_pool_size, 4) float32 - next to every candidate of lg_pool its wall's row as the shadow
     * test wants it, (ax, ay, bx - ax, by - ay), written by ms_bake.  ms_render then has a list's walls in the trip that
     * brings its candidates, instead of one trip later (the rays that need them are the ones a launch waits for).  NULL:
     * ms_render fetches the rows from `lines` by the candidates' wall numbers. */
    float*       lg_pool_rows;
    /* Optional sharing of static geometry between envs (NULL = every env on its own; no counterpart in the reference,
     * whose scene.py:75-100 and kernels.cu:270-293 redo identical floorplans env by env): env_geom[n] is the FIRST env
     * whose walls and light POSITIONS are bit-identical to env n's (itself for a representative).  Light intensities
     * and textures stay per env.  ms_bake then works out light visibility - the O(texels x lights x walls) part,
     * which depends on walls and light positions only - once per representative, and members of a group may share one
     * light grid (equal lg_starts / lg_geom rows); the per-env part (the sum over unblocked lights with the env's
     * own intensities, kernels.cu:261-267) runs for every env as before, so baked_vals are the reference's bit for bit. */
    const int*   env_geom;
    /* Optional scratch for ms_bake (NULL = its self-contained one-pass kernel): one visibility bit per
     * (texel, light) of every representative env.  The bits of env n's representative start at word
     * bake_vis_starts[n] and take lights(n) x ceil(texels(n)/64) 64-bit words, row per light.  Contents undefined
     * before and after the call. */
    unsigned long long* bake_vis;
    const long long*    bake_vis_starts;   /* (N,) */
    long long           bake_vis_words;    /* size of bake_vis, for bounds checking */
    /* Optional wall grid (wg_cells NULL = none; no counterpart in the reference, whose kernels meet every line of an
     * env for every ray and every agent, kernels.cu:203-205,352-377): a per-floorplan uniform grid whose cells each
     * hold two lists of static walls (indices among the env's static lines, i.e. line index - n_agents*n_model):
     *   vis   every wall that can matter to a ray cast from ANY point of the cell: a wall is left out only when one
     *         other wall provably stands between it and the whole cell - with room to spare for the reference's
     *         1e-4 hysteresis, its near plane and its rounding - so that the order-dependent nearest-hit fold over
     *         the listed walls ends exactly where the fold over all of them does;
     *   near  every wall that comes within wg_reach of the cell: all an agent in the cell whose step reaches no
     *         farther than that can collide with.
     * ms_render / ms_physics look the agent's cell up and walk its list instead of the env's lines; agents outside
     * the grid, or faster than wg_reach allows, meet every line as before.  Filled by ms_wallgrid_scan +
     * ms_wallgrid_fill (below) from the static walls as they are at that moment: the walls must not move afterwards
     * (or the grid must be rebuilt / dropped).  Envs that share their walls (env_geom) share their cells.
     *   wg_cells  (sum cells + 1, 4) uint32: [first vis entry (in wg_pool, from wg_pool_base[n]), vis count, first near entry (in
     *             wg_near_rows), near count within wg_reach_lo | near count in all << 16]
     *   wg_starts (N,) first cell of env n;   wg_geom (N, 4) float: grid origin x, y, cells along x, cells along y
     *             (0 cells: this env has no grid);   wg_cell: cell size in metres
     *   wg_pool_base (N,) int64, required with wg_cells: where in wg_pool the vis lists of env n's floorplan start, in entries;
     *             a cell's "first vis entry" counts from there.  (Round 5: a world of 4096 distinct 1000-wall floorplans - the
     *             reference's cubicasa pool is 4492 - has 6 x 10^9 vis entries at 0.25 m cells, more than a 32-bit offset
     *             reaches; per floorplan it is a few million.)  Envs that share their walls share the value.
     *   wg_pool   the vis lists, one uint32 per entry: wall index | first step << 16 | last step << 24 of the arc of
     *             directions the wall can be seen in from the cell (steps of 1/64 of a quarter turn-like unit, modulo 256:
     *             ms_render skips entries whose arc misses its rays'); at least 64 entries longer than the lists need
     *   wg_near_rows  (., 4) float: the near lists as copies of the walls' rows (ax, ay, bx, by), per cell the walls
     *             within wg_reach_lo of it first, then those within wg_reach
     *   wg_near   vis lists hold for near planes (MsConfig.agent_radius) below this and fields of view up to
     *             MS_WALLGRID_MAX_FOV degrees; ms_render ignores the grid otherwise */
    const unsigned*       wg_cells;
    const int*            wg_starts;
    const float*          wg_geom;
    float                 wg_cell;
    float                 wg_reach_lo, wg_reach;
    float                 wg_near;
    const unsigned*       wg_pool;
    const long long*      wg_pool_base;
    const float*          wg_near_rows;
    /* Optional: the largest distance of a point of `model` from the agent's origin, 0 = not known.  When it is below
     * the near plane (MsConfig.agent_radius, as in the reference: core.py:14, scene.py:25-33), no ray of an agent can
     * hit the agent's own outline (kernels.cu:369) and ms_render does not try. */
    float model_radius;
} MsScenery;

/* Replaces `Agents` (common.h:157-177). Updated IN PLACE by ms_physics. */
typedef struct MsAgents {
    float* angles;        /* (N, A)    degrees           */
    float* positions;     /* (N, A, 2) metres            */
    float* angvelocity;   /* (N, A)    degrees / second  */
    float* velocity;      /* (N, A, 2) metres / second   */
    /* Optional heading cache (NULL = none; no counterpart in the reference), (N, A, 4): [angle, sin, cos, unused].
     * ms_physics, which has each agent's new angle in hand, leaves its sine and cosine here; ms_render uses an
     * entry when its angle equals the agent's current one bit for bit, and works the pair out itself otherwise
     * (an agent turned by the caller in between).  Same function, same bits either way - it saves ms_render a launch.
     * Must start as NaNs (or any value no angle takes); pass NULL to ms_render to get its self-contained path. */
    float* headings;
    /* Optional fan schedule (NULL = none; no counterpart in the reference), (2, N, A) int: [costs | order].  Where every agent
     * is ONE wave of ms_render - at most 64 rays, one 64-ray group a wave, two launches a step - the wave leaves a small
     * integer in costs[n A + a]: an estimate of how long it lived, from what it counted on its way (pair windows, list
     * length, a ray on an agent, lights left open, rays redone by the literal fold).  The next ms_step_physics / ms_physics
     * sorts each XCD's run of fans by it, slowest first, into order[slot] = fan - a few extra waves of its own launch - and
     * the ms_render behind it starts its waves in that order: a frame's slow fans are, by and large, the last frame's, and
     * a launch that starts them first does not end waiting for them.  Which fan a wave is changes nothing it computes:
     * same bits with and without.  `costs` may hold anything (every value is a class; the sort writes a permutation of
     * each run whatever it reads); `order` must start as the identity, 0 .. N A - 1, so that a render before any physics
     * call is served.  A table sorted for one (N, A) must not be handed to a call with another.
     * (The field is the struct's last and MS_ABI_VERSION stays 17: a caller built against the header without it must be
     * rebuilt - the library reads the field of every MsAgents it is given.) */
    int* schedule;
} MsAgents;

/* Replaces `Render` (common.h:216-222). Caller-allocated outputs.  With a light grid in the scenery any of the
 * five per-ray outputs may be NULL (not wanted: skipped); without one all five are required. */
typedef struct MsRender {
    int*   indices;       /* (N, A, R)    line index within the env, -1 on a miss */
    float* locations;     /* (N, A, R)    position along the line, NaN on a miss  */
    float* dots;          /* (N, A, R)    ray . line direction,    NaN on a miss  */
    float* distances;     /* (N, A, R)    metres, +inf on a miss                  */
    float* screen;        /* (N, A, R, 3) linear RGB, 0 on a miss                 */
    /* Optional scratch, not an output: lets ms_render compute every agent's sin/cos once, ahead of the
     * raycast, and hand the ray groups that need dynamic lighting from its first kernel to its second as
     * a compact list.  At least MS_RENDER_WORKSPACE_INTS(N, A, R) 4-byte words, 8-byte aligned, contents
     * undefined before and after the call; NULL selects slower in-kernel paths. */
    int*   workspace;
    /* Optional pooled observations, written by the render kernel itself instead of by a chain of host-side tensor
     * ops over the per-ray outputs (replaces modules.py:138-145,170-184,211-224: downsample().mean(), Depth, RGB).
     * Each pixel is the mean over `obs_subsample` adjacent rays; obs_subsample must be a power of two dividing
     * both 64 and the resolution.  NULL = not wanted.
     *   obs_rgb    (N, A, 3, R/obs_subsample)  channel-major, as the reference's RGB module returns it
     *   obs_depth  (N, A, R/obs_subsample)     mean of 1 - clamp((distance - agent_radius)/obs_max_depth, 0, 1), the quotient taken
     *                                          as ATen takes a tensor over a scalar: times the binary32 reciprocal */
    float* obs_rgb;
    float* obs_depth;
    int    obs_subsample;
    float  obs_max_depth;
    /* Optional, with obs_subsample set: what the two central observation pixels of each agent show - the index of
     * the agent whose outline the pixel's middle ray (ray pixel*obs_subsample + obs_subsample/2) landed on, else -1.
     * It is all Deathmatch reads from `indices` (demo/envs/deathmatch.py:54-58,74-80).  (N, A, 2) */
    int*   obs_centre;
    /* Optional first-sight bookkeeping (replaces demo/envs/explorer.py:34-58, a scatter over every texel of every env
     * per step): each ray that hits marks the texel under it - textures_starts[line] + min(floor(width*location),
     * width - 1), explorer.py:38-41 - by writing its env's epoch into seen_stamp, and texels whose stamp was not the
     * epoch yet are counted into seen_count.  Bumping an env's epoch forgets all its texels at once.
     *   seen_stamp (sum T,) int, seen_epoch (N,) int, seen_count (N,) int (added to, atomically) */
    int*       seen_stamp;
    const int* seen_epoch;
    int*       seen_count;
} MsRender;

/* 4-byte words of MsRender.workspace needed for N envs, A agents, R rays */
#define MS_RENDER_WORKSPACE_INTS(N, A, R) (18 + (long long)(N)*(A)*(((R) + 63)/64) + 2*(long long)(N)*(A))

int         ms_abi_version(void);
const char* ms_strerror(int code);
/* hipError_t of the most recent failing HIP call made by this library on this thread (0 if none). */
int         ms_last_hip_error(void);
/* Number of visible HIP devices, or MS_ENODEVICE. Lets the host side fail loudly up front. */
int         ms_device_count(void);

/* Replaces `bake(scenery)` (wrappers.cpp:61, kernels.cu:270-293): static lighting of every texel
 * into scenery->baked_vals. `config` is unused by this stage and may be NULL (the reference's bake reads none of the
 * initialize() constants and runs before any Core exists, scene.py:98). */
int ms_bake(const MsScenery* scenery, const MsConfig* config, void* hip_stream);

/* Optional prologue of the physics step: what the reference's movement modules do with a handful of tensor ops right
 * before they call physics (modules.py:24-66 SimpleMovement, :68-118 MomentumMovement).  Per agent, with (dx, dy, dw)
 * the table row of its action and (c, s) = cos, sin of its heading in radians (binary32, as torch evaluates them):
 *   angvelocity <- keep * angvelocity + dw;  velocity <- keep * velocity + (c dx - s dy, s dx + c dy)
 * written back to the agents' tensors as the modules do, then the step proceeds.  keep = 1 - decay; keep = 0 assigns. */
typedef struct MsMovement {
    const long long* actions;   /* (N, A) row of `table` per agent (clamped to the table) */
    const float*     table;     /* (n_actions, 3) [dx, dy, dw]: agent-frame velocity and angular velocity deltas */
    int              n_actions;
    float            keep;
} MsMovement;

/* Optional bookkeeping around the physics step: what the reference's environments do with a few dozen tensor ops
 * right before and after it - lifespans (modules.py:328-381), respawns (modules.py:298-326) and the IMU observation
 * (modules.py:240-270).  Every part is optional (NULL pointer = skipped).  Per agent, in this order:
 *   tick     lifespans += 1;  respawn_mask |= lifespans >= max_lifespans;  where the mask is set, lifespans = 0 and
 *            max_lifespans = fresh_max (drawn by the caller, as `actions` are)
 *   respawn  where respawn_mask is set: pose = spawn table row `respawn_choice` (clamped to the table) of this agent,
 *            velocities = 0.  respawn_after = 0: before the movement prologue and the step, so the new pose is what
 *            moves and collides (Deathmatch's order, demo/envs/deathmatch.py:96-99); respawn_after = 1: after the
 *            step's integration (Explorer's order, demo/envs/explorer.py:83-90)
 *   imu      of the state the call leaves behind: [angvelocity/imu_ang_scale, (c vx + s vy)/imu_speed_scale,
 *            (-s vx + c vy)/imu_speed_scale] with (c, s) = cos, sin of the heading in radians, binary32 as torch does - the
 *            quotients included: a tensor over a scalar is `a * (1.f/b)` in ATen */
typedef struct MsStepExtras {
    unsigned char*   respawn_mask;      /* (N, A) bytes, non-zero = respawn; written back when lifespans tick  */
    const long long* respawn_choice;    /* (N, A) */
    const float*     spawn_positions;   /* (N, A, n_spawns, 2) */
    const float*     spawn_angles;      /* (N, A, n_spawns)    */
    int              n_spawns;
    int              respawn_after;
    int*             lifespans;         /* (N, A) */
    int*             max_lifespans;     /* (N, A) */
    const int*       fresh_max;         /* (N, A) */
    float*           imu;               /* (N, A, 3) */
    float            imu_ang_scale, imu_speed_scale;
} MsStepExtras;

/* Replaces `physics(scenery, agents) -> Physics` (wrappers.cpp:69, kernels.cu:179-230):
 * collision-limited integration of the agents, in place; `progress` is the (N, A) output that
 * the reference returns as Physics.progress. */
int ms_move_physics(const MsScenery* scenery, const MsAgents* agents, const MsMovement* movement /* NULL: none */,
                    float* progress, const MsConfig* config, void* hip_stream);
int ms_physics(const MsScenery* scenery, const MsAgents* agents, float* progress,
               const MsConfig* config, void* hip_stream);
/* The same step with the environment's bookkeeping around it in the same launch (movement and extras may be NULL). */
int ms_step_physics(const MsScenery* scenery, const MsAgents* agents, const MsMovement* movement, const MsStepExtras* extras,
                    float* progress, const MsConfig* config, void* hip_stream);

/* Sliding contacts (no counterpart in the reference, whose step stops an agent dead - velocity and spin - at
 * whatever its disc touches): the same step with a second contact phase in the same launch, opt-in.  Per agent, after the
 * respawn, lifespan and movement prologue of ms_step_physics, every operation in binary32 in the order written:
 *   phase A   u = v/fps; x1 = the least of collision_cc against the env's other agents at their start-of-step (p_b, u_b) and of
 *             collision_cs over the env's static rows: ms_step_physics' `progress`, bit for bit.  !(x1 < 1): the step ends as
 *             ms_step_physics ends it - every output of every agent of an env in which nobody was blocked is the plain step's.
 *   contact   (p1, ang1) = the integration with x1.  A blocker is an obstacle whose own collision value equals x1; its offset d
 *             = p1 - q, q the nearest point of a static row (a, b) - a + t (b - a), t = dot(p1 - a, b - a)/dot(b - a, b - a)
 *             clamped to [0, 1], NaN as 0 - or, of agent b, p_b + x1 u_b.  l = |d|; !(l > 0) or a non-finite l: passed over.
 *             n = (d.x/l + 0, d.y/l + 0), vn = dot(v, n); the winner is the least (vn, n.x, n.y), lexicographically under
 *             float < - by value, so that any order of meeting the obstacles, and copies of a row, agree.  No winner, or
 *             !(vn < 0): the plain step's dead stop at p1.
 *   phase B   v' = v - ((1 + bounce) vn) n; r1 = 1 - x1; u2 = (v' r1)/fps; x2 = the least of collision_cs(p1, u2, row) and of
 *             collision_cc(p1, u2, p1_b, u2_b) against the other agents as phase A left them (u2_b = 0 for one that does not
 *             slide); p = p1 + x2 u2; angle = normalize(ang1 + x2 (r1 w)/fps); x2 < 1: v = 0, w = 0 - a dead stop as ever -
 *             else v = v', w kept.
 * `progress` = x1, as before.  Respawns after the step, the IMU reading and the heading cache take the final state.
 * 0 <= bounce <= 1 (0.05 is a good value: without an outward part a tangential second move is stopped by collision_cs' side
 * test at once), n_agents <= 64: MS_EINVAL / MS_EUNSUPPORTED otherwise, before anything is launched. */
typedef struct MsSlide {
    float          bounce;
    float*         slid;      /* (N, A) or NULL: x2 r1, the share of the step spent sliding; 0 where no slide was attempted       */
    unsigned char* stopped;   /* (N, A) or NULL: 1 where the step's collisions zeroed the velocity (a respawn is not counted)     */
} MsSlide;
int ms_slide_physics(const MsScenery* scenery, const MsAgents* agents, const MsMovement* movement, const MsStepExtras* extras,
                     const MsSlide* slide, float* progress, const MsConfig* config, void* hip_stream);

/* Replaces `render(scenery, agents) -> Render` (wrappers.cpp:82, kernels.cu:297-475):
 * draw (rewrites the agent rows of lines_vals) -> raycast -> shade, one fused launch. */
int ms_render(const MsScenery* scenery, const MsAgents* agents, const MsRender* out,
              const MsConfig* config, void* hip_stream);

/* One step of the hot path - ms_physics then ms_render (the reference's every env.step(): wrappers.cpp:69 + :82) - in one
 * call, and where the shapes allow it in ONE LAUNCH: with one agent per env and at most 64 rays (BASELINE config 2: Explorer's
 * shape) the agent is a single wavefront, which runs its env's physics step (kernels.cu:179-230) and renders from the pose it
 * ends on (kernels.cu:297-475); nothing crosses waves, so there is nothing to order between two launches.  Every other shape
 * (several agents per env, more than 64 rays, a wall grid that serves one half of the step only) is ms_physics followed by
 * ms_render, as if the caller had made the two calls.  Which of the two it is, is decided before anything is launched: a call
 * that ms_render would refuse is refused before the physics step moves any agent.  Same results as the two calls, bit for
 * bit, either way. */
int ms_step_render(const MsScenery* scenery, const MsAgents* agents, float* progress, const MsRender* out,
                   const MsConfig* config, void* hip_stream);
/* ... with the movement prologue and the env's bookkeeping of ms_step_physics around the step (either may be NULL): a whole
 * env.step() of a single-agent env of up to 64 rays - the reference's tutorial env, demo/envs/minimal.py: SimpleMovement, physics,
 * render - is then one launch. */
int ms_move_step_render(const MsScenery* scenery, const MsAgents* agents, const MsMovement* movement, const MsStepExtras* extras,
                        float* progress, const MsRender* out, const MsConfig* config, void* hip_stream);

/* What the reference's Deathmatch env does between one frame and the next - `_reset` + `_shoot` + the `health` observation,
 * megastep/demo/envs/deathmatch.py:46-88: some twenty tensor ops on (N, A) tensors - as one element-wise launch behind
 * ms_render, whose obs_centre it reads.  Per agent-row i = n A + a, in this order:
 *   revive   where `dead` is set (the mask this step's physics launch respawned by): health = 1, damage = 0      (:46-52)
 *   shoot    hits = distinct agents in centre[i][0..1] (ids outside 0 .. A-1 are nobody); wounds = agents b of the env with
 *            a in centre[b][0..1]; outside = position below -clearance or above upper[n] (= extent + clearance) in x or y;
 *            damage += hit_damage * hits;  health += -hit_damage * (wounds + outside) - tick_damage               (:54-72)
 *   report   reset_out = the incoming `dead`; reward = hits; health_obs = health; dead = health <= 0 - the next step's
 *            respawn mask; matchings[i][b] = b in centre[i][0..1]   (each optional: NULL = skipped, except `dead`) */
typedef struct MsDeathmatch {
    const int*      centre;        /* (N, A, 2): MsRender.obs_centre of this frame                              */
    const float*    positions;     /* (N, A, 2): MsAgents.positions                                             */
    const float*    upper;         /* (N, 2): the floorplan's extent (masks.shape * res) + clearance            */
    float           clearance, hit_damage, tick_damage;       /* the reference's: 1, .05, .001                 */
    float*          health;        /* (N, A) in / out                                                           */
    float*          damage;        /* (N, A) in / out                                                           */
    unsigned char*  dead;          /* (N, A) in: revived at this step's start; out: dead now                    */
    unsigned char*  reset_out;     /* (N, A) out, optional                                                      */
    float*          reward;        /* (N, A) out, optional                                                      */
    float*          health_obs;    /* (N, A) out, optional                                                      */
    unsigned char*  matchings;     /* (N, A, A) out, optional                                                   */
} MsDeathmatch;
int ms_deathmatch_shoot(int n_envs, int n_agents, const MsDeathmatch* dm, void* hip_stream);

/* What the reference's Explorer env does between one frame and the next - `_reward`'s arithmetic, `_reset`'s counters and the
 * episode rule of `step`, megastep/demo/envs/explorer.py:45-90 - as one launch of N threads behind ms_render, whose first-sight
 * tally (MsRender.seen_count; the stamps and epochs are MsRender.seen_stamp / seen_epoch) it reads.  Per env n, in this order:
 *   reward   reset_out = over (this step began with a respawn); reward = over ? 0 : (tally - before) * (1.f/pixels) - in
 *            binary32, the reciprocal rounded first: what ATen makes of an int tensor over a Python int on the device (as of
 *            every tensor over a scalar: see ms_step_physics' IMU), so the env's tensor-op path gives the same bits at any
 *            pixel count, not only at powers of two;
 *            potential = tally, length_out = lengths - as this step leaves them (for display; optional)
 *   next     lengths += 1;  over = lengths >= tally + slack - the NEXT step's respawn mask (MsStepExtras.respawn_mask,
 *            respawn_after = 1) - and where it is set: epoch += 1 (the env forgets every texel at once), tally = lengths = 0;
 *            before = tally */
typedef struct MsExplorer {
    int*            tally;         /* (N) in / out: MsRender.seen_count                                          */
    int*            before;        /* (N) in / out: tally at the last reward                                      */
    int*            lengths;       /* (N) in / out: episode lengths                                               */
    int*            epoch;         /* (N) in / out: MsRender.seen_epoch                                           */
    unsigned char*  over;          /* (N) in: respawned this step; out: to be respawned by the next               */
    int             slack;         /* steps an episode lasts on top of one per texel seen (the reference's 200)   */
    int             pixels;        /* observation pixels per agent: res / subsample                               */
    unsigned char*  reset_out;     /* (N) out, optional                                                           */
    float*          reward;        /* (N) out                                                                     */
    float*          potential;     /* (N) out, optional                                                           */
    int*            length_out;    /* (N) out, optional                                                           */
} MsExplorer;
int ms_explorer_books(int n_envs, const MsExplorer* books, void* hip_stream);

/* Ray queries against the scenery (no counterpart in the reference, whose only rays are the render's camera fans,
 * kernels.cu:326-382): R rays per env, each from its own origin along its own direction vector, cast by the reference's
 * per-ray rule (kernels.cu:349-382) statement for statement - over the env's lines in line order, q = intersect(p, ru, L),
 * a hit when 0 <= q.t <= 1, better when near/|ru| < q.s < nearest - 1e-4; dot = dot(ru, v)/(|ru||v| + 1e-6), distance =
 * nearest*|ru| - with the same outputs and miss values as ms_render.  With agents, the lines are the static walls and every
 * agent's model drawn at its current pose (the rows ms_render would leave in lines_vals, computed in registers: lines_vals
 * is only read); without (NULL), the static walls alone.  The wall grid is used where it is exact - the origin inside its
 * env's grid, near*1.001 < wg_near and 1 <= |ru|^2 <= 64 - and every line of the env otherwise; same bits either way. */
typedef struct MsRaycast {
    int          n_rays;      /* R: rays per env                                                              */
    const float* origins;     /* (N, R, 2) p, 8-byte aligned                                                  */
    const float* dirs;        /* (N, R, 2) ru (any length), 8-byte aligned                                    */
    float        near_plane;  /* hits at s <= near/|ru| are ignored (ms_render: MsConfig.agent_radius)        */
    int*         indices;     /* (N, R) line index within the env, -1 on a miss      (each output NULL = not wanted) */
    float*       locations;   /* (N, R) position along the line, NaN on a miss       */
    float*       dots;        /* (N, R) ray . line direction,    NaN on a miss       */
    float*       distances;   /* (N, R) metres, +inf on a miss                       */
    int*         agents;      /* (N, R) agent whose model the ray hit, else -1       */
    int*         grid_rays;   /* optional counter (tests): rays that took the wall grid are added to grid_rays[0] */
} MsRaycast;
/* config: agent_radius is unused (the near plane travels in MsRaycast), res and fov are not needed either; it may be NULL. */
int ms_raycast(const MsScenery* scenery, const MsAgents* agents /* NULL: static walls only */, const MsRaycast* rays,
               const MsConfig* config, void* hip_stream);
/* The direction vector ru of every camera ray ms_render casts with `config` (res, fov): (N, A, res, 2), by the render's own
 * device code (ray_y, kernels.cu:234-236,334-337).  Cast from the agents' positions by ms_raycast with near = agent_radius
 * and the agents, these rays give ms_render's indices, locations, dots and distances bit for bit.  Reads angles only. */
int ms_camera_rays(const MsAgents* agents, int n_envs, int n_agents, const MsConfig* config, float* dirs, void* hip_stream);

/* Shading of rays the caller gives (the reference shades only the rays of its own render, shader_kernel, kernels.cu:407-450):
 * for ray r of env n, with the index, location and dot ms_raycast wrote for it, screen[n, r] is what ms_render's `screen` holds
 * for a ray with those values - (0, 0, 0) on a miss (index < 0) and for an index that is no line of the env (nothing is read for
 * it) or a location outside [0, 1] (which ms_raycast never writes for a hit); else, with f = the 2-tap texel filter at `location` along the line, (1 - dot^2) intensity (f.lw tl[k] + f.rw tr[k]), where
 * intensity is the baked light under the filter on a static line, and on an agent's row (index < n_agents n_model) the
 * reference's light_intensity at the hit point a (1 - location) + b location of the row (a, b) drawn from the agent's CURRENT
 * pose - in registers: lines_vals is neither read for it nor written.  Without agents (NULL) rays on an agent's row are black.
 * Every operation is the render's own binary32 operation in the render's order: on the rays of ms_camera_rays, cast from the
 * agents' positions, the result is ms_render's `screen` bit for bit.  A light grid in the scenery (lg_vals) is used where it is
 * there; without one the lights are tested against every static line.  Same bits either way. */
typedef struct MsShade {
    int          n_rays;      /* R: rays per env                                                              */
    const int*   indices;     /* (N, R) as ms_raycast writes them                                             */
    const float* locations;   /* (N, R)                                                                       */
    const float* dots;        /* (N, R)                                                                       */
    float*       screen;      /* (N, R, 3) out                                                                */
} MsShade;
/* config: nothing of it is needed; it may be NULL. */
int ms_shade(const MsScenery* scenery, const MsAgents* agents /* NULL: agent rows are black */, const MsShade* query,
             const MsConfig* config, void* hip_stream);

/* Rays of cameras that stand anywhere: camera c of env n at poses[n, c] = (x, y, heading in degrees) casts `res` rays, ray 0
 * leftmost as in the render; origins and dirs are (N, C res, 2), camera after camera, ready for ms_raycast.
 *   MS_CAMERA_PLANE  the render's projection, 0 < fov < 180: sincospi(heading/180) and the column's ray on the screen plane, by
 *                    the device code behind ms_camera_rays (same bits for the same heading, res and fov)
 *   MS_CAMERA_RING   rays evenly spaced in angle, 0 < fov <= 360: ray r points along heading + fov (res - 2r - 1)/(2 res)
 *                    degrees; unit vectors.  360 is a panorama, which no plane can show. */
#define MS_CAMERA_PLANE 0
#define MS_CAMERA_RING  1
typedef struct MsCameraPoses {
    int          n_envs, n_cameras, res;   /* N, C, rays per camera                                           */
    const float* poses;       /* (N, C, 3) x, y, heading in degrees                                           */
    float        fov;         /* degrees                                                                      */
    int          projection;  /* MS_CAMERA_PLANE or MS_CAMERA_RING                                            */
    float*       origins;     /* (N, C res, 2) out, 8-byte aligned                                            */
    float*       dirs;        /* (N, C res, 2) out, 8-byte aligned                                            */
} MsCameraPoses;
int ms_camera_pose_rays(const MsCameraPoses* cameras, void* hip_stream);

/* Top-down pictures of the envs (the reference draws them with matplotlib, plotting.py; no kernel): image k shows env
 * envs[k] through n_views views.  A view is six floats g, an affine map from pixel coordinates to world metres; every
 * step below is one binary32 operation, in this order, without contraction.
 *   pixel (row i from the top, column j):  u = j + 0.5, w = i + 0.5, x = (g0 u + g1 w) + g2, y = (g3 u + g4 w) + g5
 *   line l of the env (env-local, rows (ax, ay, bx, by)):  vx = bx - ax, vy = by - ay, px = x - ax, py = y - ay,
 *     vv = vx vx + vy vy, t = vv > 0 ? (px vx + py vy)/vv : 0 clamped to [0, 1] (a NaN stays NaN),
 *     dx = px - t vx, dy = py - t vy, d2 = dx dx + dy dy; the line covers the pixel when d2 <= h h (h = half_width)
 *   the winner: the covering line of least d2, the lower index on equal d2 (a NaN never covers); its colour is texel
 *     q = min((int)(t (float)width_l), width_l - 1) of the line: texture[q] baked[q] for a static line when `lit`,
 *     texture[q] otherwise, (0, 0, 0) for a line without texels; a pixel no line covers: `background` and index -1.
 * With agents, the A M agent rows are drawn at the agents' current poses (the rows ms_render would leave in lines_vals, in
 * registers: nothing is written to the scenery); without (NULL), they are read as lines_vals holds them.  An env id out of
 * [0, n_envs) gives an image of `background` and -1; env ids are read on the device only. */
typedef struct MsOverhead {
    int          n_images;       /* K                                                                    */
    int          n_views;        /* V: views per image                                                   */
    int          height, width;  /* H, W: pixels                                                         */
    const int*   envs;           /* (K,) env of every image; NULL: image k shows env k                   */
    const float* views;          /* (K, V, 6) g0..g5 of every view                                       */
    float        half_width;     /* h, metres (>= 0)                                                      */
    int          lit;            /* static lines' texels times their baked light                         */
    float        background[3];  /* linear RGB of a pixel no line covers                                 */
    float*       rgb;            /* (K, V, 3, H, W) linear RGB, planar   (either output NULL = not wanted; not both) */
    int*         indices;        /* (K, V, H, W) env-local line index, -1 where none                    */
} MsOverhead;
int ms_overhead(const MsScenery* scenery, const MsAgents* agents /* NULL: agent rows as stored */, const MsOverhead* overhead,
                void* hip_stream);

/* Rollouts: what happens if agent (n, a) takes each of K candidate action plans of H steps, in one launch (no counterpart in
 * the reference, where the only way to know is to step a copy of the world once per plan and step).  The scenery and the
 * agents are READ ONLY.  For every (n, a, k), from agent (n, a)'s (p, ang, v, w) as they stand, for h = 0 .. H-1 in this order
 * - every statement the one ms_move_physics makes (kernels.cu:179-230, modules.py:57-66,106-118), on the same functions:
 *   move      (v, w) <- the movement prologue (MsMovement) of table row actions[n, a, k, h], clamped to the table
 *   walls     x = min(1, collision_cs(p, v/fps, wall, agent_radius)) over ALL static lines of env n (those from
 *             n_agents*n_model on); the wall grid's near lists and the reach culls stand in front of the test where
 *             ms_physics uses them - the pose inside the grid, the reach at most wg_reach - and every static line otherwise:
 *             every value lies in [+0, 1] and the fold is a minimum, so the bits are the same
 *   others    with others = 1: x = min(x, collision_cc(p, v/fps, p_b, (0, 0), agent_radius)) over the env's other agents b != a
 *             where the call found them - they stand still for the whole horizon; others = 0: they are absent
 *   advance   the integration epilogue: p += x v/fps, ang likewise and normalised; x < 1: v = w = 0
 * Outputs (one writer each): the state after step H-1, progress = the least x, stops = the steps with x < 1, first_stop = the
 * first of them (H: none), and optionally the position after every step.  With a mask only the marked agents are rolled and
 * the rows of the others are left as they are.  Not in a rollout: other agents that move (MsScenarios below), respawns,
 * lifespans, the IMU.
 * Nothing is allocated, no global atomics, nothing waits for the host: the call can be captured in a HIP graph.  1 <= K <= 256,
 * 1 <= H <= 64, n_actions >= 1, others in {0, 1}: MS_EINVAL otherwise, before anything is launched.
 * slide = 1: `walls`, `others` and `advance` are the sliding step's (MsSlide above: phase A, the contact, phase B with `bounce`),
 * the others at rest in both phases; stops and first_stop count the steps whose velocity was zeroed, and `slides` the steps
 * that slid the whole of their remainder (x2 = 1).  slide in {0, 1}, 0 <= bounce <= 1 with slide: MS_EINVAL otherwise.  (The
 * three fields are the struct's last and MS_ABI_VERSION stays 17: a zeroed tail is the call as it was.) */
typedef struct MsRollouts {
    int                  n_candidates;  /* K                                                                           */
    int                  horizon;       /* H                                                                           */
    const long long*     actions;       /* (N, A, K, H) rows of `table`; shared_plans != 0: (K, H), the same for every agent */
    int                  shared_plans;
    const float*         table;         /* (n_actions, 3) [dx, dy, dw], as MsMovement's                                */
    int                  n_actions;
    float                keep;          /* as MsMovement's                                                             */
    int                  others;        /* 1: the env's other agents are obstacles, at rest; 0: absent                 */
    const unsigned char* mask;          /* (N, A) bytes, optional: non-zero = roll this agent                          */
    float*               positions;     /* (N, A, K, 2) out, 8-byte aligned                                            */
    float*               angles;        /* (N, A, K) out                                                               */
    float*               velocity;      /* (N, A, K, 2) out, 8-byte aligned                                            */
    float*               angvelocity;   /* (N, A, K) out                                                               */
    float*               progress;      /* (N, A, K) out                                                               */
    int*                 stops;         /* (N, A, K) out                                                               */
    int*                 first_stop;    /* (N, A, K) out                                                               */
    float*               trail;         /* (N, A, K, H, 2) out, optional, 8-byte aligned                               */
    int                  slide;         /* 1: every step is the sliding step                                           */
    float                bounce;        /* as MsSlide's                                                                */
    int*                 slides;        /* (N, A, K) out, optional: the steps that slid their whole remainder          */
} MsRollouts;
int ms_rollouts(const MsScenery* scenery, const MsAgents* agents, const MsRollouts* rollouts, const MsConfig* config,
                void* hip_stream);

/* Scenarios: whole envs forked S ways and stepped H times, every agent on a plan of its own, in one launch - the multi-agent
 * completion of MsRollouts (no counterpart in the reference, where the only way to know is to step a copy of the world once
 * per scenario and step).  The scenery and the agents are READ ONLY.  For every env n and scenario s, from ALL agents'
 * (p, ang, v, w) as they stand, for h = 0 .. H-1 in this order - every statement the one ms_move_physics makes of a copy of
 * env n (kernels.cu:179-230, modules.py:57-66,106-118), on the same functions:
 *   move      for every agent a: (v_a, w_a) <- the movement prologue (MsMovement) of table row act(n, s, a, h), clamped
 *   meet      for every agent a: x_a = min(1, collision_cs(p_a, v_a/fps, wall, agent_radius) over ALL static lines of env n,
 *             collision_cc(p_a, v_a/fps, p_b, v_b/fps, agent_radius) over every other agent b != a) - everybody's (p, v) after
 *             `move` and before `advance`: the ordered-pair test of kernels.cu:193-205, the other's moved velocity where
 *             MsRollouts has (0, 0).  The reach culls and the wall grid's near lists stand in front of the tests where
 *             ms_physics uses them - the pose inside the grid, the reach at most wg_reach - and every static line otherwise:
 *             every value lies in [+0, 1] and the fold is a minimum, so the bits are the same
 *   advance   for every agent: the integration epilogue with x_a; x_a < 1: v_a = w_a = 0
 * Where act comes from - focal = 0 (joint): actions (N, S, A, H), or (S, A, H) with shared != 0; the outputs have one row per
 * (n, s, a) and the mask is (N,).  focal = 1: n_scenarios is K; scenario (f, k) puts agent f on actions[n, f, k, :] - (N, A, K, H),
 * or (K, H) with shared != 0 - and every other agent b on base[n, b, :] ((N, A, H)); only agent f's row is written, the outputs
 * are MsRollouts' (N, A, K, ..) and the mask is (N, A), the focal agents.  Focal is joint on the expanded tensor.
 * Outputs (one writer each): the state after step H-1, progress = the least x, stops = the steps with x < 1, first_stop = the
 * first of them (H: none), and optionally the position after every step.  A row the mask leaves out is not written.
 * Not in a scenario: sliding steps, respawns, lifespans, the IMU.  Nothing is allocated, no global atomics, nothing waits
 * for the host: the call can be captured in a HIP graph.  1 <= n_scenarios <= 256, 1 <= H <= 64, n_actions >= 1, keep a number,
 * focal and shared in {0, 1}, every pointer and its alignment, a wall grid given whole: MS_EINVAL otherwise; more than 64
 * agents an env: MS_EUNSUPPORTED (a lane an agent) - all before anything is launched. */
typedef struct MsScenarios {
    int                  n_scenarios;   /* S; focal: K                                                                 */
    int                  horizon;       /* H                                                                           */
    int                  focal;         /* 0: joint; 1: focal                                                          */
    const long long*     actions;       /* joint (N, S, A, H) | shared (S, A, H); focal (N, A, K, H) | shared (K, H); 8-byte aligned */
    int                  shared;
    const long long*     base;          /* focal: (N, A, H), what the agents that are not focal do; joint: not read    */
    const float*         table;         /* (n_actions, 3) [dx, dy, dw], as MsMovement's                                */
    int                  n_actions;
    float                keep;          /* as MsMovement's                                                             */
    const unsigned char* mask;          /* joint (N,), focal (N, A) bytes, optional: non-zero = roll                   */
    float*               positions;     /* joint (N, S, A, 2), focal (N, A, K, 2) out, 8-byte aligned                  */
    float*               angles;        /* (N, S, A) | (N, A, K) out, as every output below                            */
    float*               velocity;      /* (.., 2) out, 8-byte aligned                                                 */
    float*               angvelocity;
    float*               progress;
    int*                 stops;
    int*                 first_stop;
    float*               trail;         /* (.., H, 2) out, optional, 8-byte aligned                                    */
} MsScenarios;
int ms_scenarios(const MsScenery* scenery, const MsAgents* agents, const MsScenarios* scenarios, const MsConfig* config,
                 void* hip_stream);

/* Shortest-path distance fields on the floorplans: how far it is from a point to a goal when one has to walk round the
 * walls.  Every step below is one binary32 operation, in the order given, without contraction: tests/test_navfield_host.py
 * restates it in numpy bit for bit (nav_rule), and the GPU tests hold the kernels to EQUALITY with it.
 *   nav grid      Env n's cells are squares of side c = cell; column j, row i (y grows with i) has the centre
 *                 x = ((float)(jx0 + j) + 0.5f)*c, y = ((float)(iy0 + i) + 0.5f)*c.  geom[n] = (jx0, iy0, nx, ny) is the
 *                 caller's (cuda.nav_grid: the static walls' bounding box and one cell of margin); env n's nx*ny cells
 *                 start at starts[n], row-major: ragged, not padded.
 *   free cells    A cell is blocked (0) when any STATIC line of its env (lines from n_agents*n_model on) covers its centre
 *                 under MsOverhead's rule with half_width = r = clearance - the same vx, vy, px, py, vv, t, dx, dy, d2
 *                 sequence, d2 <= r*r; a NaN never covers - else free (1).  Agent rows are not looked at.
 *   edges         A free cell is joined to its free 4-neighbours with weight ws = c, and to a free diagonal neighbour with
 *                 weight wd = c*1.41421356f only if the two cells that share a side with both are free too (no corner is
 *                 cut).  c <= 1.4f*r is required: a wall across an edge between two free centres would come within half
 *                 the edge's length, at most c sqrt(2)/2 <= 0.99 r, of the nearer one, which would then be blocked - so
 *                 no path of the graph passes through a wall, however thin or oblique.
 *   anchors       of a point p = (x, y): fx = floorf(x/c - 0.5f), fy likewise; without anchors when either is a NaN or
 *                 |.| >= 2^30; else j0 = (int)fx - jx0, i0 = (int)fy - iy0 and the anchors are those of the four cells
 *                 (i0 + {0,1}, j0 + {0,1}) that lie in the grid and are free.  leg(a) = sqrtf(dx*dx + dy*dy), (dx, dy)
 *                 from the anchor's centre to p, the root correctly rounded.  A leg is at most c sqrt(2) <= 1.98 r long:
 *                 from a point further than r from every wall (an agent's centre, a spawn point) it crosses no wall.
 *   field         of goal p: D[a] = leg(a) at p's anchors, then the least fixed point of D[v] = min(D[v], D[u] + w(u, v))
 *                 over all edges; +inf on blocked cells, on cells no path reaches, everywhere when p has no anchor.
 *                 x -> fl(x + w) is monotone and every value a cell ever holds is the left-to-right binary32 sum along a
 *                 path from an anchor, so the fixed point does not depend on the order of relaxation: it is what Dijkstra
 *                 with binary32 additions returns.  The 8-connected metric: up to 8 % above the any-angle shortest path.
 *   query         g(p) = min over p's anchors a of (D[a] + leg(a)); +inf without an anchor or with a goal index out of
 *                 [0, n_goals).
 * All outputs are the caller's; nothing is allocated, nothing waits for the device: all three calls can be captured in a
 * HIP graph.  Every argument is checked in full before the first launch (MS_EINVAL). */
typedef struct MsNavGrid {
    int                  n_envs;       /* N                                                                            */
    float                cell;         /* c, metres (> 0, <= 1.4f*clearance)                                           */
    float                clearance;    /* r, metres (> 0)                                                              */
    const int*           geom;         /* (N, 4) jx0, iy0, nx, ny; 16-byte aligned                                     */
    const long long*     starts;       /* (N+1,) first cell of every env; starts[N] = all cells                        */
    int                  max_framed;   /* the largest (nx + 2)*(ny + 2) of any env with cells (0: no env has any): sizes
                                          the launches; a larger env still gets the right bits, slowly                  */
    unsigned char*       free_cells;   /* (starts[N],) 1 free, 0 blocked: written by ms_nav_free, read by the others   */
} MsNavGrid;
typedef struct MsNavFields {
    int                  n_goals;      /* G: goals (fields) per env                                                    */
    const float*         goals;        /* (N, G, 2) x, y; 8-byte aligned                                               */
    const unsigned char* mask;         /* (N, G) non-zero: compute this field; NULL: all.  Read on the device only.    */
    float*               fields;       /* G*starts[N] floats: field (n, g) at G*starts[n] + g*nx*ny, row-major         */
    int*                 passes;       /* (N, G) or NULL: relaxation passes each computed field took (telemetry)       */
} MsNavFields;
typedef struct MsNavQuery {
    int                  n_points;     /* P: points per env                                                            */
    const float*         points;       /* (N, P, 2) x, y; 8-byte aligned                                               */
    const int*           goal;         /* (N, P) which of the env's fields each point asks; NULL: P == G, point k field k */
    const float*         fields;       /* as MsNavFields.fields                                                        */
    int                  n_goals;      /* G of `fields`                                                                */
    float*               out;          /* (N, P) g(p)                                                                  */
} MsNavQuery;
/* ms_nav_free    fills grid->free_cells from the scenery's static walls (one-off per scenery and (cell, clearance)).
 * ms_nav_fields  computes the fields of the marked goals, one workgroup per field, the field resident in LDS while it
 *                fits (about 32 000 cells); fields that are masked out are left as they are.
 * ms_nav_query   g(p) for P points per env, each against one of the env's G fields. */
int ms_nav_free(const MsScenery* scenery, const MsNavGrid* grid, void* hip_stream);
int ms_nav_fields(const MsNavGrid* grid, const MsNavFields* fields, void* hip_stream);
int ms_nav_query(const MsNavGrid* grid, const MsNavQuery* query, void* hip_stream);

/* Paths and look-ahead waypoints on the distance fields: which way to go, not only how far.  As above every step is one
 * binary32 operation in the order given, without contraction; tests/test_navpath_host.py restates it in numpy (path_rule)
 * and the kernels - and their host instantiations, ms_host_nav_waypoint / ms_host_nav_path - are held to EQUALITY with it.
 * c, free, centre, leg and the anchor corner (i0, j0) are MsNavGrid's; D is the field of goal q = goals[n, g]; p the point.
 *   start         over p's anchor cells in the query's order - t = 0..3, cell (i0 + (t>>1), j0 + (t&1)), in range, D < +inf:
 *                 a* is the first that attains the least fl(D[a] + leg(p, a)) (replaced on a strict <, from +inf).  None:
 *                 no path - exactly when ms_nav_query gives +inf, a goal index out of [0, n_goals) and an env without
 *                 cells included.
 *   hop           from cell v = (i, j).  If v is one of the four cells (iq0 + {0,1}, jq0 + {0,1}) round q (q has an anchor
 *                 corner) and leg(q, v) == D[v], the chain ends at v: its next and last point is q itself.  Otherwise over
 *                 the neighbours u = (i + di, j + dj) in the order (di, dj) = (0,+1) (+1,0) (0,-1) (-1,0) (+1,+1) (+1,-1)
 *                 (-1,-1) (-1,+1): a neighbour counts if it is in range and free, a diagonal one only if (i + di, j) and
 *                 (i, j + dj) are free too; its value is fl(D[u] + w), w = c straight, c*1.41421356f diagonal.  The next
 *                 cell is the first neighbour that attains the least value (replaced on a strict <, from +inf), provided
 *                 D[u] < D[v] - at a fixed point of the relaxation that least value IS D[v].  No such neighbour (a stale or
 *                 foreign field): the chain is BROKEN and stops there; D falls at every hop, so no input makes a chain
 *                 longer than the env's cells.
 *   chain         x_0 = centre(a*), x_1, ... the centres of the cells the hops reach, the last point q.
 *   sight         from p to a point x: dx = x.x - p.x, dy = x.y - p.y, len = sqrtf(dx*dx + dy*dy), k = ceilf(len/(0.5f*c)),
 *                 K = (int)k (no sight when k is not below 2^20); for s = 1 .. K-1: t = (float)s/(float)K, the sample
 *                 (p.x + dx*t, p.y + dy*t), its anchor corner (i0, j0): all four cells (i0 + {0,1}, j0 + {0,1}) must be in
 *                 range and free.  True when every sample passes (vacuously for K <= 1).  Every point of the segment is
 *                 within c/2 of a sample or an end, so inside the block of four free cells round that sample or inside a
 *                 free end cell: the centre of the cell it lies in is free and within 0.71 c <= 0.99 r of it - a wall
 *                 through the point would have blocked that centre (the edges' argument, the same 1 % margin).
 *   waypoint      with look-ahead L (1..64): the candidates are the first L chain points x_0 .. x_{n-1} (n < L where the chain
 *                 ends or breaks earlier).  The base index b = 1 when leg(p, x_0) <= 0.5f*c and n >= 2, else 0: x_b is
 *                 always admissible (for b = 1, p lies inside cell x_0 and p -> x_1 stays in x_0, x_1 and the two open side
 *                 cells of a diagonal; without it a point ON a centre next to a wall would be sent to where it stands).
 *                 k > b is admissible when sight(p, x_k).  The waypoint is x_k for the LARGEST admissible k; hops = k.
 *                 NaN, NaN and hops = -1 without a path.  A broken chain offers the points it got.
 *   path          p, x_0, x_1, ..., q into (N, P, M, 2), NaN in the slots not written; counts = the number of points of the
 *                 whole path however long (the first M are written), 0 without a path, the number got, negated, for a
 *                 broken chain.
 * Other agents are no obstacles: the grid is the building.  Nothing is allocated, nothing waits, no float atomics: both
 * calls can be captured in a HIP graph.  Every argument is checked in full before the first launch (MS_EINVAL). */
typedef struct MsNavWaypoints {
    int                  n_points;     /* P: points per env                                                            */
    const float*         points;       /* (N, P, 2) x, y; 8-byte aligned                                               */
    const int*           goal;         /* (N, P) which of the env's fields each point follows; NULL: P == G, point k field k */
    const float*         fields;       /* as MsNavFields.fields                                                        */
    const float*         goals;        /* (N, G, 2) the fields' goals, as MsNavFields.goals; 8-byte aligned            */
    int                  n_goals;      /* G of `fields` and `goals`                                                    */
    int                  lookahead;    /* L, 1..64                                                                     */
    float*               waypoints;    /* (N, P, 2) out; 8-byte aligned                                                */
    int*                 hops;         /* (N, P) out, or NULL: the chosen index k, -1 without a path                   */
} MsNavWaypoints;
typedef struct MsNavPaths {
    int                  n_points;     /* P                                                                            */
    const float*         points;       /* (N, P, 2); 8-byte aligned                                                    */
    const int*           goal;         /* (N, P) or NULL, as above                                                     */
    const float*         fields;
    const float*         goals;        /* (N, G, 2); 8-byte aligned                                                    */
    int                  n_goals;
    int                  max_points;   /* M >= 2: points written per path                                              */
    float*               paths;        /* (N, P, M, 2) out                                                             */
    int*                 counts;       /* (N, P) out                                                                   */
} MsNavPaths;
/* ms_nav_waypoints  one wavefront per point (the per-step call of an expert: N x A points).
 * ms_nav_paths      one lane per point; walks every chain to its end. */
int ms_nav_waypoints(const MsNavGrid* grid, const MsNavWaypoints* waypoints, void* hip_stream);
int ms_nav_paths(const MsNavGrid* grid, const MsNavPaths* paths, void* hip_stream);

/* Seeded fields: how far it is on foot to the NEAREST of a set of cells, and which way - the distance to the nearest floor an
 * agent has not seen (the frontier), to the nearest door cell, to any of K pickups.  The graph, its weights and the binary32
 * discipline are MsNavGrid's; tests/test_navseed_host.py restates the rule in numpy (seed_rule) and the kernels - and their
 * host instantiations, ms_host_nav_seed_field / _waypoint / _path - are held to EQUALITY with it.
 *   marks         a byte per cell and field, in MsNavSeen.maps' / MsNavFields.fields' layout: field (n, g) reads the nx*ny
 *                 bytes from G*starts[n] + g*nx*ny (a seen map is one).  `among`, starts[N] bytes in free_cells' layout shared
 *                 by an env's fields, or NULL.  Both are read when the call runs, not kept.
 *   seed          cell k is a seed of field (n, g) when free[k] & 1, and among == NULL or among[k] & 1, and
 *                 (marks[k] & 1) == where, where in {0, 1}.
 *   field         D[seed] = +0.f, then the least fixed point of D[v] = min(D[v], fl(D[u] + w(u, v))) over MsNavGrid's edges:
 *                 +inf on blocked cells, on cells no seed reaches, everywhere without a seed.  Every value is still the
 *                 left-to-right binary32 sum along a path from some seed and x -> fl(x + w) is monotone: the fixed point does
 *                 not depend on the order of relaxation, and is what a multi-source Dijkstra with binary32 additions returns,
 *                 as bits.  D[v] == 0 exactly on seeds: every other cell holds a sum of positive weights.
 *   n_seeds       the seeds of field (n, g); 0 for an env without cells.
 *   query         ms_nav_query serves a seeded field as it is.
 *   following     MsNavWaypoints' rule with one change - there is no goal point.  start: unchanged.  hop: from cell v, if
 *                 D[v] == 0.f the chain ends at v: centre(v) is its last point and nothing follows it; otherwise the hop
 *                 is unchanged.  chain, sight, the base index b and "the largest admissible k": unchanged.  A start whose a*
 *                 is a seed has the chain [x_0]: the waypoint is x_0 and hops = 0.  NaN, NaN and hops = -1 where the query
 *                 gives +inf.  path: p, x_0, ..., the seed's centre; counts positive when the chain ended on a seed, the
 *                 number got, negated, for a broken chain, 0 without a path.
 * One launch each, the launches of ms_nav_fields / ms_nav_waypoints / ms_nav_paths; masked-out fields keep fields, passes and
 * n_seeds as they are.  Nothing is allocated, nothing waits: all can be captured in a HIP graph.  Every argument is checked in
 * full before the launch (MS_EINVAL). */
typedef struct MsNavSeedFields {
    int                  n_fields;     /* G: fields per env                                                            */
    const unsigned char* marks;        /* G*starts[N] bytes, bit 0: the field's layout                                 */
    int                  where;        /* 0 or 1: a seed's mark                                                        */
    const unsigned char* among;        /* (starts[N],) bit 0: the cell may be a seed; NULL: every free cell may        */
    const unsigned char* mask;         /* (N, G) non-zero: compute this field; NULL: all.  Read on the device only.    */
    float*               fields;       /* G*starts[N] floats out, as MsNavFields.fields                                */
    int*                 passes;       /* (N, G) or NULL: relaxation passes each computed field took (telemetry)       */
    int*                 n_seeds;      /* (N, G) or NULL: the seeds of each computed field                             */
} MsNavSeedFields;
typedef struct MsNavSeedWaypoints {    /* MsNavWaypoints without goals                                                 */
    int                  n_points;
    const float*         points;       /* (N, P, 2); 8-byte aligned                                                    */
    const int*           goal;         /* (N, P) which of the env's fields each point follows; NULL: P == G            */
    const float*         fields;       /* as MsNavSeedFields.fields                                                    */
    int                  n_goals;      /* G of `fields`                                                                */
    int                  lookahead;    /* L, 1..64                                                                     */
    float*               waypoints;    /* (N, P, 2) out; 8-byte aligned                                                */
    int*                 hops;         /* (N, P) out, or NULL                                                          */
} MsNavSeedWaypoints;
typedef struct MsNavSeedPaths {        /* MsNavPaths without goals                                                     */
    int                  n_points;
    const float*         points;       /* (N, P, 2); 8-byte aligned                                                    */
    const int*           goal;         /* (N, P) or NULL, as above                                                     */
    const float*         fields;
    int                  n_goals;
    int                  max_points;   /* M >= 2                                                                       */
    float*               paths;        /* (N, P, M, 2) out                                                             */
    int*                 counts;       /* (N, P) out                                                                   */
} MsNavSeedPaths;
int ms_nav_seed_fields(const MsNavGrid* grid, const MsNavSeedFields* fields, void* hip_stream);
int ms_nav_seed_waypoints(const MsNavGrid* grid, const MsNavSeedWaypoints* waypoints, void* hip_stream);
int ms_nav_seed_paths(const MsNavGrid* grid, const MsNavSeedPaths* paths, void* hip_stream);

/* Cost fields: seeded fields over per-cell cost layers - an inflation layer that keeps paths off the walls, unseen floor priced
 * instead of forbidden, cells an opponent sees or another agent's territory made dear.  Grid, seeds (marks, where, among), graph
 * and corner rule are MsNavSeedFields' as they stand; tests/test_navcost_host.py restates the rule in numpy (cost_rule) and the
 * kernels - and their host instantiations, ms_host_nav_cost_field / _waypoint / _path - are held to EQUALITY with it.
 *   costs         a float per cell: one store per env in free_cells' layout (n_costs == 1: env n's nx*ny floats from starts[n],
 *                 shared by its fields) or one per field in the fields' layout (n_costs == n_fields: field (n, g)'s from
 *                 G*starts[n] + g*nx*ny).  Read when the call runs, not kept.
 *   multiplier    of cell v, from x = costs[v] in binary32: k_v = x >= 1.f ? fminf(x, 256.f) : (x < 1.f ? 1.f : 256.f) - values
 *                 below 1 count as 1, +inf counts as 256 (NAV_COST_MAX), and a NaN is the dearest, not the cheapest.  No cost
 *                 closes a cell: which cells are free, which diagonals are open and what a waypoint's sight crosses are untouched.
 *   weights       a step from v to a neighbour, towards the seeds, costs ws_v = fl(c*k_v) when straight and
 *                 wd_v = fl(fl(c*1.41421356f)*k_v) when diagonal: the weight depends on the cell being LEFT and on the kind of
 *                 step only.  Multiplying by 1.f is exact: k = 1 everywhere gives MsNavSeedFields' weights, and its bits.
 *   field         D[seed] = +0.f whatever the seed's own cost, then the least fixed point of
 *                 D[v] = min(D[v], fl(min over straight u of D[u] + ws_v), fl(min over open diagonal u of D[u] + wd_v)).
 *                 x -> fl(x + w) is monotone for every w, so the min may be taken first, every value is the left-to-right
 *                 binary32 sum along a path from some seed, and the fixed point does not depend on the order of relaxation: it
 *                 is what a multi-source Dijkstra with binary32 additions over these directed weights returns, as bits.
 *   following     MsNavSeedFields' rule with the weights of the cell the hop leaves: from v the first of the eight neighbours,
 *                 in MsNavWaypoints' order, that attains the least fl(D[u] + w_t(v)), provided D[u] < D[v]; the chain ends on
 *                 D == 0.f.  Start, sight, look-ahead, the base index and the paths' counts: unchanged.
 *   query         ms_nav_query serves a cost field as it is: the leg from a point to its anchor's centre, under a cell long,
 *                 is charged at 1, whatever the cells under it cost.
 *   strictness    a hop needs fl(D + w) > D, which holds while D < c*2^24; with k <= 256 that is so for chains of fewer than
 *                 about 46 000 hops at the maximal cost - more cells than the largest LDS tier holds.  Beyond that a chain is
 *                 reported broken (NaN waypoint, negated count), as a stale field is today.  Nothing hangs.
 * One launch each; masked-out fields keep fields, passes and n_seeds as they are.  Nothing is allocated, nothing waits: all can
 * be captured in a HIP graph.  Every argument is checked in full before the launch (MS_EINVAL): what the seeded entries refuse,
 * a NULL or misaligned costs, an n_costs that is neither 1 nor the number of fields. */
typedef struct MsNavCostFields {
    int                  n_fields;     /* G: fields per env                                                            */
    const unsigned char* marks;        /* as MsNavSeedFields.marks                                                     */
    int                  where;        /* 0 or 1: a seed's mark                                                        */
    const unsigned char* among;        /* as MsNavSeedFields.among, or NULL                                            */
    const unsigned char* mask;         /* (N, G) non-zero: compute this field; NULL: all.  Read on the device only.    */
    float*               fields;       /* G*starts[N] floats out                                                       */
    int*                 passes;       /* (N, G) or NULL                                                               */
    int*                 n_seeds;      /* (N, G) or NULL                                                               */
    const float*         costs;        /* n_costs*starts[N] floats; 4-byte aligned                                     */
    int                  n_costs;      /* 1: a store per env; G: a store per field                                     */
} MsNavCostFields;
typedef struct MsNavCostWaypoints {    /* MsNavSeedWaypoints and the costs the fields were made with                   */
    int                  n_points;
    const float*         points;       /* (N, P, 2); 8-byte aligned                                                    */
    const int*           goal;         /* (N, P) which of the env's fields each point follows; NULL: P == G            */
    const float*         fields;       /* as MsNavCostFields.fields                                                    */
    int                  n_goals;      /* G of `fields`                                                                */
    int                  lookahead;    /* L, 1..64                                                                     */
    float*               waypoints;    /* (N, P, 2) out; 8-byte aligned                                                */
    int*                 hops;         /* (N, P) out, or NULL                                                          */
    const float*         costs;        /* as MsNavCostFields.costs                                                     */
    int                  n_costs;      /* 1 or G                                                                       */
} MsNavCostWaypoints;
typedef struct MsNavCostPaths {        /* MsNavSeedPaths and the costs the fields were made with                       */
    int                  n_points;
    const float*         points;       /* (N, P, 2); 8-byte aligned                                                    */
    const int*           goal;         /* (N, P) or NULL, as above                                                     */
    const float*         fields;
    int                  n_goals;
    int                  max_points;   /* M >= 2                                                                       */
    float*               paths;        /* (N, P, M, 2) out                                                             */
    int*                 counts;       /* (N, P) out                                                                   */
    const float*         costs;        /* as MsNavCostFields.costs                                                     */
    int                  n_costs;      /* 1 or G                                                                       */
} MsNavCostPaths;
int ms_nav_cost_fields(const MsNavGrid* grid, const MsNavCostFields* fields, void* hip_stream);
int ms_nav_cost_waypoints(const MsNavGrid* grid, const MsNavCostWaypoints* waypoints, void* hip_stream);
int ms_nav_cost_paths(const MsNavGrid* grid, const MsNavCostPaths* paths, void* hip_stream);

/* Pulled paths: a field's path straightened by sight - a handful of corners where the chain is a staircase of hundreds of cells,
 * and the length of the walk along them, the any-angle reference length a score such as SPL divides by.  Grid, fields, start, hop,
 * chain and sight are MsNavWaypoints' as they stand; on a seeded field (goals NULL) they are MsNavSeedFields', on a cost field
 * (costs not NULL) MsNavCostFields', hopping with the weights of the cell left.  Nothing is restated: the kernel calls the same
 * functions.  tests/test_navpull_host.py restates the rule in numpy (pull_rule) and the kernel - and its serial host statement,
 * ms_host_nav_pull - are held to EQUALITY with it.
 *   points        P_0 = p, P_1 = x_0, P_2 = x_1, ... the points MsNavPaths would write with unlimited max_points; the last is
 *                 the goal q, on a seeded field the seed's centre.  n is their number: cells = n is MsNavPaths' count, negated
 *                 for a broken chain.  A broken chain is pulled over the points it got.
 *   pull          with reach R (1..1024), a = 0 and V = [0], while a < n-1: k is the LARGEST index in (a, min(a + R, n-1)] that
 *                 is admissible - a+1 always is (the chain's own step; the leg from p to its anchor when a = 0), any k > a+1
 *                 when sight(P_a, P_k) holds, MsNavWaypoints' sight unchanged.  Append k to V and set a = k.  R = 1 gives the
 *                 chain itself.
 *   vertices      (N, P, M, 2): the first M of P_V[.], NaN in the slots not written.  indices (N, P, M) or NULL: V, -1 beyond.
 *   counts        (N, P): len(V) however long, negated when the chain is broken, 0 without a path.  cells (N, P) or NULL: as above.
 *   lengths       (N, P): from +0.f, in vertex order, L = fl(L + sqrtf(fl(fl(dx*dx) + fl(dy*dy)))), dx, dy the binary32
 *                 differences of consecutive vertices, without contraction; +inf without a path, the length got for a broken
 *                 chain.
 *   mask          (N, P) bytes read on the device, or NULL: a point whose byte is 0 keeps every output as it stands.
 * This is greedy string pulling, not the exact Euclidean shortest path: a pulled path is an upper bound on the true shortest walk
 * and - a step of the chain being always admissible, and a sight never longer than the chain it replaces - at most the chain's
 * own length up to rounding.  Its segments keep sight's clearance argument (MsNavWaypoints, "sight"); the first, from p to x_0,
 * and every step of the chain itself keep the edges' (MsNavGrid).
 * Every loop is bounded by the input: hops by the env's cells (D falls at every hop), anchors by n, candidates by reach, samples
 * by 2^20 - a stale or garbage field ends, as it does for MsNavPaths.  One launch, a wavefront a path; nothing is allocated,
 * nothing waits, no float atomics: the call can be captured in a HIP graph.  Every argument is checked in full before the launch
 * (MS_EINVAL): what MsNavPaths refuses, a reach outside 1..1024, a max_points outside 2..2^20, an n_costs that is neither 0, 1
 * nor G, costs NULL with n_costs != 0 (or given with n_costs == 0), a NULL vertices, counts or lengths, a misaligned pointer. */
typedef struct MsNavPulls {
    int                  n_points;     /* P                                                                            */
    const float*         points;       /* (N, P, 2); 8-byte aligned                                                    */
    const int*           goal;         /* (N, P) which of the env's fields each point follows; NULL: P == G            */
    const float*         fields;       /* as MsNavFields.fields (or MsNavSeedFields', MsNavCostFields')                */
    const float*         goals;        /* (N, G, 2) the fields' goals; 8-byte aligned.  NULL: seeded fields            */
    int                  n_goals;      /* G of `fields` and `goals`                                                    */
    const float*         costs;        /* as MsNavCostFields.costs; NULL: unweighted                                   */
    int                  n_costs;      /* 0 (costs NULL), 1 or G                                                       */
    int                  reach;        /* R, 1..1024: how many points ahead an anchor looks                            */
    int                  max_points;   /* M, 2..2^20: vertices written per path                                        */
    const unsigned char* mask;         /* (N, P) non-zero: pull this point; NULL: all.  Read on the device only.       */
    float*               vertices;     /* (N, P, M, 2) out                                                             */
    int*                 indices;      /* (N, P, M) out, or NULL                                                       */
    int*                 counts;       /* (N, P) out                                                                   */
    int*                 cells;        /* (N, P) out, or NULL                                                          */
    float*               lengths;      /* (N, P) out                                                                   */
} MsNavPulls;
int ms_nav_pulls(const MsNavGrid* grid, const MsNavPulls* pulls, void* hip_stream);

/* Seen maps: which cells of the nav grid the depth rays of an agent (of any viewer) have passed over - floor coverage for
 * exploration rewards, a mask to hand a policy or to draw.  As above every step is one binary32 operation in the order given,
 * without contraction, divisions and roots correctly rounded; tests/test_navseen_host.py restates it in numpy (seen_rule) and
 * the kernel - and its host instantiation, ms_host_nav_seen - are held to EQUALITY with it.  c, geom and starts are MsNavGrid's.
 *   maps          S maps per env; map (n, s) holds one byte per cell of env n, 0 unseen, 1 seen, row-major, and starts at
 *                 S*starts[n] + s*nx*ny (MsNavFields.fields' layout).  `countable`, starts[N] bytes shared by an env's maps
 *                 (bit 0), says which cells count; NULL: the grid's free_cells.
 *   viewers       P per env, R rays each: origins (N, P, 2), dirs (N, P, R, 2) of any length, distances (N, P, R) in metres -
 *                 what ms_render / ms_raycast return for the rays of ms_camera_rays.  slot (N, P) names the map viewer p
 *                 marks; NULL: P == S and viewer k marks map k.  A slot outside [0, S) skips the viewer.
 *   a ray         origin o, direction d, distance dist: rlen = sqrtf(dx*dx + dy*dy).  The ray is skipped when a component
 *                 of o or d is not finite, rlen is not finite or not > 0, dist is a NaN or not > 0.  reach = dist < max_range ?
 *                 dist : max_range (max_range finite and > 0; a ray that missed, +inf, reaches max_range); ux = dx/rlen,
 *                 uy = dy/rlen; ex = ux*reach, ey = uy*reach; K = (int)ceilf(sqrtf(ex*ex + ey*ey)/(0.5f*c)) - the sight's
 *                 count of MsNavWaypoints, samples at most half a cell apart; the ray is skipped when that is not below 2^20
 *                 (or a NaN); K = 0 counts as 1.
 *   samples       s = 0 .. K, both ends: t = (float)s/(float)K, x = ox + ex*t, y = oy + ey*t, fx = floorf(x/c),
 *                 fy = floorf(y/c).  A sample is skipped when fx or fy is a NaN or |.| >= 2^30; else j = (int)fx - jx0,
 *                 i = (int)fy - iy0, skipped when (i, j) is outside the grid; else cell (i, j) of the viewer's map is marked.
 *   a call        1. the maps named in reset ((N, S) bytes, non-zero; NULL: none) are cleared;  2. all rays mark;
 *                 3. gained[n, s] = the cells of map (n, s) that were 0 before the marks (after the reset), are 1 after and are
 *                 countable - a cell hit by many rays, or by two viewers of one map, counts once;  4. total[n, s] =
 *                 (reset ? 0 : total[n, s]) + gained[n, s].  Either output may be NULL.  An env without cells marks nothing
 *                 and gains 0.  Marks are idempotent and the counts integers: nothing depends on the order of execution.
 *   no wall is seen through (with free_cells as the countable mask).  A cell that straddles a wall has its centre within
 *                 0.71 c <= 0.99 r of it: blocked, never countable - the cell of a hit point that rounded to the wall's far
 *                 side included.  A countable cell that holds a sample has its centre within 0.71 c of a point the ray
 *                 reached, and no wall lies between the two: it would come within 0.71 c of the centre and block the cell.
 * One launch, one workgroup per map - the map's only writer in the call - with the call's marks as a bitmask in LDS, one bit
 * per cell: max_cells, the most cells (nx*ny) any env has, sizes it.  More than 2^20 (128 KiB of bits: a 128 m square at
 * 0.125 m): MS_EUNSUPPORTED, nothing enqueued; an env with more cells than max_cells says marks nothing and gains 0.  No
 * global atomics, nothing allocated, nothing waits: the call can be captured in a HIP graph.  Every argument is checked in
 * full before the launch (MS_EINVAL). */
typedef struct MsNavSeen {
    int                  n_maps;       /* S: maps per env                                                              */
    int                  n_viewers;    /* P: viewers per env                                                           */
    int                  n_rays;       /* R: rays per viewer                                                           */
    const float*         origins;      /* (N, P, 2); 8-byte aligned                                                    */
    const float*         dirs;         /* (N, P, R, 2); 8-byte aligned                                                 */
    const float*         distances;    /* (N, P, R)                                                                    */
    const int*           slot;         /* (N, P) the map each viewer marks; NULL: P == S, viewer k map k               */
    float                max_range;    /* metres, finite and > 0                                                       */
    const unsigned char* reset;        /* (N, S) non-zero: clear the map first; NULL: none                             */
    const unsigned char* countable;    /* (starts[N],) bit 0: the cell counts; NULL: the grid's free_cells             */
    unsigned char*       maps;         /* S*starts[N] bytes in / out: map (n, s) at S*starts[n] + s*nx*ny              */
    int*                 gained;       /* (N, S) out, or NULL                                                          */
    int*                 total;        /* (N, S) in / out, or NULL                                                     */
    int                  max_cells;    /* the largest nx*ny of any env (0: no env has cells), at most 2^20             */
} MsNavSeen;
int ms_nav_seen(const MsNavGrid* grid, const MsNavSeen* seen, void* hip_stream);

/* Age maps: WHEN each cell of the nav grid was last passed over by a depth ray - idleness, for patrol, surveillance and search
 * tasks that do not end when the floor runs out.  Grid, geometry, the stores' layout, rays, samples and the cell under a sample
 * are MsNavSeen's, word for word (kernels/navseen.h: seen_ray, seen_sample).  Every number below is an integer, or an integer
 * binary32 holds exactly; tests/test_navage_host.py restates the rule in numpy (age_rule) and the kernel - and its host
 * instantiation, ms_host_nav_ages - are held to EQUALITY with it.
 *   last          S stores per env in MsNavSeen.maps' layout, one binary32 per cell: the tick at which the cell was last seen;
 *                 0.f: never since the map was cleared.  Ticks start at 1.
 *   clock         (N, S) int32 on the device: the tick of the map's last advancing call.
 *   a call        for map (n, s), in this order:  1. reset[n, s] non-zero: last of the map and clock[n, s] go to 0;
 *                 2. now = advance ? min(clock[n, s] + 1, 16777216) : clock[n, s] - 2^24, where binary32 stops holding ticks
 *                 exactly;  3. with advance, the cells under the samples of the rays of the map's viewers are the call's marked
 *                 SET: a cell under many samples, or under two viewers' rays, is in it once.  Without advance nothing is marked,
 *                 and origins, dirs, distances, slot, n_viewers and n_rays are not read;  4. for every marked cell
 *                 age = now - (int)last, then last = (float)now;  5. swept[n, s] = the marked cells that are countable;
 *                 6. gained[n, s] = those of them whose last was 0;  7. idle[n, s] = the sum of age over them, an int64;
 *                 8. clock[n, s] = now.  swept, gained and idle may each be NULL.
 *   the survey    runs after the marks of the same call - a cell just marked has age 0 - unless oldest, total_age, n_stale,
 *                 stale and ages are all NULL.  For every cell age = now - (int)last.  Over the countable cells:
 *                 oldest[n, s] = the largest age (0 when no cell counts; never below 0), total_age[n, s] = the sum of the ages,
 *                 an int64, n_stale[n, s] = the cells with age >= threshold (an int >= 1).  stale, a byte store in the maps'
 *                 layout: (countable & 1) && age >= threshold ? 1 : 0 for every cell - marks for MsNavSeedFields and
 *                 MsNavRegions, a layer for MsNavWindows and MsNavDraws as it is.  ages, a binary32 store in the same layout:
 *                 (float)age for every cell, countable or not.  Each may be NULL.
 *   an env without cells, and one with more cells than max_cells says, leaves its stores alone: its clock moves as above and
 *                 its counts, sums and oldest are 0.
 * One launch, one workgroup per map - the map's only writer - with the call's marks as a bitmask in LDS, as MsNavSeen's:
 * max_cells sizes it, more than 2^20 is MS_EUNSUPPORTED.  No global atomics, nothing allocated, nothing waits, and the clock
 * lives on the device: the call can be captured in a HIP graph, and every replay is a later tick.  Every argument is checked in
 * full before the launch (MS_EINVAL). */
typedef struct MsNavAges {
    int                  n_maps;       /* S: maps per env                                                              */
    int                  n_viewers;    /* P: viewers per env (advance; else ignored)                                   */
    int                  n_rays;       /* R: rays per viewer (advance; else ignored)                                   */
    const float*         origins;      /* (N, P, 2); 8-byte aligned                                                    */
    const float*         dirs;         /* (N, P, R, 2); 8-byte aligned                                                 */
    const float*         distances;    /* (N, P, R)                                                                    */
    const int*           slot;         /* (N, P) the map each viewer marks; NULL: P == S, viewer k map k               */
    float                max_range;    /* metres, finite and > 0                                                       */
    const unsigned char* reset;        /* (N, S) non-zero: clear the map and its clock first; NULL: none               */
    const unsigned char* countable;    /* (starts[N],) bit 0: the cell counts; NULL: the grid's free_cells             */
    int                  advance;      /* 1: the clock ticks and the rays mark; 0: the survey alone                    */
    int                  threshold;    /* T >= 1: a cell is stale at age >= T                                          */
    float*               last;         /* S*starts[N] floats in / out: map (n, s) at S*starts[n] + s*nx*ny             */
    int*                 clock;        /* (N, S) in / out                                                              */
    int*                 swept;        /* (N, S) out, or NULL                                                          */
    int*                 gained;       /* (N, S) out, or NULL                                                          */
    long long*           idle;         /* (N, S) out, or NULL; 8-byte aligned                                          */
    int*                 oldest;       /* (N, S) out, or NULL                                                          */
    long long*           total_age;    /* (N, S) out, or NULL; 8-byte aligned                                          */
    int*                 n_stale;      /* (N, S) out, or NULL                                                          */
    unsigned char*       stale;        /* S*starts[N] bytes out, in last's layout, or NULL                             */
    float*               ages;         /* S*starts[N] floats out, in last's layout, or NULL                            */
    int                  max_cells;    /* the largest nx*ny of any env (0: no env has cells), at most 2^20             */
} MsNavAges;
int ms_nav_ages(const MsNavGrid* grid, const MsNavAges* ages, void* hip_stream);

/* Map windows: per-cell stores of the nav grid - free cells, seen maps, distance fields, any marks - cropped, turned and
 * resampled into images through affine views: the egocentric map of an agent, its heading up, of what IT has seen.  As above
 * every step is one binary32 operation in the order given, without contraction, divisions correctly rounded;
 * tests/test_navwindow_host.py restates it in numpy (window_rule) and the kernel - and its host instantiation,
 * ms_host_nav_windows - are held to EQUALITY with it.  c, geom and starts are MsNavGrid's.
 *   layers        a layer holds n_fields stores per env, store (n, f) of nx*ny cells from n_fields*starts[n] + f*nx*ny on,
 *                 row-major with row 0 at the lowest y (MsNavFields.fields' and MsNavSeen.maps' layout), as bytes (is_float 0)
 *                 or binary32 floats (is_float 1).  `field` (N, P) names the store view (n, p) reads; NULL: store 0 when
 *                 n_fields == 1, else n_fields == P and view p reads store p (anything else is refused).  Field indices are
 *                 read on the device only; one outside [0, n_fields) is a BAD index, see the pixel.
 *   views         (N, P, 6): MsOverhead's six floats g0..g5 of view p of env n.
 *   sample points pixel (row i from the top, column j), k = samples, sub-sample (a, b), a and b in 0 .. k-1:
 *                 u = (float)j + ((float)b + .5f)/(float)k, w = (float)i + ((float)a + .5f)/(float)k,
 *                 x = (g0 u + g1 w) + g2, y = (g3 u + g4 w) + g5.  With k = 1 this is MsOverhead's pixel centre.
 *   the cell      under a sample, as MsNavSeen finds it: fx = floorf(x/c), fy = floorf(y/c); no cell when fx or fy is a NaN
 *                 or |.| >= 2^30; else j = (int)fx - jx0, i = (int)fy - iy0, no cell when (i, j) is outside the grid.  An env
 *                 without cells (nx <= 0 or ny <= 0) has no cell anywhere.
 *   the value     of a sample in one channel: `outside` without a cell; else, if the channel has a gate (a byte layer with a
 *                 `field` of its own) and the gate's byte at the cell is 0: `hidden`; else for a byte source 1.f when
 *                 (byte != 0) == where and 0.f otherwise, for a float source holding D at the cell v = D*scale, then
 *                 v < 1 ? (v > 0 ? v : 0) : 1 - a NaN and +inf give 1.
 *   the pixel     acc = 0.f, then acc += value over a (outer) and b (inner), then acc/(float)(k*k).  A channel whose source
 *                 index is BAD for a view has `outside` in every pixel of that image; else one whose gate index is BAD has
 *                 `hidden` in every pixel - neither through the sum.
 *   out           (N, P, C, H, W) binary32, planar.
 * One launch for every image and channel; the channels travel in the kernel's arguments by value, so `channels` is a HOST
 * array of n_channels (1..8) entries.  samples in 1..4, height and width in 1..1024, a gate must be bytes (a gate with values
 * NULL is no gate).  Every output element has one writer and a fixed serial sum: nothing depends on the order of execution.
 * Nothing is allocated, nothing is copied to the device, nothing waits: the call can be captured in a HIP graph.  Every
 * argument is checked in full before the launch (MS_EINVAL). */
typedef struct MsNavLayer {
    const void*          values;       /* n_fields*starts[N] bytes (is_float 0) or floats (is_float 1)                  */
    int                  is_float;     /* 0 or 1                                                                       */
    int                  n_fields;     /* G >= 1: stores per env                                                       */
    const int*           field;        /* (N, P) the store each view reads; NULL: n_fields == 1 or n_fields == P       */
} MsNavLayer;
typedef struct MsNavChannel {
    MsNavLayer           source;
    MsNavLayer           gate;         /* values NULL: none (the other members are then not looked at); else bytes     */
    int                  where;        /* 0 or 1: the byte that gives 1.f (byte sources)                               */
    float                scale;        /* float sources: v = D*scale                                                   */
    float                outside;      /* a sample without a cell                                                      */
    float                hidden;       /* a sample whose gate byte is 0                                                */
} MsNavChannel;
typedef struct MsNavWindows {
    int                  n_views;      /* P >= 1: views per env                                                        */
    int                  height, width;/* H, W: 1..1024                                                                */
    int                  samples;      /* k: 1..4, k*k sub-samples a pixel                                             */
    const float*         views;        /* (N, P, 6)                                                                    */
    int                  n_channels;   /* C: 1..8                                                                      */
    const MsNavChannel*  channels;     /* (C,) HOST memory                                                             */
    float*               out;          /* (N, P, C, H, W)                                                              */
} MsNavWindows;
int ms_nav_windows(const MsNavGrid* grid, const MsNavWindows* windows, void* hip_stream);

/* Cell draws: K cells drawn uniformly at random, with replacement, among the free cells of an env that satisfy a predicate on a
 * layer - goals in a band of walking distance, spawns anywhere an agent fits, a random unseen cell - from a counter the kernel
 * advances itself, so a captured step draws fresh numbers at every replay.  Every step is integer arithmetic;
 * tests/test_navdraw_host.py restates it in numpy (draw_rule) and the kernel - and its host instantiation, ms_host_nav_draws -
 * are held to EQUALITY with it.  c, geom and starts are MsNavGrid's.
 *   draw sets     P per env; set (n, p) makes K draws.  `source` and `gate` are layers as MsNavWindows reads them: set (n, p)
 *                 reads the store field[n, p] names; NULL: store 0 when n_fields == 1, else n_fields == P and set p reads
 *                 store p (anything else is refused).  A field index outside [0, n_fields), of the source or of the gate,
 *                 leaves the set without a qualifying cell.
 *   qualifying    cell k of env n (row-major, row 0 at the lowest y) qualifies for set (n, p) when  1. free_cells is non-zero
 *                 there;  2. the source's predicate holds: for a byte source (byte != 0) == where, for a binary32 source
 *                 holding D lo <= D && D <= hi - a NaN, and +-inf outside the band, fail;  3. the gate (a byte layer; values
 *                 NULL: none), if there is one, is non-zero there.  q_0 < q_1 < ... < q_{M-1} are the set's qualifying cells.
 *                 An env without cells (or with more than max_cells says) has M = 0.
 *   the hash      mix(a): a ^= a >> 16; a *= 0x85ebca6b; a ^= a >> 13; a *= 0xc2b2ae35; a ^= a >> 16 (murmur3's finaliser, on
 *                 32 bits).  h = fold(seed_lo, seed_hi, n*P + p, counter[n, p], k, stream): s = 0x9e3779b9, then
 *                 s = mix(s + word) modulo 2^32 for each of the six words in that order; seed_lo / seed_hi are the low and
 *                 high 32 bits of `seed`.  fold(0, 0, 0, 0, 0, 0) = 0xe88cf1a4; fold(12345, 0, 2, 9, 4, 0) = 0xf8f4d17a.
 *   a draw        draw k picks q_r with r = ((uint64)h * M) >> 32, h of stream 0: the bias is at most M / 2^32.
 *                 uniforms[n, p, k] = (float)(h >> 8) * 2^-24 with h of stream 1, in [0, 1): a spare number per draw (a
 *                 spawn's heading).
 *   outputs       cells (N, P, K): the cell's index within its env, -1 when M = 0; points (N, P, K, 2): its centre as the nav
 *                 grid forms it, x = ((float)(jx0 + j) + 0.5f)*c, y likewise, NaN when M = 0; uniforms (N, P, K); values
 *                 (N, P, K), binary32 sources only, or NULL: D at the cell, NaN when M = 0; counts (N, P): M.
 *   the counter   (N, P) in / out: the rule reads it; the kernel then adds 1 (modulo 2^32) for every set it computed.
 *   mask          (N, P) bytes or NULL: a set whose byte is 0 is not touched at all - its outputs, its counts and its counter
 *                 keep what they held.
 * One launch, one workgroup per set, the qualifying cells as a bitmap in LDS, one bit per cell: max_cells, the most cells
 * (nx*ny) any env has, sizes it.  More than 2^20: MS_EUNSUPPORTED, nothing enqueued.  K in 1..256, a gate must be bytes, lo
 * and hi must not be NaN (they are not looked at for a byte source), values must be NULL for a byte source.  No atomics,
 * nothing allocated, nothing waits: the call can be captured in a HIP graph.  Every argument is checked in full before the
 * launch (MS_EINVAL). */
typedef struct MsNavDraws {
    MsNavLayer           source;
    MsNavLayer           gate;         /* values NULL: none (the other members are then not looked at); else bytes     */
    int                  where;        /* 0 or 1: the byte that qualifies (byte sources)                               */
    float                lo, hi;       /* the band, both ends in (binary32 sources)                                    */
    int                  n_sets;       /* P >= 1: draw sets per env                                                    */
    int                  n_draws;      /* K: 1..256 draws per set                                                      */
    unsigned long long   seed;
    int*                 counter;      /* (N, P) in / out                                                              */
    const unsigned char* mask;         /* (N, P) non-zero: compute this set; NULL: all                                 */
    int*                 cells;        /* (N, P, K) out                                                                */
    float*               points;       /* (N, P, K, 2) out                                                             */
    float*               uniforms;     /* (N, P, K) out                                                                */
    float*               values;       /* (N, P, K) out, or NULL                                                       */
    int*                 counts;       /* (N, P) out                                                                   */
    int                  max_cells;    /* the largest nx*ny of any env (0: no env has cells), at most 2^20             */
} MsNavDraws;
int ms_nav_draws(const MsNavGrid* grid, const MsNavDraws* draws, void* hip_stream);

/* Regions: which cells of the nav grid belong together - the connected components of any per-cell mask, each cell labelled with
 * its component and the component's area: the rooms an agent can walk between, the clusters the unseen floor falls into.  Every
 * step is integer arithmetic but the area; tests/test_navregion_host.py restates it in numpy (region_rule, a flood fill) and the
 * kernels - and their host instantiations, ms_host_nav_regions / _region_query / _region_masks - are held to EQUALITY with it.
 * c, geom and starts are MsNavGrid's.
 *   regions field (n, g) is field g of env n, G per env; its stores use the fields' layout: field (n, g) starts at
 *                 G*starts[n] + g*nx*ny, row-major, row 0 at the lowest y.
 *   open cells    without marks (NULL): cell k is open when free_cells[k] & 1.  With marks (a byte per cell and field, the
 *                 fields' layout), where in {0, 1} and among (a byte per cell of the grid, or NULL): when MsNavSeedFields' seed
 *                 predicate holds - free[k] & 1, and among == NULL or among[k] & 1, and (marks[k] & 1) == where; the kernels
 *                 call the very function the seeded fields call, so a frontier field's seeds ARE a frontier regions field's
 *                 open cells.  among is not looked at without marks.
 *   edges         two open cells are joined when they are 4-neighbours inside the env's nx x ny; rows do not wrap.  On the free
 *                 cells this is exactly the connectivity of MsNavGrid's graph: a diagonal edge u - v exists only when both
 *                 cells that share a side with u and v are free, and then u - side - v is a path of straight edges; so the
 *                 regions of the grid are exactly the sets on which a distance field is finite.
 *   labels        int32 per cell: the least row-major index, within the env, of an open cell of the cell's component; -1 on a
 *                 closed cell.  Canonical: any algorithm and any schedule gives the same.
 *   areas         binary32 per cell: (float)cells_in_component*(c*c), those two binary32 multiplications in that order; 0.f
 *                 on a closed cell.  A float layer in square metres: MsNavDraws' band and MsNavChannel's scale read it as it is.
 *   summary       (N, G) int32 each: counts - the regions; open_cells - the open cells; largest - the label of the region with
 *                 the most cells, the least such label on a tie, -1 without an open cell; largest_cells - its cells (0 then);
 *                 passes (or NULL) - the passes the propagation took (telemetry: depends on the schedule).  An env without
 *                 cells: 0, 0, -1, 0, 0.
 *   query         a point's anchors are MsNavGrid's four cells (i0 + (t>>1), j0 + (t&1)), t = 0..3; labels_at (N, P, 4) holds
 *                 the label under each, -1 where the anchor is outside the grid or closed; all -1 for a NaN point, one further
 *                 out than 2^30 cells, an env without cells, a field index outside [0, G).  field (N, P) names the regions
 *                 field each point asks; NULL: MsNavLayer's rule - field 0 when G == 1, else G == P and point p asks field p.
 *   masks         P requests per env; out holds P byte stores per env in the fields' layout (request (n, p) at
 *                 P*starts[n] + p*nx*ny).  A byte is 1 where labels[k] >= 0 and labels[k] is in the request's wanted set: the
 *                 non-negative anchor labels of points[n, p] (up to four: a point between two diagonally touching cells wants
 *                 two regions), or the one label wanted[n, p] (-1, or any label no cell holds: an empty mask).  Exactly one of
 *                 points and wanted is given.  field: as the query's.  Every byte of every store is written.  With P = 1 the
 *                 store has free_cells' layout: an among, a countable mask or a gate as it is.
 * ms_nav_regions: one launch, one workgroup per field, the labels in LDS while the field fits ((nx + 2)*(ny + 2) int32 in 40,
 * 80 or 160 KiB, chosen by max_framed); a larger field is labelled in its `labels` store, to the same bits.  Fields that are
 * masked out keep labels, areas and summary as they are.  marks and among are read when the call runs.  Integer atomics only,
 * one writer per output element, nothing allocated, nothing waits: all three calls can be captured in a HIP graph.  Every
 * argument is checked in full before the launch (MS_EINVAL). */
typedef struct MsNavRegions {
    int                  n_fields;     /* G: regions fields per env                                                    */
    const unsigned char* marks;        /* G*starts[N] bytes, bit 0: the fields' layout; NULL: the open cells are the free cells */
    int                  where;        /* 0 or 1: an open cell's mark (with marks)                                     */
    const unsigned char* among;        /* (starts[N],) bit 0: the cell may be open; NULL: every free cell may (with marks) */
    const unsigned char* mask;         /* (N, G) non-zero: compute this field; NULL: all.  Read on the device only.    */
    int*                 labels;       /* G*starts[N] int32 out                                                        */
    float*               areas;        /* G*starts[N] floats out                                                       */
    int*                 counts;       /* (N, G) out                                                                   */
    int*                 open_cells;   /* (N, G) out                                                                   */
    int*                 largest;      /* (N, G) out                                                                   */
    int*                 largest_cells;/* (N, G) out                                                                   */
    int*                 passes;       /* (N, G) out, or NULL                                                          */
} MsNavRegions;
typedef struct MsNavRegionQuery {
    int                  n_points;     /* P: points per env                                                            */
    const float*         points;       /* (N, P, 2) x, y                                                               */
    const int*           field;        /* (N, P) the regions field each point asks; NULL: G == 1 or G == P             */
    const int*           labels;       /* as MsNavRegions.labels                                                       */
    int                  n_fields;     /* G of `labels`                                                                */
    int*                 labels_at;    /* (N, P, 4) out                                                                */
} MsNavRegionQuery;
typedef struct MsNavRegionMasks {
    int                  n_requests;   /* P: requests per env                                                          */
    const float*         points;       /* (N, P, 2), or NULL: `wanted` is given                                        */
    const int*           wanted;       /* (N, P) one label each, or NULL: `points` is given                            */
    const int*           field;        /* (N, P) the regions field each request reads; NULL: G == 1 or G == P          */
    const int*           labels;       /* as MsNavRegions.labels                                                       */
    int                  n_fields;     /* G of `labels`                                                                */
    unsigned char*       out;          /* P*starts[N] bytes out                                                        */
} MsNavRegionMasks;
int ms_nav_regions(const MsNavGrid* grid, const MsNavRegions* regions, void* hip_stream);
int ms_nav_region_query(const MsNavGrid* grid, const MsNavRegionQuery* query, void* hip_stream);
int ms_nav_region_masks(const MsNavGrid* grid, const MsNavRegionMasks* masks, void* hip_stream);

/* View fields: what can be seen from a place - the cells of the nav grid whose centre is in sight of a viewpoint, how many of them
 * count, and how many of those a seen map has not seen yet: the score of a candidate standpoint, the cells an opponent at p sees.
 * Every step below is one binary32 operation, in the order given, without contraction; tests/test_navview_host.py restates it in
 * numpy (view_rule) and the kernel - and its host instantiation, ms_host_nav_views - is held to EQUALITY with it.  c, geom and
 * starts are MsNavGrid's.  P viewpoints per env; for viewpoint (px, py) = points[n, p] and cell (i, j) of env n:
 *   centre        x = ((float)(jx0 + j) + 0.5f)*c, y = ((float)(iy0 + i) + 0.5f)*c - MsNavGrid's.
 *   range         rx = x - px, ry = y - py, rr = rx*rx + ry*ry; in range iff rr <= R2, R2 = max_range*max_range formed once.
 *   cone          with headings (hx, hy) = headings[n, p]: hlen = sqrtf(hx*hx + hy*hy); a viewpoint whose hlen is not finite or not
 *                 > 0 sees nothing; len = sqrtf(rr), dotp = hx*rx + hy*ry, lim = (cos_half*len)*hlen; in the cone iff dotp >= lim
 *                 (a cell whose centre is the viewpoint is in every cone).
 *   a wall        is a row (ax, ay, bx, by) of the env's STATIC lines (rows n_agents*n_model .. L - 1 of the env in
 *                 MsScenery.lines_vals: the rows ms_nav_free reads).  It blocks the cell iff all three hold:
 *                 meets   min(ax, bx) <= max(px, x) && max(ax, bx) >= min(px, x), and the same in y (comparisons only: any cull
 *                         of far walls consistent with it is bit-safe);
 *                 apart   vx = bx - ax, vy = by - ay, o1 = vx*(py - ay) - vy*(px - ax), o2 = vx*(y - ay) - vy*(x - ax):
 *                         (o1 < 0 && o2 > 0) || (o1 > 0 && o2 < 0) - viewpoint and centre strictly on opposite sides of the wall's line;
 *                 across  o3 = rx*(ay - py) - ry*(ax - px), o4 = rx*(by - py) - ry*(bx - px):
 *                         (o3 <= 0 && o4 >= 0) || (o3 >= 0 && o4 <= 0) - the wall's ends on opposite sides of the sight line, zero
 *                         included, so that a sight line through the vertex two walls share is blocked.
 *                 A wall with a NaN fails a comparison of `apart` and blocks nothing.
 *   visible       iff px and py are finite, the cell is in range, in the cone if one is given, and no static wall blocks it.  The
 *                 agents' own lines are not looked at: the grid is the building.
 *   values        store (n, p) holds 1 on visible cells and 0 on all others, for EVERY cell of the env, free or not (a blocked cell on
 *                 the viewer's side of a wall is a known obstacle), in the seen maps' layout: store (n, p) at P*starts[n] + p*nx*ny,
 *                 row-major, row 0 at the lowest y.  Every byte of a computed store is written: it needs no clearing.  A byte a
 *                 cell: ms_nav_seed_fields' marks, ms_nav_regions' marks, an MsNavLayer as it is.
 *   counts        counts[n, p] = the visible cells whose countable byte has bit 0 set (countable: free_cells' layout; required).
 *   gains         with unseen (the byte store of seen maps, S = n_maps per env: map (n, s) at S*starts[n] + s*nx*ny) and slot (N, P)
 *                 (NULL: map p when P == S, map 0 when S == 1): gains[n, p] = the visible countable cells whose byte in map
 *                 slot[n, p] has bit 0 clear; 0 for a slot outside 0 .. S - 1.
 *   mask          (N, P) bytes: a viewpoint marked 0 keeps its bytes, its count and its gain untouched.
 *   no cells      an env without cells: counts and gains 0, nothing stored.
 * Refused before any launch (MS_EINVAL): P < 1; a NULL points or countable; no output at all (values, counts and gains all NULL);
 * max_range not positive and finite; cos_half outside [-1, 1] (or a NaN) when headings is given; gains without unseen; unseen with
 * S < 1, or without slot when S is neither 1 nor P; points or headings not 8-byte aligned; a scenery of another number of envs.
 * One launch, one workgroup per viewpoint: the walls whose box meets the box of everything in range are staged in LDS (more than
 * 512 of them: read from the scenery instead, same result), a lane a cell of the window round the viewpoint.  With values == NULL no
 * byte is written: scoring needs no store.  Integer counts with one writer each, no atomics, nothing allocated, nothing waits: the
 * call can be captured in a HIP graph. */
typedef struct MsNavViews {
    int                  n_points;     /* P: viewpoints per env                                                         */
    const float*         points;       /* (N, P, 2) x, y; 8-byte aligned                                                */
    const float*         headings;     /* (N, P, 2) any length, or NULL: no cone; 8-byte aligned                        */
    float                max_range;    /* R, metres (> 0, finite)                                                       */
    float                cos_half;     /* the cosine of half the cone's angle, in [-1, 1] (with headings)               */
    const unsigned char* countable;    /* (starts[N],) bit 0: the cell counts                                           */
    const unsigned char* unseen;       /* S*starts[N] bytes, bit 0: seen; NULL: no gains                                */
    int                  n_maps;       /* S of `unseen`                                                                 */
    const int*           slot;         /* (N, P) the map each viewpoint is scored against; NULL: S == 1 or S == P       */
    const unsigned char* mask;         /* (N, P) non-zero: compute this viewpoint; NULL: all.  Read on the device only. */
    unsigned char*       values;       /* P*starts[N] bytes out, or NULL                                                */
    int*                 counts;       /* (N, P) out, or NULL                                                           */
    int*                 gains;        /* (N, P) out, or NULL                                                           */
} MsNavViews;
int ms_nav_views(const MsScenery* scenery, const MsNavGrid* grid, const MsNavViews* views, void* hip_stream);

/* Percepts: which of a set of points - the other agents, pickups, a goal object - each eye of an env can see, how far away and
 * which way each is, and which are nearest: the entity observation behind a visibility mask of tag, hide-and-seek, foraging and
 * search tasks, and their "seen by" predicate.  The rule is the view fields' (MsNavViews above), applied to eye/point pairs instead
 * of a viewpoint and cell centres - the kernel calls the very functions nav_view_kernel calls - so a point is visible exactly when
 * a cell whose centre it is would be.  Every step is one binary32 operation, in the order given, without contraction;
 * tests/percept_rule.py restates it in numpy and the kernel - and its host instantiation, ms_host_percepts - is held to EQUALITY
 * with it.  Per env E eyes, P points and the env's STATIC walls as they stand in MsScenery.lines_vals (rows n_agents*n_model ..
 * L - 1): the agents' rows are not read, BODIES DO NOT OCCLUDE.  For eye (px, py) = eyes[n, e] and point (x, y) = points[n, p]:
 *   candidate     iff valid[n, p] != 0 (NULL: every point exists), pairs allows it (pairs[e, p] != 0 with pairs_shape 1,
 *                 pairs[n, e, p] != 0 with pairs_shape 2; NULL: every pair), px and py are finite, with headings (hx, hy) =
 *                 headings[n, e] hlen = sqrtf(hx*hx + hy*hy) is finite and > 0, and rx = x - px, ry = y - py, rr = rx*rx + ry*ry,
 *                 rr <= R2 (R2 = max_range*max_range formed once), and with headings hx*rx + hy*ry >= (cos_half*sqrtf(rr))*hlen.
 *                 A NaN point is never a candidate (rr <= R2 fails); a point on the eye (rr == 0) is one, in every cone.
 *   visible       iff a candidate and no static wall blocks it - MsNavViews' meets, apart and across.  Nothing blocks a point on
 *                 the eye; a wall with a NaN blocks nothing.
 *   visible       (N, E, P) bytes: 1 visible, 0 not.
 *   squares       (N, E, P): rr where visible, +inf elsewhere.
 *   offsets       (N, E, P, 2): (rx, ry), in the world frame, where visible, NaN elsewhere.
 *   counts        (N, E): the visible points.
 *   nearest       (N, E, K): the visible points in ascending order of the pair (bits of rr, p) - rr is not negative, so its
 *                 binary32 bits order as its value, and equal distances go to the lower index; entries beyond counts hold -1.
 *   near_offsets, near_distances   (N, E, K, 2) and (N, E, K): (rx, ry) and sqrtf(rr) of those K; NaN and +inf beyond counts.
 *   mask          (N, E) bytes: an eye marked 0 is not computed, and every output row of it keeps what it held.
 * No trigonometry and no division: a frame of the eye's own (forward, left) is the caller's arithmetic.  Each output may be NULL
 * (not wanted), each element has exactly one writer.  Limits: 1 <= E <= 64, 1 <= P <= 1024, 0 <= K <= 16.
 * Refused before any launch (MS_EINVAL): a NULL eyes or points; E, P or K outside those limits; every output NULL; max_range not
 * positive and finite; cos_half outside [-1, 1] (or a NaN) when headings is given; pairs without pairs_shape 1 or 2, or a
 * pairs_shape other than 0 without pairs; eyes, headings, points, offsets or near_offsets not 8-byte aligned; squares, counts,
 * nearest or near_distances not 4-byte aligned.
 * One launch, one workgroup per env: the walls whose box meets the box of everything in range of some unmasked eye are staged in
 * LDS (more than 512 of them: read from the scenery instead, same result), a wave an eye, a lane the points lane + 64 j, the
 * nearest K by K rounds of a wave-wide minimum.  No atomics, nothing allocated, nothing waits: the call can be captured in a
 * HIP graph. */
typedef struct MsPercepts {
    int                  n_eyes;         /* E: eyes per env (1 .. 64)                                                     */
    int                  n_points;       /* P: points per env (1 .. 1024)                                                 */
    int                  n_nearest;      /* K: nearest visible points listed per eye (0 .. 16)                            */
    const float*         eyes;           /* (N, E, 2) x, y; 8-byte aligned                                                */
    const float*         headings;       /* (N, E, 2) any length, or NULL: no cone; 8-byte aligned                        */
    const float*         points;         /* (N, P, 2) x, y; 8-byte aligned                                                */
    const unsigned char* valid;          /* (N, P) non-zero: the point exists; NULL: all                                  */
    const unsigned char* pairs;          /* non-zero: the eye takes an interest in the point; NULL: every pair            */
    int                  pairs_shape;    /* 0: no pairs; 1: pairs is (E, P), shared by all envs; 2: pairs is (N, E, P)    */
    const unsigned char* mask;           /* (N, E) non-zero: compute this eye; NULL: all.  Read on the device only.       */
    float                max_range;      /* R, metres (> 0, finite)                                                       */
    float                cos_half;       /* the cosine of half the cone's angle, in [-1, 1] (with headings)               */
    unsigned char*       visible;        /* (N, E, P) out, or NULL                                                        */
    float*               squares;        /* (N, E, P) out, or NULL                                                        */
    float*               offsets;        /* (N, E, P, 2) out, or NULL; 8-byte aligned                                     */
    int*                 counts;         /* (N, E) out, or NULL                                                           */
    int*                 nearest;        /* (N, E, K) out, or NULL                                                        */
    float*               near_offsets;   /* (N, E, K, 2) out, or NULL; 8-byte aligned                                     */
    float*               near_distances; /* (N, E, K) out, or NULL                                                        */
} MsPercepts;
int ms_percepts(const MsScenery* scenery, const MsPercepts* percepts, void* hip_stream);

/* Basins: WHICH seed a cell of a seeded field leads to - whose agent is nearest (a geodesic Voronoi diagram of the floor), which
 * frontier cluster, which pickup a cell drains to - and how many cells each seed, or each id, holds.  Every output is an integer
 * with one definition; tests/test_navbasin_host.py restates it in numpy (basin_rule, point_mark_rule, basin_query_rule: chains
 * followed cell by cell) and the kernels - and their host instantiations, ms_host_nav_basins / _basin_query / _point_marks - are
 * held to EQUALITY with it.  c, geom and starts are MsNavGrid's.  Take field (n, g) of an MsNavSeedFields store, its values D AS THEY
 * STAND when the call runs, and a cell v of env n's grid:
 *   succ(v)       what MsNavSeedFields' `following` hop does from v - the kernels call the very function ms_nav_seed_paths and
 *                 ms_nav_seed_waypoints follow: if D[v] == 0.f the chain ends at v, a seed; otherwise the next cell is the first of
 *                 the eight neighbours (MsNavWaypoints' order and rules) that attains the least fl(D[u] + w), provided D[u] < D[v];
 *                 without such a neighbour the chain is BROKEN at v (a stale or foreign field).
 *   end(v)        the seed the chain v, succ(v), succ(succ(v)), ... ends on.  A hop needs a strictly lower value: whatever floats
 *                 the store holds, the successor graph has no cycle and every chain ends or breaks within the env's cells.
 *   label(v)      -1 when v is blocked (free_cells[v] & 1 clear), when D[v] is not < +inf (a NaN too), or when v's chain breaks;
 *                 otherwise end(v)'s row-major index within the env's grid - or, with ids, ids[first + end(v)] as stored: ids is an
 *                 int32 per cell and field in the fields' layout (field (n, g) at first = G*starts[n] + g*nx*ny); a negative id
 *                 reads as "no basin" wherever a label is tested.  ids must not be the labels store.
 *   sizes         with n_ids = K in 1..256: sizes[n, g, k] = the cells whose label is k, 0 <= k < K; labels outside that range are
 *                 counted nowhere.  K = 0: no sizes (the pointer must be NULL then, and non-NULL otherwise).
 *   reached       reached[n, g] = the cells with label >= 0.  passes (or NULL): the passes the jumps took (telemetry: depends on
 *                 the schedule; at most ceil(log2(longest chain)) + 1).  An env without cells: sizes 0, reached 0, passes 0.
 *   query         from a point p: MsNavWaypoints' start picks the anchor a* the query's minimum is attained at, and the answer is
 *                 the label stored at a*; -1 exactly where ms_nav_query gives +inf (a NaN point, an env without cells and a field
 *                 index outside [0, G) included).  field (N, P): the field each point asks; NULL: MsNavLayer's rule - field 0
 *                 when G == 1, else G == P and point k asks field k.
 *   point marks   the seeds of "nearest agent": for point (n, k) every FREE cell among its four anchors (MsNavGrid's, in the
 *                 query's order) gets mark byte 1 and id min(what it holds, id_k), id_k = point_ids[n, k], or k without
 *                 point_ids.  The store is picked by `field` as the query's.  Two points that share an anchor leave the lower id;
 *                 a point without an anchor (a NaN, one further out than 2^30 cells, a field index out of range, an env without
 *                 cells) marks nothing.  Nothing is cleared: the caller zeroes marks and fills ids (with INT_MAX) beforehand.
 *   masks         ms_nav_region_masks turns the labels store into byte layers as it is (labels = MsNavBasins.labels, wanted = ids).
 * ms_nav_basins: one launch, one workgroup per field: succ once per cell into an int32 per cell in LDS while the env fits (40, 80
 * or 160 KiB, chosen by max_framed, which bounds the cells from above), then pointer jumps N[k] = N[N[k]] in place until a pass
 * changes nothing; a larger env runs the same jumps in its `labels` store, to the same result.  Fields that are masked out keep
 * labels, sizes, reached and passes as they are.  Integer atomics only, one writer per output element, nothing allocated, nothing
 * waits: all three calls can be captured in a HIP graph.  Every argument is checked in full before the launch (MS_EINVAL). */
typedef struct MsNavBasins {
    int                  n_fields;     /* G: fields per env                                                            */
    const float*         fields;       /* as MsNavSeedFields.fields                                                    */
    const int*           ids;          /* G*starts[N] int32, the fields' layout; NULL: a label is the seed's cell index */
    int                  n_ids;        /* K, 0..256: the ids counted in sizes                                          */
    const unsigned char* mask;         /* (N, G) non-zero: compute this field; NULL: all.  Read on the device only.    */
    int*                 labels;       /* G*starts[N] int32 out                                                        */
    int*                 sizes;        /* (N, G, K) out; NULL exactly when K == 0                                      */
    int*                 reached;      /* (N, G) out                                                                   */
    int*                 passes;       /* (N, G) out, or NULL                                                          */
} MsNavBasins;
typedef struct MsNavBasinQuery {
    int                  n_points;     /* P: points per env                                                            */
    const float*         points;       /* (N, P, 2) x, y                                                               */
    const int*           field;        /* (N, P) the field each point asks; NULL: G == 1 or G == P                     */
    const float*         fields;       /* as MsNavSeedFields.fields                                                    */
    const int*           labels;       /* as MsNavBasins.labels                                                        */
    int                  n_fields;     /* G of `fields` and `labels`                                                   */
    int*                 out;          /* (N, P) out                                                                   */
} MsNavBasinQuery;
typedef struct MsNavPointMarks {
    int                  n_points;     /* P: points per env                                                            */
    const float*         points;       /* (N, P, 2) x, y                                                               */
    const int*           field;        /* (N, P) the store each point marks; NULL: G == 1 or G == P                    */
    const int*           point_ids;    /* (N, P) the id of each point; NULL: point k has id k                          */
    int                  n_fields;     /* G of `marks` and `ids`                                                       */
    unsigned char*       marks;        /* G*starts[N] bytes in / out                                                   */
    int*                 ids;          /* G*starts[N] int32 in / out                                                   */
} MsNavPointMarks;
int ms_nav_basins(const MsNavGrid* grid, const MsNavBasins* basins, void* hip_stream);
int ms_nav_basin_query(const MsNavGrid* grid, const MsNavBasinQuery* query, void* hip_stream);
int ms_nav_point_marks(const MsNavGrid* grid, const MsNavPointMarks* marks, void* hip_stream);

/* Zones: a label and a number together - per zone of a labels layer the cells, the marked cells, the least value and the cell that
 * attains it: how far each agent is from the nearest cell of each frontier cluster and which cell that is, how much of each room has
 * been seen, the oldest cell of each territory.  Every output is an integer or a copied float with one definition;
 * tests/test_navzone_host.py restates it in numpy (zone_rule: loops over cells, a min over (value bits, cell)) and the kernel - and
 * its host instantiation, ms_host_nav_zones - are held to EQUALITY with it.  geom, starts and c are MsNavGrid's.
 *   stores        A call covers F = n_fields fields per env and reads three layers in the fields' layout - a layer of S stores per
 *                 env keeps store (n, f) at S*starts[n] + f*nx*ny, row-major: labels (int32, L = n_labels stores), values (float32,
 *                 V = n_values stores, or NULL) and marks (uint8, M = n_marks stores, or NULL, with `where`).  Each of L, V, M is 1
 *                 or F; a layer with one store serves every field.  K = max_zones, 1..256.
 *   zone(v)       ranked = 1: the labels are canonical cell indices (MsNavRegions.labels, MsNavBasins.labels without ids).  A cell v
 *                 is a ROOT when labels[v] == v; zone k is the k-th root in ascending index order, and zone(v) is the rank of
 *                 labels[v] among the roots - none when labels[v] < 0, when it is not a cell of the env, when it is not a root, and
 *                 when its rank is K or more.  ranked = 0: the label is the zone (MsNavBasins.labels with ids, any int layer):
 *                 zone(v) = labels[v] when 0 <= labels[v] < K, else none.
 *   cells         cells[n, f, k] = the cells v with zone(v) == k.
 *   marked        those of them with (marks[v] != 0) == where; equals cells without marks.
 *   least         the least values[v] over the zone's cells that TAKE PART: the value's sign bit is clear and it is < +inf (NaN,
 *                 negatives and -0 are left out), and - with within_marks = 1 - the cell is marked.  +inf when none does, and
 *                 without values.  The float is copied, never computed.
 *   nearest       the least cell index (row-major within the env) attaining `least`; -1 when none.
 *   points        the centre of the `nearest` cell, x = ((float)(jx0 + j) + 0.5f)*c, y likewise - the very function the paths and
 *                 the cell draws give a cell's centre by; (NaN, NaN) when nearest is -1.
 *   roots         ranked = 1: the label zone k stands for - the k-th root - and -1 beyond the last zone; ranked = 0: k where
 *                 cells[n, f, k] > 0, else -1.
 *   n_zones       ranked = 1: the number of roots - it may exceed K: zones from K on are counted here and nowhere else;
 *                 ranked = 0: the number of k with cells[n, f, k] > 0.
 * Fields that are masked out keep every output as it is.  An env without cells writes zeros, +inf, -1 and NaN.
 * ms_nav_zones: one launch, one workgroup of 256 lanes per field; its LDS (5 KiB: the list of roots, two counters and one 64-bit
 * key a zone) does not grow with the env, so there are no tiers and no global-memory path.  Ranked: the first K roots are compacted
 * in index order by ballots and a workgroup prefix, every cell then finds its label in that list by binary search; per zone integer
 * atomics for the counts and ONE 64-bit LDS atomic min on (value bits << 32) | cell - a non-negative binary32 orders as its bits,
 * so this is the rule exactly.  One writer per output element, nothing allocated, nothing waits: the call can be captured in a HIP
 * graph.  Every argument is checked in full before the launch: NULL labels or outputs, a store count that is neither 1 nor F,
 * max_zones outside 1..256, where / ranked / within_marks other than 0 or 1, a misaligned pointer: MS_EINVAL, nothing enqueued. */
typedef struct MsNavZones {
    int                  n_fields;     /* F: fields per env                                                            */
    const int*           labels;       /* L*starts[N] int32                                                            */
    int                  n_labels;     /* L: 1 or F                                                                    */
    const float*         values;       /* V*starts[N] floats, or NULL: least is +inf, nearest -1                       */
    int                  n_values;     /* V: 1 or F (not read without values)                                          */
    const unsigned char* marks;        /* M*starts[N] bytes, or NULL: every cell counts as marked                      */
    int                  n_marks;      /* M: 1 or F (not read without marks)                                           */
    int                  where;        /* 0 or 1: a cell is marked when (marks[v] != 0) == where (not read without marks) */
    int                  within_marks; /* 0 or 1: only marked cells take part in least and nearest                      */
    int                  ranked;       /* 1: zone = the rank of the label among the roots; 0: zone = the label          */
    int                  max_zones;    /* K, 1..256                                                                    */
    const unsigned char* mask;         /* (N, F) non-zero: compute this field; NULL: all.  Read on the device only.    */
    int*                 cells;        /* (N, F, K) out                                                                */
    int*                 marked;       /* (N, F, K) out                                                                */
    float*               least;        /* (N, F, K) out                                                                */
    int*                 nearest;      /* (N, F, K) out                                                                */
    float*               points;       /* (N, F, K, 2) out                                                             */
    int*                 roots;        /* (N, F, K) out                                                                */
    int*                 n_zones;      /* (N, F) out                                                                   */
} MsNavZones;
int ms_nav_zones(const MsNavGrid* grid, const MsNavZones* zones, void* hip_stream);

/* Clearance: how much room there is - the distance from a place to the nearest wall, which wall that is, and which way it lies;
 * per cell of the nav grid (a float layer: a band for ms_nav_draws, a channel for ms_nav_windows; and the free bytes of several
 * body sizes from one pass over the walls) and per point, the other agents' bodies counted (a proximity reading).  What
 * ms_nav_free folds and throws away, kept.  Every step below is one binary32 operation, in the order given, without
 * contraction; tests/test_navclear_host.py restates it in numpy (clear_rule) and the kernels - and their host instantiations,
 * ms_host_nav_clearance / ms_host_nav_clear_query - are held to EQUALITY with it.  With R = max_range:
 *   a line        For a point (x, y) and row l = (ax, ay, bx, by) of its env: vx, vy, px, py, vv, t, dx, dy, d2 by MsOverhead's
 *                 statements, statement for statement.  The row is a CANDIDATE when d2 <= R*R (R*R formed once; a NaN never is).
 *   the winner    the candidate of least d2, of least l among those: MsOverhead's winner at half_width R.
 *   field         for cell (i, j) of env n's grid, at its centre (MsNavGrid's), over the env's STATIC rows (l from
 *                 n_agents*n_model on: the rows ms_nav_free reads):
 *                   values   sqrtf(d2) of the winner, the root correctly rounded; +inf without one.  (starts[N],) float32, free
 *                            cells' layout: an MsNavLayer of one store.
 *                   nearest  the winner's l (env-local, agent rows counted: ms_overhead's indices); -1 without one.
 *                   fits     K = n_radii stores an env in the fields' layout - store (n, k) at K*starts[n] + k*nx*ny - byte k
 *                            0 when there is a winner and its d2 <= r_k*r_k (r_k = radii[k], the square formed once), else 1:
 *                            with r_k <= R, exactly the free byte ms_nav_free writes at clearance r_k.
 *                 mask (N,) bytes: an env marked 0 keeps all its stores untouched.  An env without cells: nothing stored.
 *   query         for point (n, p) = (x, y), anywhere (no grid): the same statements and winner over the env's static rows and,
 *                 with agents, the agent rows 0 .. n_agents*n_model - 1 too, drawn at the agents' current poses as ms_overhead
 *                 draws them (nothing is written to the scenery) - except rows s*n_model .. (s + 1)*n_model - 1 of the agent
 *                 s = skip[n, p]; a value outside 0 .. n_agents - 1 (-1, say) skips none.  Without agents no agent row is met
 *                 and skip is not read.
 *                   distances  as values.    nearest  as above.
 *                   towards    (-dx/d, -dy/d) with d = sqrtf(d2) and the winner's dx, dy: the unit vector from the point to the
 *                              nearest point of the winner; (0, 0) when d == 0 or there is no winner.
 *                 A point with a NaN coordinate has no winner.  mask (N, P) bytes: a point marked 0 keeps its outputs untouched.
 * Refused before any launch (MS_EINVAL): a NULL struct or values; a scenery (or query) of another number of envs; max_range not
 * positive and finite; n_radii outside 0..8; fits NULL with n_radii > 0 or given with 0; a radius that is not positive or is
 * above max_range (as binary32); max_tiles < 1 for a grid with cells; a query with P < 1, NULL points, no output at all, or points
 * or towards not 8-byte aligned.  One launch each; every value has one writer; no atomics; nothing allocated, nothing waits:
 * both calls can be captured in a HIP graph. */
typedef struct MsNavClearance {
    float                max_range;    /* R, metres (> 0, finite)                                                      */
    int                  n_radii;      /* K, 0..8                                                                      */
    float                radii[8];     /* r_k, metres (> 0, <= R); the first K are read                                */
    int                  max_tiles;    /* the most 16 x 16 tiles - ceil(nx/16)*ceil(ny/16) - of any env: sizes the launch; an
                                          env of more still gets the right bits, a tile after another                  */
    const unsigned char* mask;         /* (N,) non-zero: compute this env; NULL: all.  Read on the device only.        */
    float*               values;       /* (starts[N],) out                                                             */
    int*                 nearest;      /* (starts[N],) out, or NULL                                                    */
    unsigned char*       fits;         /* K*starts[N] bytes out; NULL exactly when K == 0                              */
} MsNavClearance;
typedef struct MsNavClearQuery {
    int                  n_envs;       /* N: the scenery's                                                             */
    int                  n_points;     /* P: points per env                                                            */
    const float*         points;       /* (N, P, 2) x, y; 8-byte aligned                                               */
    const int*           skip;         /* (N, P) the agent whose own rows each point passes over, or NULL: none        */
    float                max_range;    /* R, metres (> 0, finite)                                                      */
    const unsigned char* mask;         /* (N, P) non-zero: compute this point; NULL: all.  Read on the device only.    */
    float*               distances;    /* (N, P) out, or NULL                                                          */
    int*                 nearest;      /* (N, P) out, or NULL                                                          */
    float*               towards;      /* (N, P, 2) out, or NULL; 8-byte aligned                                       */
} MsNavClearQuery;
int ms_nav_clearance(const MsScenery* scenery, const MsNavGrid* grid, const MsNavClearance* clearance, void* hip_stream);
int ms_nav_clear_query(const MsScenery* scenery, const MsAgents* agents /* NULL: static walls only */, const MsNavClearQuery* query,
                       void* hip_stream);

/* Items: things in the world that agents see, touch and collect - pickups, a goal object.  A store the caller owns, one call a step
 * that takes items (ms_item_collect) and one that draws them into rendered or cast rays (ms_item_overlay); the return of a taken
 * item composes what exists (MsNavDraws with mask = due, then a select).  Every step below is one binary32 operation, in the order
 * given, without contraction; tests/item_rule.py restates it in numpy and the kernels - and their host instantiations,
 * ms_host_item_collect and ms_host_item_overlay - are held to EQUALITY with it.  DESIGN.md section 3.34.
 * The store, P items an env (1 .. 1024):
 *   positions     (N, P, 2).  AN ITEM IS PRESENT EXACTLY WHEN BOTH COORDINATES ARE FINITE; an absent item holds (NaN, NaN), which
 *                 ms_nav_point_marks marks nothing for, ms_percepts never sees, the overlay's fold never hits and the reach test
 *                 fails for: every consumer treats an absent item correctly without a `valid` mask.
 *   timers        (N, P) int32: the calls left until an absent item is due to return; negative: never.
 *   kinds         (N, P) int32 in [0, K), 1 <= K <= 8 (an item of a kind outside that range is taken and counted nowhere).
 *   colors        (N, P, 3) linear RGB (the overlay's).
 * ms_item_collect, one call a step, the agents (px, py) = agents->positions[n, a] as they stand; reach2 = reach*reach formed once:
 *   reset         reset[n] != 0 ((N,) bytes; NULL: none): every item of the env becomes absent with timer 0, taker -1 and due 1,
 *                 the env's counts are 0; nothing is collected in that env in this call.
 *   candidate     otherwise, for a present item k at (x, y), agent a is a candidate iff takers[n, a] != 0 (NULL: everyone), px and
 *                 py are finite, rx = x - px, ry = y - py, rr = rx*rx + ry*ry, rr <= reach2, and - unless through_walls - no
 *                 static wall of the env (rows n_agents*n_model .. L - 1) blocks the pair: MsNavViews' meets, apart and across,
 *                 the agent as the viewpoint and the item as the centre, by the function ms_percepts calls.  BODIES DO NOT OCCLUDE.
 *   taker         (N, P): the candidate with the least (bits of rr, a) - the nearest, equal distances to the lower index; -1
 *                 without one (and for an absent item).
 *   taken         an item with a taker becomes absent - (NaN, NaN) is stored - and its timer is set to `delay`.
 *   tick          an item that was absent on entry has timer = timer > 0 ? timer - 1 : timer.
 *   due           (N, P) bytes: 1 exactly when the item is absent after this call and its timer is 0; otherwise 0.
 *   counts        (N, A, K): the items of kind j that agent a took in this call; rewritten whole by every call.
 * Every output is an integer or a stored NaN and each element has one writer.  taker, counts and due may each be NULL (not wanted).
 * Limits: 1 <= A <= 64 (MsScenery.n_agents), 1 <= P <= 1024, 1 <= K <= 8; `delay` is any int.
 * Refused before any launch (MS_EINVAL): a NULL agents or agents->positions, or positions not 8-byte aligned; A, P or K outside
 * those limits; a NULL positions, timers or kinds; reach not positive and finite; through_walls neither 0 nor 1; the store's
 * positions not 8-byte aligned; timers, kinds, taker or counts not 4-byte aligned.
 * One launch, a wave an env, a lane the items lane + 64 j; integer LDS atomics for the counts, no float atomics; nothing
 * allocated, nothing waits: the call can be captured in a HIP graph. */
typedef struct MsItemCollect {
    int                  n_items;        /* P: items per env (1 .. 1024)                                                   */
    int                  n_kinds;        /* K: kinds (1 .. 8)                                                              */
    float*               positions;      /* (N, P, 2) in/out; 8-byte aligned                                               */
    int*                 timers;         /* (N, P) in/out                                                                  */
    const int*           kinds;          /* (N, P)                                                                         */
    const unsigned char* takers;         /* (N, A) non-zero: the agent may take; NULL: everyone                            */
    const unsigned char* reset;          /* (N,) non-zero: empty the env's store; NULL: none                               */
    float                reach;          /* metres (> 0, finite)                                                           */
    int                  delay;          /* the timer of a taken item                                                      */
    int                  through_walls;  /* 1: walls do not block a taker                                                  */
    int*                 taker;          /* (N, P) out, or NULL                                                            */
    int*                 counts;         /* (N, A, K) out, or NULL                                                         */
    unsigned char*       due;            /* (N, P) out, or NULL                                                            */
} MsItemCollect;
int ms_item_collect(const MsScenery* scenery, const MsAgents* agents, const MsItemCollect* collect, void* hip_stream);

/* ms_item_overlay draws the items over the planes ms_render or ms_raycast wrote for a set of rays - a pass of its own: those
 * kernels are not touched.  Rays as ms_raycast takes them: dirs (N, R, 2), origins (N, Q, 2) with R % Q == 0, ray r starting at
 * origin r / (R/Q) (a render's fan: Q = A, the agents' positions, dirs of ms_camera_rays, the MsRender's planes as (N, A res); a
 * raycast's rays: Q = R).  For origin p = (px, py), ray direction ru and item k at c = (cx, cy):
 *   billboard     a segment of length 2*radius that always faces p: ux = cx - px, uy = cy - py, l = sqrtf(ux*ux + uy*uy),
 *                 nx = (-uy/l)*radius, ny = (ux/l)*radius, row = (cx - nx, cy - ny, cx + nx, cy + ny).  An absent item and an
 *                 origin that sits on the item give a row with a NaN, which is never hit.
 *   fold          from the state (s, idx, t) = (+inf, -1, NaN) the env's items are met in ascending k by the very function
 *                 ms_raycast folds its lines with (kernels.cu:352-377: hit iff 0 <= t <= 1, better iff near_plane/|ru| < s and
 *                 s < best s - 1e-4, the 1e-4 hysteresis included), |ru| = sqrtf(ru.x*ru.x + ru.y*ru.y).
 *   winner        item k with d = s*|ru|, dt = dtop/(dbot + 1e-6f) by ms_raycast's own closing lines (dtop = ru . v, dbot =
 *                 |ru|*|v|, v the billboard's direction) and dn = 1 - dt*dt REPLACES THE RAY WHEN d < distances[n, r] - strict; a
 *                 miss holds +inf.  Written only where the item wins: distances = d; screen[c] = dn*colors[n, k, c] (items are
 *                 emissive: no light is read); indices = lines_widths[n] + k, deliberately no line of the env - ms_shade reads
 *                 nothing for such an index and leaves black; locations = t; dots = dt.
 *   items         (N, R) int32, written for every ray: the k that won it, else -1.
 * An agent's body nearer than the item hides it, an item nearer than a wall hides the wall; items do not hide each other beyond
 * the fold's own rule.  distances is required, the other planes may be NULL; screen needs colors.
 * Refused before any launch (MS_EINVAL): P outside 1 .. 1024; R < 1, Q < 1 or R % Q != 0; a NULL positions, origins, dirs or
 * distances; screen without colors; radius not positive and finite; near_plane negative or a NaN; positions, origins or dirs not
 * 8-byte aligned; colors, distances, indices, locations, dots, screen or items not 4-byte aligned.  MS_EUNSUPPORTED: N*R, or the
 * launch's workgroups, beyond 2^31 - 1.
 * One launch: a workgroup takes up to 256 rays of one origin, builds the P billboards for that origin a lane an item (one sqrtf
 * and two divisions per item and origin, not per ray), compacts the rows without a NaN in ascending k into LDS, and every lane
 * folds its ray over them.  Nothing allocated, nothing waits: the call can be captured in a HIP graph. */
typedef struct MsItemOverlay {
    int          n_items;      /* P: items per env (1 .. 1024)                                                              */
    int          n_rays;       /* R: rays per env                                                                           */
    int          n_origins;    /* Q: origins per env; R % Q == 0                                                            */
    const float* positions;    /* (N, P, 2) the store's; 8-byte aligned                                                     */
    const float* colors;       /* (N, P, 3), or NULL (then no screen)                                                       */
    const float* origins;      /* (N, Q, 2); 8-byte aligned                                                                 */
    const float* dirs;         /* (N, R, 2); 8-byte aligned                                                                 */
    float        radius;       /* half the billboard's length, metres (> 0, finite)                                         */
    float        near_plane;   /* as MsRaycast's (>= 0)                                                                     */
    float*       distances;    /* (N, R) in/out                                                                             */
    int*         indices;      /* (N, R) in/out, or NULL                                                                    */
    float*       locations;    /* (N, R) in/out, or NULL                                                                    */
    float*       dots;         /* (N, R) in/out, or NULL                                                                    */
    float*       screen;       /* (N, R, 3) in/out, or NULL                                                                 */
    int*         items;        /* (N, R) out, or NULL                                                                       */
} MsItemOverlay;
int ms_item_overlay(const MsScenery* scenery, const MsItemOverlay* overlay, void* hip_stream);

/* Builds the wall grid (MsScenery.wg_*): per level of cells two launches with a prefix sum by the caller in between.
 *   ms_wallgrid_scan  for every cell of every env listed in `reps` (the representatives, MsScenery.env_geom; n_reps of
 *                     them) works out which static walls belong on the cell's lists: one bit per wall into `bits` - the
 *                     row of cell c (grid-local) of env n and kind k (0 vis, 1 near within wg_reach_lo, 2 near beyond that)
 *                     starts at word bits_starts[n] + (3 c + k) * ceil(walls(n)/32) - and the three counts into
 *                     counts[3*(wg_starts[n] + c) + k].  Reads wg_starts, wg_geom, wg_cell, wg_reach_lo, wg_reach, wg_near
 *                     of the scenery; `bits` and `counts` must start zeroed.
 *                     `parent`: a coarser grid over the same envs, scanned and filled before (same origin, cells a whole
 *                     multiple of wg_cell in size, near lists as indices): only what is on a parent cell's lists is looked
 *                     at for the cells inside it - exact (a wall hidden from, or out of reach of, the larger cell is so for
 *                     every cell within) and an order of magnitude less work on large floorplans.  NULL: every wall.
 *                     max_groups: with a parent the most parent cells any listed env has, without ceil(most cells / 4).
 *   ms_wallgrid_fill  writes the lists: the set bits of each row, in order, from the cell's wg_cells offsets (which the
 *                     caller has filled in from the counts) - vis lists as entries of `vis_entries` (MsScenery.wg_pool's
 *                     format) from the env's wg_pool_base on (which the scenery must carry then), near lists as rows into
 *                     `near_rows`; or, for a parent level (both NULL; wg_pool_base is not looked at), both lists as
 *                     16-bit indices into `pool`.
 * An env with more than 65535 static walls must have a grid of 0 cells. */
#define MS_WALLGRID_MAX_FOV 165.f
typedef struct MsWallGridParent {
    const unsigned* cells; const int* starts; const float* geom; float cell; const unsigned short* pool;
} MsWallGridParent;
int ms_wallgrid_scan(const MsScenery* scenery, const MsWallGridParent* parent, const int* reps, int n_reps, int max_groups,
                     const long long* bits_starts, unsigned* bits, unsigned* counts, void* hip_stream);
int ms_wallgrid_fill(const MsScenery* scenery, const int* reps, int n_reps, int max_cells,
                     const long long* bits_starts, const unsigned* bits, unsigned short* pool, unsigned* vis_entries,
                     float* near_rows, void* hip_stream);
/* The host instantiations of the kernels' culls (ms_host_*) and the debug switches (ms_debug_*), which exist for the CPU
 * tests and A/B runs only, are declared in megastep_hip_test.h: not part of the interface a maintainer binds. */

#ifdef __cplusplus
}
#endif
#endif /* MEGASTEP_HIP_H */
