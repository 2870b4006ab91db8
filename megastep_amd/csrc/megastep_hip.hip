// megastep_hip.hip -- gfx950 (MI355X / CDNA4) simulation core behind include/megastep_hip.h.
//
// One translation unit: this file holds the switches, the probe macros and the host side of the C-ABI (argument checks,
// launches); the kernels are in kernels/*.h, included below inside the anonymous namespace - math.h (scalar helpers shared
// with the ms_host_* test hooks), physics.h, slide.h, rollout.h, scenario.h, lighting.h, render.h, bake.h, wallgrid.h, raycast.h, overhead.h, navfield.h, navclear.h, navregion.h, navview.h, percept.h, navpath.h, navpull.h, navbasin.h, navzone.h, navseen.h, navage.h, navwindow.h, navdraw.h; culltest.h (the ms_test_* probes of the culls) last.
//
// Thirty-two kernels, all written wave64-first (DESIGN.md section 3 has the full story of each):
//
//   physics_kernel<MOVE, EXTRA, PACK>   one wavefront per env (PACK = 1: per few consecutive envs, side by side - large
//                   worlds of few agents per env): lane = agent for the state, the reach and the agent-agent
//                   tests; the walls from the near lists of the agents' cells of the wall grid (rows of the dozen walls
//                   within reach, dealt to the lanes one (wall, agent) pair each) - or, where no list applies, a sweep
//                   over all the env's walls (buffer loads in flight, lane = wall, reach boxes in scalar registers,
//                   compacted pairs); the exact collision test, atomicMin fold, integration epilogue; leaves each
//                   agent's sin/cos for the renderer.  MOVE = 1 runs the movement modules' velocity update first,
//                   EXTRA = 1 the envs' respawn / lifespan / IMU bookkeeping.  Where the agents carry a fan schedule, the
//                   launch's first blocks sort the last render's costs into the next render's starting order.
//                                                            (reference: kernels.cu:179-230, modules.py:24-118,263-366)
//   rollout_kernel      candidate action plans rolled through that step: one wavefront per (agent, 64 plans), a lane a plan,
//                   the state in registers for the whole horizon; each step a lane walks the near list of the cell it stands
//                   in (or, where no list applies, its env's static rows) through the step's own functions.   (no counterpart)
//   rollout_walls_kernel   the same rule by physics_kernel's scheme - a lane a wall, the candidates one after another, the
//                   surviving pairs compacted in LDS before the exact test: behind ms_debug_rollout_scheme, for A/B runs.
//   scenario_kernel     whole envs forked S ways, every agent on its own plan: a wavefront holds 64 / A whole scenarios, a lane
//                   an agent of one; each step the lanes of a scenario show each other their moved (p, v/fps) through LDS and
//                   meet as physics_kernel's ordered pairs do, then walk their cells' near lists as rollout_kernel.  (no counterpart)
//   render_kernel<OBS, SHADE, NG, STEP>   (OBS = 2: pooled observations only, no plane stores in the kernel; STEP = 1: a
//                   single-agent env's physics step first, in the same wave - ms_step_render's one launch a step)
//                   one wavefront per (env, agent, 64-ray group) - or, NG = 4, per four such groups
//                   that share one list of lines, the launch's last envs left to one-group waves (256 rays and up on large
//                   launches; SHADE = 0: no shading pass, for callers that want no colour).  The lines it meets: the other agents'
//                   and the walls on the vis list of the agent's cell of the wall grid, less those whose view arc misses
//                   the wave's rays.  Pass 1 (lane = line) turns every line into a conservative interval of the wave's
//                   rays and compacts the visible ones into an LDS list; pass 2 deals the (line, ray) pairs of the list
//                   to the lanes, 64 at a time, one exact intersection each, merged per ray with one 64-bit LDS atomic;
//                   the order-dependent nearest-hit rule is resolved from the three smallest keys (or a literal fold
//                   where it must be); rays that landed on an agent are lit through the light grid; shading; optional
//                   pooled observations, crosshair ids and first-sight books.  draw, raycast and shader (three launches +
//                   five allocations in the reference) are one launch.
//                                                            (reference: kernels.cu:297-475)
//   render_prep_kernel, dynlight_kernel   the renderer's helpers for callers without a heading cache / light grid.
//   visibility_kernel, bake_sum_kernel    the two-phase bake: per (representative env, light) the walls that can shadow
//                   each angular bin; per texel the sum over the lights, occluders looked up by bin.
//   bake_kernel     the one-pass bake: one workgroup per env, lane = texel, the env's occluders staged once in LDS.
//                                                            (reference: kernels.cu:238-293)
//   lightgrid_kernel, lightlist_kernel   per (cell, light) LIT / DARK / UNKNOWN verdicts and candidate walls.
//   wallgrid_scan_kernel, wallgrid_fill_kernel   the wall grid: per cell of a floorplan which walls can matter to a ray
//                   from the cell (one wall hiding another from the whole cell, exactly) and which an agent in it can
//                   touch; and the lists made of that.   (replaces the all-lines loops kernels.cu:203-205,352-377)
//   raycast_kernel, camera_rays_kernel   ray queries: one lane per caller-given ray (origin, direction), the reference's
//                   per-ray fold over the agents drawn in registers and the vis list of the origin's cell (or every
//                   wall); and the render's own camera rays as data.   (reference: kernels.cu:234-236,349-382; no
//                   counterpart as an entry point)
//   overhead_kernel     top-down pictures: one workgroup per 16 x 16 tile of an image, the env's lines culled against the
//                   tile's footprint into LDS, then each lane's pixel folded over them.   (reference: plotting.py draws
//                   these with matplotlib, one env at a time on the host)
//   nav_free_kernel, nav_relax_kernel, nav_query_kernel   shortest-path distance fields: which cells of a grid over a floorplan
//                   keep the agent's radius clear of every wall; per goal one workgroup that relaxes the 8-connected field in
//                   LDS until nothing changes - from a goal's anchors, or (SEEDED) from a set of cells at 0: the distance to
//                   the nearest of them; and the distance from any point to a goal, four gathers.   (no counterpart)
//   nav_waypoint_kernel, nav_path_kernel   which way to go on those fields: one wavefront per point descends the field a
//                   neighbour a lane and picks the furthest of the next cells the point can see; and whole paths, a lane
//                   each.   (no counterpart)
//   nav_pull_kernel     pulled paths: one wavefront per path walks the whole chain once through a ring in LDS and straightens
//                   it by sight, the candidates of a window a lane each: a handful of vertices, and the path's length.
//                                                            (no counterpart)
//   nav_seen_kernel     seen maps: one workgroup per map marks the grid cells under the samples of its viewers' depth rays in
//                   an LDS bitmask, merges it into the map and counts the countable cells seen for the first time.
//                                                            (no counterpart)
//   nav_age_kernel      age maps: the same scheme with a binary32 tick per cell - the marked set takes the map's clock, the
//                   countable cells swept, gained and their summed age are counted, and a survey behind a second barrier gives
//                   every cell's age, the largest and the summed age and the stale cells.
//                                                            (no counterpart)
//   nav_window_kernel   map windows: per-cell stores (free cells, seen maps, fields) cropped and turned into images through
//                   affine views, every image and channel in one launch, a lane a pixel.
//                                                            (no counterpart)
//   nav_draw_kernel     cell draws: one workgroup per draw set ballots the env's qualifying cells into an LDS bitmap, scans the
//                   popcounts and picks each draw's cell by rank, from a hash of a counter it moves on itself.
//                                                            (no counterpart)
//   nav_view_kernel     view fields: one workgroup per viewpoint culls the env's static walls into LDS and tests the centre of
//                   every cell in range against them, a lane a cell: the cells in sight, how many count, how many are new.
//                                                            (no counterpart)
//   percept_kernel      percepts: one workgroup per env culls the env's static walls into LDS; a wave an eye, a lane the points
//                   lane + 64 j, each pair through the view fields' own predicates: which points each eye sees, how far and which
//                   way, the count, and the nearest K by K rounds of a wave-wide minimum.
//                                                            (no counterpart)
//   nav_clear_kernel, nav_clear_query_kernel   clearance: the distance to the nearest wall - per cell, overhead_kernel's scheme on
//                   the grid's 16 x 16 tiles (the env's static rows culled against the tile's box into LDS, a second cull by the
//                   wave's own worst best while it folds); per point one wave, the lanes striding the rows (the other agents'
//                   bodies too) and a shuffle minimum.   (no counterpart)
//   explorer_kernel    the Explorer env's books between frames (reward, episode rule, forgetting) as one launch.
//                                                            (reference: demo/envs/explorer.py:45-90)
//   deathmatch_kernel   the Deathmatch env's game logic between frames (revive, crosshairs, hits and wounds, health, damage,
//                   reward, next step's dead) as one element-wise launch behind ms_render.
//                                                            (reference: demo/envs/deathmatch.py:46-88)
//
// Numerics contract: IEEE binary32 evaluated as the reference source is written -- compiled with
// -ffp-contract=off, correctly rounded divide/sqrt, no fast-math -- so that collision masks and hit
// indices are bit-identical to the CPU oracle and floats agree far inside the 1e-5 tolerance.
// Every shortcut below (division-free tests, culling, hoisting) is exact, not approximate.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <vector>
#include "../../include/megastep_hip_test.h"

namespace {

constexpr float AMBIENT = .1f;      // kernels.cu:9
constexpr float LUMINANCE = 2.f;    // kernels.cu:240
constexpr int WAVE = 64;
constexpr int WG = 256;             // 4 waves per workgroup
constexpr int WAVES = WG/WAVE;

// The library keeps NO process-wide state: what the entry points need travels in their arguments (MsConfig by value).  What
// follows is per THREAD - the last HIP error, and the test / A-B hooks of megastep_hip_test.h (ms_debug_*), which pin choices
// ms_render / ms_step_physics otherwise make from the shapes: a thread that pins one changes its own calls only, every other
// thread gets the product's behaviour.  (Round 4 had these as plain globals: a test hook changed the launches of the whole process.)
thread_local int g_last_hip_error = 0;
thread_local int g_pair_telemetry = 0;      // ms_debug_pair_telemetry
thread_local int g_ray_groups = 0;          // ms_debug_ray_groups: 0 = ms_render picks render_kernel's NG from the resolution
thread_local int g_physics_pack = 0;        // ms_debug_physics_pack: 0 = ms_step_physics picks the envs a physics wave takes side by side, k >= 1 = k
thread_local float g_tail_rounds = -1.f;    // ms_debug_ray_group_tail: < 0 = ms_render's own share of one-group waves at the end of a launch of wide ones
thread_local int g_tail_envs = -1;          //   ... >= 0: that many envs exactly
thread_local int g_last_step_fused = 0;     // ms_debug_last_step_fused: did this thread's last ms_step_render go out as one launch?
thread_local int g_last_render_groups = 0;  // ms_debug_last_render_groups: the NG this thread's last ms_render launched
thread_local int g_overhead_cull = 1;       // ms_debug_overhead_cull: 0 = ms_overhead's tiles keep every line
thread_local int g_nav_cost_variant = -1;   // ms_debug_nav_cost_variant: where ms_nav_cost_fields' launch keeps the multipliers (-1: its own choice)
thread_local int g_nav_pull_scheme = -1;    // ms_debug_nav_pull_scheme: how ms_nav_pulls' waves test their sights (-1: its own choice)
thread_local int g_rollout_scheme = -1;     // ms_debug_rollout_scheme: how ms_rollouts' waves meet their walls (-1: its own choice)
thread_local int g_nav_clear_cull = -1;     // ms_debug_nav_clear_cull: which culls ms_nav_clearance's launch runs (-1: its own choice)
thread_local long long g_clear_folds = 0, g_clear_pairs = 0;      // ms_host_nav_clear_folds: the last ms_host_nav_clearance's
thread_local int g_render_order = 1;        // ms_debug_render_order: 0 = MsAgents.schedule is neither sorted nor followed

// The agents as the kernels take them: MsAgents less its fan schedule, which only physics_kernel's sort waves (FanSort) and the
// render instantiations of one ray group a wave (RenderConstsOrder) are given, behind their other arguments - so that the
// kernel-argument segment of every kernel is byte for byte what it was before there was a schedule (render.h, RenderConstsStep:
// the wide colour instantiations' time moves with their argument layout).
struct AgentsK { float* angles; float* positions; float* angvelocity; float* velocity; float* headings; };
AgentsK agents_k(const MsAgents& a) { return AgentsK{a.angles, a.positions, a.angvelocity, a.velocity, a.headings}; }

// -DMS_PROBE=1 (`make probe`, tools/probe_waves.py): every wave of physics_kernel and render_kernel leaves a record of
// time stamps (s_memtime at its start, at a few points where something it waited for has arrived, at its end) and of
// the SIMD it ran on, for a picture of how a launch fills and drains the chip.  Compiled out of the product library.
#ifndef MS_PROBE
#define MS_PROBE 0
#endif
#if MS_PROBE
constexpr int PROBE_STAMPS = 8;        // a record: 8 stamps (low 32 bits of s_memtime), then where the wave ran
constexpr int PROBE_WORDS = 16;        // ... the real-time counter at its start and end, and five numbers of the wave's choosing
__device__ unsigned* g_probe = nullptr;                // one record per wave, indexed by the wave's number in its launch
__device__ long long g_probe_cap = 0;
// (one VGPR: lane k holds stamp k, the low 32 bits of s_memtime - a wave's record costs the kernel one register and no
// traffic until its end; records are indexed by wave, not drawn from a cursor: thousands of atomics on one address
// would be the slowest thing in the launch)
struct Probe {
    unsigned t = 0u, real0 = (unsigned)wall_clock64();
    __device__ void done(const int lane, const long long wave) {
        if (g_probe && wave < g_probe_cap) {
            unsigned v = t;
            if (lane == PROBE_STAMPS) v = ((unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4) & 0xffffu) | ((unsigned)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xf) << 16);   // HW_ID, XCC_ID
            if (lane == PROBE_STAMPS + 1) v = real0;                    // s_memtime counts per XCD; the 100 MHz real-time counter is the chip's
            if (lane == PROBE_STAMPS + 2) v = (unsigned)wall_clock64();
            if (lane < PROBE_WORDS) g_probe[wave*PROBE_WORDS + lane] = v;     // (lanes 11..15: numbers left by PROBE_VAL)
        }
    }
};
#define PROBE_STAMP(k) { const unsigned c_ = (unsigned)clock64(); asm volatile("v_writelane_b32 %0, %1, " #k : "+v"(probe_.t) : "s"(c_)); }
#define PROBE_INIT Probe probe_; PROBE_STAMP(0)
// a stamp once `v` (a float or an int the wave has been waiting for) is in a register
#define PROBE_AT(i, v) { asm volatile("" :: "v"(v)); PROBE_STAMP(i) }
#define PROBE_DONE(wave) { PROBE_STAMP(7) probe_.done(lane, (long long)(wave)); }
// a (wave-uniform) number instead of a time in slot k
#define PROBE_VAL(k, x) { const unsigned c_ = (unsigned)__builtin_amdgcn_readfirstlane((int)(x)); asm volatile("v_writelane_b32 %0, %1, " #k : "+v"(probe_.t) : "s"(c_)); }
#else
#define PROBE_INIT
#define PROBE_AT(i, v)
#define PROBE_DONE(tag)
#define PROBE_VAL(k, x)
#endif

#include "kernels/math.h"
#include "kernels/physics.h"
#include "kernels/slide.h"
#include "kernels/rollout.h"
#include "kernels/scenario.h"
#include "kernels/lighting.h"
#include "kernels/render.h"
#include "kernels/bake.h"
#include "kernels/wallgrid.h"
#include "kernels/raycast.h"
#include "kernels/shade.h"
#include "kernels/overhead.h"
#include "kernels/navfield.h"
#include "kernels/navclear.h"
#include "kernels/navregion.h"
#include "kernels/navview.h"
#include "kernels/percept.h"
#include "kernels/navpath.h"
#include "kernels/navpull.h"
#include "kernels/navbasin.h"
#include "kernels/navzone.h"
#include "kernels/navseen.h"
#include "kernels/navage.h"
#include "kernels/navwindow.h"
#include "kernels/navdraw.h"
#include "kernels/envlogic.h"
#include "kernels/culltest.h"

// ------------------------------------------------------------------------------------------------
// launch geometry (host): what ms_render / ms_step_physics decide before a launch - also behind ms_host_render_plan /
// ms_host_physics_pack, so that tests walk whole launches on the CPU (tests/test_launch_geometry.py)
// ------------------------------------------------------------------------------------------------
// Ray groups per wave (render_kernel's NG): an agent's groups of 64 rays share the wave's list of walls instead of each wave
// building its own.  Measured: four groups pay from 256 rays up - a quarter of the vector instructions saved
// without colour, a sixth with - IF the launch has two and a half rounds of such waves to fill the machine with and every XCD's
// last envs are left to waves of one group (render_block): 4096 x 4 x 512 rays 157.5 -> 139.0 us (colourless 127.4 -> 104.7),
// C5's share 216.7 -> 196.7; with a round or less of them - 4096 x 1 x 256 rays - a quarter is LOST.  Two groups never pay.
// `pinned`: ms_debug_ray_groups (1, 2, 4; else the rule above).  The one-group waves' share: `tail_rounds` rounds of the
// machine's wave slots' worth of the wide waves' work (< 0: half a round), or `tail_envs` envs exactly if >= 0.
struct RenderPlan { int ng; long long n_blocks; };
RenderPlan render_plan(const int n_envs, const int n_agents, const int R, const int slots, const int pinned, const float tail_rounds,
                       const int tail_envs_exact, RenderConsts& rc) {
    int ng = 1;
    if (R >= 4*WAVE && 2LL*n_envs*n_agents*((R + 4*WAVE - 1)/(4*WAVE)) >= 5LL*slots) ng = 4;   // (2.5 rounds, the one-group waves' half included)
    if (pinned == 1 || pinned == 2 || pinned == 4) ng = pinned;
    int tail = 0;
    const int G1 = (R + WAVE - 1)/WAVE;
    const int envs_lo = n_envs/8, envs_rem = n_envs % 8, envs_hi = envs_lo + (envs_rem ? 1 : 0);
    if (ng > 1) {
        const double rounds = tail_rounds >= 0.f ? (double)tail_rounds : 0.5;
        const long long tail_envs = tail_envs_exact >= 0 ? tail_envs_exact : (long long)ceil(rounds*slots*ng/((double)n_agents*G1));
        tail = (int)std::min<long long>((tail_envs + 7)/8, envs_hi);                        // per XCD
        if (tail >= envs_hi && !(pinned > 1)) ng = 1;                 // nothing left for the wide waves: the plain kernel
    }
    const int G = (R + ng*WAVE - 1)/(ng*WAVE);
    rc.by_f = divisor_of((unsigned)(n_agents*G));
    rc.by_g = divisor_of((unsigned)G);
    rc.by_f1 = divisor_of((unsigned)(n_agents*G1));
    rc.by_g1 = divisor_of((unsigned)G1);
    rc.envs_lo = envs_lo; rc.envs_rem = envs_rem; rc.tail = tail;
    // (NG > 1: every XCD as many blocks as the one with the most envs needs)
    const long long n_blocks = ng > 1 ? 8LL*((long long)(envs_hi - std::min(tail, envs_hi))*n_agents*G + (long long)std::min(tail, envs_hi)*n_agents*G1)
                                      : (long long)n_envs*n_agents*G;
    return RenderPlan{ng, n_blocks};
}

// Envs per wave (physics_kernel's PACK), with a wall grid (without one an env's walls are streamed, and there is nothing to put
// side by side) and while a wave's agents stay within half its lanes: as many as bring the launch down to about 4096 waves -
// 32768 envs of one agent are 5.3 rounds of waves with a lane or two at work each: 30.2 us; eight to a wave 9.7 (four 13.6,
// sixteen 10.2); 16384 x 4 agents 22.2 -> 13.3 (eight: 17.8), 8192 x 4 13.4 -> 10.2 - and two even at 4096 envs, where one round
// of short waves becomes half a round of waves twice as busy (8.7 -> 8.2 us; three 8.7, four 9.5; one agent per env 7.1 -> 6.4).
// `pinned`: ms_debug_physics_pack (>= 1; else the rule).
int physics_pack_of(const int n_envs, const int n_agents, const bool gridded, const int pinned) {
    int pack = 1;
    if (gridded && n_agents <= 16) {
        pack = n_envs > 6144 ? std::min((n_envs + 4095)/4096, 16) : n_envs >= 3072 ? 2 : 1;
        pack = std::max(std::min(pack, WAVE/2/n_agents), 1);
    }
    if (pinned >= 1) pack = (gridded && (long long)pinned*n_agents <= WAVE) ? pinned : 1;
    return pack;
}

// ------------------------------------------------------------------------------------------------
// host side of the C-ABI
// ------------------------------------------------------------------------------------------------
int hip_fail(hipError_t e) { g_last_hip_error = (int)e; return MS_EHIP; }
int launch_status() { const hipError_t e = hipGetLastError(); return e == hipSuccess ? MS_OK : hip_fail(e); }   // (after the launches)

// The wave slots render_kernel has on the CURRENT device (CUs x 4 SIMDs x the waves per SIMD its registers are held to): what
// sizes a launch's choice of ray groups and its tail.  Looked up once per device (a process may drive several, of different
// sizes: round 4 kept the first caller's); a benign race - every writer stores the same number.
int wave_slots_here() {
    constexpr int MAX_DEVICES = 64;
    static std::atomic<int> slots_of[MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256*4*MS_WAVES;
    if (dev >= 0 && dev < MAX_DEVICES) { const int known = slots_of[dev].load(std::memory_order_relaxed); if (known) return known; }
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const int slots = cus*4*MS_WAVES_WIDE;                             // (what sizes launches of wide waves: theirs)
    if (dev >= 0 && dev < MAX_DEVICES) slots_of[dev].store(slots, std::memory_order_relaxed);
    return slots;
}

bool scenery_ok(const MsScenery* s) {
    return s && s->n_envs > 0 && s->n_agents > 0 && s->n_model > 0 && s->lines_vals && s->lines_widths &&
           s->lines_starts && s->model && ((uintptr_t)s->lines_vals % 16 == 0) && ((uintptr_t)s->model % 16 == 0);
}
bool agents_ok(const MsAgents* a) { return a && a->angles && a->positions && a->angvelocity && a->velocity; }
bool config_ok(const MsConfig* c) {
    return c && c->res > 0 && c->fps > 0.f && c->agent_radius > 0.f && c->fov > 0.f && c->fov < 180.f;
}
AgentsK agents_or_none(const MsAgents* a) { return a ? agents_k(*a) : AgentsK{nullptr, nullptr, nullptr, nullptr, nullptr}; }
// The fan schedule serves launches in which every agent is ONE wave of the render: at most 64 rays (ms_step_physics sorts on this
// alone - it cannot know what the render behind it will be asked for; a table nobody follows costs it a few dozen short waves).
bool schedule_serves(const MsAgents* a, const MsScenery* sc, const int R) {
    return g_render_order && a->schedule && R <= WAVE && (long long)sc->n_envs*sc->n_agents <= 0x3fffffffLL;
}

// kernels.cu:22: the camera's half-width at unit distance, as every launch that casts its rays works it out
float half_screen_of(const float fov) { return tanf(3.14159265358979323846f/180.f*fov/2.); }

// The light grid is all or nothing: render_kernel lights agent-hit rays itself when it is there.
bool light_grid_in(const MsScenery* sc) { return sc->lg_vals && sc->lg_starts && sc->lg_geom && sc->lg_cell > 0.f; }
// The wall grid's vis lists serve rays of this near plane: they were built for near planes below wg_near (wallgrid_scan_kernel).
bool vis_lists_serve(const MsScenery* sc, const float near_plane) {
    return sc->wg_cells && sc->wg_starts && sc->wg_geom && sc->wg_pool && sc->wg_pool_base && sc->wg_cell > 0.f &&
           near_plane*1.001f < sc->wg_near;
}

// (the optional structs of ms_step_physics / ms_move_step_render, checked alike)
bool step_options_ok(const MsMovement* mv, const MsStepExtras* ex) {
    if (mv && (!mv->actions || !mv->table || mv->n_actions < 1 || !(mv->keep == mv->keep))) return false;
    if (ex) {
        if (ex->spawn_positions && (!ex->spawn_angles || !ex->respawn_mask || !ex->respawn_choice || ex->n_spawns < 1 ||
                                    ((uintptr_t)ex->spawn_positions % 8))) return false;
        if (ex->lifespans && (!ex->max_lifespans || !ex->fresh_max)) return false;
        if (ex->imu && !(ex->imu_ang_scale == ex->imu_ang_scale && ex->imu_speed_scale == ex->imu_speed_scale)) return false;
    }
    return true;
}
// ... and as the kernels take them: all-NULL structs for none, the IMU scales inverted (the kernels multiply: see their IMU reading)
void step_options_of(const MsMovement* mv, const MsStepExtras* ex, MsMovement& mvv, MsStepExtras& exv) {
    mvv = mv ? *mv : MsMovement{nullptr, nullptr, 0, 0.f};
    exv = ex ? *ex : MsStepExtras{nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 1.f, 1.f};
    exv.imu_ang_scale = 1.f/exv.imu_ang_scale; exv.imu_speed_scale = 1.f/exv.imu_speed_scale;
}

// ray_interval's launch-invariant values as ms_render works them out, the per-wave ones as render_kernel does: wave `wave` of
// 64 x groups rays (ms_host_ray_interval_wide and ms_test_ray_interval)
RaySpan ray_span_of(const int res, const float fov, const float agent_radius, const int groups, const int wave) {
    const float half_screen = half_screen_of(fov);
    const float x_clip = 0.5f*agent_radius/sqrtf(1.f + half_screen*half_screen), c_b = 0.5f*(float)res/half_screen;
    const int nr = WAVE*groups, r0 = wave*nr;
    const float c_a = 0.5f*((float)res - 1.f), g0 = (float)r0;
    const int r_last = (r0 + nr - 1 < res - 1) ? r0 + nr - 1 : res - 1;
    return RaySpan{x_clip, c_a, c_b, g0, (float)(r_last - r0), (float)nr};
}

// One element a lane (arithmetic_test_kernel and kernels/culltest.h): `ok` = every pointer the kernel reads is there.
template <typename... Params, typename... Args>
int launch_elements(void (*kernel)(Params...), const bool ok, const long long count, void* stream, Args... args) {
    if (count < 0 || !ok) return MS_EINVAL;
    if (count == 0) return MS_OK;
    const long long blocks = (count + WG - 1)/WG;
    if (blocks > 0x7fffffffLL) return MS_EUNSUPPORTED;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(WG), 0, (hipStream_t)stream, args..., count);
    return launch_status();
}

}  // namespace

extern "C" {

int ms_abi_version(void) { return MS_ABI_VERSION; }

const char* ms_strerror(int code) {
    switch (code) {
        case MS_OK: return "ok";
        case MS_EINVAL: return "invalid argument (null/misaligned pointer, non-positive size or bad config)";
        case MS_EHIP: return "a HIP runtime call failed (see ms_last_hip_error)";
        case MS_EUNSUPPORTED: return "shape not supported by the gfx950 kernels";
        case MS_ENODEVICE: return "no HIP device visible";
        default: return "unknown megastep_hip error";
    }
}

int ms_last_hip_error(void) { return g_last_hip_error; }

int ms_device_count(void) {
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { g_last_hip_error = (int)e; return MS_ENODEVICE; }
    return n;
}

void ms_host_sincospi(float x, float* s, float* c) { sincospi_f(x, *s, *c); }

int ms_host_bake_point_bin(float light_x, float light_y, float x, float y) { return bake_point_bin(p2(light_x, light_y), p2(x, y)); }
void ms_host_bake_wall_bins(float light_x, float light_y, float ax, float ay, float bx, float by, int* first, int* count) {
    bake_wall_bins(p2(light_x, light_y), ax, ay, bx, by, *first, *count);
}

#if MS_PROBE
// (probe builds only, not part of the ABI) buf: device memory of capacity records of 11 32-bit words (8 stamps, HW_ID |
// XCC_ID << 16, the real-time counter at the wave's start and end), or NULL to stop recording
int ms_debug_probe(unsigned* buf, long long capacity) {
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_probe), &buf, sizeof buf) != hipSuccess) return hip_fail(hipGetLastError());
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_probe_cap), &capacity, sizeof capacity) != hipSuccess) return hip_fail(hipGetLastError());
    return MS_OK;
}
#endif

int ms_debug_ray_groups(int groups) { g_ray_groups = groups; return MS_OK; }
int ms_debug_last_render_groups(void) { return g_last_render_groups; }
int ms_debug_physics_pack(int envs) { g_physics_pack = envs; return MS_OK; }
int ms_host_physics_pack(int n_envs, int n_agents, int gridded, int pinned) { return physics_pack_of(n_envs, n_agents, gridded != 0, pinned); }
long long ms_host_render_plan(int n_envs, int n_agents, int res, int slots, int pinned_groups, float tail_rounds, int tail_envs, int* groups) {
    RenderConsts rc;
    const RenderPlan plan = render_plan(n_envs, n_agents, res, slots, pinned_groups, tail_rounds, tail_envs, rc);
    if (groups) *groups = plan.ng;
    return plan.n_blocks;
}
int ms_host_render_block(int n_envs, int n_agents, int res, int slots, int pinned_groups, float tail_rounds, int tail_envs, long long block, int* out4) {
    RenderConsts rc;
    const RenderPlan plan = render_plan(n_envs, n_agents, res, slots, pinned_groups, tail_rounds, tail_envs, rc);
    int fan = 0;
    if (block < 0 || block >= plan.n_blocks) return -1;
    return render_block((int)block, (int)plan.n_blocks, n_agents, res, plan.ng, rc, out4[0], out4[1], out4[2], out4[3], fan) ? 1 : 0;
}
int ms_debug_ray_group_tail(float rounds, int envs) { g_tail_rounds = rounds; g_tail_envs = envs; return MS_OK; }
int ms_debug_pair_telemetry(int on) { g_pair_telemetry = on ? 1 : 0; return MS_OK; }
int ms_debug_render_order(int on) { g_render_order = on ? 1 : 0; return MS_OK; }
int ms_host_order_fans(int n_fans, const int* costs, int* order) {
    // fan_sort_wave, sort wave after sort wave: the classes' first ranks, slowest class first, then every fan its class's next rank
    if (n_fans < 1 || !costs || !order) return -1;
    const int K = fan_sort_per_run(n_fans);
    for (int block = 0; block < 8*K; block++) {
        int first_fan, count, first_slot, next[FAN_CLASSES] = {0};
        fan_sort_part(n_fans, K, block, first_fan, count, first_slot);
        for (int i = 0; i < count; i++) next[fan_class(costs[first_fan + i])]++;
        for (int c = FAN_CLASSES - 1, rank = 0; c >= 0; c--) { const int m = next[c]; next[c] = rank; rank += m; }
        for (int i = 0; i < count; i++) order[first_slot + K*next[fan_class(costs[first_fan + i])]++] = first_fan + i;
    }
    return 8*K;
}

int ms_test_arithmetic(const float* n, const float* d, float* q_inrange, float* q_ieee, const float* x, float* r_any, float* r_ieee,
                       long long count, void* stream) {
    const bool ok = !((q_inrange || q_ieee) && !(n && d)) && !((r_any || r_ieee) && !x);
    return launch_elements(arithmetic_test_kernel, ok, count, stream, n, d, q_inrange, q_ieee, x, r_any, r_ieee);
}
int ms_test_agents_apart(const float* me, const float* other, const float* radius, unsigned char* apart, long long count, void* stream) {
    return launch_elements(agents_apart_test_kernel, me && other && radius, count, stream, me, other, radius, apart);
}
int ms_test_wall_beyond(const float* agent, const float* wall, const float* radius, float* reach, unsigned char* beyond, long long count,
                        void* stream) {
    return launch_elements(wall_beyond_test_kernel, agent && wall && radius, count, stream, agent, wall, radius, reach, beyond);
}
int ms_test_ray_interval(const float* pose, const float* line, int res, float fov, float agent_radius, int groups, int wave, int* first,
                         int* rays, long long count, void* stream) {
    // (a wave of a launch ms_render could make: config_ok's ranges, NG of 1, 2 or 4, a run of rays that starts below res)
    if (!(res > 0 && fov > 0.f && fov < 180.f && agent_radius > 0.f && (groups == 1 || groups == 2 || groups == 4) && wave >= 0 &&
          (long long)wave*WAVE*groups < res)) return MS_EINVAL;
    return launch_elements(ray_interval_test_kernel, pose && line, count, stream, pose, line, ray_span_of(res, fov, agent_radius, groups, wave), first, rays);
}
int ms_test_wedge(const float* right, const float* left, int* wa, int* wb, long long count, void* stream) {
    return launch_elements(wedge_test_kernel, right && left, count, stream, right, left, wa, wb);
}
int ms_test_cell_at(const float* geom, const float* cell, const float* point, int* index, unsigned char* inside, long long count, void* stream) {
    return launch_elements(cell_at_test_kernel, geom && cell && point, count, stream, geom, cell, point, index, inside);
}
int ms_test_tex_filter(const float* x, const int* w, int* l, int* r, float* lw, float* rw, long long count, void* stream) {
    return launch_elements(tex_filter_test_kernel, x && w, count, stream, x, w, l, r, lw, rw);
}
int ms_test_light_blocked(const float* light, const float* to, const float* a, const float* v, unsigned char* blocked, long long count,
                          void* stream) {
    return launch_elements(light_blocked_test_kernel, light && to && a && v, count, stream, light, to, a, v, blocked);
}

void ms_host_ray_interval_wide(const float* pose, const float* line, int res, float fov, float agent_radius, int groups, int wave,
                               int* first, int* count) {
    ray_interval_of(pose, line, ray_span_of(res, fov, agent_radius, groups, wave), *first, *count);
}
void ms_host_ray_interval(const float* pose, const float* line, int res, float fov, float agent_radius, int group, int* first, int* count) {
    ms_host_ray_interval_wide(pose, line, res, fov, agent_radius, 1, group, first, count);
}

int ms_host_lightgrid_cell(const float* walls, int n_walls, const float* lights, int n_lights, float ox, float oy, int nx, int ny,
                           float cell, int c, unsigned* words, unsigned* candidates, int max_candidates) {
    // lightgrid_kernel's verdicts and lightlist_kernel's candidates for one cell, from the predicates those are compiled from
    const LgCell k = lg_cell_of(make_float4(ox, oy, (float)nx, (float)ny), cell, c);
    const int num_i = n_lights < LG_LIGHTS ? n_lights : LG_LIGHTS;
    words[0] = words[1] = words[2] = words[3] = 0u;
    int count = 0;
    for (int i = 0; i < num_i; i++) {
        const LgView v = lg_view_of(k, p2(lights[3*i], lights[3*i + 1]));
        bool touched = false, dark = false;
        for (int j = 0; j < n_walls && !dark; j++) {
            const float4 w = make_float4(walls[4*j], walls[4*j + 1], walls[4*j + 2] - walls[4*j], walls[4*j + 3] - walls[4*j + 1]);
            if (!lg_touches(k, v, w)) continue;
            touched = true;
            dark = lg_shadows(v, w);
        }
        const unsigned st = dark ? 2u : (touched ? 0u : 1u);
        words[i >> 4] |= st << (2*(i & 15));
        if (st == 0u) {
            for (int j = 0; j < n_walls; j++) {
                const float4 w = make_float4(walls[4*j], walls[4*j + 1], walls[4*j + 2] - walls[4*j], walls[4*j + 3] - walls[4*j + 1]);
                if (!lg_touches(k, v, w)) continue;
                if (count < max_candidates) candidates[count] = 0x80000000u | ((unsigned)i << 24) | (unsigned)j;
                count++;
            }
        }
    }
    return count;
}

int ms_host_fold_hits(const float* s, const int* line, int n_hits, const int* order, float* nearest_s, int* nearest_line) {
    // one ray's hits through the three slots the way a wave plays them: windows of 64 in the given order, and within a
    // window in lockstep - every hit's first merge, then the second merges of those that go on, then the third
    unsigned long long best = ~0ull, second = ~0ull, third = ~0ull;
    for (int w0 = 0; w0 < n_hits; w0 += WAVE) {
        const int nw = (n_hits - w0 < WAVE) ? n_hits - w0 : WAVE;
        unsigned long long lose1[WAVE], lose2[WAVE];
        bool on[WAVE];
        for (int k = 0; k < nw; k++) {
            const int h = order[w0 + k];
            const unsigned long long key = hit_key(s[h], line[h]);
            on[k] = hit_loser_matters(key, s[h], slot_min(&best, key), lose1[k]);
        }
        for (int k = 0; k < nw; k++) if (on[k]) {
            const unsigned long long old2 = slot_min(&second, lose1[k]);
            lose2[k] = old2 > lose1[k] ? old2 : lose1[k];
        }
        for (int k = 0; k < nw; k++) if (on[k] && lose2[k] != ~0ull) slot_min(&third, lose2[k]);
    }
    *nearest_s = INFINITY; *nearest_line = -1;
    return hit_resolve(best, second, third, *nearest_s, *nearest_line) ? 1 : 0;
}

float ms_host_wall_reach(const float* agent, float agent_radius) { return wall_reach(p2(agent[0], agent[1]), p2(agent[2], agent[3]), agent_radius); }

int ms_host_wall_beyond_reach(const float* agent, const float* wall, float agent_radius) {
    const float reach = wall_reach(p2(agent[0], agent[1]), p2(agent[2], agent[3]), agent_radius);
    return wall_beyond(make_float4(agent[0], agent[1], agent[2], agent[3]), make_float4(wall[0], wall[1], wall[2], wall[3]),
                       reach_squared(reach)) ? 1 : 0;
}

int ms_host_agents_apart(const float* me, const float* other, float agent_radius) {
    return agents_apart(make_float4(me[0], me[1], me[2], me[3]), make_float4(other[0], other[1], other[2], other[3]), agent_radius) ? 1 : 0;
}

int ms_host_wall_hidden(float x0, float y0, float x1, float y1, const float* o, const float* w, float near_plane) {
    const WgCell k{x0, y0, x1, y1};
    const WgTarget t = wg_target(k, make_float4(w[0], w[1], w[2], w[3]));
    return wg_hides(k, t, make_float4(o[0], o[1], o[2], o[3]), near_plane) ? 1 : 0;
}

void ms_host_wallgrid_cell(const float* walls, int n_walls, float ox, float oy, int nx, int ny, float cell, int c,
                           float near_plane, float reach_lo, float reach, unsigned char* vis, unsigned char* close) {
    const float4* ln = reinterpret_cast<const float4*>(walls);
    const WgCell k = wg_cell_of(make_float4(ox, oy, (float)nx, (float)ny), cell, c);
    for (int t = 0; t < n_walls; t++) {
        const WgTarget tg = wg_target(k, ln[t]);
        bool hidden = false;
        for (int o = 0; o < n_walls && !hidden; o++) hidden = (o != t) && wg_hides(k, tg, ln[o], near_plane);
        vis[t] = hidden ? 0 : 1;
        close[t] = wg_close(k, ln[t], reach) ? (wg_close(k, ln[t], reach_lo) ? 2 : 1) : 0;
    }
}

void ms_host_wall_sectors(float x0, float y0, float x1, float y1, const float* o, int* first, int* count, const float* w, int* sector) {
    const float cx = .5f*(x0 + x1), cy = .5f*(y0 + y1);
    wg_sectors_of(cx, cy, make_float4(o[0], o[1], o[2], o[3]), *first, *count);
    *sector = wg_sector_of(cx, cy, make_float4(w[0], w[1], w[2], w[3]));
}
void ms_host_wall_arc(float x0, float y0, float x1, float y1, const float* w, int* lo8, int* hi8) {
    wg_arc(WgCell{x0, y0, x1, y1}, make_float4(w[0], w[1], w[2], w[3]), *lo8, *hi8);
}
void ms_host_wedge(float right_x, float right_y, float left_x, float left_y, int* wa8, int* wb8) {
    wg_wedge(pseudo_angle(right_x, right_y), pseudo_angle(left_x, left_y), *wa8, *wb8);
}
int ms_host_wedge_meets(float right_x, float right_y, float left_x, float left_y, int lo8, int hi8) {
    int wa8, wb8;
    ms_host_wedge(right_x, right_y, left_x, left_y, &wa8, &wb8);
    return wg_arcs_meet(lo8, hi8, wa8, wb8) ? 1 : 0;
}

static bool wallgrid_ok(const MsScenery* sc) {
    return sc->wg_starts && sc->wg_geom && sc->wg_cell > 0.f && sc->wg_reach_lo >= 0.f && sc->wg_reach >= sc->wg_reach_lo &&
           sc->wg_near > 0.f && ((uintptr_t)sc->wg_geom % 16 == 0);
}

int ms_wallgrid_scan(const MsScenery* sc, const MsWallGridParent* parent, const int* reps, int n_reps, int max_groups,
                     const long long* bits_starts, unsigned* bits, unsigned* counts, void* stream) {
    if (!scenery_ok(sc) || !wallgrid_ok(sc) || !reps || n_reps < 0 || max_groups < 0 || !bits_starts || !bits || !counts) return MS_EINVAL;
    WgParent par{nullptr, nullptr, nullptr, 0.f, nullptr};
    if (parent) {
        if (!parent->cells || !parent->starts || !parent->geom || !parent->pool || !(parent->cell >= sc->wg_cell) ||
            ((uintptr_t)parent->cells % 16) || ((uintptr_t)parent->geom % 16)) return MS_EINVAL;
        par = WgParent{parent->cells, parent->starts, parent->geom, parent->cell, parent->pool};
    }
    if (n_reps == 0 || max_groups == 0) return MS_OK;
    if (n_reps > 65535) return MS_EUNSUPPORTED;
    hipLaunchKernelGGL(wallgrid_scan_kernel, dim3((unsigned)max_groups, (unsigned)n_reps), dim3(WG), 0, (hipStream_t)stream,
                       *sc, par, reps, bits_starts, bits, counts);
    return launch_status();
}

int ms_wallgrid_fill(const MsScenery* sc, const int* reps, int n_reps, int max_cells,
                     const long long* bits_starts, const unsigned* bits, unsigned short* pool, unsigned* vis_entries, float* near_rows,
                     void* stream) {
    if (!scenery_ok(sc) || !wallgrid_ok(sc) || !sc->wg_cells || ((uintptr_t)sc->wg_cells % 16) || !reps || n_reps < 0 || max_cells < 0 ||
        !bits_starts || !bits || ((vis_entries != nullptr) != (near_rows != nullptr)) || (!pool && !vis_entries) || (vis_entries && !sc->wg_pool_base) ||
        ((uintptr_t)near_rows % 16) || ((uintptr_t)vis_entries % 4)) return MS_EINVAL;
    if (n_reps == 0 || max_cells == 0) return MS_OK;
    const long long blocks = (2LL*max_cells + WAVES - 1)/WAVES;
    if (blocks > 0x7fffffffLL || n_reps > 65535) return MS_EUNSUPPORTED;
    hipLaunchKernelGGL(wallgrid_fill_kernel, dim3((unsigned)blocks, (unsigned)n_reps), dim3(WG), 0, (hipStream_t)stream,
                       *sc, reps, bits_starts, bits, pool, reinterpret_cast<float4*>(near_rows), vis_entries);
    return launch_status();
}

int ms_step_physics(const MsScenery* sc, const MsAgents* ag, const MsMovement* mv, const MsStepExtras* ex, float* progress,
                    const MsConfig* cfg, void* stream) {
    if (!scenery_ok(sc) || !agents_ok(ag) || !progress || !config_ok(cfg)) return MS_EINVAL;
    if (!step_options_ok(mv, ex) || ((uintptr_t)ag->schedule % 4)) return MS_EINVAL;
    if (sc->wg_cells && (!sc->wg_starts || !sc->wg_geom || !sc->wg_near_rows || !(sc->wg_cell > 0.f) || ((uintptr_t)sc->wg_cells % 16) ||
                         ((uintptr_t)sc->wg_geom % 16) || ((uintptr_t)sc->wg_near_rows % 16))) return MS_EINVAL;
    const int pack = physics_pack_of(sc->n_envs, sc->n_agents, sc->wg_cells != nullptr, g_physics_pack);
    // per wave: 2 float4 + a float + an unsigned per agent, rounded up to whole float4s
    const size_t slice = ((sizeof(float)*8 + sizeof(float) + sizeof(unsigned))*(size_t)sc->n_agents*pack + 15)/16;
    if (slice*16 > 56*1024) return MS_EUNSUPPORTED;
    MsMovement mvv; MsStepExtras exv;
    step_options_of(mv, ex, mvv, exv);
    MsScenery scn = *sc;
    if (!sc->wg_cells) { scn.wg_geom = sc->lines_vals; scn.wg_starts = sc->lines_starts; }   // (rows the kernel may read: see there)
    const hipStream_t hs = (hipStream_t)stream;
    const Divisor by_a = divisor_of((unsigned)sc->n_agents);
    const AgentsK agk = agents_k(*ag);
    // the fan schedule's sort waves, in front of the launch's own (physics.h): last frame's render costs into this frame's order
    FanSort fs{nullptr, 0, 1, 0};
    if (schedule_serves(ag, sc, cfg->res)) {
        fs.schedule = ag->schedule; fs.n_fans = sc->n_envs*sc->n_agents;
        fs.per_run = fan_sort_per_run(fs.n_fans); fs.n_blocks = 8*fs.per_run;
    }
    // one wavefront per env (several envs per wave, one AFTER the other: 2 -> +25 %, 4 -> +85 % at 4096 envs; side by side: PACK)
#define MS_LAUNCH_PHYSICS_P(M, E, P) \
    hipLaunchKernelGGL((physics_kernel<M, E, P>), dim3(fs.n_blocks + (sc->n_envs + pack - 1)/pack), dim3(WAVE), slice*16, hs, scn, agk, progress, cfg->agent_radius, cfg->fps, mvv, exv, pack, by_a, fs)
#define MS_LAUNCH_PHYSICS(M, E) { if (pack > 1) MS_LAUNCH_PHYSICS_P(M, E, 1); else MS_LAUNCH_PHYSICS_P(M, E, 0); }
    if (mv && ex) MS_LAUNCH_PHYSICS(1, 1)
    else if (ex) MS_LAUNCH_PHYSICS(0, 1)
    else if (mv) MS_LAUNCH_PHYSICS(1, 0)
    else MS_LAUNCH_PHYSICS(0, 0)
#undef MS_LAUNCH_PHYSICS_P
#undef MS_LAUNCH_PHYSICS
    return launch_status();
}

int ms_move_physics(const MsScenery* sc, const MsAgents* ag, const MsMovement* mv, float* progress, const MsConfig* cfg,
                    void* stream) {
    return ms_step_physics(sc, ag, mv, nullptr, progress, cfg, stream);
}

int ms_physics(const MsScenery* sc, const MsAgents* ag, float* progress, const MsConfig* cfg, void* stream) {
    return ms_step_physics(sc, ag, nullptr, nullptr, progress, cfg, stream);
}

void ms_host_move_velocity(float keep, float ang, const float* delta, float* v, float* w) {
    float2 vv = make_float2(v[0], v[1]);
    move_velocity(keep, ang, delta[0], delta[1], delta[2], vv, *w);
    v[0] = vv.x; v[1] = vv.y;
}

// what ms_slide_physics and ms_host_slide refuse alike of an MsSlide and the shape it is for
static int slide_status(const MsSlide* sl, const int n_agents) {
    if (!sl || !(sl->bounce >= 0.f && sl->bounce <= 1.f)) return MS_EINVAL;
    if (n_agents > WAVE) return MS_EUNSUPPORTED;                         // (a lane an agent)
    return MS_OK;
}

int ms_slide_physics(const MsScenery* sc, const MsAgents* ag, const MsMovement* mv, const MsStepExtras* ex, const MsSlide* sl,
                     float* progress, const MsConfig* cfg, void* stream) {
    if (!scenery_ok(sc) || !agents_ok(ag) || !progress || !config_ok(cfg)) return MS_EINVAL;
    if (!step_options_ok(mv, ex) || ((uintptr_t)ag->schedule % 4)) return MS_EINVAL;
    if (sc->wg_cells && (!sc->wg_starts || !sc->wg_geom || !sc->wg_near_rows || !(sc->wg_cell > 0.f) || ((uintptr_t)sc->wg_cells % 16) ||
                         ((uintptr_t)sc->wg_geom % 16) || ((uintptr_t)sc->wg_near_rows % 16))) return MS_EINVAL;
    if (((uintptr_t)ag->positions % 8) || ((uintptr_t)ag->velocity % 8) || ((uintptr_t)ag->headings % 16)) return MS_EINVAL;
    if (const int st = slide_status(sl, sc->n_agents)) return st;
    g_last_step_fused = 0;                                               // (a sliding step is never the one-launch step)
    MsMovement mvv; MsStepExtras exv;
    step_options_of(mv, ex, mvv, exv);
    const hipStream_t hs = (hipStream_t)stream;
    // the fan schedule's sort waves, in front of the launch's own, as ms_step_physics'
    FanSort fs{nullptr, 0, 1, 0};
    if (schedule_serves(ag, sc, cfg->res)) {
        fs.schedule = ag->schedule; fs.n_fans = sc->n_envs*sc->n_agents;
        fs.per_run = fan_sort_per_run(fs.n_fans); fs.n_blocks = 8*fs.per_run;
    }
#define MS_LAUNCH_SLIDE(M, E) \
    hipLaunchKernelGGL((physics_slide_kernel<M, E>), dim3(fs.n_blocks + sc->n_envs), dim3(WAVE), 0, hs, *sc, agents_k(*ag), progress, cfg->agent_radius, cfg->fps, mvv, exv, *sl, divisor_of((unsigned)sc->n_agents), fs)
    if (mv && ex) MS_LAUNCH_SLIDE(1, 1);
    else if (ex) MS_LAUNCH_SLIDE(0, 1);
    else if (mv) MS_LAUNCH_SLIDE(1, 0);
    else MS_LAUNCH_SLIDE(0, 0);
#undef MS_LAUNCH_SLIDE
    return launch_status();
}

int ms_host_slide(const float* walls, const long long* wall_starts, int n_envs, int n_agents, const MsAgents* ag, const MsMovement* mv,
                  const MsStepExtras* ex, const MsSlide* sl, float* progress, const MsConfig* cfg) {
    if (!walls || !wall_starts || n_envs < 1 || n_agents < 1 || !agents_ok(ag) || !progress || !config_ok(cfg)) return MS_EINVAL;
    if (!step_options_ok(mv, ex)) return MS_EINVAL;
    if (const int st = slide_status(sl, n_agents)) return st;
    MsMovement mvv; MsStepExtras exv;
    step_options_of(mv, ex, mvv, exv);
    slide_serial(walls, wall_starts, n_envs, n_agents, *ag, mv ? &mvv : nullptr, exv, ex != nullptr, *sl, progress, cfg->agent_radius, cfg->fps);
    return MS_OK;
}

// what ms_rollouts and ms_host_rollouts refuse alike: the limits and the pointers of an MsRollouts
static int rollouts_status(const MsRollouts* r) {
    if (!r || r->n_candidates < 1 || r->n_candidates > 256 || r->horizon < 1 || r->horizon > 64 || r->n_actions < 1 ||
        (r->others != 0 && r->others != 1) || !(r->keep == r->keep) || !r->actions || !r->table || !r->positions || !r->angles ||
        !r->velocity || !r->angvelocity || !r->progress || !r->stops || !r->first_stop) return MS_EINVAL;
    if ((r->slide != 0 && r->slide != 1) || (r->slide && !(r->bounce >= 0.f && r->bounce <= 1.f))) return MS_EINVAL;
    return MS_OK;
}

int ms_rollouts(const MsScenery* sc, const MsAgents* ag, const MsRollouts* r, const MsConfig* cfg, void* stream) {
    if (!scenery_ok(sc) || !agents_ok(ag) || !config_ok(cfg) || rollouts_status(r) != MS_OK) return MS_EINVAL;
    if (((uintptr_t)r->actions % 8) || ((uintptr_t)r->positions % 8) || ((uintptr_t)r->velocity % 8) || ((uintptr_t)r->trail % 8) || ((uintptr_t)r->slides % 4) ||
        ((uintptr_t)ag->positions % 8) || ((uintptr_t)ag->velocity % 8)) return MS_EINVAL;
    if (sc->wg_cells && (!sc->wg_starts || !sc->wg_geom || !sc->wg_near_rows || !(sc->wg_cell > 0.f) || ((uintptr_t)sc->wg_cells % 16) ||
                         ((uintptr_t)sc->wg_geom % 16) || ((uintptr_t)sc->wg_near_rows % 16))) return MS_EINVAL;
    const int groups = (r->n_candidates + WAVE - 1)/WAVE;
    const long long blocks = (long long)sc->n_envs*sc->n_agents*groups;
    if (blocks > 0x7fffffffLL) return MS_EUNSUPPORTED;
    // Which scheme: a lane a candidate pays a wall's whole exact test however few of its lanes are candidates - measured (DESIGN
    // 3.27; 4096 envs, H = 8) 117.7 us at K = 7 against 51.9 us for a lane a wall, 151.6 against 124.9 at 24, 153.4 against 163.1 at
    // 32, 164.3 against 301.2 at 64: few candidates go candidate by candidate, a wave's worth and more a lane each.
    // (The sliding step is stated for a lane a candidate only: pinning the other scheme with it is refused, not ignored.)
    if (r->slide && g_rollout_scheme == 1) return MS_EINVAL;
    const int scheme = r->slide ? 0 : g_rollout_scheme >= 0 ? g_rollout_scheme : (r->n_candidates <= ROLL_FEW ? 1 : 0);
    if (r->slide)
        hipLaunchKernelGGL(rollout_kernel<1>, dim3((unsigned)blocks), dim3(WAVE), 0, (hipStream_t)stream, *sc, agents_k(*ag), *r,
                           cfg->agent_radius, cfg->fps, groups, divisor_of((unsigned)groups), divisor_of((unsigned)sc->n_agents));
    else if (scheme == 1)
        hipLaunchKernelGGL(rollout_walls_kernel, dim3((unsigned)blocks), dim3(WAVE), 0, (hipStream_t)stream, *sc, agents_k(*ag), *r,
                           cfg->agent_radius, cfg->fps, groups, divisor_of((unsigned)groups), divisor_of((unsigned)sc->n_agents));
    else
        hipLaunchKernelGGL(rollout_kernel<0>, dim3((unsigned)blocks), dim3(WAVE), 0, (hipStream_t)stream, *sc, agents_k(*ag), *r,
                           cfg->agent_radius, cfg->fps, groups, divisor_of((unsigned)groups), divisor_of((unsigned)sc->n_agents));
    return launch_status();
}

int ms_debug_rollout_scheme(int scheme) {
    if (scheme < -1 || scheme > 1) return MS_EINVAL;
    g_rollout_scheme = scheme;
    return MS_OK;
}

int ms_host_rollouts(const float* walls, int n_walls, const MsAgents* ag, int n_agents, const MsRollouts* r, const MsConfig* cfg) {
    if (!agents_ok(ag) || !config_ok(cfg) || rollouts_status(r) != MS_OK || n_agents < 1 || n_walls < 0 || (n_walls > 0 && !walls)) return MS_EINVAL;
    rollout_serial(walls, n_walls, *ag, n_agents, *r, cfg->agent_radius, cfg->fps);
    return MS_OK;
}

// what ms_scenarios and ms_host_scenarios refuse alike: the limits and the pointers of an MsScenarios, and the agents an env
static int scenarios_status(const MsScenarios* q, const int n_agents) {
    if (!q || q->n_scenarios < 1 || q->n_scenarios > 256 || q->horizon < 1 || q->horizon > 64 || q->n_actions < 1 ||
        (q->focal != 0 && q->focal != 1) || (q->shared != 0 && q->shared != 1) || !(q->keep == q->keep) || !q->actions ||
        (q->focal && !q->base) || !q->table || !q->positions || !q->angles || !q->velocity || !q->angvelocity || !q->progress ||
        !q->stops || !q->first_stop || n_agents < 1) return MS_EINVAL;
    if (n_agents > WAVE) return MS_EUNSUPPORTED;                         // (a lane an agent, as ms_slide_physics)
    return MS_OK;
}

int ms_scenarios(const MsScenery* sc, const MsAgents* ag, const MsScenarios* q, const MsConfig* cfg, void* stream) {
    if (!scenery_ok(sc) || !agents_ok(ag) || !config_ok(cfg)) return MS_EINVAL;
    if (const int st = scenarios_status(q, sc->n_agents)) return st;
    if (((uintptr_t)q->actions % 8) || ((uintptr_t)q->base % 8) || ((uintptr_t)q->table % 4) || ((uintptr_t)q->positions % 8) ||
        ((uintptr_t)q->velocity % 8) || ((uintptr_t)q->trail % 8) || ((uintptr_t)q->angles % 4) || ((uintptr_t)q->angvelocity % 4) ||
        ((uintptr_t)q->progress % 4) || ((uintptr_t)q->stops % 4) || ((uintptr_t)q->first_stop % 4) ||
        ((uintptr_t)ag->positions % 8) || ((uintptr_t)ag->velocity % 8)) return MS_EINVAL;
    if (sc->wg_cells && (!sc->wg_starts || !sc->wg_geom || !sc->wg_near_rows || !(sc->wg_cell > 0.f) || ((uintptr_t)sc->wg_cells % 16) ||
                         ((uintptr_t)sc->wg_geom % 16) || ((uintptr_t)sc->wg_near_rows % 16))) return MS_EINVAL;
    const int G = WAVE/sc->n_agents;                                     // whole scenarios a wave
    const int S = scenario_count(*q, sc->n_agents);
    const int groups = (S + G - 1)/G;
    const long long blocks = (long long)sc->n_envs*groups;
    if (blocks > 0x7fffffffLL) return MS_EUNSUPPORTED;
    hipLaunchKernelGGL(scenario_kernel, dim3((unsigned)blocks), dim3(WAVE), 0, (hipStream_t)stream, *sc, agents_k(*ag), *q,
                       cfg->agent_radius, cfg->fps, groups, G, divisor_of((unsigned)groups), divisor_of((unsigned)sc->n_agents));
    return launch_status();
}

int ms_host_scenarios(const float* walls, int n_walls, const MsAgents* ag, int n_agents, const MsScenarios* q, const MsConfig* cfg) {
    if (!agents_ok(ag) || !config_ok(cfg) || n_walls < 0 || (n_walls > 0 && !walls)) return MS_EINVAL;
    if (const int st = scenarios_status(q, n_agents)) return st;
    scenario_serial(walls, n_walls, *ag, n_agents, *q, cfg->agent_radius, cfg->fps);
    return MS_OK;
}

// The render call, decided in full before anything is launched: render_prepare makes every check and choice, render_enqueue
// launches what they came to.  A call refused has enqueued nothing; and given `progress` (ms_move_step_render's step),
// render_prepare tells whether the step is one launch (L.fused) - if not, L is the plain render that follows ms_step_physics.
struct RenderLaunch {
    RenderPlan plan;                                  // render_kernel's NG and blocks
    RenderConstsStep rc;                              // (the STEP = 1 part is set only where the step is fused)
    int* schedule;                                    // the fan schedule, where the launch follows it (else NULL): RenderConstsOrder's
    MsScenery scn; AgentsK agn; MsRender outn;        // the copies render_kernel gets
    const MsAgents* ag; const MsRender* out;          // the caller's, as render_prep_kernel and dynlight_kernel get them
    float agent_radius, half_screen; int R;
    bool colour, obs, no_planes;                      // which instantiation of render_kernel
    bool light_grid, walls_listed;
    bool prep;        // headings from render_prep_kernel (else from the cache, from render_kernel itself, or from the fused wave)
    bool dynlight;    // dynlight_kernel afterwards: it lights the rays that landed on an agent
    bool fused;       // the physics step in the render's waves (render_kernel<..., STEP = 1>)
};

static int render_prepare(const MsScenery* sc, const MsAgents* ag, const MsRender* out, const MsConfig* cfg, float* progress,
                          const MsMovement* mv, const MsStepExtras* ex, RenderLaunch& L) {
    if (!scenery_ok(sc) || !agents_ok(ag) || !config_ok(cfg) || !out || !sc->textures_vals || !sc->textures_widths ||
        !sc->textures_starts || !sc->baked_vals || !sc->lights_widths || !sc->lights_starts) return MS_EINVAL;
    if ((out->seen_stamp != nullptr) != (out->seen_epoch != nullptr) || (out->seen_stamp != nullptr) != (out->seen_count != nullptr)) return MS_EINVAL;
    if (out->obs_rgb || out->obs_depth || out->obs_centre) {
        const int sub = out->obs_subsample;
        if (sub < 1 || (sub & (sub - 1)) || sub > WAVE || cfg->res % sub) return MS_EINVAL;
        if (out->obs_depth && !(out->obs_max_depth > 0.f)) return MS_EINVAL;
        if (out->obs_centre && cfg->res/sub < 2) return MS_EINVAL;
    }
    if (sc->n_lights_total > 0 && !sc->lights_vals) return MS_EINVAL;
    const int R = cfg->res;
    L.R = R; L.agent_radius = cfg->agent_radius; L.ag = ag; L.out = out;
    L.light_grid = light_grid_in(sc);
    L.colour = out->screen || out->obs_rgb;                              // else: render_kernel<1,0>, which has no pass 3
    // Without a light grid the rays that land on an agent are lit by dynlight_kernel, which takes them by groups of 64.  With
    // one agent per env no ray can land on an agent line (own lines sit inside the near plane), so there is nothing to light.
    L.dynlight = !L.light_grid && sc->n_agents > 1 && L.colour;
    L.plan = render_plan(sc->n_envs, sc->n_agents, R, wave_slots_here(), L.dynlight ? 1 : g_ray_groups, g_tail_rounds, g_tail_envs, L.rc);
    // the workspace's layout (MS_RENDER_WORKSPACE_INTS): 16 counters, a queue of one entry per (env, agent, 64 rays), the headings
    const long long ws_queue = (long long)sc->n_envs*sc->n_agents*((R + WAVE - 1)/WAVE);
    if (L.plan.n_blocks > 0x7fffffffLL || ws_queue > 0x7fffff00LL) return MS_EUNSUPPORTED;
    L.rc.ws_headings = 16 + (int)((ws_queue + 1) & ~1LL);
    const float half_screen = L.half_screen = half_screen_of(cfg->fov);
    // the light grid is all or nothing (light_grid_in) ...
    L.scn = *sc;
    if (!L.light_grid) L.scn.lg_vals = nullptr;
    // ... and so is the wall grid: its vis lists were built for near planes below wg_near and ray direction vectors no
    // longer than sqrt(WG_MAX_RU2) (wallgrid_scan_kernel); a call outside that meets every wall instead
    L.walls_listed = vis_lists_serve(sc, cfg->agent_radius) && 1.f + half_screen*half_screen <= WG_MAX_RU2;
    if (L.walls_listed && (((uintptr_t)sc->wg_cells % 16) || ((uintptr_t)sc->wg_geom % 16))) return MS_EINVAL;
    if (!L.walls_listed) {                                               // (the kernel reads a row of each whatever happens: see there)
        L.scn.wg_cells = nullptr;
        L.scn.wg_geom = sc->lines_vals;                                  // at least 16 bytes per env: every env has its agents' lines
        L.scn.wg_starts = sc->lines_starts;
        L.scn.wg_pool_base = reinterpret_cast<const long long*>(sc->lines_vals);   // (16 bytes of lines per env at least: 8 are there)
    }
    // dynlight_kernel reads the per-ray outputs back and patches `screen`: only the one-kernel path can do without some of them
    const bool all_planes = out->indices && out->locations && out->dots && out->distances && out->screen;
    const bool pooled = out->obs_rgb || out->obs_depth || out->obs_centre || out->seen_stamp;
    if (L.dynlight && (!all_planes || pooled)) return MS_EUNSUPPORTED;
    if (!pooled && !out->indices && !out->locations && !out->dots && !out->distances && !out->screen) return MS_EINVAL;
    L.obs = pooled || !all_planes;
    // (colour, and not one per-ray plane wanted - the demo envs' request: the instantiation that has no plane stores in it)
    L.no_planes = L.colour && !out->indices && !out->locations && !out->dots && !out->distances && !out->screen;
    // The fused step: one agent per env and at most 64 rays - the agent is ONE wave, which runs the env's physics first and
    // renders from the pose it ends on; and a wall grid that serves both halves of the step or neither (ms_render goes without
    // it when the call's near plane or field of view is outside what its vis lists were built for, ms_step_physics never does).
    const bool physics_listed = sc->wg_cells != nullptr;
    L.fused = progress && sc->n_agents == 1 && R <= WAVE && L.plan.ng == 1 && physics_listed == L.walls_listed &&
              (!physics_listed || (sc->wg_near_rows && (uintptr_t)sc->wg_near_rows % 16 == 0));
    // Headings: from ms_physics' cache when the agents carry one and a single kernel does the whole job (then the workspace is
    // not needed at all); the fused wave works them out itself (and leaves them in the cache, if there is one); otherwise
    // render_prep_kernel, which also resets the workspace's counters - or, without a workspace, render_kernel - works them out.
    const bool cached = ag->headings && !L.dynlight;
    L.prep = !cached && !L.fused && out->workspace;
    if ((cached && (uintptr_t)ag->headings % 16) || (L.prep && (uintptr_t)out->workspace % 8)) return MS_EINVAL;
    L.agn = agents_k(*ag);
    L.outn = *out;
    // the fan schedule: every agent one fan, one launch of one-group waves behind a physics launch of its own
    L.schedule = (schedule_serves(ag, sc, R) && L.plan.ng == 1 && !L.fused) ? ag->schedule : nullptr;
    if (L.schedule && (uintptr_t)L.schedule % 4) return MS_EINVAL;
    if (!cached && !L.fused) L.agn.headings = nullptr;
    if (!L.prep) L.outn.workspace = nullptr;
    if (out->obs_depth) L.outn.obs_max_depth = 1.f/out->obs_max_depth;  // (the kernel multiplies: see the pooled depth in render.h)
    L.rc.x_clip = 0.5f*cfg->agent_radius/sqrtf(1.f + half_screen*half_screen);
    L.rc.c_b = 0.5f*(float)R/half_screen;
    L.rc.by_m = divisor_of((unsigned)sc->n_model);
    L.rc.skip_own = (sc->model_radius > 0.f && sc->model_radius*1.01f < cfg->agent_radius) ? 1 : 0;
    L.rc.inv_res = camera_inv_res(R, half_screen);
    L.rc.telemetry = g_pair_telemetry;
    // (the instantiations with optional outputs - every colourless one, and the colour one of pooled observations at one ray
    // group a wave - read which are wanted from here: see OUT_* in render.h)
    if (!L.colour || (L.obs && L.plan.ng == 1))
        L.outn.obs_subsample = (out->obs_subsample & 0xff) | (((out->indices ? OUT_INDICES : 0) | (out->locations ? OUT_LOCATIONS : 0) |
                                (out->dots ? OUT_DOTS : 0) | (out->distances ? OUT_DISTANCES : 0) | (out->obs_depth ? OUT_DEPTH : 0) |
                                (out->obs_centre ? OUT_CENTRE : 0) | (out->seen_stamp ? OUT_SEEN : 0) | (out->screen ? OUT_SCREEN : 0) |
                                (out->obs_rgb ? OUT_RGB : 0)) << 8);
    if (L.fused) {
        L.rc.progress = progress; L.rc.fps = cfg->fps; L.rc.wg_cells_physics = sc->wg_cells;
        step_options_of(mv, ex, L.rc.mv, L.rc.ex);
    }
    return MS_OK;
}

static int render_enqueue(const RenderLaunch& L, const hipStream_t hs) {
    g_last_render_groups = L.plan.ng;
    const int na = L.scn.n_envs*L.scn.n_agents;
    if (L.prep) hipLaunchKernelGGL(render_prep_kernel, dim3((na + WG - 1)/WG), dim3(WG), 0, hs, agents_k(*L.ag), L.out->workspace, na, L.rc.ws_headings);
    // (the STEP = 0 instantiations take the RenderConsts part of L.rc - those of one ray group a wave with the schedule behind it)
    RenderConstsOrder rco;
    static_cast<RenderConsts&>(rco) = L.rc; rco.schedule = L.schedule;
#define MS_LAUNCH_RENDER(O, S, NG_, STEP_) hipLaunchKernelGGL((render_kernel<O, S, NG_, STEP_>), dim3((int)L.plan.n_blocks), dim3(WAVE), 0, hs, \
                                                              L.scn, L.agn, L.outn, L.agent_radius, L.half_screen, L.R, (int)L.plan.n_blocks, L.rc)
#define MS_LAUNCH_RENDER_OS(NG_) { if (!L.colour) MS_LAUNCH_RENDER(1, 0, NG_, 0); else if (L.no_planes) MS_LAUNCH_RENDER(2, 1, NG_, 0); \
                                   else if (L.obs) MS_LAUNCH_RENDER(1, 1, NG_, 0); else MS_LAUNCH_RENDER(0, 1, NG_, 0); }
    if (L.fused) { if (!L.colour) MS_LAUNCH_RENDER(1, 0, 1, 1); else if (L.obs) MS_LAUNCH_RENDER(1, 1, 1, 1); else MS_LAUNCH_RENDER(0, 1, 1, 1); }
    else if (L.plan.ng == 4) MS_LAUNCH_RENDER_OS(4)
    else if (L.plan.ng == 2) MS_LAUNCH_RENDER_OS(2)
    else {
#define MS_LAUNCH_RENDER_1(O, S) hipLaunchKernelGGL((render_kernel<O, S, 1, 0>), dim3((int)L.plan.n_blocks), dim3(WAVE), 0, hs, \
                                                    L.scn, L.agn, L.outn, L.agent_radius, L.half_screen, L.R, (int)L.plan.n_blocks, rco)
        if (!L.colour) MS_LAUNCH_RENDER_1(1, 0); else if (L.no_planes) MS_LAUNCH_RENDER_1(2, 1);
        else if (L.obs) MS_LAUNCH_RENDER_1(1, 1); else MS_LAUNCH_RENDER_1(0, 1);
#undef MS_LAUNCH_RENDER_1
    }
#undef MS_LAUNCH_RENDER_OS
#undef MS_LAUNCH_RENDER
    if (L.dynlight) hipLaunchKernelGGL(dynlight_kernel, dim3((int)L.plan.n_blocks), dim3(WG), 0, hs, L.scn, agents_k(*L.ag), *L.out, L.R);
    return launch_status();
}

int ms_deathmatch_shoot(int n_envs, int n_agents, const MsDeathmatch* dm, void* stream) {
    if (n_envs <= 0 || n_agents <= 0 || !dm || !dm->centre || !dm->positions || !dm->upper || !dm->health || !dm->damage || !dm->dead ||
        ((uintptr_t)dm->centre % 8) || ((uintptr_t)dm->positions % 8) || ((uintptr_t)dm->upper % 8) ||
        !(dm->clearance == dm->clearance) || !(dm->hit_damage == dm->hit_damage) || !(dm->tick_damage == dm->tick_damage)) return MS_EINVAL;
    const long long rows = (long long)n_envs*n_agents, blocks = (rows + WG - 1)/WG;
    if (blocks > 0x7fffffffLL) return MS_EUNSUPPORTED;
    hipLaunchKernelGGL(deathmatch_kernel, dim3((unsigned)blocks), dim3(WG), 0, (hipStream_t)stream, *dm, n_envs, n_agents);
    return launch_status();
}

int ms_explorer_books(int n_envs, const MsExplorer* ex, void* stream) {
    if (n_envs <= 0 || !ex || !ex->tally || !ex->before || !ex->lengths || !ex->epoch || !ex->over || !ex->reward || ex->pixels <= 0 ||
        ((uintptr_t)ex->tally % 4) || ((uintptr_t)ex->before % 4) || ((uintptr_t)ex->lengths % 4) || ((uintptr_t)ex->epoch % 4)) return MS_EINVAL;
    hipLaunchKernelGGL(explorer_kernel, dim3((unsigned)((n_envs + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, *ex, n_envs);
    return launch_status();
}

int ms_render(const MsScenery* sc, const MsAgents* ag, const MsRender* out, const MsConfig* cfg, void* stream) {
    RenderLaunch L;
    const int planned = render_prepare(sc, ag, out, cfg, nullptr, nullptr, nullptr, L);
    return planned != MS_OK ? planned : render_enqueue(L, (hipStream_t)stream);
}

int ms_move_step_render(const MsScenery* sc, const MsAgents* ag, const MsMovement* mv, const MsStepExtras* ex, float* progress,
                        const MsRender* out, const MsConfig* cfg, void* stream) {
    if (!progress || !step_options_ok(mv, ex)) return MS_EINVAL;
    RenderLaunch L;
    const int planned = render_prepare(sc, ag, out, cfg, progress, mv, ex, L);
    g_last_step_fused = 0;
    if (planned != MS_OK) return planned;
    const int p = L.fused ? MS_OK : ms_step_physics(sc, ag, mv, ex, progress, cfg, stream);
    const int r = p != MS_OK ? p : render_enqueue(L, (hipStream_t)stream);
    g_last_step_fused = L.fused && r == MS_OK;
    return r;
}
int ms_step_render(const MsScenery* sc, const MsAgents* ag, float* progress, const MsRender* out, const MsConfig* cfg, void* stream) {
    return ms_move_step_render(sc, ag, nullptr, nullptr, progress, out, cfg, stream);
}
int ms_debug_last_step_fused(void) { return g_last_step_fused; }

// Ray queries (raycast.h): arguments checked in full before anything is launched.
int ms_raycast(const MsScenery* sc, const MsAgents* ag, const MsRaycast* rq, const MsConfig* cfg, void* stream) {
    (void)cfg;
    if (!scenery_ok(sc) || !rq || rq->n_rays < 1 || !rq->origins || !rq->dirs || !(rq->near_plane >= 0.f) ||
        ((uintptr_t)rq->origins % 8) || ((uintptr_t)rq->dirs % 8)) return MS_EINVAL;
    if (ag && (!ag->angles || !ag->positions || ((uintptr_t)ag->positions % 8))) return MS_EINVAL;
    const long long total = (long long)sc->n_envs*rq->n_rays;
    if (total > 0x7fffff00LL) return MS_EUNSUPPORTED;
    const bool gridded = vis_lists_serve(sc, rq->near_plane);
    if (gridded && (((uintptr_t)sc->wg_cells % 16) || ((uintptr_t)sc->wg_geom % 16))) return MS_EINVAL;
    const unsigned blocks = (unsigned)((total + WG - 1)/WG);
    hipLaunchKernelGGL(raycast_kernel, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, *sc, agents_or_none(ag), *rq, ag ? 1 : 0,
                       gridded ? 1 : 0, (int)total);
    return launch_status();
}

int ms_camera_rays(const MsAgents* ag, int n_envs, int n_agents, const MsConfig* cfg, float* dirs, void* stream) {
    if (!ag || !ag->angles || n_envs < 1 || n_agents < 1 || !config_ok(cfg) || !dirs || ((uintptr_t)dirs % 8)) return MS_EINVAL;
    const long long total = (long long)n_envs*n_agents*cfg->res;
    if ((long long)n_envs*n_agents > 0x7fffffffLL || total > 0x7fffff00LL*(long long)WG) return MS_EUNSUPPORTED;
    const float half_screen = half_screen_of(cfg->fov);
    hipLaunchKernelGGL(camera_rays_kernel, dim3((unsigned)((total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, ag->angles,
                       n_envs*n_agents, cfg->res, half_screen, camera_inv_res(cfg->res, half_screen), reinterpret_cast<float2*>(dirs));
    return launch_status();
}

// Shading of given rays (shade.h): arguments checked in full before anything is launched.  What both ms_shade and ms_host_shade
// refuse: a scenery without textures or baked light, lights announced but not given, a query that lacks a plane, R < 1, agents
// without poses.
static int shade_status(const MsScenery* sc, const MsAgents* ag, const MsShade* q) {
    if (!scenery_ok(sc) || !q || q->n_rays < 1 || !q->indices || !q->locations || !q->dots || !q->screen || !sc->textures_vals ||
        !sc->textures_widths || !sc->textures_starts || !sc->baked_vals || !sc->lights_widths || !sc->lights_starts ||
        (sc->n_lights_total > 0 && !sc->lights_vals) || ((uintptr_t)q->indices % 4) || ((uintptr_t)q->locations % 4) ||
        ((uintptr_t)q->dots % 4) || ((uintptr_t)q->screen % 4)) return MS_EINVAL;
    if (ag && (!ag->angles || !ag->positions || ((uintptr_t)ag->positions % 8))) return MS_EINVAL;
    if ((long long)sc->n_envs*q->n_rays > 0x7fffff00LL/3) return MS_EUNSUPPORTED;
    return MS_OK;
}
int ms_shade(const MsScenery* sc, const MsAgents* ag, const MsShade* q, const MsConfig* cfg, void* stream) {
    (void)cfg;
    if (const int status = shade_status(sc, ag, q); status != MS_OK) return status;
    // a light grid is used whole or refused: verdict rows are read 16 bytes at a time, list headers 8, the candidates' rows 16
    const bool gridded = sc->lg_vals != nullptr;
    if (gridded && (!light_grid_in(sc) || ((uintptr_t)sc->lg_vals % 16) || ((uintptr_t)sc->lg_geom % 16) || ((uintptr_t)sc->lg_list % 8) ||
                    ((uintptr_t)sc->lg_pool_rows % 16) || (sc->lg_list && !sc->lg_pool))) return MS_EINVAL;
    const long long total = (long long)sc->n_envs*q->n_rays;
    hipLaunchKernelGGL(shade_kernel, dim3((unsigned)((total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, *sc, agents_or_none(ag), *q,
                       ag ? 1 : 0, gridded ? 1 : 0, divisor_of((unsigned)sc->n_model), (int)total);
    return launch_status();
}
int ms_host_shade(const MsScenery* sc, const MsAgents* ag, const MsShade* q) {
    if (const int status = shade_status(sc, ag, q); status != MS_OK) return status;
    shade_serial(*sc, ag, *q);
    return MS_OK;
}

int ms_camera_pose_rays(const MsCameraPoses* cams, void* stream) {
    if (!cams || cams->n_envs < 1 || cams->n_cameras < 1 || cams->res < 1 || !cams->poses || !cams->origins || !cams->dirs ||
        ((uintptr_t)cams->poses % 4) || ((uintptr_t)cams->origins % 8) || ((uintptr_t)cams->dirs % 8) || !(cams->fov > 0.f)) return MS_EINVAL;
    if (cams->projection == MS_CAMERA_PLANE ? !(cams->fov < 180.f) : (cams->projection != MS_CAMERA_RING || !(cams->fov <= 360.f))) return MS_EINVAL;
    const long long total = (long long)cams->n_envs*cams->n_cameras*cams->res;
    if (total > 0x7fffff00LL) return MS_EUNSUPPORTED;
    const bool plane = cams->projection == MS_CAMERA_PLANE;
    const float half_screen = plane ? half_screen_of(cams->fov) : 0.f;
    hipLaunchKernelGGL(camera_pose_rays_kernel, dim3((unsigned)((total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, *cams, half_screen,
                       plane ? camera_inv_res(cams->res, half_screen) : 0.f, total);
    return launch_status();
}

// Top-down pictures (overhead.h): arguments checked in full before anything is launched; the env ids are the kernel's to check.
int ms_overhead(const MsScenery* sc, const MsAgents* ag, const MsOverhead* ov, void* stream) {
    if (!scenery_ok(sc) || !ov || ov->n_images < 1 || ov->n_views < 1 || ov->height < 1 || ov->width < 1 || !ov->views ||
        (!ov->rgb && !ov->indices) || !(ov->half_width >= 0.f) || !(ov->half_width < INFINITY)) return MS_EINVAL;
    if (ov->rgb && (!sc->textures_vals || !sc->textures_widths || !sc->textures_starts || (ov->lit && !sc->baked_vals))) return MS_EINVAL;
    if (ag && (!ag->angles || !ag->positions || ((uintptr_t)ag->positions % 8))) return MS_EINVAL;
    if (ov->height > (1 << 15) || ov->width > (1 << 15)) return MS_EUNSUPPORTED;
    OvArgs a;
    a.envs = ov->envs; a.views = ov->views; a.rgb = ov->rgb; a.indices = ov->indices;
    a.n_views = ov->n_views; a.height = ov->height; a.width = ov->width;
    a.tiles_x = (ov->width + OV_TILE - 1)/OV_TILE; a.tiles_y = (ov->height + OV_TILE - 1)/OV_TILE;
    a.half_width = ov->half_width; a.h2 = ov->half_width*ov->half_width;
    a.bg_r = ov->background[0]; a.bg_g = ov->background[1]; a.bg_b = ov->background[2];
    a.lit = ov->lit ? 1 : 0; a.with_agents = ag ? 1 : 0; a.cull = g_overhead_cull ? 1 : 0;
    // (a launch of at most 2^22 blocks - 2^30 lanes - at a time: the (image, view, tile) number is 64-bit, the grid's is not)
    const long long total = (long long)ov->n_images*ov->n_views*a.tiles_x*a.tiles_y;
    const long long per_launch = 1LL << 22;
    for (long long b0 = 0; b0 < total; b0 += per_launch) {
        a.block0 = b0;
        const unsigned blocks = (unsigned)(total - b0 < per_launch ? total - b0 : per_launch);
        hipLaunchKernelGGL(overhead_kernel, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, *sc, agents_or_none(ag), a);
        if (const int status = launch_status(); status != MS_OK) return status;
    }
    return MS_OK;
}

int ms_debug_overhead_cull(int on) { g_overhead_cull = on; return MS_OK; }

int ms_host_overhead_keeps(const float* g, int height, int width, int tile_row, int tile_col, float half_width, const float* line) {
    const int i0 = tile_row*OV_TILE, j0 = tile_col*OV_TILE;
    const OvBox box = ov_footprint(g[0], g[1], g[2], g[3], g[4], g[5], i0, j0, i0 + OV_TILE - 1 < height - 1 ? i0 + OV_TILE - 1 : height - 1,
                                   j0 + OV_TILE - 1 < width - 1 ? j0 + OV_TILE - 1 : width - 1);
    return ov_keeps(box, half_width, make_float4(line[0], line[1], line[2], line[3])) ? 1 : 0;
}

// Distance fields (navfield.h): every argument checked in full before the first launch; nothing is allocated, nothing waits.
static bool nav_grid_ok(const MsNavGrid* g) {
    return g && g->n_envs > 0 && g->cell > 0.f && g->cell < INFINITY && g->clearance > 0.f && g->clearance < INFINITY &&
           g->cell <= 1.4f*g->clearance && g->geom && g->starts && g->free_cells && g->max_framed >= 0 && ((uintptr_t)g->geom % 16 == 0);
}
static NavArgs nav_args(const MsNavGrid* g) { return NavArgs{g->geom, g->starts, g->n_envs, g->cell, g->clearance}; }

int ms_nav_free(const MsScenery* sc, const MsNavGrid* grid, void* stream) {
    if (!scenery_ok(sc) || !nav_grid_ok(grid) || grid->n_envs != sc->n_envs) return MS_EINVAL;
    if (grid->n_envs > 65535) return MS_EUNSUPPORTED;
    if (grid->max_framed == 0) return MS_OK;
    const unsigned blocks = (unsigned)(((long long)grid->max_framed + WG - 1)/WG);        // (at least the largest env's cells)
    hipLaunchKernelGGL(nav_free_kernel, dim3(blocks, (unsigned)grid->n_envs), dim3(WG), 0, (hipStream_t)stream, *sc, nav_args(grid), grid->free_cells);
    return launch_status();
}

// The three LDS tiers of the kernels that keep an env's field in LDS (relaxation, regions, basins) and the threads of each
// tier's instantiations.  A launch takes the least tier whose capacity - by the kernel's own capacity function - holds the
// largest env's framed field: more workgroups a CU (an env that still does not fit - or is larger than max_framed says - runs in
// global memory).
constexpr int NAV_TIER_LDS[3] = {NAV_LDS_SMALL, NAV_LDS_MEDIUM, NAV_LDS_LARGE}, NAV_TIER_THREADS[3] = {512, 1024, 1024};
static int nav_tier(const MsNavGrid* grid, int (*capacity)(int)) {
    return grid->max_framed <= capacity(NAV_TIER_LDS[0]) ? 0 : grid->max_framed <= capacity(NAV_TIER_LDS[1]) ? 1 : 2;
}
static int nav_capacity_for(const MsNavGrid* grid, int (*capacity)(int)) { return capacity(NAV_TIER_LDS[nav_tier(grid, capacity)]); }
static int nav_host_capacities(int* capacities, int (*capacity)(int)) {
    if (!capacities) return MS_EINVAL;
    for (int t = 0; t < 3; t++) capacities[t] = capacity(NAV_TIER_LDS[t]);
    return MS_OK;
}

// The launch of either relaxation.
static int nav_relax_launch(const MsNavGrid* grid, const NavFieldArgs& f, long long total, bool seeded, void* stream) {
    static void (*const kernels[3][2])(NavArgs, NavFieldArgs) = {                   // [tier][seeded, single-goal]
        {nav_relax_kernel<NAV_LDS_SMALL, 512, true>, nav_relax_kernel<NAV_LDS_SMALL, 512, false>},
        {nav_relax_kernel<NAV_LDS_MEDIUM, 1024, true>, nav_relax_kernel<NAV_LDS_MEDIUM, 1024, false>},
        {nav_relax_kernel<NAV_LDS_LARGE, 1024, true>, nav_relax_kernel<NAV_LDS_LARGE, 1024, false>}};
    const int t = nav_tier(grid, nav_capacity);
    hipLaunchKernelGGL(kernels[t][seeded ? 0 : 1], dim3((unsigned)total), dim3(NAV_TIER_THREADS[t]), 0, (hipStream_t)stream, nav_args(grid), f);
    return launch_status();
}

// ... and of the weighted one (MsNavCostFields), in either variant of where a cell's multiplier lives: read from global memory
// every pass (the seeded kernel's bytes a cell and its tiers) or kept in LDS (its own capacity, its own tier).  The library's
// choice is the first (DESIGN.md 3.24 has the reasons); the other stays reachable through ms_debug_nav_cost_variant for A/B runs.
static int nav_cost_launch(const MsNavGrid* grid, const NavFieldArgs& f, long long total, void* stream) {
    static void (*const kernels[3][2])(NavArgs, NavFieldArgs) = {                   // [tier][from global memory, in LDS]
        {nav_relax_kernel<NAV_LDS_SMALL, 512, true, NAV_COST_GLOBAL>, nav_relax_kernel<NAV_LDS_SMALL, 512, true, NAV_COST_LDS>},
        {nav_relax_kernel<NAV_LDS_MEDIUM, 1024, true, NAV_COST_GLOBAL>, nav_relax_kernel<NAV_LDS_MEDIUM, 1024, true, NAV_COST_LDS>},
        {nav_relax_kernel<NAV_LDS_LARGE, 1024, true, NAV_COST_GLOBAL>, nav_relax_kernel<NAV_LDS_LARGE, 1024, true, NAV_COST_LDS>}};
    const int in_lds = g_nav_cost_variant == 1 ? 1 : 0;
    const int t = in_lds ? nav_tier(grid, nav_cost_capacity) : nav_tier(grid, nav_capacity);
    hipLaunchKernelGGL(kernels[t][in_lds], dim3((unsigned)total), dim3(NAV_TIER_THREADS[t]), 0, (hipStream_t)stream, nav_args(grid), f);
    return launch_status();
}

int ms_nav_fields(const MsNavGrid* grid, const MsNavFields* nf, void* stream) {
    if (!nav_grid_ok(grid) || !nf || nf->n_goals < 1 || !nf->goals || !nf->fields || ((uintptr_t)nf->goals % 8)) return MS_EINVAL;
    const long long total = (long long)grid->n_envs*nf->n_goals;
    if (total > 0x7fffffffLL) return MS_EUNSUPPORTED;
    const NavFieldArgs f{nf->goals, nf->mask, grid->free_cells, nf->fields, nf->passes, nf->n_goals, nullptr, nullptr, 0, nullptr, nullptr, 0};
    return nav_relax_launch(grid, f, total, false, stream);
}

int ms_nav_seed_fields(const MsNavGrid* grid, const MsNavSeedFields* sf, void* stream) {
    if (!nav_grid_ok(grid) || !sf || sf->n_fields < 1 || !sf->marks || !sf->fields || (sf->where != 0 && sf->where != 1) ||
        ((uintptr_t)sf->fields % 4) || ((uintptr_t)sf->passes % 4) || ((uintptr_t)sf->n_seeds % 4)) return MS_EINVAL;
    const long long total = (long long)grid->n_envs*sf->n_fields;
    if (total > 0x7fffffffLL) return MS_EUNSUPPORTED;
    const NavFieldArgs f{nullptr, sf->mask, grid->free_cells, sf->fields, sf->passes, sf->n_fields, sf->marks, sf->among, sf->where, sf->n_seeds,
                         nullptr, 0};
    return nav_relax_launch(grid, f, total, true, stream);
}

// Cost fields (MsNavCostFields): the seeded entries' checks, and the costs'.
static bool nav_costs_ok(const float* costs, int n_costs, int n_fields) {
    return costs && ((uintptr_t)costs % 4 == 0) && (n_costs == 1 || n_costs == n_fields);
}

int ms_nav_cost_fields(const MsNavGrid* grid, const MsNavCostFields* cf, void* stream) {
    if (!nav_grid_ok(grid) || !cf || cf->n_fields < 1 || !cf->marks || !cf->fields || (cf->where != 0 && cf->where != 1) ||
        ((uintptr_t)cf->fields % 4) || ((uintptr_t)cf->passes % 4) || ((uintptr_t)cf->n_seeds % 4) ||
        !nav_costs_ok(cf->costs, cf->n_costs, cf->n_fields)) return MS_EINVAL;
    const long long total = (long long)grid->n_envs*cf->n_fields;
    if (total > 0x7fffffffLL) return MS_EUNSUPPORTED;
    const NavFieldArgs f{nullptr, cf->mask, grid->free_cells, cf->fields, cf->passes, cf->n_fields, cf->marks, cf->among, cf->where, cf->n_seeds,
                         cf->costs, cf->n_costs};
    return nav_cost_launch(grid, f, total, stream);
}

int ms_debug_nav_cost_variant(int variant) {
    if (variant < -1 || variant > 1) return MS_EINVAL;
    g_nav_cost_variant = variant;
    return MS_OK;
}

int ms_nav_query(const MsNavGrid* grid, const MsNavQuery* nq, void* stream) {
    if (!nav_grid_ok(grid) || !nq || nq->n_points < 1 || nq->n_goals < 1 || !nq->points || !nq->fields || !nq->out ||
        (!nq->goal && nq->n_points != nq->n_goals) || ((uintptr_t)nq->points % 8)) return MS_EINVAL;
    const long long total = (long long)grid->n_envs*nq->n_points;
    if (total > 0x7fffff00LL) return MS_EUNSUPPORTED;
    const NavQueryArgs q{nq->points, nq->goal, nq->fields, nq->out, nq->n_points, nq->n_goals, total};
    hipLaunchKernelGGL(nav_query_kernel, dim3((unsigned)((total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, nav_args(grid), q);
    return launch_status();
}

// Paths and waypoints (navpath.h): the same discipline.
static bool nav_follow_ok(const MsNavGrid* grid, int n_points, const float* points, const int* goal, const float* fields, int n_goals) {
    return nav_grid_ok(grid) && n_points >= 1 && n_goals >= 1 && points && fields && (goal || n_points == n_goals) &&
           ((uintptr_t)points % 8 == 0) && ((uintptr_t)fields % 4 == 0) && ((uintptr_t)goal % 4 == 0);
}
static bool nav_goals_ok(const float* goals) { return goals && ((uintptr_t)goals % 8 == 0); }

// The two launches, for fields of goals and - goals NULL - for seeded fields, and - costs not NULL, n_costs 1 or n_goals - for cost
// fields (the WEIGHTED instantiations); the arguments are checked by then.
static int nav_waypoints_launch(const MsNavGrid* grid, int n_points, const float* points, const int* goal, const float* fields, const float* goals,
                                int n_goals, int lookahead, float* waypoints, int* hops, const float* costs, int n_costs, void* stream) {
    const long long total = (long long)grid->n_envs*n_points;
    if ((total + WAVES - 1)/WAVES > 0x7fffffffLL) return MS_EUNSUPPORTED;
    const NavPathArgs q{points, goal, fields, goals, grid->free_cells, waypoints, hops, nullptr, nullptr, n_points, n_goals, lookahead, 0, total,
                        costs, n_costs};
    const bool weighted = costs != nullptr;
    hipLaunchKernelGGL(weighted ? nav_waypoint_kernel<true> : nav_waypoint_kernel<false>, dim3((unsigned)((total + WAVES - 1)/WAVES)), dim3(WG), 0, (hipStream_t)stream, nav_args(grid), q);
    return launch_status();
}
static int nav_paths_launch(const MsNavGrid* grid, int n_points, const float* points, const int* goal, const float* fields, const float* goals,
                            int n_goals, int max_points, float* paths, int* counts, const float* costs, int n_costs, void* stream) {
    const long long total = (long long)grid->n_envs*n_points;
    if (total > 0x7fffff00LL) return MS_EUNSUPPORTED;
    const NavPathArgs q{points, goal, fields, goals, grid->free_cells, nullptr, nullptr, paths, counts, n_points, n_goals, 0, max_points, total,
                        costs, n_costs};
    const bool weighted = costs != nullptr;
    hipLaunchKernelGGL(weighted ? nav_path_kernel<true> : nav_path_kernel<false>, dim3((unsigned)((total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, nav_args(grid), q);
    return launch_status();
}
static bool nav_waypoints_ok(int lookahead, const float* waypoints, const int* hops) {
    return lookahead >= 1 && lookahead <= WAVE && waypoints && ((uintptr_t)waypoints % 8 == 0) && ((uintptr_t)hops % 4 == 0);
}
static bool nav_paths_ok(int max_points, const float* paths, const int* counts) {
    return max_points >= 2 && paths && counts && ((uintptr_t)paths % 4 == 0) && ((uintptr_t)counts % 4 == 0);
}

int ms_nav_waypoints(const MsNavGrid* grid, const MsNavWaypoints* w, void* stream) {
    if (!w || !nav_follow_ok(grid, w->n_points, w->points, w->goal, w->fields, w->n_goals) || !nav_goals_ok(w->goals) ||
        !nav_waypoints_ok(w->lookahead, w->waypoints, w->hops)) return MS_EINVAL;
    return nav_waypoints_launch(grid, w->n_points, w->points, w->goal, w->fields, w->goals, w->n_goals, w->lookahead, w->waypoints, w->hops, nullptr, 0, stream);
}

int ms_nav_paths(const MsNavGrid* grid, const MsNavPaths* np, void* stream) {
    if (!np || !nav_follow_ok(grid, np->n_points, np->points, np->goal, np->fields, np->n_goals) || !nav_goals_ok(np->goals) ||
        !nav_paths_ok(np->max_points, np->paths, np->counts)) return MS_EINVAL;
    return nav_paths_launch(grid, np->n_points, np->points, np->goal, np->fields, np->goals, np->n_goals, np->max_points, np->paths, np->counts, nullptr, 0, stream);
}

int ms_nav_seed_waypoints(const MsNavGrid* grid, const MsNavSeedWaypoints* w, void* stream) {
    if (!w || !nav_follow_ok(grid, w->n_points, w->points, w->goal, w->fields, w->n_goals) ||
        !nav_waypoints_ok(w->lookahead, w->waypoints, w->hops)) return MS_EINVAL;
    return nav_waypoints_launch(grid, w->n_points, w->points, w->goal, w->fields, nullptr, w->n_goals, w->lookahead, w->waypoints, w->hops, nullptr, 0, stream);
}

int ms_nav_seed_paths(const MsNavGrid* grid, const MsNavSeedPaths* np, void* stream) {
    if (!np || !nav_follow_ok(grid, np->n_points, np->points, np->goal, np->fields, np->n_goals) ||
        !nav_paths_ok(np->max_points, np->paths, np->counts)) return MS_EINVAL;
    return nav_paths_launch(grid, np->n_points, np->points, np->goal, np->fields, nullptr, np->n_goals, np->max_points, np->paths, np->counts, nullptr, 0, stream);
}

int ms_nav_cost_waypoints(const MsNavGrid* grid, const MsNavCostWaypoints* w, void* stream) {
    if (!w || !nav_follow_ok(grid, w->n_points, w->points, w->goal, w->fields, w->n_goals) ||
        !nav_waypoints_ok(w->lookahead, w->waypoints, w->hops) || !nav_costs_ok(w->costs, w->n_costs, w->n_goals)) return MS_EINVAL;
    return nav_waypoints_launch(grid, w->n_points, w->points, w->goal, w->fields, nullptr, w->n_goals, w->lookahead, w->waypoints, w->hops, w->costs,
                                w->n_costs, stream);
}

int ms_nav_cost_paths(const MsNavGrid* grid, const MsNavCostPaths* np, void* stream) {
    if (!np || !nav_follow_ok(grid, np->n_points, np->points, np->goal, np->fields, np->n_goals) ||
        !nav_paths_ok(np->max_points, np->paths, np->counts) || !nav_costs_ok(np->costs, np->n_costs, np->n_goals)) return MS_EINVAL;
    return nav_paths_launch(grid, np->n_points, np->points, np->goal, np->fields, nullptr, np->n_goals, np->max_points, np->paths, np->counts,
                            np->costs, np->n_costs, stream);
}

// Pulled paths (navpull.h, MsNavPulls): one entry for fields of goals, seeded fields (goals NULL) and cost fields (costs not NULL).
// The library's scheme is a lane a candidate; the waypoint kernel's, a lane a sample, stays reachable through
// ms_debug_nav_pull_scheme for A/B runs.
int ms_nav_pulls(const MsNavGrid* grid, const MsNavPulls* np, void* stream) {
    if (!np || !nav_follow_ok(grid, np->n_points, np->points, np->goal, np->fields, np->n_goals) || ((uintptr_t)np->goals % 8) ||
        np->reach < 1 || np->reach > NAV_PULL_REACH || np->max_points < 2 || np->max_points > NAV_PULL_POINTS ||
        !np->vertices || !np->counts || !np->lengths || ((uintptr_t)np->vertices % 4) || ((uintptr_t)np->indices % 4) ||
        ((uintptr_t)np->counts % 4) || ((uintptr_t)np->cells % 4) || ((uintptr_t)np->lengths % 4) ||
        (np->n_costs == 0 ? np->costs != nullptr : !nav_costs_ok(np->costs, np->n_costs, np->n_goals))) return MS_EINVAL;
    const long long total = (long long)grid->n_envs*np->n_points;
    if ((total + WAVES - 1)/WAVES > 0x7fffffffLL) return MS_EUNSUPPORTED;
    const NavPullArgs u{NavPathArgs{np->points, np->goal, np->fields, np->goals, grid->free_cells, nullptr, nullptr, np->vertices, np->counts,
                                    np->n_points, np->n_goals, 0, np->max_points, total, np->costs, np->n_costs},
                        np->mask, np->indices, np->cells, np->lengths, np->reach, nav_pull_ring(np->reach)};
    static void (*const kernels[2][2])(NavArgs, NavPullArgs) = {                    // [weighted][a lane a candidate, a lane a sample]
        {nav_pull_kernel<false, false>, nav_pull_kernel<false, true>}, {nav_pull_kernel<true, false>, nav_pull_kernel<true, true>}};
    hipLaunchKernelGGL(kernels[np->costs != nullptr][g_nav_pull_scheme == 1], dim3((unsigned)((total + WAVES - 1)/WAVES)), dim3(WG),
                       (size_t)WAVES*u.ring*sizeof(int), (hipStream_t)stream, nav_args(grid), u);
    return launch_status();
}

int ms_debug_nav_pull_scheme(int scheme) {
    if (scheme < -1 || scheme > 1) return MS_EINVAL;
    g_nav_pull_scheme = scheme;
    return MS_OK;
}

static bool nav_host_env(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* goal, const float* point,
                         NavEnv& g) {
    if (!geom || !free_cells || !D || !goal || !point || !(cell > 0.f) || geom[2] <= 0 || geom[3] <= 0) return false;
    g = NavEnv{geom[0], geom[1], geom[2], geom[3], cell, free_cells, D, nullptr};
    return true;
}

int ms_host_nav_waypoint(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* goal, const float* point,
                         int lookahead, float* waypoint) {
    if (lookahead < 1 || lookahead > WAVE || !waypoint) return -2;
    waypoint[0] = waypoint[1] = NAN;
    NavEnv g;
    if (!nav_host_env(geom, cell, free_cells, D, goal, point, g)) return -1;
    return nav_waypoint_serial(g, nav_goal(g, goal[0], goal[1]), point[0], point[1], lookahead, waypoint[0], waypoint[1]);
}

int ms_host_nav_path(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* goal, const float* point,
                     int max_points, float* points) {
    if (max_points < 2 || !points) return 0;
    NavEnv g;
    if (!nav_host_env(geom, cell, free_cells, D, goal, point, g)) {
        for (int k = 0; k < 2*max_points; k++) points[k] = NAN;
        return 0;
    }
    return nav_path(g, nav_goal(g, goal[0], goal[1]), point[0], point[1], (long long)g.nx*g.ny, max_points, points);
}

int ms_host_nav_seed_waypoint(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* point, int lookahead,
                              float* waypoint) {
    if (lookahead < 1 || lookahead > WAVE || !waypoint) return -2;
    waypoint[0] = waypoint[1] = NAN;
    NavEnv g;
    if (!nav_host_env(geom, cell, free_cells, D, point, point, g)) return -1;
    return nav_waypoint_serial(g, nav_seeded(), point[0], point[1], lookahead, waypoint[0], waypoint[1]);
}

int ms_host_nav_seed_path(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* point, int max_points,
                          float* points) {
    if (max_points < 2 || !points) return 0;
    NavEnv g;
    if (!nav_host_env(geom, cell, free_cells, D, point, point, g)) {
        for (int k = 0; k < 2*max_points; k++) points[k] = NAN;
        return 0;
    }
    return nav_path(g, nav_seeded(), point[0], point[1], (long long)g.nx*g.ny, max_points, points);
}

int ms_host_nav_cost_waypoint(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* costs, const float* point,
                              int lookahead, float* waypoint) {
    if (lookahead < 1 || lookahead > WAVE || !waypoint) return -2;
    waypoint[0] = waypoint[1] = NAN;
    NavEnv g;
    if (!costs || !nav_host_env(geom, cell, free_cells, D, point, point, g)) return -1;
    g.cost = costs;
    return nav_waypoint_serial(g, nav_seeded(), point[0], point[1], lookahead, waypoint[0], waypoint[1]);
}

int ms_host_nav_cost_path(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* costs, const float* point,
                          int max_points, float* points) {
    if (max_points < 2 || !points) return 0;
    NavEnv g;
    if (!costs || !nav_host_env(geom, cell, free_cells, D, point, point, g)) {
        for (int k = 0; k < 2*max_points; k++) points[k] = NAN;
        return 0;
    }
    g.cost = costs;
    return nav_path(g, nav_seeded(), point[0], point[1], (long long)g.nx*g.ny, max_points, points);
}

int ms_host_nav_pull(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* goal, const float* costs,
                     const float* point, int reach, int max_points, float* vertices, int* indices, float* length) {
    if (reach < 1 || reach > NAV_PULL_REACH) return -2;
    if (max_points < 2 || max_points > NAV_PULL_POINTS || !vertices || !length) return 0;
    NavEnv g;
    if (!nav_host_env(geom, cell, free_cells, D, point, point, g)) {
        for (int k = 0; k < max_points; k++) {
            vertices[2*k] = vertices[2*k + 1] = NAN;
            if (indices) indices[k] = -1;
        }
        *length = INFINITY;
        return 0;
    }
    g.cost = costs;
    return nav_pull_serial(g, goal ? nav_goal(g, goal[0], goal[1]) : nav_seeded(), point[0], point[1], reach, max_points, vertices, indices,
                           nullptr, *length);
}

// The seeded relaxation on host arrays, and - costs not NULL - the weighted one: the kernel's fill and per-cell functions, swept.
static int nav_host_seed_field(const int* geom, float cell, const unsigned char* free_cells, const unsigned char* marks, int where,
                               const unsigned char* among, const float* costs, int framed, float* D, int* n_seeds) {
    if (!geom || !(cell > 0.f) || !(cell < INFINITY) || (where != 0 && where != 1) || geom[2] < 0 || geom[3] < 0) return -1;
    const int nx = geom[2], ny = geom[3];
    const long long cells = (long long)nx*ny;
    if (n_seeds) *n_seeds = 0;
    if (cells <= 0) return 0;
    if (!free_cells || !marks || !D || (long long)(nx + 2)*(ny + 2) > 0x7fffffffLL) return -1;
    float ws = cell, wd = cell*NAV_DIAGONAL;
    int seeds = 0, sweeps = 0;
    if (framed) {
        // as the kernel fills its LDS: the frame, the bytes, the seeds; then nav_cell_framed swept in place
        const int P = nx + 2, n = (nx + 2)*(ny + 2);
        std::vector<float> d(n);
        std::vector<unsigned char> m(n);
        std::vector<float> mult(costs ? n : 0);                         // (as NAV_COST_LDS keeps them)
        for (int k = 0; k < n; k++) {
            long long at;
            const int fb = nav_frame_free(free_cells, nx, ny, P, k, at);
            const bool seed = fb && nav_is_seed(free_cells, among, marks, at, where);
            d[k] = seed ? 0.f : INFINITY;
            m[k] = (unsigned char)(fb | (seed ? 32 : 0));
            if (costs) mult[k] = fb ? nav_cost_multiplier(costs[at]) : 1.f;
            seeds += seed;
        }
        for (int k = 0; k < n; k++)
            if (m[k] & 1) m[k] = (unsigned char)(nav_frame_open(m.data(), k, P) | (m[k] & 32));
        for (bool changed = true; changed; sweeps++) {
            changed = false;
            for (int k = 0; k < n; k++) {
                if (!(m[k] & 1)) continue;
                if (costs) nav_cost_weights(cell, mult[k], ws, wd);
                const float v = nav_cell_framed(d.data(), m[k], k, P, d[k], ws, wd);
                if (v < d[k]) { d[k] = v; changed = true; }
            }
        }
        for (long long k = 0; k < cells; k++) D[k] = d[(k / nx + 1)*P + k % nx + 1];
    } else {
        for (long long k = 0; k < cells; k++) {
            const bool seed = nav_is_seed(free_cells, among, marks, k, where);
            D[k] = seed ? 0.f : INFINITY;
            seeds += seed;
        }
        for (bool changed = true; changed; sweeps++) {
            changed = false;
            for (long long k = 0; k < cells; k++) {
                if (!(free_cells[k] & 1)) continue;
                if (costs) nav_cost_weights(cell, nav_cost_multiplier(costs[k]), ws, wd);
                const float v = nav_cell_stored(D, free_cells, nx, ny, k, D[k], ws, wd);
                if (v < D[k]) { D[k] = v; changed = true; }
            }
        }
    }
    if (n_seeds) *n_seeds = seeds;
    return sweeps;
}

int ms_host_nav_seed_field(const int* geom, float cell, const unsigned char* free_cells, const unsigned char* marks, int where,
                           const unsigned char* among, int framed, float* D, int* n_seeds) {
    return nav_host_seed_field(geom, cell, free_cells, marks, where, among, nullptr, framed, D, n_seeds);
}

int ms_host_nav_cost_field(const int* geom, float cell, const unsigned char* free_cells, const unsigned char* marks, int where,
                           const unsigned char* among, const float* costs, int framed, float* D, int* n_seeds) {
    if (!costs && geom && (long long)geom[2]*geom[3] > 0) return -1;
    return nav_host_seed_field(geom, cell, free_cells, marks, where, among, costs, framed, D, n_seeds);
}

int ms_host_nav_field_capacity(int* capacities) { return nav_host_capacities(capacities, nav_capacity); }
int ms_host_nav_cost_capacity(int* capacities) { return nav_host_capacities(capacities, nav_cost_capacity); }

// Seen maps (navseen.h): the same discipline; an env of more than 2^20 cells is refused, and nothing is enqueued.
constexpr int NAV_SEEN_MAX_CELLS = 1 << 20;
static bool nav_seen_ok(const MsNavSeen* v) {
    return v && v->n_maps >= 1 && v->n_viewers >= 1 && v->n_rays >= 1 && v->origins && v->dirs && v->distances && v->maps &&
           (v->slot || v->n_viewers == v->n_maps) && v->max_range > 0.f && v->max_range < INFINITY &&
           v->max_cells >= 0 && ((uintptr_t)v->origins % 8 == 0) && ((uintptr_t)v->dirs % 8 == 0) && ((uintptr_t)v->distances % 4 == 0) &&
           ((uintptr_t)v->slot % 4 == 0) && ((uintptr_t)v->gained % 4 == 0) && ((uintptr_t)v->total % 4 == 0);
}

int ms_nav_seen(const MsNavGrid* grid, const MsNavSeen* v, void* stream) {
    if (!nav_grid_ok(grid) || !nav_seen_ok(v)) return MS_EINVAL;
    const long long total = (long long)grid->n_envs*v->n_maps;
    if (v->max_cells > NAV_SEEN_MAX_CELLS || total > 0x7fffffffLL || (long long)grid->n_envs*v->n_viewers > 0x7fffffffLL/v->n_rays)
        return MS_EUNSUPPORTED;
    const NavSeenArgs q{v->origins, v->dirs, v->distances, v->slot, v->reset, v->countable ? v->countable : grid->free_cells, v->maps,
                        v->gained, v->total, v->n_maps, v->n_viewers, v->n_rays, v->max_cells, v->max_range};
    const size_t lds = (size_t)((v->max_cells + 31)/32)*sizeof(unsigned);                   // (at most 128 KiB of the CU's 160)
    if (lds > 64*1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(nav_seen_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds) != hipSuccess) return hip_fail(hipGetLastError());
    hipLaunchKernelGGL(nav_seen_kernel, dim3((unsigned)total), dim3(WG), lds, (hipStream_t)stream, nav_args(grid), q);
    return launch_status();
}

int ms_host_nav_seen(const int* geom, float cell, const unsigned char* countable, int n_maps, int n_viewers, int n_rays,
                     const float* origins, const float* dirs, const float* distances, const int* slot, float max_range,
                     const unsigned char* reset, unsigned char* maps, int* gained, int* total) {
    if (!geom || !(cell > 0.f) || !(cell < INFINITY) || n_maps < 1 || n_viewers < 1 || n_rays < 1 || !origins || !dirs || !distances ||
        !maps || !countable || !(slot || n_viewers == n_maps) || !(max_range > 0.f) || !(max_range < INFINITY)) return -1;
    seen_serial(NavCells{geom[0], geom[1], geom[2], geom[3], cell}, countable, n_maps, n_viewers, n_rays, origins, dirs, distances, slot,
                max_range, reset, maps, gained, total);
    return 0;
}

// Age maps (navage.h): the same discipline, and the seen maps' limit; one check serves the launch and the host instantiation.
static int nav_ages_check(const MsNavAges* v) {
    if (!v || v->n_maps < 1 || !v->last || !v->clock || v->threshold < 1 || (v->advance != 0 && v->advance != 1) ||
        !(v->max_range > 0.f) || !(v->max_range < INFINITY) || v->max_cells < 0 ||
        ((uintptr_t)v->last % 4) || ((uintptr_t)v->clock % 4) || ((uintptr_t)v->swept % 4) || ((uintptr_t)v->gained % 4) ||
        ((uintptr_t)v->idle % 8) || ((uintptr_t)v->oldest % 4) || ((uintptr_t)v->total_age % 8) || ((uintptr_t)v->n_stale % 4) ||
        ((uintptr_t)v->ages % 4)) return MS_EINVAL;
    if (v->advance && (v->n_viewers < 1 || v->n_rays < 1 || !v->origins || !v->dirs || !v->distances ||
                       !(v->slot || v->n_viewers == v->n_maps) || ((uintptr_t)v->origins % 8) || ((uintptr_t)v->dirs % 8) ||
                       ((uintptr_t)v->distances % 4) || ((uintptr_t)v->slot % 4))) return MS_EINVAL;
    return v->max_cells > NAV_SEEN_MAX_CELLS ? MS_EUNSUPPORTED : MS_OK;
}
static NavAgeArgs nav_age_args(const MsNavAges* v, const unsigned char* countable) {
    return NavAgeArgs{v->origins, v->dirs, v->distances, v->slot, v->reset, countable, v->last, v->clock, v->swept, v->gained, v->idle,
                      v->oldest, v->total_age, v->n_stale, v->stale, v->ages, v->n_maps, v->advance ? v->n_viewers : 0,
                      v->advance ? v->n_rays : 0, v->max_cells, v->advance, v->threshold, v->max_range};
}

int ms_nav_ages(const MsNavGrid* grid, const MsNavAges* v, void* stream) {
    if (!nav_grid_ok(grid)) return MS_EINVAL;
    const int status = nav_ages_check(v);
    if (status != MS_OK) return status;
    const long long total = (long long)grid->n_envs*v->n_maps;
    if (total > 0x7fffffffLL || (v->advance && (long long)grid->n_envs*v->n_viewers > 0x7fffffffLL/v->n_rays)) return MS_EUNSUPPORTED;
    const size_t lds = (size_t)((v->max_cells + 31)/32)*sizeof(unsigned);                   // (at most 128 KiB of the CU's 160)
    if (lds > 64*1024 - 256 && hipFuncSetAttribute(reinterpret_cast<const void*>(nav_age_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)lds) != hipSuccess) return hip_fail(hipGetLastError());
    hipLaunchKernelGGL(nav_age_kernel, dim3((unsigned)total), dim3(WG), lds, (hipStream_t)stream, nav_args(grid),
                       nav_age_args(v, v->countable ? v->countable : grid->free_cells));
    return launch_status();
}

int ms_host_nav_ages(const int* geom, float cell, const MsNavAges* v) {
    if (!geom || !(cell > 0.f) || !(cell < INFINITY)) return MS_EINVAL;
    const int status = nav_ages_check(v);
    if (status != MS_OK) return status;
    if (!v->countable) return MS_EINVAL;
    if (geom[2] > 0 && geom[3] > 0 && (long long)geom[2]*geom[3] > NAV_SEEN_MAX_CELLS) return MS_EUNSUPPORTED;
    age_serial(NavCells{geom[0], geom[1], geom[2], geom[3], cell}, nav_age_args(v, v->countable));
    return MS_OK;
}

// Map windows (navwindow.h): the same discipline; the channels go into the kernel's arguments by value.
static bool nav_layer_ok(const MsNavLayer& l, const int n_views) {
    return l.values && (l.is_float == 0 || l.is_float == 1) && l.n_fields >= 1 && (l.field || l.n_fields == 1 || l.n_fields == n_views) &&
           ((uintptr_t)l.field % 4 == 0) && (!l.is_float || (uintptr_t)l.values % 4 == 0);
}
static bool nav_windows_ok(const MsNavWindows* w) {
    if (!w || w->n_views < 1 || w->height < 1 || w->height > WIN_MAX_SIDE || w->width < 1 || w->width > WIN_MAX_SIDE ||
        w->samples < 1 || w->samples > WIN_MAX_SAMPLES || w->n_channels < 1 || w->n_channels > WIN_MAX_CHANNELS || !w->views ||
        !w->channels || !w->out || ((uintptr_t)w->views % 4) || ((uintptr_t)w->out % 4)) return false;
    for (int c = 0; c < w->n_channels; c++) {
        const MsNavChannel& ch = w->channels[c];
        if (!nav_layer_ok(ch.source, w->n_views) || (ch.where != 0 && ch.where != 1)) return false;
        if (ch.gate.values && (!nav_layer_ok(ch.gate, w->n_views) || ch.gate.is_float)) return false;
    }
    return true;
}
static NavWindowArgs nav_window_args(const MsNavWindows* w) {
    NavWindowArgs q{w->views, w->out, w->n_views, w->height, w->width, w->n_channels, {}};
    for (int c = 0; c < w->n_channels; c++) {
        const MsNavChannel& ch = w->channels[c];
        const bool gated = ch.gate.values != nullptr;
        q.ch[c] = WinChannel{ch.source.values, ch.source.field, static_cast<const unsigned char*>(ch.gate.values), gated ? ch.gate.field : nullptr,
                             ch.source.n_fields, gated ? ch.gate.n_fields : 1, ch.source.is_float, ch.where, ch.scale, ch.outside, ch.hidden};
    }
    return q;
}

int ms_nav_windows(const MsNavGrid* grid, const MsNavWindows* w, void* stream) {
    if (!nav_grid_ok(grid) || !nav_windows_ok(w)) return MS_EINVAL;
    const long long images = (long long)grid->n_envs*w->n_views;
    if (images > 0x7fffffffLL) return MS_EUNSUPPORTED;
    const NavWindowArgs q = nav_window_args(w);
    const dim3 blocks((unsigned)images, (unsigned)((w->height*w->width + WG - 1)/WG));      // (y: at most 4096)
    const hipStream_t s = (hipStream_t)stream;
    switch (w->samples) {
        case 1: hipLaunchKernelGGL(nav_window_kernel<1>, blocks, dim3(WG), 0, s, nav_args(grid), q); break;
        case 2: hipLaunchKernelGGL(nav_window_kernel<2>, blocks, dim3(WG), 0, s, nav_args(grid), q); break;
        case 3: hipLaunchKernelGGL(nav_window_kernel<3>, blocks, dim3(WG), 0, s, nav_args(grid), q); break;
        default: hipLaunchKernelGGL(nav_window_kernel<4>, blocks, dim3(WG), 0, s, nav_args(grid), q); break;
    }
    return launch_status();
}

int ms_host_nav_windows(const MsNavGrid* grid, const MsNavWindows* w) {
    if (!nav_grid_ok(grid) || !nav_windows_ok(w)) return MS_EINVAL;
    const NavWindowArgs q = nav_window_args(w);
    switch (w->samples) {
        case 1: win_serial<1>(nav_args(grid), q); break;
        case 2: win_serial<2>(nav_args(grid), q); break;
        case 3: win_serial<3>(nav_args(grid), q); break;
        default: win_serial<4>(nav_args(grid), q); break;
    }
    return MS_OK;
}

// Cell draws (navdraw.h): the same discipline; the bitmap's size is the seen maps'.
static int nav_draws_check(const MsNavGrid* grid, const MsNavDraws* d) {
    if (!nav_grid_ok(grid) || !d || d->n_sets < 1 || d->n_draws < 1 || d->n_draws > DRAW_MAX_DRAWS || !nav_layer_ok(d->source, d->n_sets) ||
        (d->where != 0 && d->where != 1) || (d->gate.values && (!nav_layer_ok(d->gate, d->n_sets) || d->gate.is_float)) ||
        (d->source.is_float && (d->lo != d->lo || d->hi != d->hi)) || (d->values && !d->source.is_float) ||
        !d->counter || !d->cells || !d->points || !d->uniforms || !d->counts || d->max_cells < 0 ||
        ((uintptr_t)d->counter % 4) || ((uintptr_t)d->cells % 4) || ((uintptr_t)d->points % 4) || ((uintptr_t)d->uniforms % 4) ||
        ((uintptr_t)d->values % 4) || ((uintptr_t)d->counts % 4)) return MS_EINVAL;
    if (d->max_cells > NAV_SEEN_MAX_CELLS || (long long)grid->n_envs*d->n_sets > 0x7fffffffLL/d->n_draws) return MS_EUNSUPPORTED;
    return MS_OK;
}
static NavDrawArgs nav_draw_args(const MsNavGrid* grid, const MsNavDraws* d) {
    const bool gated = d->gate.values != nullptr;
    return NavDrawArgs{d->source.values, d->source.field, static_cast<const unsigned char*>(d->gate.values), gated ? d->gate.field : nullptr,
                       grid->free_cells, d->mask, d->counter, d->cells, d->points, d->uniforms, d->values, d->counts,
                       d->source.n_fields, gated ? d->gate.n_fields : 1, d->source.is_float, d->where, d->lo, d->hi,
                       (unsigned)(d->seed & 0xffffffffull), (unsigned)(d->seed >> 32), d->n_sets, d->n_draws, d->max_cells};
}

int ms_nav_draws(const MsNavGrid* grid, const MsNavDraws* d, void* stream) {
    const int status = nav_draws_check(grid, d);
    if (status != MS_OK) return status;
    const size_t lds = (size_t)((d->max_cells + 63)/64 + WG)*sizeof(unsigned long long);      // (at most 130 KiB of the CU's 160)
    if (lds > 64*1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(nav_draw_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds) != hipSuccess) return hip_fail(hipGetLastError());
    hipLaunchKernelGGL(nav_draw_kernel, dim3((unsigned)((long long)grid->n_envs*d->n_sets)), dim3(WG), lds, (hipStream_t)stream,
                       nav_args(grid), nav_draw_args(grid, d));
    return launch_status();
}

int ms_host_nav_draws(const MsNavGrid* grid, const MsNavDraws* d) {
    const int status = nav_draws_check(grid, d);
    if (status != MS_OK) return status;
    draw_serial(nav_args(grid), nav_draw_args(grid, d));
    return MS_OK;
}

// Regions (navregion.h): the same discipline; the launch's LDS is chosen as the relaxation's, by the largest framed field.
static int nav_regions_check(const MsNavGrid* grid, const MsNavRegions* r) {
    if (!nav_grid_ok(grid) || !r || r->n_fields < 1 || (r->marks && r->where != 0 && r->where != 1) || !r->labels || !r->areas || !r->counts ||
        !r->open_cells || !r->largest || !r->largest_cells || ((uintptr_t)r->labels % 4) || ((uintptr_t)r->areas % 4) ||
        ((uintptr_t)r->counts % 4) || ((uintptr_t)r->open_cells % 4) || ((uintptr_t)r->largest % 4) || ((uintptr_t)r->largest_cells % 4) ||
        ((uintptr_t)r->passes % 4)) return MS_EINVAL;
    if ((long long)grid->n_envs*r->n_fields > 0x7fffffffLL) return MS_EUNSUPPORTED;
    return MS_OK;
}
static NavRegionArgs nav_region_args(const MsNavGrid* grid, const MsNavRegions* r) {
    return NavRegionArgs{grid->free_cells, r->marks, r->marks ? r->among : nullptr, r->mask, r->labels, r->areas, r->counts, r->open_cells,
                         r->largest, r->largest_cells, r->passes, r->n_fields, r->marks ? r->where : 1};
}
static int nav_region_query_check(const MsNavGrid* grid, const MsNavRegionQuery* q) {
    if (!nav_grid_ok(grid) || !q || q->n_points < 1 || q->n_fields < 1 || !q->points || !q->labels || !q->labels_at ||
        (!q->field && q->n_fields != 1 && q->n_fields != q->n_points) || ((uintptr_t)q->points % 4) || ((uintptr_t)q->field % 4) ||
        ((uintptr_t)q->labels % 4) || ((uintptr_t)q->labels_at % 4)) return MS_EINVAL;
    if ((long long)grid->n_envs*q->n_points > 0x7fffff00LL/4) return MS_EUNSUPPORTED;
    return MS_OK;
}
static int nav_region_masks_check(const MsNavGrid* grid, const MsNavRegionMasks* m) {
    if (!nav_grid_ok(grid) || !m || m->n_requests < 1 || m->n_fields < 1 || (m->points != nullptr) == (m->wanted != nullptr) || !m->labels ||
        !m->out || (!m->field && m->n_fields != 1 && m->n_fields != m->n_requests) || ((uintptr_t)m->points % 4) || ((uintptr_t)m->wanted % 4) ||
        ((uintptr_t)m->field % 4) || ((uintptr_t)m->labels % 4)) return MS_EINVAL;
    if ((long long)grid->n_envs*m->n_requests > 0x7fffffffLL) return MS_EUNSUPPORTED;
    return MS_OK;
}

int ms_nav_regions(const MsNavGrid* grid, const MsNavRegions* r, void* stream) {
    const int status = nav_regions_check(grid, r);
    if (status != MS_OK) return status;
    static void (*const kernels[3])(NavArgs, NavRegionArgs) = {nav_region_kernel<NAV_LDS_SMALL, 512>, nav_region_kernel<NAV_LDS_MEDIUM, 1024>,
                                                               nav_region_kernel<NAV_LDS_LARGE, 1024>};
    const int t = nav_tier(grid, region_capacity);
    hipLaunchKernelGGL(kernels[t], dim3((unsigned)((long long)grid->n_envs*r->n_fields)), dim3(NAV_TIER_THREADS[t]), 0, (hipStream_t)stream,
                       nav_args(grid), nav_region_args(grid, r));
    return launch_status();
}

int ms_nav_region_query(const MsNavGrid* grid, const MsNavRegionQuery* q, void* stream) {
    const int status = nav_region_query_check(grid, q);
    if (status != MS_OK) return status;
    const long long total = (long long)grid->n_envs*q->n_points;
    const NavRegionQueryArgs a{q->points, q->field, q->labels, q->labels_at, q->n_points, q->n_fields, total};
    hipLaunchKernelGGL(nav_region_query_kernel, dim3((unsigned)((total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, nav_args(grid), a);
    return launch_status();
}

int ms_nav_region_masks(const MsNavGrid* grid, const MsNavRegionMasks* m, void* stream) {
    const int status = nav_region_masks_check(grid, m);
    if (status != MS_OK) return status;
    if (grid->max_framed == 0) return MS_OK;                            // (no env has cells: nothing to write)
    const long long runs = ((long long)grid->max_framed + WG - 1)/WG;  // (at least the largest env's cells; the kernel strides beyond)
    const NavRegionMaskArgs a{m->points, m->wanted, m->field, m->labels, m->out, m->n_requests, m->n_fields};
    hipLaunchKernelGGL(nav_region_mask_kernel, dim3((unsigned)((long long)grid->n_envs*m->n_requests), (unsigned)(runs < 4096 ? runs : 4096)), dim3(WG), 0,
                       (hipStream_t)stream, nav_args(grid), a);
    return launch_status();
}

int ms_host_nav_regions(const MsNavGrid* grid, const MsNavRegions* r) {
    const int status = nav_regions_check(grid, r);
    if (status != MS_OK) return status;
    region_serial(nav_args(grid), nav_region_args(grid, r), nav_capacity_for(grid, region_capacity));
    return MS_OK;
}

int ms_host_nav_region_query(const MsNavGrid* grid, const MsNavRegionQuery* q) {
    const int status = nav_region_query_check(grid, q);
    if (status != MS_OK) return status;
    const long long total = (long long)grid->n_envs*q->n_points;
    const NavRegionQueryArgs a{q->points, q->field, q->labels, q->labels_at, q->n_points, q->n_fields, total};
    for (long long at = 0; at < total; at++) region_query_one(nav_args(grid), a, at);
    return MS_OK;
}

int ms_host_nav_region_masks(const MsNavGrid* grid, const MsNavRegionMasks* m) {
    const int status = nav_region_masks_check(grid, m);
    if (status != MS_OK) return status;
    region_mask_serial(nav_args(grid), NavRegionMaskArgs{m->points, m->wanted, m->field, m->labels, m->out, m->n_requests, m->n_fields});
    return MS_OK;
}

int ms_host_nav_region_capacity(int* capacities) { return nav_host_capacities(capacities, region_capacity); }

// Basins (navbasin.h): the same discipline; the launch's LDS is chosen by max_framed, which bounds every env's cells from above.
static int nav_basins_check(const MsNavGrid* grid, const MsNavBasins* b) {
    if (!nav_grid_ok(grid) || !b || b->n_fields < 1 || !b->fields || !b->labels || !b->reached || b->n_ids < 0 || b->n_ids > BASIN_MAX_IDS ||
        (b->sizes != nullptr) != (b->n_ids > 0) || b->ids == b->labels || ((uintptr_t)b->fields % 4) || ((uintptr_t)b->ids % 4) ||
        ((uintptr_t)b->labels % 4) || ((uintptr_t)b->sizes % 4) || ((uintptr_t)b->reached % 4) || ((uintptr_t)b->passes % 4)) return MS_EINVAL;
    if ((long long)grid->n_envs*b->n_fields > 0x7fffffffLL/(b->n_ids > 0 ? b->n_ids : 1)) return MS_EUNSUPPORTED;
    return MS_OK;
}
static NavBasinArgs nav_basin_args(const MsNavGrid* grid, const MsNavBasins* b) {
    return NavBasinArgs{grid->free_cells, b->fields, b->ids, b->mask, b->labels, b->sizes, b->reached, b->passes, b->n_fields, b->n_ids};
}
static int nav_basin_query_check(const MsNavGrid* grid, const MsNavBasinQuery* q) {
    if (!nav_grid_ok(grid) || !q || q->n_points < 1 || q->n_fields < 1 || !q->points || !q->fields || !q->labels || !q->out ||
        (!q->field && q->n_fields != 1 && q->n_fields != q->n_points) || ((uintptr_t)q->points % 4) || ((uintptr_t)q->field % 4) ||
        ((uintptr_t)q->fields % 4) || ((uintptr_t)q->labels % 4) || ((uintptr_t)q->out % 4)) return MS_EINVAL;
    if ((long long)grid->n_envs*q->n_points > 0x7fffff00LL) return MS_EUNSUPPORTED;
    return MS_OK;
}
static NavBasinQueryArgs nav_basin_query_args(const MsNavGrid* grid, const MsNavBasinQuery* q) {
    return NavBasinQueryArgs{q->points, q->field, grid->free_cells, q->fields, q->labels, q->out, q->n_points, q->n_fields,
                             (long long)grid->n_envs*q->n_points};
}
static int nav_point_marks_check(const MsNavGrid* grid, const MsNavPointMarks* m) {
    if (!nav_grid_ok(grid) || !m || m->n_points < 1 || m->n_fields < 1 || !m->points || !m->marks || !m->ids ||
        (!m->field && m->n_fields != 1 && m->n_fields != m->n_points) || ((uintptr_t)m->points % 4) || ((uintptr_t)m->field % 4) ||
        ((uintptr_t)m->point_ids % 4) || ((uintptr_t)m->ids % 4)) return MS_EINVAL;
    if ((long long)grid->n_envs*m->n_points > 0x7fffff00LL) return MS_EUNSUPPORTED;
    return MS_OK;
}
static NavPointMarkArgs nav_point_mark_args(const MsNavGrid* grid, const MsNavPointMarks* m) {
    return NavPointMarkArgs{m->points, m->field, m->point_ids, grid->free_cells, m->marks, m->ids, m->n_points, m->n_fields,
                            (long long)grid->n_envs*m->n_points};
}

int ms_nav_basins(const MsNavGrid* grid, const MsNavBasins* b, void* stream) {
    const int status = nav_basins_check(grid, b);
    if (status != MS_OK) return status;
    static void (*const kernels[3])(NavArgs, NavBasinArgs) = {nav_basin_kernel<NAV_LDS_SMALL, 512>, nav_basin_kernel<NAV_LDS_MEDIUM, 1024>,
                                                              nav_basin_kernel<NAV_LDS_LARGE, 1024>};
    const int t = nav_tier(grid, basin_capacity);
    hipLaunchKernelGGL(kernels[t], dim3((unsigned)((long long)grid->n_envs*b->n_fields)), dim3(NAV_TIER_THREADS[t]), 0, (hipStream_t)stream,
                       nav_args(grid), nav_basin_args(grid, b));
    return launch_status();
}

int ms_nav_basin_query(const MsNavGrid* grid, const MsNavBasinQuery* q, void* stream) {
    const int status = nav_basin_query_check(grid, q);
    if (status != MS_OK) return status;
    const NavBasinQueryArgs a = nav_basin_query_args(grid, q);
    hipLaunchKernelGGL(nav_basin_query_kernel, dim3((unsigned)((a.total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, nav_args(grid), a);
    return launch_status();
}

int ms_nav_point_marks(const MsNavGrid* grid, const MsNavPointMarks* m, void* stream) {
    const int status = nav_point_marks_check(grid, m);
    if (status != MS_OK) return status;
    const NavPointMarkArgs a = nav_point_mark_args(grid, m);
    hipLaunchKernelGGL(nav_point_mark_kernel, dim3((unsigned)((a.total + WG - 1)/WG)), dim3(WG), 0, (hipStream_t)stream, nav_args(grid), a);
    return launch_status();
}

int ms_host_nav_basins(const MsNavGrid* grid, const MsNavBasins* b) {
    const int status = nav_basins_check(grid, b);
    if (status != MS_OK) return status;
    basin_serial(nav_args(grid), nav_basin_args(grid, b), nav_capacity_for(grid, basin_capacity));
    return MS_OK;
}

int ms_host_nav_basin_query(const MsNavGrid* grid, const MsNavBasinQuery* q) {
    const int status = nav_basin_query_check(grid, q);
    if (status != MS_OK) return status;
    const NavBasinQueryArgs a = nav_basin_query_args(grid, q);
    for (long long at = 0; at < a.total; at++) basin_query_one(nav_args(grid), a, at);
    return MS_OK;
}

int ms_host_nav_point_marks(const MsNavGrid* grid, const MsNavPointMarks* m) {
    const int status = nav_point_marks_check(grid, m);
    if (status != MS_OK) return status;
    const NavPointMarkArgs a = nav_point_mark_args(grid, m);
    for (long long at = 0; at < a.total; at++) point_mark_one(nav_args(grid), a, at);
    return MS_OK;
}

int ms_host_nav_basin_capacity(int* capacities) { return nav_host_capacities(capacities, basin_capacity); }

// Zones (navzone.h): the same discipline; one instantiation - the kernel's LDS does not grow with the env.
static int nav_zones_check(const MsNavGrid* grid, const MsNavZones* z) {
    const auto stores_ok = [&](int count) { return count == 1 || count == z->n_fields; };
    if (!nav_grid_ok(grid) || !z || z->n_fields < 1 || z->max_zones < 1 || z->max_zones > ZONE_MAX || !z->labels || !stores_ok(z->n_labels) ||
        (z->values && !stores_ok(z->n_values)) || (z->marks && (!stores_ok(z->n_marks) || (z->where != 0 && z->where != 1))) ||
        (z->ranked != 0 && z->ranked != 1) || (z->within_marks != 0 && z->within_marks != 1) || !z->cells || !z->marked || !z->least ||
        !z->nearest || !z->points || !z->roots || !z->n_zones || ((uintptr_t)z->labels % 4) || ((uintptr_t)z->values % 4) ||
        ((uintptr_t)z->cells % 4) || ((uintptr_t)z->marked % 4) || ((uintptr_t)z->least % 4) || ((uintptr_t)z->nearest % 4) ||
        ((uintptr_t)z->points % 4) || ((uintptr_t)z->roots % 4) || ((uintptr_t)z->n_zones % 4)) return MS_EINVAL;
    if ((long long)grid->n_envs*z->n_fields > 0x7fffffffLL/(2*z->max_zones)) return MS_EUNSUPPORTED;
    return MS_OK;
}
static NavZoneArgs nav_zone_args(const MsNavZones* z) {
    return NavZoneArgs{z->labels, z->values, z->marks, z->mask, z->cells, z->marked, z->least, z->nearest, z->points, z->roots, z->n_zones,
                       z->n_fields, z->n_labels, z->values ? z->n_values : 1, z->marks ? z->n_marks : 1, z->marks ? z->where : 1,
                       z->within_marks, z->ranked, z->max_zones};
}

int ms_nav_zones(const MsNavGrid* grid, const MsNavZones* z, void* stream) {
    const int status = nav_zones_check(grid, z);
    if (status != MS_OK) return status;
    hipLaunchKernelGGL(nav_zone_kernel, dim3((unsigned)((long long)grid->n_envs*z->n_fields)), dim3(ZONE_THREADS), 0, (hipStream_t)stream,
                       nav_args(grid), nav_zone_args(z));
    return launch_status();
}

int ms_host_nav_zones(const MsNavGrid* grid, const MsNavZones* z) {
    const int status = nav_zones_check(grid, z);
    if (status != MS_OK) return status;
    zone_serial(nav_args(grid), nav_zone_args(z));
    return MS_OK;
}

// View fields (navview.h): the same discipline.  An env of more than 2^30 cells cannot be (MsNavGrid's geom is 32768 a side at most
// in cuda.nav_grid; here it is max_framed, an int, that bounds it).
static int nav_views_check(const MsNavGrid* grid, const MsNavViews* v) {
    if (!nav_grid_ok(grid) || !v || v->n_points < 1 || !v->points || !v->countable || (!v->values && !v->counts && !v->gains) ||
        !(v->max_range > 0.f) || !(v->max_range < INFINITY) || (v->headings && !(v->cos_half >= -1.f && v->cos_half <= 1.f)) ||
        (v->gains && !v->unseen) || (v->unseen && v->n_maps < 1) ||
        (v->unseen && !v->slot && v->n_maps != 1 && v->n_maps != v->n_points) || ((uintptr_t)v->points % 8) || ((uintptr_t)v->headings % 8) ||
        ((uintptr_t)v->slot % 4) || ((uintptr_t)v->counts % 4) || ((uintptr_t)v->gains % 4)) return MS_EINVAL;
    if ((long long)grid->n_envs*v->n_points > 0x7fffffffLL || grid->max_framed > (1 << 30)) return MS_EUNSUPPORTED;
    return MS_OK;
}
static NavViewArgs nav_view_args(const MsNavViews* v, const int capacity) {
    return NavViewArgs{v->points, v->headings, v->mask, v->countable, v->unseen, v->unseen ? v->slot : nullptr, v->values, v->counts, v->gains,
                       v->n_points, v->unseen ? v->n_maps : 0, capacity, v->max_range, v->max_range*v->max_range, v->headings ? v->cos_half : 0.f};
}

int ms_nav_views(const MsScenery* sc, const MsNavGrid* grid, const MsNavViews* v, void* stream) {
    if (!scenery_ok(sc) || !nav_grid_ok(grid) || grid->n_envs != sc->n_envs) return MS_EINVAL;
    const int status = nav_views_check(grid, v);
    if (status != MS_OK) return status;
    hipLaunchKernelGGL(nav_view_kernel, dim3((unsigned)((long long)grid->n_envs*v->n_points)), dim3(WG), 0, (hipStream_t)stream, *sc, nav_args(grid),
                       nav_view_args(v, VIEW_WALL_CAPACITY));
    return launch_status();
}

int ms_host_nav_views(const MsNavGrid* grid, const MsNavViews* v, const float* walls, const long long* wall_starts, int capacity) {
    const int status = nav_views_check(grid, v);
    if (status != MS_OK) return status;
    if (!walls || !wall_starts || capacity > VIEW_WALL_CAPACITY) return MS_EINVAL;
    view_serial(nav_args(grid), nav_view_args(v, capacity > 0 ? capacity : VIEW_WALL_CAPACITY), reinterpret_cast<const float4*>(walls), wall_starts);
    return MS_OK;
}

int ms_host_nav_view_capacity(void) { return VIEW_WALL_CAPACITY; }

// Percepts (percept.h): the same discipline.  The limits keep a lane's points within sixteen and a round's key within a lane.
static int percepts_check(const MsPercepts* p) {
    if (!p || p->n_eyes < 1 || p->n_eyes > PERCEPT_MAX_EYES || p->n_points < 1 || p->n_points > PERCEPT_MAX_POINTS || p->n_nearest < 0 ||
        p->n_nearest > PERCEPT_MAX_NEAREST || !p->eyes || !p->points || !(p->max_range > 0.f) || !(p->max_range < INFINITY) ||
        (p->headings && !(p->cos_half >= -1.f && p->cos_half <= 1.f)) || p->pairs_shape < 0 || p->pairs_shape > 2 ||
        (p->pairs != nullptr) != (p->pairs_shape != 0) ||
        (!p->visible && !p->squares && !p->offsets && !p->counts && !p->nearest && !p->near_offsets && !p->near_distances) ||
        ((uintptr_t)p->eyes % 8) || ((uintptr_t)p->headings % 8) || ((uintptr_t)p->points % 8) || ((uintptr_t)p->offsets % 8) ||
        ((uintptr_t)p->near_offsets % 8) || ((uintptr_t)p->squares % 4) || ((uintptr_t)p->counts % 4) || ((uintptr_t)p->nearest % 4) ||
        ((uintptr_t)p->near_distances % 4)) return MS_EINVAL;
    return MS_OK;
}
static PerceptArgs percept_args(const MsPercepts* p, const int capacity) {
    return PerceptArgs{p->eyes, p->headings, p->points, p->valid, p->pairs, p->mask, p->visible, p->squares, p->offsets, p->counts, p->nearest,
                       p->near_offsets, p->near_distances, p->n_eyes, p->n_points, p->n_nearest, p->pairs_shape == 2 ? 1 : 0, capacity,
                       p->max_range, p->max_range*p->max_range, p->headings ? p->cos_half : 0.f};
}

int ms_percepts(const MsScenery* sc, const MsPercepts* p, void* stream) {
    if (!scenery_ok(sc)) return MS_EINVAL;
    const int status = percepts_check(p);
    if (status != MS_OK) return status;
    hipLaunchKernelGGL(percept_kernel, dim3((unsigned)sc->n_envs), dim3(WG), 0, (hipStream_t)stream, *sc, percept_args(p, VIEW_WALL_CAPACITY));
    return launch_status();
}

int ms_host_percepts(const MsPercepts* p, int n_envs, const float* walls, const long long* wall_starts, int capacity) {
    const int status = percepts_check(p);
    if (status != MS_OK) return status;
    if (n_envs < 1 || !walls || !wall_starts || capacity < 0 || capacity > VIEW_WALL_CAPACITY) return MS_EINVAL;
    percept_serial(percept_args(p, capacity > 0 ? capacity : VIEW_WALL_CAPACITY), n_envs, reinterpret_cast<const float4*>(walls), wall_starts);
    return MS_OK;
}

// Clearance (navclear.h): the same discipline.  CLEAR_DEFAULT_CULL is the instantiation ms_nav_clearance launches (DESIGN.md 3.23
// has the measurements that chose it); the other stays reachable through ms_debug_nav_clear_cull for A/B runs.
constexpr int CLEAR_DEFAULT_CULL = CLEAR_TILE_WAVE;
static int nav_clearance_check(const MsNavGrid* grid, const MsNavClearance* c) {
    if (!nav_grid_ok(grid) || !c || !(c->max_range > 0.f) || !(c->max_range < INFINITY) || c->n_radii < 0 || c->n_radii > CLEAR_MAX_RADII ||
        !c->values || (c->n_radii > 0) != (c->fits != nullptr) || ((uintptr_t)c->values % 4) || ((uintptr_t)c->nearest % 4) ||
        (grid->max_framed > 0 && c->max_tiles < 1)) return MS_EINVAL;
    for (int k = 0; k < c->n_radii; k++)
        if (!(c->radii[k] > 0.f) || !(c->radii[k] <= c->max_range)) return MS_EINVAL;
    if (grid->n_envs > 65535) return MS_EUNSUPPORTED;
    return MS_OK;
}
static ClearArgs nav_clear_args(const MsNavClearance* c, const int cull) {
    ClearArgs q{c->mask, c->values, c->nearest, c->fits, c->n_radii, cull, c->max_range, c->max_range*c->max_range, {}};
    for (int k = 0; k < c->n_radii; k++) q.r2[k] = c->radii[k]*c->radii[k];
    return q;
}
static int nav_clear_query_check(const MsNavClearQuery* q) {
    if (!q || q->n_envs < 1 || q->n_points < 1 || !q->points || (!q->distances && !q->nearest && !q->towards) || !(q->max_range > 0.f) ||
        !(q->max_range < INFINITY) || ((uintptr_t)q->points % 8) || ((uintptr_t)q->towards % 8) || ((uintptr_t)q->skip % 4) ||
        ((uintptr_t)q->distances % 4) || ((uintptr_t)q->nearest % 4)) return MS_EINVAL;
    if ((long long)q->n_envs*q->n_points > 0x7fffffffLL) return MS_EUNSUPPORTED;
    return MS_OK;
}
static ClearQueryArgs nav_clear_query_args(const MsNavClearQuery* q, const bool with_agents) {
    return ClearQueryArgs{q->points, with_agents ? q->skip : nullptr, q->mask, q->distances, q->nearest, q->towards, q->n_points, with_agents ? 1 : 0,
                          (long long)q->n_envs*q->n_points, q->max_range*q->max_range};
}

int ms_nav_clearance(const MsScenery* sc, const MsNavGrid* grid, const MsNavClearance* c, void* stream) {
    if (!scenery_ok(sc) || !nav_grid_ok(grid) || grid->n_envs != sc->n_envs) return MS_EINVAL;
    const int status = nav_clearance_check(grid, c);
    if (status != MS_OK) return status;
    if (grid->max_framed == 0) return MS_OK;
    const int cull = g_nav_clear_cull < 0 ? CLEAR_DEFAULT_CULL : g_nav_clear_cull;
    const dim3 blocks((unsigned)c->max_tiles, (unsigned)grid->n_envs);
    if (cull == CLEAR_TILE_WAVE)
        hipLaunchKernelGGL(nav_clear_kernel<true>, blocks, dim3(WG), 0, (hipStream_t)stream, *sc, nav_args(grid), nav_clear_args(c, 1));
    else
        hipLaunchKernelGGL(nav_clear_kernel<false>, blocks, dim3(WG), 0, (hipStream_t)stream, *sc, nav_args(grid), nav_clear_args(c, cull != CLEAR_BRUTE));
    return launch_status();
}

int ms_nav_clear_query(const MsScenery* sc, const MsAgents* ag, const MsNavClearQuery* q, void* stream) {
    if (!scenery_ok(sc)) return MS_EINVAL;
    const int status = nav_clear_query_check(q);
    if (status != MS_OK) return status;
    if (q->n_envs != sc->n_envs || (ag && (!ag->angles || !ag->positions || ((uintptr_t)ag->positions % 8)))) return MS_EINVAL;
    const long long total = (long long)q->n_envs*q->n_points;
    hipLaunchKernelGGL(nav_clear_query_kernel, dim3((unsigned)((total + WAVES - 1)/WAVES)), dim3(WG), 0, (hipStream_t)stream, *sc, agents_or_none(ag),
                       nav_clear_query_args(q, ag != nullptr));
    return launch_status();
}

int ms_debug_nav_clear_cull(int mode) {
    if (mode < -1 || mode > CLEAR_TILE_WAVE) return MS_EINVAL;
    g_nav_clear_cull = mode;
    return MS_OK;
}

int ms_host_nav_clearance(const MsNavGrid* grid, const MsNavClearance* c, const float* walls, const long long* wall_starts, int flags) {
    const int status = nav_clearance_check(grid, c);
    if (status != MS_OK) return status;
    if (!walls || !wall_starts || flags < CLEAR_BRUTE || flags > CLEAR_TILE_WAVE) return MS_EINVAL;
    clear_serial(nav_args(grid), nav_clear_args(c, flags != CLEAR_BRUTE), reinterpret_cast<const float4*>(walls), wall_starts, 0, flags, &g_clear_folds,
                 &g_clear_pairs);
    return MS_OK;
}

long long ms_host_nav_clear_folds(long long* pairs) {
    if (pairs) *pairs = g_clear_pairs;
    return g_clear_folds;
}

int ms_host_nav_clear_chunk(void) { return OV_CHUNK; }

int ms_host_nav_clear_query(const MsNavClearQuery* q, const float* rows, const long long* row_starts, int n_agents, int n_model, int with_agents,
                            int flags) {
    const int status = nav_clear_query_check(q);
    if (status != MS_OK) return status;
    if (!rows || !row_starts || n_agents < 1 || n_model < 1 || flags < 0 || flags > 1) return MS_EINVAL;
    clear_query_serial(nav_clear_query_args(q, with_agents != 0), n_agents, n_model, reinterpret_cast<const float4*>(rows), row_starts, flags != 0);
    return MS_OK;
}

int ms_bake(const MsScenery* sc, const MsConfig* cfg, void* stream) {
    (void)cfg;
    if (!scenery_ok(sc) || !sc->textures_widths || !sc->textures_starts || !sc->textures_inverse ||
        !sc->baked_vals || !sc->lights_widths || !sc->lights_starts) return MS_EINVAL;
    if (sc->n_lights_total > 0 && !sc->lights_vals) return MS_EINVAL;
    if (sc->n_texels_total > 0 && sc->bake_vis &&
        (!sc->bake_vis_starts || sc->bake_vis_words < 0 || !sc->lines_inverse || ((uintptr_t)sc->bake_vis % 8))) return MS_EINVAL;
    if (sc->lg_vals && (!sc->lg_starts || !sc->lg_geom || !(sc->lg_cell > 0.f) || sc->lg_max_cells <= 0 || ((uintptr_t)sc->lg_vals % 16) ||
                        ((uintptr_t)sc->lg_geom % 16) || (sc->lg_list != nullptr) != (sc->lg_pool != nullptr) ||
                        (sc->lg_pool && sc->lg_pool_size < 1) || (sc->lg_pool_rows && (!sc->lg_pool || ((uintptr_t)sc->lg_pool_rows % 16))) ||
                        ((uintptr_t)sc->lg_list % 8))) return MS_EINVAL;
    if (sc->n_texels_total > 0 && sc->bake_vis) {
        // two phases: visibility once per representative env and light, then the per-env sums
        const char* be = getenv("MEGASTEP_BAKE_BINS");                 // =0: every texel meets every wall (A/B runs)
        const bool bins = !(be && be[0] == '0');
        if (sc->n_lights_total > 0)
            hipLaunchKernelGGL(visibility_kernel, dim3(sc->n_lights_total), dim3(WG), 0, (hipStream_t)stream, *sc, bins ? 1 : 0);
        const long long blocks = ((long long)sc->n_texels_total + WG - 1)/WG;
        hipLaunchKernelGGL(bake_sum_kernel, dim3((unsigned)blocks), dim3(WG), 0, (hipStream_t)stream, *sc);
    } else if (sc->n_texels_total > 0) {
        hipLaunchKernelGGL(bake_kernel, dim3(sc->n_envs), dim3(WG), 0, (hipStream_t)stream, *sc);
    }
    if (sc->lg_vals) {
        const dim3 cells((sc->lg_max_cells + WG - 1)/WG, sc->n_envs);
        hipLaunchKernelGGL(lightgrid_kernel, cells, dim3(WG), 0, (hipStream_t)stream, *sc);
        if (sc->lg_list) {
            if (hipMemsetAsync(sc->lg_pool, 0, sizeof(unsigned), (hipStream_t)stream) != hipSuccess) return hip_fail(hipGetLastError());
            hipLaunchKernelGGL(lightlist_kernel, cells, dim3(WG), 0, (hipStream_t)stream, *sc);
        }
    }
    return launch_status();
}

}  // extern "C"
