// megastep_hip.hip -- gfx950 (MI355X / CDNA4) simulation core behind include/megastep_hip.h.
//
// One translation unit: this file holds the constants, the switches and the probe macros, and includes the rest, a family a file:
//   kernels/*.h   the kernels, inside the anonymous namespace: math.h (scalar helpers shared with the ms_host_* test hooks)
//                 first, step.h (what the step kernels share: physics, slide, rollout, scenario) behind it, culltest.h (the
//                 ms_test_* probes of the culls) last;
//   host/*.h      the host side of the C-ABI - argument checks, argument structs, launches, the ms_host_* / ms_test_* /
//                 ms_debug_* hooks: common.h (what every family shares) first, then a file a family as under kernels/.
//
// Thirty-four kernels, all written wave64-first (DESIGN.md section 3 has the full story of each):
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
//   item_collect_kernel, item_overlay_kernel   items: a wave an env takes the items in an agent's reach - a lane the items
//                   lane + 64 j, the agents at uniform addresses, the walls walked only where a ballot finds an item in reach - and
//                   settles timers, due flags and per-kind counts; a workgroup an origin builds the items' billboards once into
//                   LDS and folds each of its rays over them by raycast_kernel's own ray_fold, over the planes a render or a
//                   raycast wrote.   (no counterpart)
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
#include "kernels/step.h"
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
#include "kernels/items.h"
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

}  // namespace

// The host side of the C-ABI: each file keeps its helpers in the anonymous namespace and its entries extern "C".
#include "host/common.h"
#include "host/probes.h"
#include "host/wallgrid.h"
#include "host/step.h"
#include "host/render.h"
#include "host/envlogic.h"
#include "host/rays.h"
#include "host/nav.h"
#include "host/navmaps.h"
#include "host/navsets.h"
#include "host/sight.h"
#include "host/items.h"
#include "host/bake.h"
