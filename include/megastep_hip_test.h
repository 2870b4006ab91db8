/* megastep_hip_test.h -- what libmegastep_hip.so exports for its own test suite and A/B runs, on top of megastep_hip.h:
 * host instantiations of the device functions the kernels cull with (so that the CPU suite can check every cull against
 * the oracle without a GPU), and debug switches.  Nothing here is part of the drop-in boundary. */
#ifndef MEGASTEP_HIP_TEST_H
#define MEGASTEP_HIP_TEST_H
#include "megastep_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Host instantiation of render_kernel's pass 1 for one line (reference: the all-lines loop kernels.cu:352-377, which it
 * culls): pose = (x, y, sin, cos of the heading), line = (ax, ay, bx, by), `group` = which 64 rays of the agent's `res`:
 * rays first .. first + count - 1 of the group (0-based within it) are the only ones the kernel intersects with the line. */
void ms_host_ray_interval(const float* pose, const float* line, int res, float fov, float agent_radius, int group, int* first, int* count);
/* ... and for a wave that serves `groups` (1, 2, 4) groups of 64 rays (render_kernel's NG): `wave` = which run of 64 x groups
 * rays of the agent's; first / count within that run. */
void ms_host_ray_interval_wide(const float* pose, const float* line, int res, float fov, float agent_radius, int groups, int wave,
                               int* first, int* count);
/* Pins the number of 64-ray groups a render wave serves (1, 2, 4; 0 = ms_render picks it from the request: DESIGN 3.6).
 * Per calling THREAD (like every ms_debug_* switch: the library keeps no process-wide state - a thread that pins something
 * changes its own calls only); for A/B runs and tests - every setting produces the same bits. */
int ms_debug_ray_groups(int groups);
/* Pins the number of envs a physics wave takes side by side (physics_kernel's PACK; 0 = ms_step_physics picks it from the
 * world's size, 1 = one, k = k where k x n_agents <= 64 and there is a wall grid, else one).  Per calling thread; A/B runs and
 * tests - every setting produces the same bits. */
int ms_debug_physics_pack(int envs);
/* What the calling thread's last ms_render launched: the 64-ray groups per wave (render_kernel's NG: 1, 2, 4) it settled on -
 * the pins, the scenery (no light grid: one group), the build (A/B raycasts: one) and the device's wave slots all taken into
 * account, which a caller re-deriving the rule cannot know; 0 before the thread's first call.  bench.py labels its
 * lines with it. */
int ms_debug_last_render_groups(void);
/* Did the calling thread's last ms_step_render go out as one launch (1) or as ms_physics + ms_render (0)?  (ms_slide_physics
 * sets it to 0: a sliding step followed by ms_render is always two launches.) */
int ms_debug_last_step_fused(void);
/* The launch geometry ms_render / ms_step_physics decide on the host, and the render kernel's own block -> rays mapping
 * (render_block), for tests that walk whole launches on the CPU.  `slots`: the machine's wave slots for the render kernel (CUs x
 * 4 SIMDs x 6 waves; 6144 on MI355X); pinned_groups / tail_rounds / tail_envs as the ms_debug_* hooks (0 / < 0 / < 0: the rules).
 * ms_host_render_plan returns the number of one-wave blocks and the ray groups per wave; ms_host_render_block fills out4 =
 * (env, agent, first ray, rays) for block `block` and returns 1, or 0 for a spare block, -1 outside the launch.
 * ms_host_physics_pack: the envs a physics wave takes side by side. */
long long ms_host_render_plan(int n_envs, int n_agents, int res, int slots, int pinned_groups, float tail_rounds, int tail_envs, int* groups);
int ms_host_render_block(int n_envs, int n_agents, int res, int slots, int pinned_groups, float tail_rounds, int tail_envs, long long block, int* out4);
int ms_host_physics_pack(int n_envs, int n_agents, int gridded, int pinned);
/* The fan schedule (MsAgents.schedule): 0 = ms_step_physics sorts nothing and ms_render deals its waves in fan order whether the
 * agents carry a schedule or not, 1 = they use it where the shape qualifies.  Per calling thread; A/B runs and tests - either
 * setting produces the same bits. */
int ms_debug_render_order(int on);
/* Host mirror of the sort ms_step_physics' extra waves do, for CPU tests: order[slot] = fan for the n_fans = N A one-fan blocks
 * of a render launch, from costs[fan] (any 32-bit pattern: a cost's class is min((unsigned)cost, 63)).  XCD x's run of slots -
 * [x q + min(x, r), ...) with q = n_fans / 8, r = n_fans % 8, the first r runs one longer: render_block's - holds a permutation
 * of the same run of fans, classes descending.  (Fans of one class may come in another order on the device.)  Returns the
 * number of sort blocks the launch would carry. */
int ms_host_order_fans(int n_fans, const int* costs, int* order);
/* A launch of waves of several groups ends with waves of one group for its last envs; their share, in rounds of the machine's
 * wave slots' worth of the wide waves' work (< 0: ms_render's own, half a round; 0: none; large: every env), or, if
 * envs >= 0, that many envs exactly.  Per calling thread; A/B runs and tests - every setting produces the same bits. */
int ms_debug_ray_group_tail(float rounds, int envs);
/* Has ms_render's waves add their (line, ray) pair and pair-window counts to workspace[3] and [4] (two atomics per wave on
 * one address: milliseconds at 10^5 waves - tools/pair_stats.py only).  Per calling thread. */
int ms_debug_pair_telemetry(int on);
/* ms_overhead's tile cull: 0 makes every tile keep every line of its env (pass 1 keeps all), 1 (the default) culls.  Per
 * calling thread; tests - either setting produces the same bits. */
int ms_debug_overhead_cull(int on);
/* Host instantiation of ms_overhead's tile cull, for CPU tests: may line = (ax, ay, bx, by) cover any pixel of tile
 * (tile_row, tile_col) - 16 x 16 pixels, clipped to a height x width image - under view (g0..g5) at half width h?  1 = the
 * kernel keeps the line for that tile, 0 = it drops it. */
int ms_host_overhead_keeps(const float* view, int height, int width, int tile_row, int tile_col, float half_width, const float* line);
/* Host instantiations of the path rule's device functions (kernels/navpath.h: start, hop, sight) for ONE env and ONE query on
 * HOST arrays: geom = (jx0, iy0, nx, ny), free_cells and D (ny x nx, row-major) the env's free bytes and the goal's field,
 * goal and point (x, y).  ms_host_nav_waypoint writes the waypoint (NaN, NaN without a path) and returns the chosen index
 * (-1 without a path; -2: lookahead outside 1..64); ms_host_nav_path writes max_points x 2 floats (NaN in the slots not
 * written) and returns MsNavPaths' count (max_points < 2: 0, nothing written). */
int ms_host_nav_waypoint(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* goal,
                         const float* point, int lookahead, float* waypoint);
int ms_host_nav_path(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* goal,
                     const float* point, int max_points, float* points);
/* Host instantiations of the seeded fields (MsNavSeedFields) for ONE env on HOST arrays: geom, free_cells as above, marks
 * (ny x nx bytes: one field's), among (ny x nx bytes) or NULL.  ms_host_nav_seed_field seeds D (ny x nx, out) by the kernel's
 * own predicate and sweeps the kernel's own per-cell function over it, in place, until a sweep lowers nothing - framed != 0:
 * on a framed copy with the bytes the kernel keeps in LDS (nav_cell_framed), else on D as stored (nav_cell_stored, the
 * global-memory path); writes the number of seeds to n_seeds (or NULL) and returns the sweeps taken, 0 for an env without
 * cells, -1 for arguments ms_nav_seed_fields would refuse.  ms_host_nav_seed_waypoint / _path follow a seeded field D as
 * nav_waypoint_kernel / nav_path_kernel do, with the returns of ms_host_nav_waypoint / ms_host_nav_path. */
int ms_host_nav_seed_field(const int* geom, float cell, const unsigned char* free_cells, const unsigned char* marks, int where,
                           const unsigned char* among, int framed, float* D, int* n_seeds);
int ms_host_nav_seed_waypoint(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* point,
                              int lookahead, float* waypoint);
int ms_host_nav_seed_path(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* point,
                          int max_points, float* points);
/* ms_host_nav_field_capacity writes the three capacities, in framed cells, of nav_relax_kernel's instantiations (single-goal and
 * seeded alike): MS_OK, or MS_EINVAL for NULL. */
int ms_host_nav_field_capacity(int* capacities);
/* Host instantiations of the cost fields (MsNavCostFields) for ONE env on HOST arrays: ms_host_nav_seed_field / _waypoint / _path
 * with `costs` (ny x nx floats: one field's) - the kernel's own multiplier and weights, a cell's multiplier kept beside the framed
 * copy (framed != 0, as the kernel's LDS variant keeps it) or read from `costs` every sweep (the global-memory path, and the other
 * variant); the followers hop with the weights of the cell they leave.  Returns as the seeded hooks', -1 also for NULL costs.
 * ms_host_nav_cost_capacity writes the three capacities, in framed cells, of the instantiations that keep the multipliers in LDS
 * (a float, a float and a byte a cell): MS_OK, or MS_EINVAL for NULL.
 * ms_debug_nav_cost_variant: where ms_nav_cost_fields' launch keeps the multipliers - 0 = read from global memory every pass (the
 * seeded kernel's capacities, ms_host_nav_field_capacity), 1 = in LDS (ms_host_nav_cost_capacity); -1 = the library's own choice;
 * anything else: MS_EINVAL.  Per calling thread; A/B runs and tests - every setting produces the same bits. */
int ms_host_nav_cost_field(const int* geom, float cell, const unsigned char* free_cells, const unsigned char* marks, int where,
                           const unsigned char* among, const float* costs, int framed, float* D, int* n_seeds);
int ms_host_nav_cost_waypoint(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* costs,
                              const float* point, int lookahead, float* waypoint);
int ms_host_nav_cost_path(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* costs,
                          const float* point, int max_points, float* points);
int ms_host_nav_cost_capacity(int* capacities);
int ms_debug_nav_cost_variant(int variant);
/* The pulled paths' rule (MsNavPulls) stated serially over the path rule's own functions (kernels/navpull.h: nav_pull_serial over
 * nav_start, nav_hop and nav_sight) for ONE env and ONE query on HOST arrays: geom, free_cells, D and point as above; goal (x, y),
 * or NULL for a seeded field; costs (ny x nx floats), or NULL for unweighted hops.  Writes max_points x 2 floats to vertices (NaN
 * in the slots not written), max_points ints to indices (or NULL; -1 beyond) and the length (+inf without a path); returns
 * MsNavPulls' counts.  -2: reach outside 1..1024; max_points outside 2..2^20, a NULL vertices or length: 0, nothing written.
 * ms_debug_nav_pull_scheme: how ms_nav_pulls' waves test a window's sights - 0 = a lane a candidate, each walking its own samples;
 * 1 = candidate after candidate, its samples a lane each (the waypoint kernel's scheme); -1 = the library's own choice (0);
 * anything else: MS_EINVAL.  Per calling thread; A/B runs and tests - either setting produces the same bits. */
int ms_host_nav_pull(const int* geom, float cell, const unsigned char* free_cells, const float* D, const float* goal,
                     const float* costs, const float* point, int reach, int max_points, float* vertices, int* indices,
                     float* length);
int ms_debug_nav_pull_scheme(int scheme);
/* Host instantiation of the seen maps' rule (kernels/navseen.h: the ray, the sample - the very functions every lane of
 * nav_seen_kernel evaluates) for ONE env on HOST arrays, one call of ms_nav_seen: geom = (jx0, iy0, nx, ny), countable
 * (ny x nx bytes), origins (P, 2), dirs (P, R, 2), distances (P, R), slot (P) or NULL (then P == S), reset (S) or NULL, maps
 * (S, ny, nx) in / out, gained (S) out and total (S) in / out, either or NULL.  Returns 0, or -1 for arguments ms_nav_seen
 * would refuse.  An env without cells (nx*ny <= 0) marks nothing and gains 0. */
int ms_host_nav_seen(const int* geom, float cell, const unsigned char* countable, int n_maps, int n_viewers, int n_rays,
                     const float* origins, const float* dirs, const float* distances, const int* slot, float max_range,
                     const unsigned char* reset, unsigned char* maps, int* gained, int* total);
/* Host instantiation of the age maps' rule (kernels/navage.h over navseen.h's ray and sample - the very functions every lane of
 * nav_age_kernel evaluates - with a call's marks as the kernel's bitmask, and the merge and the survey stated serially) for ONE
 * env on HOST arrays, one call of ms_nav_ages: geom = (jx0, iy0, nx, ny); every pointer of `ages` is host memory and holds the
 * one env's share - countable (ny x nx bytes, required), origins (P, 2), dirs (P, R, 2), distances (P, R), slot (P), reset (S),
 * last, stale and ages (S, ny, nx), clock and the counts (S); max_cells is not read.  Returns what ms_nav_ages would: MS_OK,
 * MS_EINVAL for arguments it would refuse (a NULL countable too), MS_EUNSUPPORTED for more than 2^20 cells. */
int ms_host_nav_ages(const int* geom, float cell, const MsNavAges* ages);
/* Host instantiation of the map windows' rule (kernels/navwindow.h: the sample point, the cell, the channel value and the
 * pixel's sum - the very functions every lane of nav_window_kernel evaluates) for one whole call of ms_nav_windows on HOST
 * arrays: every pointer of `grid` (geom, starts; free_cells is checked, not read) and of `windows` (views, the layers' values and
 * fields, out) is host memory.  Returns what ms_nav_windows would: MS_OK, or MS_EINVAL for arguments it would refuse. */
int ms_host_nav_windows(const MsNavGrid* grid, const MsNavWindows* windows);
/* Host instantiation of the cell draws' rule (kernels/navdraw.h: the predicate, the hash, the rank and the n-th-set-bit select -
 * the very functions every lane of nav_draw_kernel evaluates) for one whole call of ms_nav_draws on HOST arrays, swept serially:
 * every pointer of `grid` and of `draws` is host memory.  Returns what ms_nav_draws would: MS_OK, MS_EINVAL for arguments it
 * would refuse, MS_EUNSUPPORTED for more than 2^20 cells an env. */
int ms_host_nav_draws(const MsNavGrid* grid, const MsNavDraws* draws);
/* Host instantiations of the regions' rule (kernels/navregion.h: the open test, the fill, one cell's lowered and jumped value,
 * the count at the roots, the area, the largest key, the anchor labels and the mask byte - the very functions every lane of
 * nav_region_kernel, nav_region_query_kernel and nav_region_mask_kernel evaluates) for one whole call each on HOST arrays, swept
 * serially: every pointer of `grid` and of the argument struct is host memory.  ms_host_nav_regions labels a field on a framed
 * copy when it fits the LDS of the launch ms_nav_regions would choose by grid->max_framed, else in its `labels` store - the
 * kernel's two paths.  They return what the device entries would: MS_OK, or MS_EINVAL for arguments they would refuse.
 * ms_host_nav_region_capacity writes the three capacities, in framed cells, of nav_region_kernel's instantiations. */
int ms_host_nav_regions(const MsNavGrid* grid, const MsNavRegions* regions);
int ms_host_nav_region_query(const MsNavGrid* grid, const MsNavRegionQuery* query);
int ms_host_nav_region_masks(const MsNavGrid* grid, const MsNavRegionMasks* masks);
int ms_host_nav_region_capacity(int* capacities);
/* Host instantiations of the basins' rule (kernels/navbasin.h: a cell's successor through nav_hop, the jump, the label, the anchor
 * nav_start picks and a point's marks - the very functions every lane of nav_basin_kernel, nav_basin_query_kernel and
 * nav_point_mark_kernel evaluates) for one whole call each on HOST arrays, swept serially: every pointer of `grid` and of the
 * argument struct is host memory.  ms_host_nav_basins jumps in a copy of the successors when the env fits the LDS of the launch
 * ms_nav_basins would choose by grid->max_framed, else in its `labels` store - the kernel's two paths.  They return what the device
 * entries would: MS_OK, or MS_EINVAL for arguments they would refuse.  ms_host_nav_basin_capacity writes the three capacities, in
 * cells, of nav_basin_kernel's instantiations. */
int ms_host_nav_basins(const MsNavGrid* grid, const MsNavBasins* basins);
int ms_host_nav_basin_query(const MsNavGrid* grid, const MsNavBasinQuery* query);
int ms_host_nav_point_marks(const MsNavGrid* grid, const MsNavPointMarks* marks);
int ms_host_nav_basin_capacity(int* capacities);
/* Host instantiation of the zones' rule (kernels/navzone.h: the root test, the rank of a label in the list of roots, a cell's zone,
 * its mark, its key and a zone's stores - the very functions every lane of nav_zone_kernel evaluates) for one whole call of
 * ms_nav_zones on HOST arrays, swept serially: every pointer of `grid` and of `zones` is host memory.  Returns what ms_nav_zones
 * would: MS_OK, or MS_EINVAL for arguments it would refuse. */
int ms_host_nav_zones(const MsNavGrid* grid, const MsNavZones* zones);
/* Host instantiation of the view fields' rule (kernels/navview.h: view_in_range, view_in_cone, view_wall_blocks, the window and the
 * wall cull - the very functions every lane of nav_view_kernel evaluates) for one whole call of ms_nav_views on HOST arrays, swept
 * serially: every pointer of `grid` and of `views` is host memory, and in place of an MsScenery `walls` holds the STATIC rows of all
 * envs, four floats each, env n's rows wall_starts[n] .. wall_starts[n + 1] - 1.  It goes through the kernel's window and cull, and
 * through both wall paths: a viewpoint that keeps more than `capacity` rows (0: the kernel's, ms_host_nav_view_capacity(); a smaller
 * one lets a test reach the other path with few walls) sweeps all its env's rows instead of the staged ones.  Returns what
 * ms_nav_views would: MS_OK, or MS_EINVAL for arguments it would refuse (and for a capacity above the kernel's). */
int ms_host_nav_views(const MsNavGrid* grid, const MsNavViews* views, const float* walls, const long long* wall_starts, int capacity);
int ms_host_nav_view_capacity(void);
/* Host instantiation of the percepts' rule (kernels/percept.h over kernels/navview.h: the eye, the candidate, view_wall_blocks, the
 * wall cull, the box of a wave's 64 points, the key of the nearest and the stores - the very functions every lane of percept_kernel
 * evaluates) for one whole call of ms_percepts on HOST arrays, swept serially: every pointer of `percepts` is host memory, and in
 * place of an MsScenery there are n_envs and `walls`, the STATIC rows of all envs, four floats each, env n's rows wall_starts[n] ..
 * wall_starts[n + 1] - 1.  It goes through both wall paths: an env that keeps more than `capacity` rows (0: the kernel's,
 * ms_host_nav_view_capacity(); a smaller one lets a test reach the other path with few walls) sweeps all its rows instead of the
 * staged ones.  Returns what ms_percepts would: MS_OK, or MS_EINVAL for arguments it would refuse (and for n_envs < 1, NULL walls
 * or a capacity above the kernel's). */
int ms_host_percepts(const MsPercepts* percepts, int n_envs, const float* walls, const long long* wall_starts, int capacity);
/* Host instantiations of the items' rule (kernels/items.h: the reach test over view_wall_blocks, the key, the settling of an item
 * and its stores; the billboard, ray_fold itself, the winner's closing lines and its stores - the very functions every lane of
 * item_collect_kernel and item_overlay_kernel evaluates) for one whole call each on HOST arrays, swept serially: every pointer of
 * the argument struct is host memory.  ms_host_item_collect: in place of an MsScenery and an MsAgents there are n_envs, n_agents,
 * `agent_positions` (N, A, 2) and `walls`, the STATIC rows of all envs, four floats each, env n's rows wall_starts[n] ..
 * wall_starts[n + 1] - 1.  ms_host_item_overlay: in place of an MsScenery there are n_envs and `lines_widths` (N,), each env's
 * number of lines (agents' rows included; NULL is allowed where `indices` is).  They return what the device calls would: MS_OK, or
 * MS_EINVAL / MS_EUNSUPPORTED for arguments those would refuse (and for n_envs < 1, n_agents outside 1 .. 64, a NULL
 * agent_positions, walls or wall_starts, or `indices` without lines_widths). */
int ms_host_item_collect(const MsItemCollect* collect, int n_envs, int n_agents, const float* agent_positions, const float* walls,
                         const long long* wall_starts);
int ms_host_item_overlay(const MsItemOverlay* overlay, int n_envs, const int* lines_widths);
/* Host instantiations of the clearance rule (kernels/navclear.h: the tile's box, the list, ov_keeps and ov_fold, the second cull,
 * the winner's order and the stores - the very functions every lane of nav_clear_kernel and nav_clear_query_kernel evaluates) for
 * one whole call each on HOST arrays, swept serially: every pointer of `grid` and of the argument struct is host memory.
 * ms_host_nav_clearance: in place of an MsScenery `walls` holds the STATIC rows of all envs, four floats each, env n's rows
 * wall_starts[n] .. wall_starts[n + 1] - 1, and `nearest` numbers them from 0 within their env (the device's index less
 * n_agents*n_model).  It goes through the kernel's 16 x 16 tiles, its windows of 256 rows and its list of
 * ms_host_nav_clear_chunk() rows, folded and emptied when it could overflow.  flags: 0 = no cull (every tile keeps every row:
 * brute force), 1 = the tile cull, 2 = the tile cull and the second cull, emulated over the same 16 x 4 groups of cells and the
 * same runs of 64 list rows in the same order.  ms_host_nav_clear_folds: the (cell, row) pairs the calling thread's last
 * ms_host_nav_clearance folded, and into *pairs (or NULL) all the pairs there were.
 * ms_host_nav_clear_query: `rows` holds ALL rows of all envs as the query is to meet them - the n_agents*n_model agent rows of an
 * env first, at whatever poses the caller drew them (the host draws none), env n's rows row_starts[n] .. row_starts[n + 1] - 1;
 * with_agents = 0 passes over them as a query without agents does.  flags: 0 = one serial fold, 1 = the rows dealt to 64 bests as
 * the kernel's lanes stride them, merged by the kernel's butterfly.
 * Both return what the device entries would: MS_OK, or MS_EINVAL for arguments they would refuse (and for NULL rows or flags out
 * of range).
 * ms_debug_nav_clear_cull: which culls ms_nav_clearance's launch runs - 0, 1, 2 as the flags above; -1 = the library's own choice.
 * Per calling thread; A/B runs and tests - every setting produces the same bits. */
int ms_host_nav_clearance(const MsNavGrid* grid, const MsNavClearance* clearance, const float* walls, const long long* wall_starts, int flags);
long long ms_host_nav_clear_folds(long long* pairs);
int ms_host_nav_clear_chunk(void);
int ms_host_nav_clear_query(const MsNavClearQuery* query, const float* rows, const long long* row_starts, int n_agents, int n_model,
                            int with_agents, int flags);
int ms_debug_nav_clear_cull(int mode);
/* The kernels' arithmetic shortcuts against what they stand for, element by element on the device (DEVICE pointers, `count`
 * elements each): q_inrange[i] = div_inrange(n[i], d[i]) - the division without range scaling the render kernel uses where its
 * operands are in range by construction (kernels/math.h) - next to q_ieee[i] = n[i] / d[i] as the compiler expands a correctly
 * rounded division; r_any[i] = sqrt_any(x[i]) next to r_ieee[i] = sqrtf(x[i]).  tests/test_gpu_numerics.py holds them against
 * each other bit for bit over the ranges the call sites guarantee.  Any output pointer may be NULL. */
int ms_test_arithmetic(const float* n, const float* d, float* q_inrange, float* q_ieee, const float* x, float* r_any, float* r_ieee,
                       long long count, void* hip_stream);
/* The DEVICE builds of the culls and shortcuts whose device text is not the host's (v_rcp_f32 for a division, one refined
 * reciprocal for two divisions, sign tests for two quotients), element by element (kernels/culltest.h): each evaluates the very
 * functions the product kernels call on `count` elements - DEVICE pointers, one element a lane; rows of 4 floats are (count, 4),
 * points (count, 2).  Any output pointer may be NULL; MS_EINVAL for a NULL input, a negative count or (ms_test_ray_interval) a
 * shape no render launch has.  tests/test_gpu_culls.py holds them to the oracle at their thresholds.
 *   ms_test_agents_apart   apart[i] = agents_apart(me[i], other[i], radius[i]): ms_host_agents_apart's arguments.
 *   ms_test_wall_beyond    reach[i] = wall_reach(agent[i], radius[i]), beyond[i] = wall_beyond(agent[i], wall[i], reach_squared(reach[i])):
 *                          ms_host_wall_reach's and ms_host_wall_beyond_reach's arguments.
 *   ms_test_ray_interval   first[i], rays[i] = agent_frame + ray_interval of line[i] from pose[i] = (x, y, sin, cos) for wave `wave` of
 *                          64 x groups rays: ms_host_ray_interval_wide's arguments, the launch-invariant values formed by the same code.
 *   ms_test_wedge          wa[i], wb[i] = wg_wedge(pseudo_angle_fast(right[i]), pseudo_angle_fast(left[i])): the run of steps of a wave
 *                          whose rightmost / leftmost ray point along right[i] / left[i], as render_kernel forms it.
 *   ms_test_cell_at        index[i], inside[i] = wg_cell_at(geom[i] = (x0, y0, nx, ny), cell[i], point[i]).
 *   ms_test_tex_filter     l[i], r[i], lw[i], rw[i] = tex_filter(x[i], w[i]).
 *   ms_test_light_blocked  blocked[i] = light_blocked(I = light[i], U = to[i], a[i], v[i]): does the wall (a, a + v) stand between the
 *                          light and the point I + U? */
int ms_test_agents_apart(const float* me, const float* other, const float* radius, unsigned char* apart, long long count, void* hip_stream);
int ms_test_wall_beyond(const float* agent, const float* wall, const float* radius, float* reach, unsigned char* beyond, long long count,
                        void* hip_stream);
int ms_test_ray_interval(const float* pose, const float* line, int res, float fov, float agent_radius, int groups, int wave, int* first,
                         int* rays, long long count, void* hip_stream);
int ms_test_wedge(const float* right, const float* left, int* wa, int* wb, long long count, void* hip_stream);
int ms_test_cell_at(const float* geom, const float* cell, const float* point, int* index, unsigned char* inside, long long count,
                    void* hip_stream);
int ms_test_tex_filter(const float* x, const int* w, int* l, int* r, float* lw, float* rw, long long count, void* hip_stream);
int ms_test_light_blocked(const float* light, const float* to, const float* a, const float* v, unsigned char* blocked, long long count,
                          void* hip_stream);
/* Host instantiation of the light grid's build (ms_bake; accelerates kernels.cu:238-268) for one cell c (row-major in a grid
 * of nx x ny cells of size `cell` from (ox, oy)), over n_walls walls (n_walls x 4 floats: ax, ay, bx, by) and n_lights
 * lights (n_lights x 3: x, y, intensity), HOST memory: words[4] = the lights' 2-bit verdicts as in lg_vals (0 unknown, 1 lit,
 * 2 dark); candidates = the (light, wall) pairs of the cell's list as in lg_pool (0x80000000 | light << 24 | wall), at most
 * max_candidates of them written; returns how many there are. */
int ms_host_lightgrid_cell(const float* walls, int n_walls, const float* lights, int n_lights, float ox, float oy, int nx, int ny,
                           float cell, int c, unsigned* words, unsigned* candidates, int max_candidates);
/* Host restatement of how render_kernel's pass 2 settles a ray's nearest hit (reference: the order-dependent fold
 * kernels.cu:369-376): the n_hits hits (s[i] > near plane, line[i]) go through the kernel's three key slots in the order
 * `order` (a permutation of 0..n_hits-1), 64 to a window, lockstep within a window as a wavefront plays them.  Returns 1
 * when the slots cannot tell (the kernel then redoes the ray by the literal fold), else 0 with the hit in *nearest_s /
 * *nearest_line (-1: none). */
int ms_host_fold_hits(const float* s, const int* line, int n_hits, const int* order, float* nearest_s, int* nearest_line);
/* Host instantiation of ms_physics' reach cull in front of the agent-agent collision test (reference: kernels.cu:119-133,
 * 193-200), for CPU tests: me, other = (x, y, vx/fps, vy/fps); 1 = the pair cannot collide this step, the test is skipped. */
int ms_host_agents_apart(const float* me, const float* other, float agent_radius);
/* ... and of the reach cull in front of the agent-wall test (kernels.cu:135-171,202-205): agent = (x, y, vx/fps, vy/fps),
 * wall = (ax, ay, bx, by); 1 = the wall is beyond the agent's reach this step, the test is skipped.  (The host evaluates the
 * foot of the perpendicular with a true division, the kernel with v_rcp_f32: this is NOT the device's arithmetic.  The device's
 * verdicts are probed by ms_test_wall_beyond, at the threshold this one bisects to: tests/test_gpu_culls.py.) */
int ms_host_wall_beyond_reach(const float* agent, const float* wall, float agent_radius);
/* ... and the reach itself, which also picks the tier of the cell's near list (wg_reach_lo, wg_reach) or the sweep. */
float ms_host_wall_reach(const float* agent, float agent_radius);
/* Host instantiation of the movement prologue (kernels/physics.h: move_velocity), for CPU tests: delta = (dx, dy, dw), v (2 floats)
 * and w in / out.  Its sine and cosine are the host libm's, which need not round as torch's or the device's do. */
void ms_host_move_velocity(float keep, float ang, const float* delta, float* v, float* w);
/* The rollouts' rule (MsRollouts) stated serially over the kernel's own per-step functions (kernels/rollout.h) for ONE env on HOST
 * arrays: `walls` the env's n_walls STATIC rows, four floats each; every pointer of `agents` ((A,) and (A, 2) arrays; headings and
 * schedule are not read) and of `rollouts` is host memory and holds the one env's share - actions (A, K, H), or (K, H) with
 * shared_plans; mask (A,) or NULL; the outputs (A, K, ..).  There is no wall grid on the host: every candidate meets every wall,
 * behind the reach cull.  Returns what ms_rollouts would: MS_OK, MS_EINVAL for arguments it would refuse (and for NULL walls with
 * n_walls > 0, n_agents < 1). */
int ms_host_rollouts(const float* walls, int n_walls, const MsAgents* agents, int n_agents, const MsRollouts* rollouts,
                     const MsConfig* config);
/* The scenarios' rule (MsScenarios) stated serially over the kernel's own per-step functions (kernels/scenario.h, kernels/rollout.h)
 * for ONE env on HOST arrays, as ms_host_rollouts: `walls` the env's n_walls STATIC rows; every pointer of `agents` and of
 * `scenarios` is host memory and holds the one env's share - joint actions (S, A, H), focal (A, K, H) or shared (K, H), base
 * (A, H); mask (1,) joint, (A,) focal, or NULL; the outputs (S, A, ..) or (A, K, ..).  Every agent meets every other agent and
 * every wall, behind the reach culls.  Returns what ms_scenarios would: MS_OK, MS_EINVAL for arguments it would refuse (and
 * for NULL walls with n_walls > 0, n_agents < 1), MS_EUNSUPPORTED for more than 64 agents. */
int ms_host_scenarios(const float* walls, int n_walls, const MsAgents* agents, int n_agents, const MsScenarios* scenarios,
                      const MsConfig* config);
/* ms_debug_rollout_scheme: how ms_rollouts' waves meet a step's walls - 0 = a lane a candidate, each walking the near list of its
 * own cell; 1 = physics_kernel's scheme: a lane a wall, the wave's candidates one after another, the surviving pairs compacted in
 * LDS before the exact test; -1 = the library's own choice (1 up to 24 candidates an agent, else 0); anything else: MS_EINVAL.  Per calling thread; A/B runs and tests -
 * either setting produces the same bits. */
int ms_debug_rollout_scheme(int scheme);
/* The sliding step (MsSlide) stated serially over the kernel's own per-agent functions (kernels/slide.h) for n_envs whole envs on
 * HOST arrays: `walls` holds the STATIC rows of all envs, four floats each, env n's rows wall_starts[n] .. wall_starts[n + 1] - 1;
 * every pointer of `agents` (headings and schedule are not read), `movement`, `extras` (either may be NULL), `slide` and
 * `progress` is host memory, shaped as ms_slide_physics'.  There is no wall grid on the host: every agent meets every row of its
 * env, behind the reach cull.  The movement and the IMU reading use the host libm's sine and cosine.  Returns what
 * ms_slide_physics would: MS_OK, MS_EINVAL for arguments it would refuse (and for NULL walls or wall_starts, n_envs < 1,
 * n_agents < 1), MS_EUNSUPPORTED for more than 64 agents an env. */
int ms_host_slide(const float* walls, const long long* wall_starts, int n_envs, int n_agents, const MsAgents* agents,
                  const MsMovement* movement, const MsStepExtras* extras, const MsSlide* slide, float* progress,
                  const MsConfig* config);
/* The serial host statement of ms_shade (kernels/shade.h), on HOST arrays: ray after ray through the per-ray
 * functions shade_kernel calls - the texel filter, the drawn row, the shadow test, the sum - the lights taken the plain way,
 * light after light against row after row.  Of `scenery` it reads n_envs, n_agents, n_model, lights_*, lines_vals / widths /
 * starts, textures_vals / widths / starts, model and baked_vals (host pointers, lines_vals and model 16-byte aligned); of
 * `agents` (NULL: agent rows are black) angles and positions.  Returns what ms_shade would for such arguments: MS_OK or
 * MS_EINVAL. */
int ms_host_shade(const MsScenery* scenery, const MsAgents* agents, const MsShade* query);
/* Host instantiation of the scan's test, for CPU tests: does wall o = (ax, ay, bx, by) hide wall w from every point of
 * the cell [x0, x1] x [y0, y1] (as ms_wallgrid_scan grows it) for near planes below `near_plane`? */
int ms_host_wall_hidden(float x0, float y0, float x1, float y1, const float* o, const float* w, float near_plane);
/* The scan's sort of a cell's occluders into sectors of directions (wallgrid_scan_kernel, WG_SECTORS): the run of sectors
 * [first, first + count) modulo 64 that occluder o touches as seen from the centre of the cell [x0, x1] x [y0, y1], and the one
 * sector target w's middle lies in - a target is only tried against the occluders of its sector, so whenever ms_host_wall_hidden
 * says o hides w from the cell, `sector` must be in o's run (tests/test_wallgrid.py). */
void ms_host_wall_sectors(float x0, float y0, float x1, float y1, const float* o, int* first, int* count, const float* w, int* sector);
/* ... and of the scan of one whole cell (c, row-major in a grid of nx x ny cells of size `cell` from (ox, oy)) over
 * n_walls walls (n_walls x 4 floats, HOST memory): vis[t] = 1 where wall t goes on the cell's vis list, close[t] = 2 / 1
 * where it is within reach_lo / reach of the cell. */
void ms_host_wallgrid_cell(const float* walls, int n_walls, float ox, float oy, int nx, int ny, float cell, int c,
                           float near_plane, float reach_lo, float reach, unsigned char* vis, unsigned char* close);

/* ... and of the arcs: the run of steps [*lo8, *hi8] (modulo 256) of directions wall w can be seen in from the cell; and
 * whether a wave whose rightmost / leftmost ray point along (right_x, right_y) / (left_x, left_y) would keep such a wall;
 * ms_host_wedge: that wave's own run of steps [*wa8, *wb8].  (The host takes pseudo_angle with a division, render_kernel
 * pseudo_angle_fast with v_rcp_f32: ms_test_wedge gives the device's run.) */
void ms_host_wall_arc(float x0, float y0, float x1, float y1, const float* w, int* lo8, int* hi8);
void ms_host_wedge(float right_x, float right_y, float left_x, float left_y, int* wa8, int* wb8);
int  ms_host_wedge_meets(float right_x, float right_y, float left_x, float left_y, int lo8, int hi8);

/* Scalar helper exported for tests: sin(pi x), cos(pi x) exactly as the kernels evaluate them. */
void ms_host_sincospi(float x, float* s, float* c);
/* Helpers exported for tests of ms_bake's culling (host instantiations of the device functions): the angular bin
 * (of MS_BAKE_BINS around a light) a point falls in, and the circular run of bins [first, first + count) a wall can
 * shadow.  A wall obstructs a point from the light (kernels.cu:238-259) only if the point's bin is in the wall's run. */
#define MS_BAKE_BINS 64
int  ms_host_bake_point_bin(float light_x, float light_y, float x, float y);   /* -1: undecidable, test every wall */
void ms_host_bake_wall_bins(float light_x, float light_y, float ax, float ay, float bx, float by, int* first, int* count);

#ifdef __cplusplus
}
#endif
#endif /* MEGASTEP_HIP_TEST_H */
