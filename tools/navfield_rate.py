"""What the distance fields cost on the MI355X, next to the torch formulation a user would otherwise write:

    python tools/navfield_rate.py [--envs 4096] [--distinct 1024] [--repeats 10] [--warmup 3] [--torch-envs 256] [--json out.json]
                                  [--only fields|query|torch|envs|expert|seen|frontier|window|draws|regions|views|basins|clearance|cost|ages|pulls|zones] [--large]

The world is the headline's: `--envs` envs over `--distinct` distinct synthetic floorplans, one agent each, one goal an env
from the spawn table.  Timed with HIP events around single calls after a warm-up, the median of the repeats reported:
  (a) cuda.distance_fields (ms_nav_fields) for all the goals, and the pass count of the slowest field;
  (b) one DistanceFields.at (ms_nav_query) of one point an env;
  (c) PointGoal(envs).step eager and replayed as a HIP graph, next to Explorer(envs).step;
  (t) the yardstick for (a): the same fields by torch - the grids padded to the largest plan, (N, H, W) tensors, eight
      shifted minimums a sweep, swept until nothing changes (checked every 16 sweeps: each check is a host round trip).  It
      runs on the first `--torch-envs` envs and is scaled to `--envs`; its fields are compared with the kernel's as bits -
      a third statement of the rule beside tests/test_navfield_host.nav_rule and the kernel.
  (e) the shortest-path expert: one DistanceFields.waypoints (ms_nav_waypoints) of one agent an env and one DistanceFields.paths
      (ms_nav_paths, 256 points a path); PointGoal(envs): expert() + step() eager and replayed as a HIP graph, next to step()
      alone; and from a 200-step rollout of PointGoal(64), under the expert and under the compass policy of the PointGoal tests
      (turn until the goal's straight line is ahead, then walk; one step in four random): arrivals, episodes, and the mean of
      (metres walked)/(walking distance at the episode's start) over the episodes that arrived.
  (s) the seen maps, at Explorer's shape - `--envs` envs x 1 agent x 256 rays: one SeenMaps.mark (ms_nav_seen) on a rendered
      frame - on maps that already hold the frame's cells (nothing to store), and with every map reset by the call (everything
      to clear and store) - next to the cuda.render launch that made the frame's distances; the torch formulation of the same
      rule on the same inputs (a padded (N, R, samples) index tensor, then a scatter and a second pass for the count), on the
      first `--torch-envs` envs and scaled, its maps and counts compared with the kernel's; FloorCoverage(envs).step eager
      and replayed as a HIP graph.
  (f) the frontier fields, at Explorer's shape: SeenMaps.frontier_fields (ms_nav_seed_fields) for `--envs` maps right after one
      marked frame, and again once the maps hold 80 % of the countable floor (every cell but a random fifth marked by hand),
      with the passes of the slowest field, next to cuda.distance_fields of one goal an env on the same grid; one seeded
      waypoints call of one agent an env; FloorCoverage(envs): expert() + step() eager and replayed as a HIP graph, next to
      step() alone under random actions.
  (w) the map windows, at `--envs` envs x 1 agent, on seen maps that hold one rendered frame: one cuda.local_maps
      (ms_nav_windows) of floor and wall at 32 x 32 with samples=1 through cuda.agent_views (radius 4 m), and one of floor, wall and
      the frontier distance at 64 x 64 with samples=2 - each timed as 20 calls back to back between two events, with the output's
      bytes (N A C H W 4: essentially the kernel's algorithmic traffic) over that time next to the 6.3 TB/s the HBM sustains
      (MI355X_MICROARCH.md; 8 TB/s spec) - next to the torch formulation of the same rule on the same inputs (index arithmetic
      and gathers; the first `--torch-envs` envs, scaled; outputs compared as bits) and to modules.Overhead at the same size;
      FloorCoverage(envs, local_map=True).step eager and replayed as a HIP graph, next to FloorCoverage(envs).step.
  (d) the cell draws, at `--envs` envs x 1 agent: one cuda.cell_draws (ms_nav_draws) of K = 1 and one of K = 64 in the band 2 to 8 m
      of the distance field round a spawn point - each timed as 20 CellDraws.again() back to back between two events - next to
      the torch formulation of the same rule on the same inputs (the qualify mask padded to the largest plan, a cumsum, the same
      hash in int64 tensor ops and a searchsorted; the first `--torch-envs` envs, scaled; its cells compared with the kernel's);
      PointGoal(envs, goal_range=(2., 8.), sampled_spawns=True).step eager and replayed as a HIP graph, next to the plain
      PointGoal(envs).step.
  (r) the regions, at `--envs` envs x 1 agent, the maximum and median `passes` reported for every regions call: one cuda.regions
      (ms_nav_regions) of the grid next to floorcoverage.reachable() on the same grid - the single-goal field launch it
      replaces - with Regions.masks(points=) of the same point compared with reachable()'s mask as bytes; the torch formulation
      of min-label propagation (the grids padded to the largest plan, four shifted minimums a sweep, swept until nothing
      changes, checked every 16 sweeps; the first `--torch-envs` envs, scaled; labels compared for equality);
      SeenMaps.frontier_regions right after one marked frame, and with 80 % seen; one Regions.masks call;
      PointGoal(envs, goal_range=(2., 8.), sampled_spawns=True, one_region=True).step eager and replayed as a HIP graph, next
      to the same env without one_region.
  (v) the view fields, at `--envs` envs: one cuda.view_fields (ms_nav_views) of P = 1 viewpoint an env at R = 10 m with the byte
      store, and one of P = 16 candidate standpoints an env at R = 5 m with store=False and gains against seen maps that hold one
      rendered frame - each timed as 20 ViewFields.update() back to back between two events - next to the torch formulation of
      the same rule at the same shape (the grids padded to the largest plan, the walls padded to the most an env has, a loop over
      the wall index of (envs, H, W) binary32 tensor ops in the rule's order; the first `--torch-envs` envs, scaled; bytes,
      counts and gains compared for equality: the one gate on time is that the kernel is the faster); for time only,
      cuda.raycast of a ring of 720 rays an env plus SeenMaps.mark of them; FloorCoverage(envs): expert('views') + step()
      eager and replayed as a HIP graph, next to expert() + step(); and FloorCoverage(64), 300 steps, in one run under
      expert('views'), expert('frontier') and uniformly random actions: episodes ended by coverage and mean final fraction.
  (z) the basins, at `--envs` envs, the maximum and median `passes` reported for every basins call: one cuda.basins
      (ms_nav_basins) of the frontier field right after one marked frame, its labels through ids = frontier_regions().labels, next
      to the seeded_fields launch before it; one cuda.basins of a two-agent cuda.point_marks field with n_ids = 2, next to the
      point_marks and seeded_fields launches before it; the torch formulation of the same rule on that field (the grids padded to
      the largest plan, the successor index by eight shifted folds in the rule's order, then N = N[N] by gathers until nothing
      changes, a host round trip a jump; the first `--torch-envs` envs, scaled; labels compared for equality); one Basins.at of
      `--envs` x 1 points; FloorCoverage(envs, n_agents=2, shared=True): expert('split') + step() eager and replayed as a HIP
      graph, next to expert() + step(); and FloorCoverage(64, n_agents=2, shared=True), 300 steps, in one run under
      expert('split'), expert('frontier') and uniformly random actions: episodes ended by coverage and mean final fraction.
  (c2) clearance, at `--envs` envs and R = 2: one cuda.clearance_fields (ms_nav_clearance) with values alone and with nearest and
      three radii, for BOTH instantiations of its kernel (the tile cull alone; the tile cull and the wave's own: ms_debug_nav_clear_cull);
      next to them cuda.nav_grid's ms_nav_free launch on the same grid (brute force over the same (cell, wall) pairs) and the torch
      formulation of the same rule (the grids padded to the largest plan, the walls padded to the most an env has, a loop over the
      wall index; the first `--torch-envs` envs, scaled; values and nearest compared for equality); one cuda.clearance of
      `--envs` x 4 points with four agents an env; modules.Proximity eager and replayed as a HIP graph, next to modules.IMU.
      `--large` draws the large plans instead.
  (k) cost fields, at `--envs` envs, the maximum and median `passes` reported for each: one cuda.cost_fields (ms_nav_cost_fields) for
      BOTH variants of where the kernel keeps a cell's multiplier (read from global memory every pass; in LDS:
      ms_debug_nav_cost_variant) next to cuda.seeded_fields on the same marks - the cells round a spawn point - for a cost of all
      ones, an inflation layer (cuda.inflation_costs of cuda.clearance_fields, radius 0.5) and a known-space layer (cuda.mark_costs
      of a seen map after one marked frame); one weighted waypoints call of `--envs` x 1 points next to the seeded one; the torch
      formulation of the same rule under the inflation layer (the first `--torch-envs` envs, scaled; compared for equal bits);
      PointGoal(envs, margin=.3): expert() + step() eager and replayed as a HIP graph, next to PointGoal(envs); and PointGoal(64),
      300 steps under the expert with and without margin=.3: arrivals, steps the follower spent stuck, mean clearance under the agents.
  (g) age maps, at `--envs` envs x 1 agent x 256 rays, medians of twice `--repeats` calls back to back: SeenMaps.mark on a rendered
      frame - the yardstick - and on the same frame one AgeMaps.mark (ms_nav_ages) without the survey, with it, and with it and the
      store of ages; the survey alone; the torch formulation of the same rule (the first `--torch-envs` envs from empty maps,
      scaled; every output compared for equality); Patrol(envs).step next to FloorCoverage(envs).step, eager and replayed as a HIP
      graph; and Patrol(64), 300 steps under expert() and under random actions: the final mean and worst idleness, in steps.
  (h) pulled paths, at `--envs` envs x 1 point, medians of 20 calls back to back: one DistanceFields.pulled (ms_nav_pulls) at reach 64
      and at 256, under either of the wave's sight schemes (a lane a candidate - the library's - and a lane a sample), next to
      paths(max_points=256) and waypoints() on the same fields and points; the mean vertices, and the pulled length over the
      chain's and over `at`; PointGoal(envs, spl=True).step eager and replayed as a HIP graph, next to the plain env; and
      PointGoal(64, spl=True), 300 steps under expert() and under random actions: the mean SPL of the episodes that ended.
  (n) zones, at `--envs` envs x 2 agents, K = 64: one cuda.zones (ms_nav_zones) of the grid's regions with one distance field, next to
      the cuda.regions launch before it - the yardstick: the zones launch reads each cell once -; one of the frontier clusters right
      after a marked frame with a distance field round each of the two agents (F = 2), next to the frontier_regions launch before it;
      for each the torch formulation of the same rule (the labels padded to the largest plan, the rank of a root by a cumulative sum,
      scatter_add counts and a scatter_reduce amin over (value bits << 32) | cell; the first `--torch-envs` envs, scaled; cells,
      least, nearest and n_zones compared for equality); FloorCoverage(envs, n_agents=2, shared=True): expert('assign') + step()
      eager and replayed as a HIP graph, next to expert('split') and expert('frontier') in the same run; and
      FloorCoverage(64, n_agents=2, shared=True), 300 steps, in one run under expert('assign'), expert('split'), expert('frontier')
      and uniformly random actions: episodes ended by coverage and mean final fraction.
`--only` picks one part (for a profiler run of its own: `rocprofv3 --kernel-trace --stats -- python tools/navfield_rate.py
--only fields`).  Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b)*1e-3)
    times = np.array(times)
    return float(np.median(times)), float(times.min()), float(times.max())


def torch_fields(grid, goals, envs):
    """The fields of goal 0 of the first `envs` envs by tensor ops, as (envs, H, W) padded to the largest grid."""
    geom = grid._host_geom[:envs]
    H, W = int(geom[:, 3].max()) + 2, int(geom[:, 2].max()) + 2
    dev = grid.free.device
    c = torch.tensor(grid.cell, dtype=torch.float32, device=dev)
    ws, wd = c, c*torch.tensor(1.41421356, dtype=torch.float32, device=dev)
    free = torch.zeros((envs, H, W), dtype=torch.bool, device=dev)
    for e in range(envs):
        s, ny, nx = grid.cells(e)
        free[e, 1:ny + 1, 1:nx + 1] = grid.free[s:s + ny*nx].reshape(ny, nx).bool()
    inf = torch.tensor(float('inf'), device=dev)

    def shifted(t, di, dj, fill):
        out = torch.full_like(t, fill)
        out[:, max(di, 0):H + min(di, 0), max(dj, 0):W + min(dj, 0)] = t[:, max(-di, 0):H + min(-di, 0), max(-dj, 0):W + min(-dj, 0)]
        return out

    open_ = {}
    for di in (-1, 1):
        for dj in (-1, 1):                                              # a diagonal step from (i - di, j - dj) into (i, j) cuts no corner
            open_[di, dj] = free & shifted(free, di, dj, False) & shifted(free, di, 0, False) & shifted(free, 0, dj, False)

    def run():
        D = torch.full((envs, H, W), float('inf'), device=dev)
        # the anchors, as the contract forms them
        g = goals[:envs, 0]
        jx0, iy0 = (torch.as_tensor(geom[:, k].astype(np.int64), device=dev) for k in (0, 1))
        j0 = torch.floor(g[:, 0]/c - .5).long() - jx0
        i0 = torch.floor(g[:, 1]/c - .5).long() - iy0
        e = torch.arange(envs, device=dev)
        for a in (0, 1):
            for b in (0, 1):
                i, j = i0 + a, j0 + b
                ok = (i >= 0) & (i < H - 2) & (j >= 0) & (j < W - 2)
                ic, jc = i.clamp(0, H - 3), j.clamp(0, W - 3)
                dx = g[:, 0] - ((jx0 + jc).float() + .5)*c
                dy = g[:, 1] - ((iy0 + ic).float() + .5)*c
                leg = torch.sqrt(dx*dx + dy*dy)
                ok = ok & free[e, ic + 1, jc + 1]
                D[e, ic + 1, jc + 1] = torch.where(ok, leg, D[e, ic + 1, jc + 1])
        sweeps = 0
        while True:
            before = D
            for _ in range(16):
                new = D
                for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                    new = torch.minimum(new, shifted(D, di, dj, float('inf')) + ws)
                for (di, dj), ok in open_.items():
                    new = torch.minimum(new, torch.where(ok, shifted(D, di, dj, float('inf')) + wd, inf))
                D = torch.where(free, new, inf)
                sweeps += 1
            if torch.equal(D, before):
                return D, sweeps
    return run


def torch_regions(grid, envs):
    """The labels of the first `envs` envs' free cells by tensor ops: (envs, H, W) int32 padded to the largest grid, a frame of closed
    cells round each; a cell's label is its own row-major index within its env; min over the four shifts until nothing changes."""
    geom = grid._host_geom[:envs]
    H, W = int(geom[:, 3].max()) + 2, int(geom[:, 2].max()) + 2
    dev = grid.free.device
    top = torch.iinfo(torch.int32).max
    free = torch.zeros((envs, H, W), dtype=torch.bool, device=dev)
    own = torch.full((envs, H, W), top, dtype=torch.int32, device=dev)
    for e in range(envs):
        s, ny, nx = grid.cells(e)
        free[e, 1:ny + 1, 1:nx + 1] = grid.free[s:s + ny*nx].reshape(ny, nx).bool()
        own[e, 1:ny + 1, 1:nx + 1] = torch.arange(ny*nx, dtype=torch.int32, device=dev).reshape(ny, nx)
    start = torch.where(free, own, torch.full_like(own, top))

    def shifted(t, di, dj):
        out = torch.full_like(t, top)
        out[:, max(di, 0):H + min(di, 0), max(dj, 0):W + min(dj, 0)] = t[:, max(-di, 0):H + min(-di, 0), max(-dj, 0):W + min(-dj, 0)]
        return out

    def run():
        L, sweeps = start, 0
        while True:
            before = L
            for _ in range(16):
                new = L
                for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                    new = torch.minimum(new, shifted(L, di, dj))
                L = torch.where(free, new, start)
                sweeps += 1
            if torch.equal(L, before):
                return torch.where(free, L, torch.full_like(L, -1)), sweeps
    return run


def torch_basins(grid, fields, ids, envs):
    """The basins of field 0 of the first `envs` envs by tensor ops, as (envs, H*W) labels padded to the largest grid: the successor
    of every cell by a fold over the eight shifted grids in the rule's order, then N = N[N] until nothing changes."""
    from megastep_amd import cuda
    geom = grid._host_geom[:envs]
    H, W = int(geom[:, 3].max()) + 2, int(geom[:, 2].max()) + 2
    dev = grid.free.device
    inf = float('inf')
    c = torch.tensor(grid.cell, dtype=torch.float32, device=dev)
    ws, wd = c, c*torch.tensor(1.41421356, dtype=torch.float32, device=dev)
    free = torch.zeros((envs, H, W), dtype=torch.bool, device=dev)
    D = torch.full((envs, H, W), inf, dtype=torch.float32, device=dev)
    name = torch.full((envs, H, W), -1, dtype=torch.int32, device=dev)   # (what a cell's label is when a chain ends on it)
    g = fields.n_goals
    for e in range(envs):
        s, ny, nx = grid.cells(e)
        free[e, 1:ny + 1, 1:nx + 1] = grid.free[s:s + ny*nx].reshape(ny, nx).bool()
        D[e, 1:ny + 1, 1:nx + 1] = fields.values[g*s:g*s + ny*nx].reshape(ny, nx)
        name[e, 1:ny + 1, 1:nx + 1] = (ids[g*s:g*s + ny*nx] if ids is not None else torch.arange(ny*nx, dtype=torch.int32, device=dev)).reshape(ny, nx)
    own = torch.arange(H*W, device=dev).reshape(1, H, W).expand(envs, H, W)
    dead = H*W                                                           # (one more slot an env, which names itself)

    def shifted(t, di, dj, fill):
        out = torch.full_like(t, fill)
        out[:, max(-di, 0):H + min(-di, 0), max(-dj, 0):W + min(-dj, 0)] = t[:, max(di, 0):H + min(di, 0), max(dj, 0):W + min(dj, 0)]
        return out

    def run():
        best, below = torch.full_like(D, inf), torch.full_like(D, inf)
        target = torch.full((envs, H, W), dead, dtype=torch.int64, device=dev)
        for di, dj in ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, -1), (-1, 1)):
            ok = shifted(free, di, dj, False)
            if di and dj:
                ok = ok & shifted(free, di, 0, False) & shifted(free, 0, dj, False)
            du = shifted(D, di, dj, inf)
            v = torch.where(ok, du + (wd if di and dj else ws), torch.full_like(D, inf))
            take = v < best
            best, below, target = torch.where(take, v, best), torch.where(take, du, below), torch.where(take, own + (di*W + dj), target)
        succ = torch.where(D == 0, own, torch.where(below < D, target, torch.full_like(target, dead)))
        succ = torch.where(free & (D < inf), succ, torch.full_like(succ, dead))
        N = torch.cat([succ.reshape(envs, -1), torch.full((envs, 1), dead, dtype=torch.int64, device=dev)], 1)
        jumps = 0
        while True:
            new = N.gather(1, N)
            jumps += 1
            if torch.equal(new, N):
                break
            N = new
        names = torch.cat([name.reshape(envs, -1), torch.full((envs, 1), -1, dtype=torch.int32, device=dev)], 1)
        return names.gather(1, N)[:, :-1].reshape(envs, H, W), jumps
    return run


def env_rates(env, n, steps, warm):
    from megastep_amd import arrdict
    A = env.action_space.shape[0]
    env.reset()
    actions = torch.randint(0, 7, (n, A), device='cuda')
    decision = arrdict.arrdict(actions=actions)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warm):
            env.step(decision)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        env.step(decision)
    torch.cuda.synchronize()
    eager = (time.perf_counter() - t)/steps
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(decision)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        actions.random_(0, 7)
        g.replay()
    torch.cuda.synchronize()
    return eager, (time.perf_counter() - t)/steps


def torch_seen(grid, countable, origins, dirs, distances, max_range, envs):
    """The seen maps' rule by tensor ops for the first `envs` envs, one viewer and one map each: returns run() -> (flat maps of
    those envs, gained (envs,)) from empty maps."""
    dev = origins.device
    c = torch.tensor(grid.cell, dtype=torch.float32, device=dev)
    geom = torch.as_tensor(grid._host_geom[:envs].astype(np.int64), device=dev)
    starts = torch.as_tensor(grid._host_starts[:envs + 1], device=dev)
    n_cells = int(grid._host_starts[envs])
    o, d, dist = origins[:envs, 0], dirs[:envs, 0], distances[:envs, 0]
    counts = (countable[:n_cells] & 1).bool()
    m = torch.tensor(max_range, dtype=torch.float32, device=dev)

    def run():
        dx, dy = d[..., 0], d[..., 1]
        rlen = torch.sqrt(dx*dx + dy*dy)
        keep = torch.isfinite(o).all(-1)[:, None] & torch.isfinite(d).all(-1) & torch.isfinite(rlen) & (rlen > 0) & (dist > 0)
        reach = torch.where(dist < m, dist, m)
        ex, ey = dx/rlen*reach, dy/rlen*reach
        k = torch.ceil(torch.sqrt(ex*ex + ey*ey)/(.5*c))
        keep = keep & (k < 1048576.)
        K = torch.where(keep, k, torch.ones_like(k)).clamp(min=1)
        s = torch.arange(int(K.max()) + 1, dtype=torch.float32, device=dev)                # (a host round trip: the padding)
        t = s/K[..., None]
        x, y = o[:, None, None, 0] + ex[..., None]*t, o[:, None, None, 1] + ey[..., None]*t
        fx, fy = torch.floor(x/c), torch.floor(y/c)
        ok = keep[..., None] & (s <= K[..., None]) & (fx.abs() < 2.**30) & (fy.abs() < 2.**30)
        j = torch.where(ok, fx, torch.zeros_like(fx)).long() - geom[:, None, None, 0]
        i = torch.where(ok, fy, torch.zeros_like(fy)).long() - geom[:, None, None, 1]
        nx, ny = geom[:, None, None, 2], geom[:, None, None, 3]
        ok = ok & (i >= 0) & (i < ny) & (j >= 0) & (j < nx)
        cell = starts[:envs, None, None] + i*nx + j
        seen = torch.zeros(n_cells + 1, dtype=torch.bool, device=dev)
        seen[torch.where(ok, cell, torch.full_like(cell, n_cells))] = True                 # the scatter (the spare slot: skipped samples)
        new = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), (seen[:n_cells] & counts).long().cumsum(0)])   # the second pass
        return seen[:n_cells], (new[starts[1:]] - new[starts[:-1]]).int()
    return run


def torch_ages(grid, countable, origins, dirs, distances, max_range, threshold, envs):
    """The age maps' rule by tensor ops for the first `envs` envs, one viewer and one map each - the marked set as torch_seen makes
    it, then a dense pass over every cell: returns run(last, clock) -> (last, clock, swept, gained, idle, oldest, total_age, n_stale,
    stale, ages), the maps flat over those envs and the numbers (envs,)."""
    dev = origins.device
    marks = torch_seen(grid, countable, origins, dirs, distances, max_range, envs)
    starts = torch.as_tensor(grid._host_starts[:envs + 1], device=dev)
    n_cells = int(grid._host_starts[envs])
    env = torch.repeat_interleave(torch.arange(envs, device=dev), starts[1:] - starts[:-1])
    counts = (countable[:n_cells] & 1).bool()

    def per_env(values):
        return torch.zeros(envs, dtype=torch.int64, device=dev).index_add_(0, env, values.long())

    def run(last, clock):
        marked, _ = marks()
        now = (clock.long() + 1).clamp(max=2**24)
        tick = now[env]
        age = tick - last.long()
        counted = marked & counts
        swept, gained, idle = per_env(counted), per_env(counted & (last == 0)), per_env(torch.where(counted, age, 0))
        last = torch.where(marked, tick.float(), last)
        age = tick - last.long()
        stale = counts & (age >= threshold)
        oldest = torch.zeros(envs, dtype=torch.int64, device=dev).scatter_reduce_(0, env, torch.where(counts, age, 0), 'amax')
        return (last, now.int(), swept.int(), gained.int(), idle, oldest.int(), per_env(torch.where(counts, age, 0)), per_env(stale).int(),
                stale.to(torch.uint8), age.float())
    return run


def torch_windows(grid, views, size, samples, channels, envs):
    """The map windows' rule by tensor ops for the first `envs` envs, one view and one store a layer each: `channels` is a list
    of (source values, is_float, where, scale, gate values or None); returns run() -> (envs, 1, C, H, W). outside = hidden = 0."""
    dev = views.device
    H, W = size
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    c, k = f32(grid.cell), f32(samples)
    geom = torch.as_tensor(grid._host_geom[:envs].astype(np.int64), device=dev)[:, :, None, None]
    starts = torch.as_tensor(grid._host_starts[:envs], device=dev)[:, None, None]
    g = views[:envs, 0, :, None, None]
    i, j = torch.arange(H, device=dev).float()[None, :, None], torch.arange(W, device=dev).float()[None, None, :]
    zero, one = f32(0.), f32(1.)

    def run():
        out = torch.zeros((envs, 1, len(channels), H, W), dtype=torch.float32, device=dev)
        for a in range(samples):
            for b in range(samples):
                u, w = j + (f32(b) + .5)/k, i + (f32(a) + .5)/k
                x, y = (g[:, 0]*u + g[:, 1]*w) + g[:, 2], (g[:, 3]*u + g[:, 4]*w) + g[:, 5]
                fx, fy = torch.floor(x/c), torch.floor(y/c)
                ok = (fx.abs() < 2.**30) & (fy.abs() < 2.**30)
                jj = torch.where(ok, fx, torch.zeros_like(fx)).long() - geom[:, 0]
                ii = torch.where(ok, fy, torch.zeros_like(fy)).long() - geom[:, 1]
                ok = ok & (ii >= 0) & (ii < geom[:, 3]) & (jj >= 0) & (jj < geom[:, 2])
                cell = torch.where(ok, starts + ii*geom[:, 2] + jj, torch.zeros_like(ii))
                for n, (values, is_float, where, scale, gate) in enumerate(channels):
                    src = values[cell]
                    if is_float:
                        v = src*f32(scale)
                        value = torch.where(v < 1, torch.where(v > 0, v, zero), one)
                    else:
                        value = torch.where((src != 0) == where, one, zero)
                    if gate is not None:
                        value = torch.where(gate[cell] == 0, zero, value)
                    out[:, 0, n] = out[:, 0, n] + torch.where(ok, value, zero)
        return out/f32(samples*samples)
    return run


def torch_draws(grid, D, lo, hi, K, seed, envs):
    """The cell draws' rule by tensor ops for the first `envs` envs, one set each, from counter 0, on a float32 source of one
    store an env: returns run() -> ((envs, K) cells, (envs,) counts)."""
    dev = D.device
    cells = torch.as_tensor(np.diff(grid._host_starts[:envs + 1]), device=dev)
    starts = torch.as_tensor(grid._host_starts[:envs], device=dev)
    span = torch.arange(int(cells.max()), device=dev)
    valid = span[None, :] < cells[:, None]
    at = torch.where(valid, starts[:, None] + span[None, :], torch.zeros_like(starts[:, None]))
    m32 = 0xffffffff

    def mix(a):
        a = a ^ (a >> 16)
        a = (a*0x85ebca6b) & m32
        a = a ^ (a >> 13)
        a = (a*0xc2b2ae35) & m32
        return a ^ (a >> 16)

    def run():
        q = valid & (grid.free[at] != 0) & (D[at] >= lo) & (D[at] <= hi)
        cum = q.long().cumsum(1)
        M = cum[:, -1]
        s = torch.full((envs, K), 0x9e3779b9, dtype=torch.int64, device=dev)
        for word in (seed & m32, seed >> 32, torch.arange(envs, device=dev)[:, None], 0, torch.arange(K, device=dev)[None, :], 0):
            s = mix((s + word) & m32)
        r = (s*M[:, None]) >> 32
        cell = torch.searchsorted(cum, r + 1)
        return torch.where(M[:, None] > 0, cell, torch.full_like(cell, -1)), M
    return run


class ExpertStep:
    """An env whose step is the expert's own: expert() + step(), the decision handed in ignored."""

    def __init__(self, env, *kind):
        self.env, self.action_space, self.kind = env, env.action_space, kind

    def reset(self):
        return self.env.reset()

    def step(self, decision):
        return self.env.step(self.env.expert(*self.kind))


def torch_views(grid, scenery, points, R, countable, maps, slot, envs):
    """ms_nav_views' rule for the first `envs` envs by tensor ops: (envs, H, W) binary32 tensors padded to the largest grid, the
    static walls padded with NaN rows (which block nothing) to the most an env has, one pass of the rule's statements per wall
    index and viewpoint.  Returns run() -> (visible (envs, P, H, W) bool, counts, gains (envs, P) int64)."""
    geom = grid._host_geom[:envs]
    H, W = int(geom[:, 3].max()), int(geom[:, 2].max())
    dev = grid.free.device
    P = points.shape[1]
    af = scenery.n_agents*scenery.model.shape[0]
    starts, widths = scenery.lines.starts[:envs].tolist(), scenery.lines.widths[:envs].tolist()
    most = max(w - af for w in widths)
    walls = torch.full((envs, most, 4), float('nan'), device=dev)
    inside = torch.zeros((envs, H, W), dtype=torch.bool, device=dev)
    counts = torch.zeros((envs, H, W), dtype=torch.bool, device=dev)
    seen = torch.zeros((envs, maps.n_maps if maps is not None else 1, H, W), dtype=torch.bool, device=dev)
    for e in range(envs):
        walls[e, :widths[e] - af] = scenery.lines.vals[starts[e] + af:starts[e] + widths[e]].reshape(-1, 4)
        first, ny, nx = grid.cells(e)
        inside[e, :ny, :nx] = True
        counts[e, :ny, :nx] = (countable[first:first + ny*nx] & 1).bool().reshape(ny, nx)
        if maps is not None:
            S = maps.n_maps
            seen[e, :, :ny, :nx] = (maps.values[S*first:S*(first + ny*nx)] & 1).bool().reshape(S, ny, nx)
    g = torch.as_tensor(geom, device=dev)
    c = torch.tensor(grid.cell, dtype=torch.float32, device=dev)
    x = (((g[:, 0, None] + torch.arange(W, device=dev)[None]).float() + .5)*c)[:, None, :].expand(envs, H, W).contiguous()
    y = (((g[:, 1, None] + torch.arange(H, device=dev)[None]).float() + .5)*c)[:, :, None].expand(envs, H, W).contiguous()
    R2 = torch.tensor(R, dtype=torch.float32, device=dev)*torch.tensor(R, dtype=torch.float32, device=dev)

    def run():
        vis = torch.zeros((envs, P, H, W), dtype=torch.bool, device=dev)
        for p in range(P):
            px, py = points[:envs, p, 0, None, None], points[:envs, p, 1, None, None]
            rx, ry = x - px, y - py
            ok = inside & (rx*rx + ry*ry <= R2) & torch.isfinite(px) & torch.isfinite(py)
            sx0, sx1, sy0, sy1 = torch.minimum(px, x), torch.maximum(px, x), torch.minimum(py, y), torch.maximum(py, y)
            for l in range(most):
                ax, ay, bx, by = (walls[:, l, k, None, None] for k in range(4))
                meets = (torch.minimum(ax, bx) <= sx1) & (torch.maximum(ax, bx) >= sx0) & (torch.minimum(ay, by) <= sy1) & (torch.maximum(ay, by) >= sy0)
                vx, vy = bx - ax, by - ay
                o1 = vx*(py - ay) - vy*(px - ax)
                o2 = vx*(y - ay) - vy*(x - ax)
                o3 = rx*(ay - py) - ry*(ax - px)
                o4 = rx*(by - py) - ry*(bx - px)
                ok &= ~(meets & (((o1 < 0) & (o2 > 0)) | ((o1 > 0) & (o2 < 0))) & (((o3 <= 0) & (o4 >= 0)) | ((o3 >= 0) & (o4 <= 0))))
            vis[:, p] = ok
        counted = vis & counts[:, None]
        gains = None
        if maps is not None:
            which = slot[:envs].long() if slot is not None else torch.zeros((envs, P), dtype=torch.long, device=dev)
            fresh = ~seen[torch.arange(envs, device=dev)[:, None], which]
            gains = (counted & fresh).sum((-1, -2))
        return vis, counted.sum((-1, -2)), gains
    return run


def torch_clearance(grid, scenery, R, envs):
    """ms_nav_clearance's rule for the first `envs` envs by tensor ops: (envs, H, W) binary32 tensors padded to the largest grid, the
    walls padded to the most an env has with NaN rows (never a candidate), a loop over the wall index in ascending order (so a
    strict `<` keeps the tie rule).  Returns run() -> (values, nearest)."""
    dev = grid.free.device
    geom = grid._host_geom[:envs]
    H, W = int(geom[:, 3].max()), int(geom[:, 2].max())
    c = torch.tensor(grid.cell, dtype=torch.float32, device=dev)
    g = torch.as_tensor(geom, device=dev)
    x = (((g[:, 0, None] + torch.arange(W, device=dev)).float() + .5)*c)[:, None, :]
    y = (((g[:, 1, None] + torch.arange(H, device=dev)).float() + .5)*c)[:, :, None]
    lines = scenery.lines
    af = scenery.n_agents*scenery.model.shape[0]
    vals, starts, widths = lines.vals.reshape(-1, 4), lines.starts.cpu().numpy(), lines.widths.cpu().numpy()
    most = int((widths[:envs] - af).max())
    rows = torch.full((envs, most, 4), float('nan'), dtype=torch.float32, device=dev)
    for e in range(envs):
        rows[e, :widths[e] - af] = vals[starts[e] + af:starts[e] + widths[e]]
    R2 = torch.tensor(R, dtype=torch.float32, device=dev)**2
    zero, one = torch.zeros((), device=dev), torch.ones((), device=dev)

    def run():
        bd = torch.full((envs, H, W), float('inf'), device=dev)
        bi = torch.full((envs, H, W), -1, dtype=torch.int32, device=dev)
        for l in range(most):
            ax, ay, bx, by = (rows[:, l, k][:, None, None] for k in range(4))
            vx, vy, px, py = bx - ax, by - ay, x - ax, y - ay
            vv = vx*vx + vy*vy
            t = torch.where(vv > 0, (px*vx + py*vy)/vv, zero)
            t = torch.where(t < 0, zero, torch.where(t > 1, one, t))
            dx, dy = px - t*vx, py - t*vy
            d2 = dx*dx + dy*dy
            take = (d2 <= R2) & (d2 < bd)
            bd = torch.where(take, d2, bd)
            bi = torch.where(take, l + af, bi)
        return torch.where(bi >= 0, bd.sqrt(), torch.full_like(bd, float('inf'))), bi
    return run


def torch_cost_fields(grid, marks, cost, envs):
    """The cost fields of the first `envs` envs (one field an env, a cost store an env) by tensor ops, as (envs, H, W) padded to the
    largest grid: the weights of the cell a step leaves, the min first and one addition per weight."""
    geom = grid._host_geom[:envs]
    H, W = int(geom[:, 3].max()) + 2, int(geom[:, 2].max()) + 2
    dev = grid.free.device
    c = torch.tensor(grid.cell, dtype=torch.float32, device=dev)
    free = torch.zeros((envs, H, W), dtype=torch.bool, device=dev)
    seeds = torch.zeros((envs, H, W), dtype=torch.bool, device=dev)
    k = torch.ones((envs, H, W), dtype=torch.float32, device=dev)
    for e in range(envs):
        s, ny, nx = grid.cells(e)
        free[e, 1:ny + 1, 1:nx + 1] = grid.free[s:s + ny*nx].reshape(ny, nx).bool()
        seeds[e, 1:ny + 1, 1:nx + 1] = (marks[s:s + ny*nx].reshape(ny, nx) & 1).bool()
        k[e, 1:ny + 1, 1:nx + 1] = cost[s:s + ny*nx].reshape(ny, nx)
    seeds &= free
    k = torch.where(k >= 1, k.clamp(max=256.), torch.where(k < 1, torch.ones_like(k), torch.full_like(k, 256.)))
    ws, wd = c*k, (c*torch.tensor(1.41421356, dtype=torch.float32, device=dev))*k
    inf = torch.tensor(float('inf'), device=dev)

    def shifted(t, di, dj, fill):
        out = torch.full_like(t, fill)
        out[:, max(di, 0):H + min(di, 0), max(dj, 0):W + min(dj, 0)] = t[:, max(-di, 0):H + min(-di, 0), max(-dj, 0):W + min(-dj, 0)]
        return out

    open_ = {}
    for di in (-1, 1):
        for dj in (-1, 1):
            open_[di, dj] = free & shifted(free, di, dj, False) & shifted(free, di, 0, False) & shifted(free, 0, dj, False)

    def run():
        D = torch.where(seeds, torch.zeros((), device=dev), inf).expand(envs, H, W).contiguous()
        sweeps = 0
        while True:
            before = D
            for _ in range(16):
                straight, diagonal = inf.expand_as(D), inf.expand_as(D)
                for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                    straight = torch.minimum(straight, shifted(D, di, dj, float('inf')))
                for (di, dj), ok in open_.items():
                    diagonal = torch.minimum(diagonal, torch.where(ok, shifted(D, di, dj, float('inf')), inf))
                D = torch.where(free, torch.minimum(D, torch.minimum(straight + ws, diagonal + wd)), inf)
                sweeps += 1
            if torch.equal(D, before):
                return D, sweeps
    return run


def torch_zones(grid, labels, values, n_values, K, envs):
    """ms_nav_zones' rule, ranked, one labels store and `n_values` value stores an env, for the first `envs` envs by tensor ops on
    (envs, C) tensors padded to the largest grid's cells: run() -> (cells (envs, K), key (envs, F, K) int64 - (bits << 32) | cell,
    the int64 maximum without one -, n_zones (envs,))."""
    dev = labels.device
    cells = [grid.cells(e) for e in range(envs)]
    C = max(ny*nx for _, ny, nx in cells)
    lab = torch.full((envs, C), -1, dtype=torch.int64, device=dev)
    val = torch.full((envs, n_values, C), float('inf'), device=dev)
    for e, (first, ny, nx) in enumerate(cells):
        n = ny*nx
        lab[e, :n] = labels[first:first + n]
        val[e, :, :n] = values[n_values*first:n_values*first + n_values*n].reshape(n_values, n)
    index = torch.arange(C, device=dev)
    none = torch.iinfo(torch.int64).max

    def run():
        root = lab == index
        rank = root.cumsum(-1) - 1
        safe = lab.clamp(min=0)
        zone = torch.where((lab >= 0) & root.gather(-1, safe), rank.gather(-1, safe), -1)
        slot = torch.where((zone >= 0) & (zone < K), zone, K)          # (a spare column for the cells without a zone)
        count = torch.zeros((envs, K + 1), dtype=torch.int64, device=dev).scatter_add_(-1, slot, torch.ones_like(slot))
        bits = val.contiguous().view(torch.int32).to(torch.int64)
        key = torch.where((bits >= 0) & (bits < 0x7f800000), (bits << 32) | index, none)
        best = torch.full((envs, n_values, K + 1), none, dtype=torch.int64, device=dev)
        best = best.scatter_reduce(-1, slot[:, None].expand(-1, n_values, -1), key, 'amin')
        return count[:, :K], best[..., :K], root.sum(-1)
    return run


def zones_equal(z, result, envs):
    """Are a Zones' cells, least, nearest and n_zones of its first `envs` envs what torch_zones' run() returned?"""
    count, best, n_zones = result
    none = best == torch.iinfo(torch.int64).max
    least = torch.where(none, 0x7f800000, best >> 32).int()
    nearest = torch.where(none, -1, best & 0xffffffff).int()
    return bool(torch.equal(z.cells[:envs], count[:, None].expand(-1, z.n_fields, -1).int()) and torch.equal(z.least[:envs].view(torch.int32), least) and
                torch.equal(z.nearest[:envs], nearest) and torch.equal(z.n_zones[:envs], n_zones[:, None].expand(-1, z.n_fields).int()))


def follower_score(env, steps):
    """`steps` steps of a PointGoal under its expert: arrivals, the (agent, step) pairs the follower counted at a dead stop, and the
    mean distance to the nearest wall under the agents."""
    from megastep_amd import cuda
    env.reset()
    arrivals = stuck = 0
    room = []
    for _ in range(steps):
        env.step(env.expert())
        arrivals += int(((env._distance < env.arrive) & ~env._goals.stranded).sum())
        stuck += int((env._follower._blocked > 0).sum())
        room.append(float(cuda.clearance(env.core.scenery, env.core.agents.positions, 2.).distances.clamp(max=2.).mean()))
    return dict(arrivals=arrivals, stuck_steps=stuck, mean_clearance=float(np.mean(room)))


def coverage_score(env, steps, policy, seed=1):
    """(episodes ended by coverage, by lifespan, mean final fraction over all episodes) of `steps` steps of a FloorCoverage under
    expert(policy), or uniformly random actions."""
    from megastep_amd import arrdict
    rng = np.random.RandomState(seed)
    n, a = env.core.n_envs, env.core.n_agents
    env.reset()
    by_coverage = by_lifespan = 0
    final = []
    for _ in range(steps):
        fraction, over = env._coverage.fraction().clone(), env._over.clone()
        done = fraction >= env.complete
        by_coverage += int((over & done).sum()); by_lifespan += int((over & ~done).sum())
        final += fraction[over].tolist()
        env.step(arrdict.arrdict(actions=torch.as_tensor(rng.randint(0, 7, (n, a)), device='cuda')) if policy == 'random' else env.expert(policy))
    final += env._coverage.fraction().reshape(-1).tolist()
    return dict(ended_by_coverage=by_coverage, ended_by_lifespan=by_lifespan, mean_final_fraction=float(np.mean(final)))


def rollout_score(env, steps, policy, seed=1):
    """(episodes, arrivals, mean walked/start distance, mean walked/distance covered - both over the episodes that arrived)
    of `steps` steps under 'expert' (env.expert()) or 'compass'; episodes in which the agent was stranded do not count."""
    from megastep_amd import arrdict
    rng = np.random.RandomState(seed)
    n, a = env.core.n_envs, env.core.n_agents
    world = env.reset()
    reset, g, stranded, at = [], [], [], []

    def note(world):
        reset.append(world.reset.cpu().numpy()); g.append(env._distance[:, 0].double().cpu().numpy())
        stranded.append(env._goals.stranded[:, 0].cpu().numpy()); at.append(env.core.agents.positions[:, 0].double().cpu().numpy())
    note(world)
    for _ in range(steps):
        if policy == 'expert':
            decision = env.expert()
        else:
            x, y = (world.obs.goal[..., k].cpu().numpy() for k in (0, 1))
            seek = np.where((y > 0) & (np.abs(x) < y), 1, np.where(x < 0, 5, 6))
            decision = arrdict.arrdict(actions=torch.as_tensor(np.where(rng.rand(n, a) < .25, rng.randint(0, 7, (n, a)), seek), device='cuda'))
        world = env.step(decision)
        note(world)
    reset, g, stranded, at = (np.stack(v) for v in (reset, g, stranded, at))
    episodes = arrivals = 0
    of_start, of_covered = [], []
    for e in range(n):
        starts = list(np.nonzero(reset[:, e])[0]) + [len(reset)]
        for s, t in zip(starts[:-1], starts[1:]):
            if stranded[s:t, e].any():
                continue
            episodes += 1
            if g[t - 1, e] < env.arrive:
                arrivals += 1
                walked = np.linalg.norm(np.diff(at[s:t, e], axis=0), axis=1).sum()
                of_start.append(walked/g[s, e]); of_covered.append(walked/(g[s, e] - g[t - 1, e]))
    mean = lambda v: float(np.mean(v)) if v else None
    return dict(episodes=episodes, arrivals=arrivals, walked_over_start_distance=mean(of_start), walked_over_distance_covered=mean(of_covered))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--distinct', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-envs', type=int, default=256)
    ap.add_argument('--only', choices=('fields', 'query', 'torch', 'envs', 'expert', 'seen', 'frontier', 'window', 'draws', 'regions', 'views', 'basins', 'clearance', 'cost', 'ages', 'pulls', 'zones'))
    ap.add_argument('--large', action='store_true')
    ap.add_argument('--json')
    args = ap.parse_args()
    from megastep_amd import arrdict, core, cubicasa, cuda, modules, scene
    from megastep_amd.demo import Explorer, FloorCoverage, Patrol, PointGoal

    np.random.seed(0); torch.manual_seed(0)
    pool = cubicasa.sample(args.distinct, split='all', n_unique=args.distinct, workers=16, context='subprocess', **(dict(large=True) if args.large else {}))
    geoms = [pool[i % len(pool)] for i in range(args.envs)]
    out = dict(envs=args.envs, distinct=len(pool))
    want = lambda part: args.only in (None, part)

    if want('fields') or want('query') or want('torch'):
        sc = scene.scenery(geoms, 1, device='cuda', bake=False)
        c = core.Core(sc, res=64)
        grid = cuda.nav_grid(sc)
        table = torch.as_tensor(modules.random_empty_positions(geoms, 1, 4), dtype=torch.float32, device='cuda')
        goals, points = table[:, :, 0].contiguous(), table[:, :, 1].contiguous()
        fields = cuda.distance_fields(grid, goals, passes=True)
        cells = np.diff(grid._host_starts)
        out.update(cells_total=int(grid.n_cells), cells_largest=int(cells.max()), cells_median=int(np.median(cells)))
        if want('fields'):
            med, lo, hi = timed(lambda: fields.update(), args.repeats, args.warmup)
            out['fields'] = dict(seconds=med, min=lo, max=hi, goals=args.envs, passes_most=int(fields.passes.max()),
                                 passes_median=int(fields.passes.median()), finite_share=float(torch.isfinite(fields.values).float().mean()))
            print(f"(a) distance_fields, {args.envs} goals: {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}]; most passes {out['fields']['passes_most']}")
        if want('query'):
            med, lo, hi = timed(lambda: fields.at(points), 5*args.repeats, args.warmup)
            out['query'] = dict(seconds=med, min=lo, max=hi, points=args.envs)
            print(f'(b) at, {args.envs} x 1 points: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]')
        if want('torch'):
            k = min(args.torch_envs, args.envs)
            run = torch_fields(grid, goals, k)
            D, sweeps = run()
            same = all(torch.equal(D[e, 1:grid.cells(e)[1] + 1, 1:grid.cells(e)[2] + 1].view(torch.int32), fields.image(e, 0).view(torch.int32))
                       for e in range(k))
            med, lo, hi = timed(lambda: run(), max(args.repeats//3, 2), 1)
            out['torch'] = dict(envs=k, seconds=med, scaled_seconds=med*args.envs/k, sweeps=sweeps, equal_bits=bool(same))
            print(f'(t) torch sweeps, {k} goals: {med*1e3:.1f} ms, {sweeps} sweeps -> {med*args.envs/k*1e3:.1f} ms for {args.envs}; equal bits: {same}')
        del sc, c, grid, fields
        torch.cuda.empty_cache()

    if want('envs'):
        for name, make in (('PointGoal', lambda: PointGoal(args.envs, geometries=geoms)), ('Explorer', lambda: Explorer(args.envs, geometries=geoms))):
            env = make()
            eager, graphed = env_rates(env, args.envs, 60, 10)
            out[name] = dict(eager_seconds=eager, graph_seconds=graphed)
            print(f'(c) {name}({args.envs}).step: eager {eager*1e3:.3f} ms, graph replay {graphed*1e3:.3f} ms')
            del env
            torch.cuda.empty_cache()

    if want('expert'):
        sc = scene.scenery(geoms, 1, device='cuda', bake=False)
        grid = cuda.nav_grid(sc)
        table = torch.as_tensor(modules.random_empty_positions(geoms, 1, 4), dtype=torch.float32, device='cuda')
        goals, points = table[:, :, 0].contiguous(), table[:, :, 1].contiguous()
        fields = cuda.distance_fields(grid, goals)
        way = torch.empty_like(points)
        med, lo, hi = timed(lambda: fields.waypoints(points, out=way), 5*args.repeats, args.warmup)
        chosen = fields.waypoints(points, hops=True)[1]
        out['waypoints'] = dict(seconds=med, min=lo, max=hi, points=args.envs, lookahead=16, with_a_path=float((chosen >= 0).float().mean()),
                                mean_index=float(chosen[chosen >= 0].float().mean()))
        print(f"(e) waypoints, {args.envs} x 1 points: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]; mean index {out['waypoints']['mean_index']:.2f}")
        med, lo, hi = timed(lambda: fields.paths(points, max_points=256), args.repeats, args.warmup)
        counts = fields.paths(points, max_points=256).counts
        out['paths'] = dict(seconds=med, min=lo, max=hi, points=args.envs, max_points=256, longest=int(counts.max()), mean_points=float(counts[counts > 0].float().mean()))
        print(f"(e) paths, {args.envs} x 1 paths of up to 256 points: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]; longest {out['paths']['longest']} points")
        del sc, grid, fields
        torch.cuda.empty_cache()
        env = PointGoal(args.envs, geometries=geoms)
        eager, graphed = env_rates(env, args.envs, 60, 10)
        del env
        torch.cuda.empty_cache()
        env = ExpertStep(PointGoal(args.envs, geometries=geoms))
        expert_eager, expert_graphed = env_rates(env, args.envs, 60, 10)
        out['expert_step'] = dict(step_eager_seconds=eager, step_graph_seconds=graphed, expert_step_eager_seconds=expert_eager,
                                  expert_step_graph_seconds=expert_graphed)
        print(f'(e) PointGoal({args.envs}): step eager {eager*1e3:.3f} ms, graph {graphed*1e3:.3f} ms; expert + step eager {expert_eager*1e3:.3f} ms, '
              f'graph {expert_graphed*1e3:.3f} ms')
        del env
        torch.cuda.empty_cache()
        small = cubicasa.sample(64, seed=7, n_unique=64)
        for policy in ('expert', 'compass'):
            torch.manual_seed(3); np.random.seed(3)
            out['rollout_' + policy] = score = rollout_score(PointGoal(64, geometries=small, bonus=0., max_lifespan=120), 200, policy)
            print(f'(e) PointGoal(64), 200 steps, {policy}: {score}')

    if want('seen'):
        sc = scene.scenery(geoms, 1, device='cuda')
        c = core.Core(sc, res=256, fov=130)
        table = torch.as_tensor(modules.random_empty_positions(geoms, 1, 4), dtype=torch.float32, device='cuda')
        c.agents.positions[:] = table[:, :, 0]
        c.agents.angles.uniform_(-180, 180)
        grid = cuda.nav_grid(sc, config=c.config)
        maps = cuda.seen_maps(grid, 1)
        frame = cuda.render(sc, c.agents, fields=('distances',))
        med, lo, hi = timed(lambda: cuda.render(sc, c.agents, fields=('distances',), out=frame), 5*args.repeats, args.warmup)
        out['seen_render'] = dict(seconds=med, min=lo, max=hi, rays=256)
        print(f'(s) render, {args.envs} x 1 x 256 rays, distances only: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]')
        origins, dirs, distances = c.agents.positions, cuda.camera_rays(c.agents), frame.distances
        gained = maps.mark(origins, dirs, distances).clone()
        everyone = torch.ones((args.envs, 1), dtype=torch.bool, device='cuda')
        buffer = torch.empty_like(gained)
        med, lo, hi = timed(lambda: maps.mark(origins, dirs, distances, out=buffer), 5*args.repeats, args.warmup)
        fresh = timed(lambda: maps.mark(origins, dirs, distances, reset=everyone, out=buffer), 5*args.repeats, args.warmup)
        cells = np.diff(grid._host_starts)
        out['seen_mark'] = dict(seconds=med, min=lo, max=hi, reset_seconds=fresh[0], reset_min=fresh[1], reset_max=fresh[2], rays=256,
                                max_range=10., cells_largest=int(cells.max()), cells_median=int(np.median(cells)),
                                gained_mean=float(gained.float().mean()), same_after_reset=bool(torch.equal(buffer, gained)))
        print(f"(s) mark, {args.envs} x 1 x 256 rays: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}] on maps that hold the cells; "
              f"{fresh[0]*1e6:.1f} us [{fresh[1]*1e6:.1f}, {fresh[2]*1e6:.1f}] with every map reset; {out['seen_mark']['gained_mean']:.0f} cells gained a map")
        k = min(args.torch_envs, args.envs)
        run = torch_seen(grid, maps.countable, origins, dirs, distances, 10., k)
        seen, new = run()
        first, last = 0, int(grid._host_starts[k])
        same = bool(torch.equal(seen, maps.values[first:last].bool()) and torch.equal(new, gained[:k, 0]))
        med, lo, hi = timed(lambda: run(), max(args.repeats//3, 2), 1)
        out['seen_torch'] = dict(envs=k, seconds=med, scaled_seconds=med*args.envs/k, equal_bits=same)
        print(f'(s) torch samples + scatter, {k} envs: {med*1e3:.2f} ms -> {med*args.envs/k*1e3:.1f} ms for {args.envs}; equal maps and counts: {same}')
        del sc, c, grid, maps
        torch.cuda.empty_cache()
        env = FloorCoverage(args.envs, geometries=geoms)
        eager, graphed = env_rates(env, args.envs, 60, 10)
        out['FloorCoverage'] = dict(eager_seconds=eager, graph_seconds=graphed)
        print(f'(s) FloorCoverage({args.envs}).step: eager {eager*1e3:.3f} ms, graph replay {graphed*1e3:.3f} ms')
        del env
        torch.cuda.empty_cache()

    if want('frontier'):
        from megastep_amd.demo.envs.floorcoverage import reachable
        sc = scene.scenery(geoms, 1, device='cuda')
        c = core.Core(sc, res=256, fov=130)
        table = torch.as_tensor(modules.random_empty_positions(geoms, 1, 4), dtype=torch.float32, device='cuda')
        c.agents.positions[:] = table[:, :, 0]
        c.agents.angles.uniform_(-180, 180)
        grid = cuda.nav_grid(sc, config=c.config)
        maps = cuda.seen_maps(grid, 1, reachable(grid, table[:, 0, 0]))
        maps.mark_render(c.agents, cuda.render(sc, c.agents, fields=('distances',)))
        frontier = maps.frontier_fields(passes=True)
        stats = lambda f: dict(passes_most=int(f.passes.max()), passes_median=int(f.passes.median()),
                               seeds_mean=float(f.n_seeds.float().mean()), seen_share=float(maps.fraction().mean()))
        med, lo, hi = timed(lambda: frontier.update(), args.repeats, args.warmup)
        out['frontier_first_frame'] = dict(seconds=med, min=lo, max=hi, fields=args.envs, **stats(frontier))
        print(f"(f) frontier_fields, {args.envs} maps after one frame: {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}]; {out['frontier_first_frame']}")
        way = torch.empty((args.envs, 1, 2), device='cuda')
        med, lo, hi = timed(lambda: frontier.waypoints(c.agents.positions, out=way), 5*args.repeats, args.warmup)
        chosen = frontier.waypoints(c.agents.positions, hops=True)[1]
        out['frontier_waypoints'] = dict(seconds=med, min=lo, max=hi, points=args.envs, lookahead=16, with_a_path=float((chosen >= 0).float().mean()),
                                         mean_index=float(chosen[chosen >= 0].float().mean()))
        print(f"(f) seeded waypoints, {args.envs} x 1 points: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]; mean index {out['frontier_waypoints']['mean_index']:.2f}")
        goals = table[:, :, 1].contiguous()
        single = cuda.distance_fields(grid, goals, passes=True)
        med, lo, hi = timed(lambda: single.update(), args.repeats, args.warmup)
        out['frontier_single_goal'] = dict(seconds=med, min=lo, max=hi, goals=args.envs, passes_most=int(single.passes.max()),
                                           passes_median=int(single.passes.median()))
        print(f"(f) distance_fields on the same grid, {args.envs} goals: {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}]; most passes {int(single.passes.max())}")
        # 80 % seen: every cell marked but a random fifth
        maps.values.copy_((torch.rand(maps.values.shape, device='cuda') >= .2).to(torch.uint8))
        counted = (maps.values[:grid.n_cells] & maps.countable[:grid.n_cells] & 1).long()
        sums = torch.cat([torch.zeros(1, dtype=torch.int64, device='cuda'), counted.cumsum(0)])
        starts = torch.as_tensor(grid._host_starts, device='cuda')
        maps.totals.copy_((sums[starts[1:]] - sums[starts[:-1]]).int()[:, None])
        med, lo, hi = timed(lambda: frontier.update(), args.repeats, args.warmup)
        out['frontier_80_percent'] = dict(seconds=med, min=lo, max=hi, fields=args.envs, **stats(frontier))
        print(f"(f) frontier_fields, {args.envs} maps 80 % seen: {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}]; {out['frontier_80_percent']}")
        del sc, c, grid, maps, frontier, single
        torch.cuda.empty_cache()
        env = FloorCoverage(args.envs, geometries=geoms)
        eager, graphed = env_rates(env, args.envs, 60, 10)
        del env
        torch.cuda.empty_cache()
        env = ExpertStep(FloorCoverage(args.envs, geometries=geoms))
        expert_eager, expert_graphed = env_rates(env, args.envs, 60, 10)
        out['frontier_expert_step'] = dict(step_eager_seconds=eager, step_graph_seconds=graphed, expert_step_eager_seconds=expert_eager,
                                           expert_step_graph_seconds=expert_graphed)
        print(f'(f) FloorCoverage({args.envs}): step eager {eager*1e3:.3f} ms, graph {graphed*1e3:.3f} ms; expert + step eager {expert_eager*1e3:.3f} ms, '
              f'graph {expert_graphed*1e3:.3f} ms')
        del env
        torch.cuda.empty_cache()

    if want('window'):
        from megastep_amd.demo.envs.floorcoverage import reachable
        HBM = 6.3e12                                                     # bytes/s the HBM sustains (MI355X_MICROARCH.md; 8e12 spec)
        sc = scene.scenery(geoms, 1, device='cuda')
        c = core.Core(sc, res=256, fov=130)
        table = torch.as_tensor(modules.random_empty_positions(geoms, 1, 4), dtype=torch.float32, device='cuda')
        c.agents.positions[:] = table[:, :, 0]
        c.agents.angles.uniform_(-180, 180)
        grid = cuda.nav_grid(sc, config=c.config)
        maps = cuda.seen_maps(grid, 1, reachable(grid, table[:, 0, 0]))
        maps.mark_render(c.agents, cuda.render(sc, c.agents, fields=('distances',)))
        frontier = maps.frontier_fields()
        floor, wall = cuda.map_channel(grid, gate=maps), cuda.map_channel(grid, where=False, gate=maps)
        far = cuda.map_channel(frontier, scale=.1)
        k, batch = min(args.torch_envs, args.envs), 20
        for name, size, samples, channels, plain in (
                ('window_32', 32, 1, [floor, wall], [(grid.free, False, True, 0., maps.values), (grid.free, False, False, 0., maps.values)]),
                ('window_64', 64, 2, [floor, wall, far], [(grid.free, False, True, 0., maps.values), (grid.free, False, False, 0., maps.values),
                                                          (frontier.values, True, True, .1, None)])):
            views = cuda.agent_views(c.agents, size, 4.)
            buffer = cuda.local_maps(grid, views, size, channels, samples=samples)

            def calls():
                for _ in range(batch):
                    cuda.local_maps(grid, views, size, channels, samples=samples, out=buffer)
            med, lo, hi = (t/batch for t in timed(calls, args.repeats, args.warmup))
            nbytes = buffer.numel()*4
            run = torch_windows(grid, views, (size, size), samples, plain, k)
            same = bool(torch.equal(run().view(torch.int32), buffer[:k].view(torch.int32)))
            tmed = timed(lambda: run(), max(args.repeats//3, 2), 1)[0]
            over = modules.Overhead(c, size=size, radius=4.)
            omed = timed(lambda: over(), args.repeats, args.warmup)[0]
            out[name] = dict(seconds=med, min=lo, max=hi, size=size, samples=samples, channels=len(channels), output_bytes=nbytes,
                             bytes_per_second=nbytes/med, share_of_hbm_sustained=nbytes/med/HBM, torch_envs=k, torch_seconds=tmed,
                             torch_scaled_seconds=tmed*args.envs/k, torch_equal_bits=same, overhead_seconds=omed)
            print(f'(w) local_maps, {args.envs} x 1 x {len(channels)} x {size} x {size}, samples={samples}: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}] a call '
                  f'({batch} back to back); {nbytes/1e6:.1f} MB out -> {nbytes/med/1e12:.2f} TB/s, {100*nbytes/med/HBM:.0f} % of 6.3 TB/s; torch, {k} envs: '
                  f'{tmed*1e3:.2f} ms -> {tmed*args.envs/k*1e3:.1f} ms for {args.envs}, equal bits: {same}; modules.Overhead at {size}: {omed*1e6:.1f} us')
            del over, buffer
        del sc, c, grid, maps, frontier
        torch.cuda.empty_cache()
        for name, make in (('FloorCoverage_local_map', lambda: FloorCoverage(args.envs, geometries=geoms, local_map=True)),
                           ('FloorCoverage_plain', lambda: FloorCoverage(args.envs, geometries=geoms))):
            env = make()
            eager, graphed = env_rates(env, args.envs, 60, 10)
            out[name] = dict(eager_seconds=eager, graph_seconds=graphed)
            print(f'(w) {name}({args.envs}).step: eager {eager*1e3:.3f} ms, graph replay {graphed*1e3:.3f} ms')
            del env
            torch.cuda.empty_cache()

    if want('draws'):
        sc = scene.scenery(geoms, 1, device='cuda', bake=False)
        c = core.Core(sc, res=64)
        grid = cuda.nav_grid(sc, config=c.config)
        table = torch.as_tensor(modules.random_empty_positions(geoms, 1, 4), dtype=torch.float32, device='cuda')
        fields = cuda.distance_fields(grid, table[:, :, 0].contiguous())
        cells = np.diff(grid._host_starts)
        k, batch = min(args.torch_envs, args.envs), 20
        for K in (1, 64):
            draws = cuda.cell_draws(grid, fields, 1, K, lo=2., hi=8., seed=7)
            cells_first, counts = draws.cells[:k, 0].long().clone(), draws.counts[:k, 0].long().clone()

            def calls():
                for _ in range(batch):
                    draws.again()
            med, lo, hi = (t/batch for t in timed(calls, args.repeats, args.warmup))
            run = torch_draws(grid, fields.values, 2., 8., K, 7, k)
            got = run()
            same = bool(torch.equal(got[0], cells_first) and torch.equal(got[1], counts))
            tmed = timed(lambda: run(), max(args.repeats//3, 2), 1)[0]
            out[f'draws_{K}'] = dict(seconds=med, min=lo, max=hi, sets=args.envs, draws=K, cells_largest=int(cells.max()), cells_median=int(np.median(cells)),
                                     qualifying_mean=float(draws.counts.float().mean()), empty_sets=int((draws.counts == 0).sum()), torch_envs=k,
                                     torch_seconds=tmed, torch_scaled_seconds=tmed*args.envs/k, torch_equal=same)
            print(f"(d) cell_draws, {args.envs} x 1 sets of {K}: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}] a call ({batch} back to back); "
                  f"{out[f'draws_{K}']['qualifying_mean']:.0f} cells qualify a set; torch, {k} envs: {tmed*1e3:.2f} ms -> {tmed*args.envs/k*1e3:.1f} ms "
                  f'for {args.envs}, equal cells and counts: {same}')
        del sc, c, grid, fields, draws
        torch.cuda.empty_cache()
        for name, make in (('PointGoal_sampled', lambda: PointGoal(args.envs, geometries=geoms, goal_range=(2., 8.), sampled_spawns=True)),
                           ('PointGoal_plain', lambda: PointGoal(args.envs, geometries=geoms))):
            env = make()
            eager, graphed = env_rates(env, args.envs, 60, 10)
            out[name] = dict(eager_seconds=eager, graph_seconds=graphed)
            print(f'(d) {name}({args.envs}).step: eager {eager*1e3:.3f} ms, graph replay {graphed*1e3:.3f} ms')
            del env
            torch.cuda.empty_cache()

    if want('regions'):
        from megastep_amd.demo.envs.floorcoverage import reachable
        sc = scene.scenery(geoms, 1, device='cuda')
        c = core.Core(sc, res=256, fov=130)
        table = torch.as_tensor(modules.random_empty_positions(geoms, 1, 4), dtype=torch.float32, device='cuda')
        c.agents.positions[:] = table[:, :, 0]
        c.agents.angles.uniform_(-180, 180)
        grid = cuda.nav_grid(sc, config=c.config)
        passes = lambda r: dict(passes_most=int(r.passes.max()), passes_median=int(r.passes.median()))
        r = cuda.regions(grid, passes=True)
        med, lo, hi = timed(lambda: r.update(), args.repeats, args.warmup)
        spawn = table[:, 0, 0].contiguous()
        rmed, rlo, rhi = timed(lambda: reachable(grid, spawn), args.repeats, args.warmup)
        layer = r.masks(points=spawn[:, None].contiguous())
        same = bool(torch.equal(layer.values[:grid.n_cells], reachable(grid, spawn)[:grid.n_cells]))
        out['regions'] = dict(seconds=med, min=lo, max=hi, fields=args.envs, regions_mean=float(r.counts.float().mean()), regions_most=int(r.counts.max()),
                              reachable_seconds=rmed, reachable_min=rlo, reachable_max=rhi, mask_equal_bytes=same, **passes(r))
        print(f"(r) regions, {args.envs} grids: {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}]; {out['regions']}")
        batch = 20

        def calls():
            for _ in range(batch):
                r.masks(points=spawn[:, None], out=layer)
        mmed, mlo, mhi = (t/batch for t in timed(calls, args.repeats, args.warmup))
        out['region_masks'] = dict(seconds=mmed, min=mlo, max=mhi, requests=args.envs, bytes=int(grid.n_cells))
        print(f'(r) masks, {args.envs} x 1 requests, {grid.n_cells/1e6:.1f} MB out: {mmed*1e6:.1f} us [{mlo*1e6:.1f}, {mhi*1e6:.1f}] a call ({batch} back to back)')
        k = min(args.torch_envs, args.envs)
        run = torch_regions(grid, k)
        L, sweeps = run()
        same = all(torch.equal(L[e, 1:grid.cells(e)[1] + 1, 1:grid.cells(e)[2] + 1], r.image(e)) for e in range(k))
        tmed = timed(lambda: run(), max(args.repeats//3, 2), 1)[0]
        out['regions_torch'] = dict(envs=k, seconds=tmed, scaled_seconds=tmed*args.envs/k, sweeps=sweeps, equal_labels=bool(same))
        print(f'(r) torch min-label sweeps, {k} grids: {tmed*1e3:.1f} ms, {sweeps} sweeps -> {tmed*args.envs/k*1e3:.1f} ms for {args.envs}; equal labels: {same}')
        maps = cuda.seen_maps(grid, 1, reachable(grid, spawn))
        maps.mark_render(c.agents, cuda.render(sc, c.agents, fields=('distances',)))
        fr = maps.frontier_regions(passes=True)
        med, lo, hi = timed(lambda: fr.update(), args.repeats, args.warmup)
        out['frontier_regions_first_frame'] = dict(seconds=med, min=lo, max=hi, fields=args.envs, regions_mean=float(fr.counts.float().mean()), **passes(fr))
        print(f"(r) frontier_regions, {args.envs} maps after one frame: {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}]; {out['frontier_regions_first_frame']}")
        maps.values.copy_((torch.rand(maps.values.shape, device='cuda') >= .2).to(torch.uint8))
        med, lo, hi = timed(lambda: fr.update(), args.repeats, args.warmup)
        out['frontier_regions_80_percent'] = dict(seconds=med, min=lo, max=hi, fields=args.envs, regions_mean=float(fr.counts.float().mean()), **passes(fr))
        print(f"(r) frontier_regions, {args.envs} maps 80 % seen: {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}]; {out['frontier_regions_80_percent']}")
        del sc, c, grid, maps, fr, r, layer
        torch.cuda.empty_cache()
        for name, extra in (('PointGoal_one_region', dict(one_region=True)), ('PointGoal_sampled', dict())):
            env = PointGoal(args.envs, geometries=geoms, goal_range=(2., 8.), sampled_spawns=True, **extra)
            eager, graphed = env_rates(env, args.envs, 60, 10)
            out[name] = dict(eager_seconds=eager, graph_seconds=graphed)
            print(f'(r) {name}({args.envs}).step: eager {eager*1e3:.3f} ms, graph replay {graphed*1e3:.3f} ms')
            del env
            torch.cuda.empty_cache()

    if want('views'):
        from megastep_amd.demo.envs.floorcoverage import reachable
        sc = scene.scenery(geoms, 1, device='cuda')
        c = core.Core(sc, res=256, fov=130)
        table = torch.as_tensor(modules.random_empty_positions(geoms, 1, 17), dtype=torch.float32, device='cuda')
        c.agents.positions[:] = table[:, :, 0]
        c.agents.angles.uniform_(-180, 180)
        grid = cuda.nav_grid(sc, config=c.config)
        maps = cuda.seen_maps(grid, 1, reachable(grid, table[:, 0, 0]))
        maps.mark_render(c.agents, cuda.render(sc, c.agents, fields=('distances',)))
        k, batch = min(args.torch_envs, args.envs), 20
        cells = np.diff(grid._host_starts)
        walls = (sc.lines.widths - sc.n_agents*sc.model.shape[0]).float()
        for name, pts, R, kw in (('views_1_store', table[:, 0, :1].contiguous(), 10., dict()),
                                 ('views_16_gains', table[:, 0, 1:17].contiguous(), 5., dict(unseen=maps, store=False))):
            v = cuda.view_fields(grid, sc, pts, R, countable=maps.countable, **kw)

            def calls():
                for _ in range(batch):
                    v.update()
            med, lo, hi = (t/batch for t in timed(calls, args.repeats, args.warmup))
            run = torch_views(grid, sc, pts, R, maps.countable, kw.get('unseen'), None, k)
            vis, counts, gains = run()
            same = bool(torch.equal(counts, v.counts[:k].long()))
            if v.gains is not None:
                same = same and bool(torch.equal(gains, v.gains[:k].long()))
            if v.values is not None:
                same = same and all(torch.equal(vis[e, p, :grid.cells(e)[1], :grid.cells(e)[2]], v.image(e, p)) for e in range(k) for p in range(pts.shape[1]))
            tmed = timed(lambda: run(), 2, 1)[0]
            out[name] = dict(seconds=med, min=lo, max=hi, viewpoints=pts.shape[1], max_range=R, store=v.values is not None, cells_largest=int(cells.max()),
                             cells_median=int(np.median(cells)), walls_mean=float(walls.mean()), walls_most=int(walls.max()),
                             counts_mean=float(v.counts.float().mean()), gains_mean=float(v.gains.float().mean()) if v.gains is not None else None,
                             torch_envs=k, torch_seconds=tmed, torch_scaled_seconds=tmed*args.envs/k, torch_equal=same,
                             faster_than_torch=bool(med < tmed*args.envs/k))
            print(f"(v) view_fields, {args.envs} x {pts.shape[1]} viewpoints, R = {R}, store={v.values is not None}: {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}] "
                  f"a call ({batch} back to back); {out[name]['counts_mean']:.0f} countable cells in sight; torch, {k} envs: {tmed*1e3:.1f} ms -> "
                  f"{tmed*args.envs/k*1e3:.0f} ms for {args.envs}, equal: {same}")
            assert same and med < tmed*args.envs/k, 'the kernel must equal the torch formulation and be the faster'
            del v, run, vis
        angle = torch.arange(720, device='cuda').float()*(2*np.pi/720)
        dirs = torch.stack([angle.cos(), angle.sin()], -1)[None].expand(args.envs, 720, 2).contiguous()
        origins = table[:, 0, :1].expand(args.envs, 720, 2).contiguous()
        ring = cuda.raycast(sc, origins, dirs, fields=('distances',), config=c.config)
        scratch = cuda.seen_maps(grid, 1, maps.countable)
        gained = torch.empty((args.envs, 1), dtype=torch.int32, device='cuda')

        def ring_and_mark():
            cuda.raycast(sc, origins, dirs, fields=('distances',), config=c.config, out=ring)
            scratch.mark(table[:, 0, :1].contiguous(), dirs[:, None], ring.distances[:, None], out=gained)
        med, lo, hi = timed(ring_and_mark, args.repeats, args.warmup)
        out['views_ring_and_mark'] = dict(seconds=med, min=lo, max=hi, rays=720)
        print(f'(v) raycast of a 720-ray ring + mark, {args.envs} envs (time only: another rule): {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}]')
        del sc, c, grid, maps, scratch, ring
        torch.cuda.empty_cache()
        for name, kind in (('FloorCoverage_views_expert', ('views',)), ('FloorCoverage_frontier_expert', ())):
            env = ExpertStep(FloorCoverage(args.envs, geometries=geoms), *kind)
            eager, graphed = env_rates(env, args.envs, 60, 10)
            out[name] = dict(expert_step_eager_seconds=eager, expert_step_graph_seconds=graphed)
            print(f'(v) {name}({args.envs}): expert + step eager {eager*1e3:.3f} ms, graph {graphed*1e3:.3f} ms')
            del env
            torch.cuda.empty_cache()
        small = cubicasa.sample(64, seed=7, n_unique=64)
        for policy in ('views', 'frontier', 'random'):
            torch.manual_seed(3); np.random.seed(3)
            out['coverage_' + policy] = score = coverage_score(FloorCoverage(64, geometries=small, max_lifespan=300), 300, policy)
            print(f'(v) FloorCoverage(64), 300 steps, {policy}: {score}')

    if want('basins'):
        from megastep_amd.demo.envs.floorcoverage import reachable
        sc = scene.scenery(geoms, 1, device='cuda')
        c = core.Core(sc, res=256, fov=130)
        table = torch.as_tensor(modules.random_empty_positions(geoms, 1, 4), dtype=torch.float32, device='cuda')
        c.agents.positions[:] = table[:, :, 0]
        c.agents.angles.uniform_(-180, 180)
        grid = cuda.nav_grid(sc, config=c.config)
        passes = lambda b: dict(passes_most=int(b.passes.max()), passes_median=int(b.passes.median()))
        maps = cuda.seen_maps(grid, 1, reachable(grid, table[:, 0, 0].contiguous()))
        maps.mark_render(c.agents, cuda.render(sc, c.agents, fields=('distances',)))
        frontier, clusters = maps.frontier_fields(passes=True), maps.frontier_regions()
        fmed, flo, fhi = timed(lambda: frontier.update(), args.repeats, args.warmup)
        b = cuda.basins(frontier, ids=clusters.labels, passes=True)
        med, lo, hi = timed(lambda: b.update(), args.repeats, args.warmup)
        out['basins_frontier'] = dict(seconds=med, min=lo, max=hi, fields=args.envs, seeded_fields_seconds=fmed, seeded_fields_min=flo,
                                      seeded_fields_max=fhi, reached_mean=float(b.reached.float().mean()), clusters_mean=float(clusters.counts.float().mean()),
                                      **passes(b))
        print(f"(z) basins of the frontier field, {args.envs} maps after one frame: {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}] next to "
              f"seeded_fields {fmed*1e3:.3f} ms; {out['basins_frontier']}")
        points = table[:, 0, 1:3].contiguous()                          # (two points an env: the two agents)
        seeds = cuda.point_marks(grid, points, n_fields=1)
        near = cuda.seeded_fields(grid, seeds.marks, 1, passes=True)
        own = cuda.basins(near, ids=seeds.ids, n_ids=2, passes=True)
        smed, slo, shi = timed(lambda: seeds.update(), args.repeats, args.warmup)
        nmed, nlo, nhi = timed(lambda: near.update(), args.repeats, args.warmup)
        med, lo, hi = timed(lambda: own.update(), args.repeats, args.warmup)
        out['basins_two_agents'] = dict(seconds=med, min=lo, max=hi, fields=args.envs, point_marks_seconds=smed, seeded_fields_seconds=nmed,
                                        seeded_fields_min=nlo, seeded_fields_max=nhi, smaller_share_mean=float((own.sizes[:, 0].min(-1).values.float()
                                                                                                           / own.reached[:, 0].clamp(min=1).float()).mean()),
                                        field_passes_most=int(near.passes.max()), **passes(own))
        print(f"(z) basins of a two-agent point_marks field, {args.envs} envs, n_ids=2: {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}] next to point_marks "
              f"{smed*1e6:.1f} us and seeded_fields {nmed*1e3:.3f} ms; {out['basins_two_agents']}")
        k = min(args.torch_envs, args.envs)
        run = torch_basins(grid, near, seeds.ids, k)
        L, jumps = run()
        same = all(torch.equal(L[e, 1:grid.cells(e)[1] + 1, 1:grid.cells(e)[2] + 1], own.image(e)) for e in range(k))
        tmed = timed(lambda: run(), max(args.repeats//3, 2), 1)[0]
        out['basins_torch'] = dict(envs=k, seconds=tmed, scaled_seconds=tmed*args.envs/k, jumps=jumps, equal_labels=bool(same))
        print(f'(z) torch successors and N = N[N], {k} grids: {tmed*1e3:.1f} ms, {jumps} jumps -> {tmed*args.envs/k*1e3:.1f} ms for {args.envs}; equal labels: {same}')
        spot = table[:, 0, 3:4].contiguous()
        amed, alo, ahi = timed(lambda: own.at(spot), 5*args.repeats, args.warmup)
        out['basins_at'] = dict(seconds=amed, min=alo, max=ahi, points=args.envs)
        print(f'(z) Basins.at, {args.envs} x 1 points: {amed*1e6:.1f} us [{alo*1e6:.1f}, {ahi*1e6:.1f}]')
        del sc, c, grid, maps, frontier, clusters, b, seeds, near, own, run, L
        torch.cuda.empty_cache()
        for name, kind in (('FloorCoverage_shared_split_expert', ('split',)), ('FloorCoverage_shared_frontier_expert', ())):
            env = ExpertStep(FloorCoverage(args.envs, n_agents=2, shared=True, geometries=geoms), *kind)
            eager, graphed = env_rates(env, args.envs, 60, 10)
            out[name] = dict(expert_step_eager_seconds=eager, expert_step_graph_seconds=graphed)
            print(f'(z) {name}({args.envs}, n_agents=2): expert + step eager {eager*1e3:.3f} ms, graph {graphed*1e3:.3f} ms')
            del env
            torch.cuda.empty_cache()
        small = cubicasa.sample(64, seed=7, n_unique=64)
        for policy in ('split', 'frontier', 'random'):
            torch.manual_seed(3); np.random.seed(3)
            env = FloorCoverage(64, n_agents=2, shared=True, geometries=small, max_lifespan=300)
            out['shared_coverage_' + policy] = score = coverage_score(env, 300, policy)
            print(f'(z) FloorCoverage(64, n_agents=2, shared=True), 300 steps, {policy}: {score}')

    if want('clearance'):
        from megastep_amd import _lib, nav
        R, radii = 2., (core.AGENT_RADIUS, .2, .3)
        sc = scene.scenery(geoms, 1, device='cuda', bake=False)
        grid = cuda.nav_grid(sc, clearance=core.AGENT_RADIUS)
        cells = np.diff(grid._host_starts)
        walls = sc.lines.widths.cpu().numpy() - sc.model.shape[0]
        shape = dict(cells_total=int(grid.n_cells), cells_largest=int(cells.max()), cells_median=int(np.median(cells)), walls_most=int(walls.max()),
                     walls_median=int(np.median(walls)), max_range=R)
        h = _lib.lib()
        bare = cuda.clearance_fields(grid, sc, R)
        full = cuda.clearance_fields(grid, sc, R, nearest=True, radii=radii)
        try:
            for mode, name in ((1, 'tile'), (2, 'tile_wave')):
                h.ms_debug_nav_clear_cull(mode)
                for clear, kind in ((bare, 'values'), (full, 'all')):
                    med, lo, hi = timed(lambda: clear.update(), 20, args.warmup)
                    out[f'clearance_{name}_{kind}'] = dict(seconds=med, min=lo, max=hi, **shape)
                    print(f'(c2) clearance_fields, {name} cull, {kind}: {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}]')
        finally:
            h.ms_debug_nav_clear_cull(-1)
        med, lo, hi = timed(lambda: nav._launch(grid.free.device, 'free', grid, None, sc._as_struct()), 20, args.warmup)
        out['clearance_nav_free'] = dict(seconds=med, min=lo, max=hi)
        print(f'(c2) ms_nav_free on the same grid: {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}]')
        k = min(args.torch_envs, args.envs)
        run = torch_clearance(grid, sc, R, k)
        V, I = run()
        same = all(torch.equal(V[e, :grid.cells(e)[1], :grid.cells(e)[2]].view(torch.int32), full.image(e).view(torch.int32)) and
                   torch.equal(I[e, :grid.cells(e)[1], :grid.cells(e)[2]], full.nearest_image(e)) for e in range(k))
        tmed = timed(lambda: run(), 2, 1)[0]
        out['clearance_torch'] = dict(envs=k, seconds=tmed, scaled_seconds=tmed*args.envs/k, equal_bits=bool(same))
        print(f'(c2) torch loop over walls, {k} grids: {tmed*1e3:.1f} ms -> {tmed*args.envs/k*1e3:.1f} ms for {args.envs}; equal bits: {same}')
        del sc, grid, bare, full, run, V, I
        torch.cuda.empty_cache()
        sc = scene.scenery(geoms, 4, device='cuda', bake=False)
        c = core.Core(sc, res=64)
        c.agents.positions[:] = torch.as_tensor(modules.random_empty_positions(geoms, 4, 1), dtype=torch.float32, device='cuda')[:, :, 0]
        own = torch.arange(4, dtype=torch.int32, device='cuda').expand(args.envs, 4).contiguous()
        reading = cuda.clearance(sc, c.agents.positions, R, agents=c.agents, skip=own)
        med, lo, hi = timed(lambda: cuda.clearance(sc, c.agents.positions, R, agents=c.agents, skip=own, out=reading), 5*args.repeats, args.warmup)
        out['clearance_query'] = dict(seconds=med, min=lo, max=hi, points=4*args.envs, in_range=float(torch.isfinite(reading.distances).float().mean()))
        print(f'(c2) clearance, {args.envs} x 4 points with agents: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]')
        for name, module in (('Proximity', modules.Proximity(c, R)), ('IMU', modules.IMU(c))):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                module()
            torch.cuda.current_stream().wait_stream(side)
            eager = timed(lambda: module(), 5*args.repeats, args.warmup)[0]
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                module()
            graphed = timed(lambda: g.replay(), 5*args.repeats, args.warmup)[0]
            out[f'clearance_{name}'] = dict(eager_seconds=eager, graph_seconds=graphed, envs=args.envs, agents=4)
            print(f'(c2) modules.{name}({args.envs} x 4): eager {eager*1e6:.1f} us, graph replay {graphed*1e6:.1f} us')
        del sc, c
        torch.cuda.empty_cache()

    if want('cost'):
        from megastep_amd import _lib
        sc = scene.scenery(geoms, 1, device='cuda')
        c = core.Core(sc, res=256, fov=130)
        table = torch.as_tensor(modules.random_empty_positions(geoms, 1, 4), dtype=torch.float32, device='cuda')
        c.agents.positions[:] = table[:, :, 0]
        c.agents.angles.uniform_(-180, 180)
        grid = cuda.nav_grid(sc, config=c.config)
        cells = np.diff(grid._host_starts)
        seeds = cuda.point_marks(grid, table[:, :, 1].contiguous(), 1)
        points = table[:, :, 0].contiguous()
        seeded = cuda.seeded_fields(grid, seeds.marks, 1, passes=True)
        med, lo, hi = timed(lambda: seeded.update(), args.repeats, args.warmup)
        out['cost_seeded'] = dict(seconds=med, min=lo, max=hi, fields=args.envs, passes_most=int(seeded.passes.max()), passes_median=int(seeded.passes.median()),
                                  cells_largest=int(cells.max()), cells_median=int(np.median(cells)))
        print(f"(k) seeded_fields on the goal's cells, {args.envs} fields: {med*1e3:.3f} ms [{lo*1e3:.3f}, {hi*1e3:.3f}]; {out['cost_seeded']}")
        maps = cuda.seen_maps(grid, 1)
        maps.mark_render(c.agents, cuda.render(sc, c.agents, fields=('distances',)))
        clear = cuda.clearance_fields(grid, sc, max_range=.5)
        layers = dict(ones=torch.ones(max(grid.n_cells, 1), device='cuda'), inflation=cuda.inflation_costs(clear, .5), known_space=cuda.mark_costs(maps))
        for name, layer in layers.items():
            fields = cuda.cost_fields(grid, seeds.marks, 1, layer, passes=True)
            values = {}
            for which, label in ((0, 'global'), (1, 'lds')):
                _lib.lib().ms_debug_nav_cost_variant(which)
                med, lo, hi = timed(lambda: fields.update(), args.repeats, args.warmup)
                values[label] = fields.values.clone()
                out[f'cost_{name}_{label}'] = dict(seconds=med, min=lo, max=hi, fields=args.envs, passes_most=int(fields.passes.max()),
                                                   passes_median=int(fields.passes.median()))
                print(f"(k) cost_fields, {name}, multipliers {'in LDS' if which else 'from global memory'}, {args.envs} fields: {med*1e3:.3f} ms "
                      f"[{lo*1e3:.3f}, {hi*1e3:.3f}]; passes most {int(fields.passes.max())}, median {int(fields.passes.median())}")
            _lib.lib().ms_debug_nav_cost_variant(-1)
            out[f'cost_{name}_variants_equal_bits'] = bool(torch.equal(values['global'].view(torch.int32), values['lds'].view(torch.int32)))
            if name == 'ones':
                out['cost_ones_equals_seeded_bits'] = bool(torch.equal(values['global'].view(torch.int32), seeded.values.view(torch.int32)))
        inflated = cuda.cost_fields(grid, seeds.marks, 1, layers['inflation'])
        way = torch.empty_like(points)
        for name, fields in (('seeded', seeded), ('cost', inflated)):
            med, lo, hi = timed(lambda: fields.waypoints(points, out=way), 5*args.repeats, args.warmup)
            chosen = fields.waypoints(points, hops=True)[1]
            out[f'cost_waypoints_{name}'] = dict(seconds=med, min=lo, max=hi, points=args.envs, lookahead=16, mean_index=float(chosen[chosen >= 0].float().mean()))
            print(f'(k) {name} waypoints, {args.envs} x 1 points: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]')
        k = min(args.torch_envs, args.envs)
        run = torch_cost_fields(grid, seeds.marks, layers['inflation'], k)
        D, sweeps = run()
        same = all(torch.equal(D[e, 1:grid.cells(e)[1] + 1, 1:grid.cells(e)[2] + 1].view(torch.int32), inflated.image(e, 0).view(torch.int32)) for e in range(k))
        med, lo, hi = timed(lambda: run(), max(args.repeats//3, 2), 1)
        out['cost_torch'] = dict(envs=k, seconds=med, scaled_seconds=med*args.envs/k, sweeps=sweeps, equal_bits=bool(same))
        print(f'(k) torch sweeps, inflation, {k} fields: {med*1e3:.1f} ms, {sweeps} sweeps -> {med*args.envs/k*1e3:.1f} ms for {args.envs}; equal bits: {same}')
        del sc, c, grid, maps, clear, seeded, inflated, fields, layers
        torch.cuda.empty_cache()
        for name, kw in (('PointGoal', {}), ('PointGoal_margin', dict(margin=.3))):
            env = ExpertStep(PointGoal(args.envs, geometries=geoms, **kw))
            eager, graphed = env_rates(env, args.envs, 60, 10)
            out[f'cost_{name}_expert_step'] = dict(eager_seconds=eager, graph_seconds=graphed)
            print(f'(k) {name}({args.envs}): expert + step eager {eager*1e3:.3f} ms, graph {graphed*1e3:.3f} ms')
            del env
            torch.cuda.empty_cache()
        small = cubicasa.sample(64, seed=7, n_unique=64)
        for name, kw in (('plain', {}), ('margin', dict(margin=.3))):
            torch.manual_seed(3); np.random.seed(3)
            out['cost_follower_' + name] = score = follower_score(PointGoal(64, geometries=small, **kw), 300)
            print(f'(k) PointGoal(64), 300 steps under the expert, {name}: {score}')

    if want('ages'):
        sc = scene.scenery(geoms, 1, device='cuda')
        c = core.Core(sc, res=256, fov=130)
        table = torch.as_tensor(modules.random_empty_positions(geoms, 1, 4), dtype=torch.float32, device='cuda')
        c.agents.positions[:] = table[:, :, 0]
        c.agents.angles.uniform_(-180, 180)
        grid = cuda.nav_grid(sc, config=c.config)
        frame = cuda.render(sc, c.agents, fields=('distances',))
        origins, dirs, distances = c.agents.positions, cuda.camera_rays(c.agents), frame.distances
        repeats = 2*args.repeats                                         # (medians of 20 calls back to back at the defaults)
        seen = cuda.seen_maps(grid, 1)
        buffer = seen.mark(origins, dirs, distances)
        med, lo, hi = timed(lambda: seen.mark(origins, dirs, distances, out=buffer), repeats, args.warmup)
        out['ages_seen_mark'] = dict(seconds=med, min=lo, max=hi, rays=256)
        print(f'(g) SeenMaps.mark, {args.envs} x 1 x 256 rays, the yardstick: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]')
        ages, lean = cuda.age_maps(grid, 1), cuda.age_maps(grid, 1, ages=False)
        sweep = ages.mark(origins, dirs, distances)
        first = {k: getattr(sweep, k).clone() for k in ('swept', 'gained', 'idle')}
        first.update({k: getattr(ages, k).clone() for k in ('last', 'clock', 'oldest', 'total_age', 'n_stale', 'stale', 'ages')})
        lean.mark(origins, dirs, distances)
        for name, maps, survey in (('mark(survey=False)', ages, False), ('mark + survey, no store of ages', lean, True), ('mark + survey + ages', ages, True)):
            med, lo, hi = timed(lambda: maps.mark(origins, dirs, distances, survey=survey, out=sweep), repeats, args.warmup)
            key = 'ages_mark' + ('' if not survey else '_survey' if maps is lean else '_survey_ages')
            out[key] = dict(seconds=med, min=lo, max=hi, rays=256, over_seen_mark=med/out['ages_seen_mark']['seconds'])
            print(f"(g) {name}, {args.envs} x 1 x 256 rays: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}], {out[key]['over_seen_mark']:.2f} x SeenMaps.mark")
        med, lo, hi = timed(lambda: ages.survey(), repeats, args.warmup)
        out['ages_survey'] = dict(seconds=med, min=lo, max=hi)
        print(f'(g) survey alone, {args.envs} maps: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]')
        k = min(args.torch_envs, args.envs)
        run = torch_ages(grid, ages.countable, origins, dirs, distances, 10., ages.threshold, k)
        n_cells = int(grid._host_starts[k])
        blank = (torch.zeros(n_cells, dtype=torch.float32, device='cuda'), torch.zeros(k, dtype=torch.int32, device='cuda'))
        got = dict(zip(('last', 'clock', 'swept', 'gained', 'idle', 'oldest', 'total_age', 'n_stale', 'stale', 'ages'), run(*blank)))
        same = all(torch.equal(v, first[name][:n_cells] if v.shape[0] == n_cells else first[name][:k, 0]) for name, v in got.items())
        med, lo, hi = timed(lambda: run(*blank), max(args.repeats//3, 2), 1)
        out['ages_torch'] = dict(envs=k, seconds=med, scaled_seconds=med*args.envs/k, equal=bool(same))
        print(f'(g) torch samples + scatter + dense pass, {k} envs: {med*1e3:.2f} ms -> {med*args.envs/k*1e3:.1f} ms for {args.envs}; equal results: {same}')
        del sc, c, grid, seen, ages, lean
        torch.cuda.empty_cache()
        for name, make in (('FloorCoverage', lambda: FloorCoverage(args.envs, geometries=geoms)), ('Patrol', lambda: Patrol(args.envs, geometries=geoms))):
            env = make()
            eager, graphed = env_rates(env, args.envs, 60, 10)
            out['ages_' + name] = dict(eager_seconds=eager, graph_seconds=graphed)
            print(f'(g) {name}({args.envs}).step: eager {eager*1e3:.3f} ms, graph replay {graphed*1e3:.3f} ms')
            del env
            torch.cuda.empty_cache()
        small = cubicasa.sample(64, seed=7, n_unique=64)
        for policy in ('expert', 'random'):
            torch.manual_seed(3); np.random.seed(3)
            env = Patrol(64, geometries=small, max_lifespan=10**6)
            world = env.reset()
            for _ in range(300):
                decision = env.expert() if policy == 'expert' else arrdict.arrdict(actions=torch.randint(0, 7, (64, 1), device='cuda'))
                world = env.step(decision)
            out['ages_rollout_' + policy] = score = dict(mean_idleness=float(env.ages.mean_age().mean()), worst_idleness=float(env.ages.oldest.float().mean()),
                                                       reward=float(world.reward.mean()))
            print(f'(g) Patrol(64), 300 steps, {policy}: {score}')

    if want('pulls'):
        from megastep_amd import _lib
        sc = scene.scenery(geoms, 1, device='cuda', bake=False)
        c = core.Core(sc, res=64)
        grid = cuda.nav_grid(sc, config=c.config)
        table = torch.as_tensor(modules.random_empty_positions(geoms, 1, 4), dtype=torch.float32, device='cuda')
        goals, points = table[:, :, 0].contiguous(), table[:, :, 1].contiguous()
        fields = cuda.distance_fields(grid, goals)
        at = fields.at(points)
        chain = fields.pulled(points, reach=1, max_points=2)
        there = chain.counts > 0
        out['pulls'] = dict(points=args.envs, with_a_path=float(there.float().mean()), chain_points_mean=float(chain.cells[there].float().mean()),
                            chain_points_most=int(chain.cells.max()))
        for reach in (64, 256):
            held = fields.pulled(points, reach=reach)
            for scheme, name in ((0, 'lane_a_candidate'), (1, 'lane_a_sample')):
                _lib.check(_lib.lib().ms_debug_nav_pull_scheme(scheme))
                med, lo, hi = timed(lambda: fields.pulled(points, reach=reach, out=held), 20, args.warmup)
                _lib.check(_lib.lib().ms_debug_nav_pull_scheme(-1))
                out['pulls'][f'reach_{reach}_{name}'] = dict(seconds=med, min=lo, max=hi)
                print(f'(h) pulled, {args.envs} x 1 paths, reach {reach}, {name.replace("_", " ")}: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]')
            out['pulls'][f'reach_{reach}'] = score = dict(
                vertices_mean=float(held.counts[there].float().mean()), vertices_most=int(held.counts.max()),
                pulled_over_chain=float((held.lengths[there]/chain.lengths[there]).mean()), pulled_over_at=float((held.lengths[there]/at[there]).mean()),
                shortened_by_2_per_cent=float((held.lengths[there] <= .98*chain.lengths[there]).float().mean()))
            print(f'(h) reach {reach}: {score}')
        med, lo, hi = timed(lambda: fields.paths(points, max_points=256), 20, args.warmup)
        out['pulls']['paths_256'] = dict(seconds=med, min=lo, max=hi)
        print(f'(h) paths(max_points=256) on the same fields and points: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]')
        way = torch.empty_like(points)
        med, lo, hi = timed(lambda: fields.waypoints(points, out=way), 20, args.warmup)
        out['pulls']['waypoints_16'] = dict(seconds=med, min=lo, max=hi)
        print(f'(h) waypoints() on the same fields and points: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]')
        del sc, grid, fields, held, chain
        torch.cuda.empty_cache()
        for name, kw in (('PointGoal', {}), ('PointGoal_spl', dict(spl=True))):
            env = PointGoal(args.envs, geometries=geoms, **kw)
            eager, graphed = env_rates(env, args.envs, 60, 10)
            out['pulls_' + name] = dict(eager_seconds=eager, graph_seconds=graphed)
            print(f'(h) PointGoal({args.envs}{", spl=True" if kw else ""}).step: eager {eager*1e3:.3f} ms, graph replay {graphed*1e3:.3f} ms')
            del env
            torch.cuda.empty_cache()
        small = cubicasa.sample(64, seed=7, n_unique=64)
        for policy in ('expert', 'random'):
            torch.manual_seed(3); np.random.seed(3)
            env = PointGoal(64, geometries=small, max_lifespan=120, spl=True)
            world = env.reset()
            scores = []
            for _ in range(300):
                decision = env.expert() if policy == 'expert' else arrdict.arrdict(actions=torch.randint(0, 7, (64, 1), device='cuda'))
                world = env.step(decision)
                scores.append(world.spl.clone())
            scores = torch.stack(scores)
            ended = ~torch.isnan(scores)
            out['pulls_rollout_' + policy] = score = dict(episodes=int(ended.sum()), arrivals=int((scores[ended] > 0).sum()),
                                                        mean_spl=float(scores[ended].mean()) if ended.any() else None,
                                                        mean_spl_of_arrivals=float(scores[ended][scores[ended] > 0].mean()) if (scores[ended] > 0).any() else None)
            print(f'(h) PointGoal(64, spl=True), 300 steps, {policy}: {score}')

    if want('zones'):
        from megastep_amd.demo.envs.floorcoverage import reachable
        K = 64
        sc = scene.scenery(geoms, 2, device='cuda')
        c = core.Core(sc, res=256, fov=130)
        table = torch.as_tensor(modules.random_empty_positions(geoms, 2, 2), dtype=torch.float32, device='cuda')
        c.agents.positions[:] = table[:, :, 0]
        c.agents.angles.uniform_(-180, 180)
        grid = cuda.nav_grid(sc, config=c.config)
        k = min(args.torch_envs, args.envs)
        # the grid's regions with one distance field
        rooms = cuda.regions(grid)
        field = cuda.distance_fields(grid, c.agents.positions[:, :1].contiguous())
        z = rooms.zones(values=field, n_zones=K)
        rmed, rlo, rhi = timed(lambda: rooms.update(), args.repeats, args.warmup)
        med, lo, hi = timed(lambda: z.update(), 2*args.repeats, args.warmup)
        run = torch_zones(grid, rooms.labels, field.values, 1, K, k)
        same = zones_equal(z, run(), k)
        tmed = timed(lambda: run(), max(args.repeats//3, 2), 1)[0]
        out['zones_regions'] = dict(seconds=med, min=lo, max=hi, fields=args.envs, regions_seconds=rmed, regions_min=rlo, regions_max=rhi,
                                    zones_mean=float(z.n_zones.float().mean()), zones_most=int(z.n_zones.max()), cells_total=int(grid.n_cells),
                                    torch_envs=k, torch_seconds=tmed, torch_scaled_seconds=tmed*args.envs/k, torch_equal=same)
        print(f"(n) zones of the grid's regions with a distance field, {args.envs} fields, K = {K}: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}] next to "
              f"regions {rmed*1e3:.3f} ms; torch, {k} envs: {tmed*1e3:.2f} ms -> {tmed*args.envs/k*1e3:.1f} ms, equal: {same}; {out['zones_regions']}")
        # the frontier clusters right after a marked frame, a distance field round each of the two agents
        maps = cuda.seen_maps(grid, 1, reachable(grid, table[:, 0, 0].contiguous()))
        slot = torch.zeros((args.envs, 2), dtype=torch.int32, device='cuda')
        maps.mark_render(c.agents, cuda.render(sc, c.agents, fields=('distances',)), slot=slot)
        clusters = maps.frontier_regions()
        around = cuda.distance_fields(grid, c.agents.positions.contiguous())
        z2 = cuda.zones(clusters, values=around, n_zones=K)
        cmed, clo, chi = timed(lambda: clusters.update(), args.repeats, args.warmup)
        amed = timed(lambda: around.update(), args.repeats, args.warmup)[0]
        med, lo, hi = timed(lambda: z2.update(), 2*args.repeats, args.warmup)
        run = torch_zones(grid, clusters.labels, around.values, 2, K, k)
        same = zones_equal(z2, run(), k)
        tmed = timed(lambda: run(), max(args.repeats//3, 2), 1)[0]
        out['zones_clusters'] = dict(seconds=med, min=lo, max=hi, fields=2*args.envs, frontier_regions_seconds=cmed, frontier_regions_min=clo,
                                     frontier_regions_max=chi, distance_fields_seconds=amed, clusters_mean=float(z2.n_zones.float().mean()),
                                     clusters_most=int(z2.n_zones.max()), reached_share=float(torch.isfinite(z2.least).any(-1).float().mean()),
                                     torch_envs=k, torch_seconds=tmed, torch_scaled_seconds=tmed*args.envs/k, torch_equal=same)
        print(f"(n) zones of the frontier clusters after one frame, {args.envs} envs x 2 agents, K = {K}: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}] next to "
              f"frontier_regions {cmed*1e3:.3f} ms and distance_fields {amed*1e3:.3f} ms; torch, {k} envs: {tmed*1e3:.2f} ms -> "
              f"{tmed*args.envs/k*1e3:.1f} ms, equal: {same}; {out['zones_clusters']}")
        del sc, c, grid, rooms, field, z, maps, clusters, around, z2, run
        torch.cuda.empty_cache()
        for kind in ('assign', 'split', 'frontier'):
            env = ExpertStep(FloorCoverage(args.envs, n_agents=2, shared=True, geometries=geoms), kind)
            eager, graphed = env_rates(env, args.envs, 60, 10)
            out[f'FloorCoverage_shared_{kind}_expert'] = dict(expert_step_eager_seconds=eager, expert_step_graph_seconds=graphed)
            print(f"(n) FloorCoverage({args.envs}, n_agents=2, shared=True), expert('{kind}') + step: eager {eager*1e3:.3f} ms, graph {graphed*1e3:.3f} ms")
            del env
            torch.cuda.empty_cache()
        small = cubicasa.sample(64, seed=7, n_unique=64)
        for policy in ('assign', 'split', 'frontier', 'random'):
            torch.manual_seed(3); np.random.seed(3)
            env = FloorCoverage(64, n_agents=2, shared=True, geometries=small, max_lifespan=300)
            out['zones_shared_coverage_' + policy] = score = coverage_score(env, 300, policy)
            print(f'(n) FloorCoverage(64, n_agents=2, shared=True), 300 steps, {policy}: {score}')

    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
