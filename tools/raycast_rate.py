"""Rays per second of cuda.raycast (ms_raycast) on the MI355X, with the wall grid and without it:

    python tools/raycast_rate.py [--envs 4096] [--rays 1024] [--distinct 1024] [--repeats 20] [--warmup 5] [--json out.json]

The world is the headline's: `--envs` envs over `--distinct` distinct synthetic floorplans, four agents each.  Every env casts
`--rays` rays against the static walls, then with the agents' bodies, in two workloads: 'scattered' - origins uniform over the
plan's bounding box, directions at random angles with lengths in [1, 4] (inside the grid's |ru|^2 range), every ray in a cell of
its own - and 'lidar' - a ring of `--rays`/agents rays around each agent, from its position; the same scenery is built twice, once baked
with the wall grid and once with bake(wall_grid=False).  Next to them, for scale: the depth-only render of the same world
(4 agents x 64 rays each).  Times are HIP events around single launches, after a warm-up; the median of the repeats is
reported (and the spread).  Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402
from megastep_amd import grids   # noqa: E402


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


def random_rays(scenery, n_rays, seed):
    """(N, R, 2) origins over each env's walls' bounding box and directions of length 1 to 4, on the device."""
    g = torch.Generator(device=scenery.lines.vals.device).manual_seed(seed)
    lo, hi = grids.wall_bounds(scenery)
    n = len(scenery.lines)
    dev = scenery.lines.vals.device
    u = torch.rand((n, n_rays, 2), generator=g, device=dev)
    origins = (lo[:, None, :] + u*(hi - lo)[:, None, :]).float().contiguous()
    ang = torch.rand((n, n_rays), generator=g, device=dev)*2*np.pi
    length = 1 + 3*torch.rand((n, n_rays), generator=g, device=dev)
    dirs = torch.stack([length*torch.cos(ang), length*torch.sin(ang)], -1).float().contiguous()
    return origins, dirs


def lidar_rays(agents, n_rays):
    """(N, R, 2): R/A rays in a ring around each agent of the env, from its position - rays that share their origins' cells."""
    n, a = agents.angles.shape
    per = n_rays//a
    ang = torch.arange(per, device=agents.angles.device, dtype=torch.float32)*(2*np.pi/per)
    ring = torch.stack([torch.cos(ang), torch.sin(ang)], -1)*1.25                      # (|ru| = 1.25: inside the grid's range)
    origins = agents.positions[:, :, None, :].expand(n, a, per, 2).reshape(n, a*per, 2).contiguous()
    dirs = ring[None, None].expand(n, a, per, 2).reshape(n, a*per, 2).contiguous()
    return origins, dirs


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--envs', type=int, default=4096)
    p.add_argument('--rays', type=int, default=1024)
    p.add_argument('--distinct', type=int, default=1024)
    p.add_argument('--agents', type=int, default=4)
    p.add_argument('--repeats', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--json', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('raycast_rate.py needs a GPU')
    from megastep_amd import core, cubicasa, cuda, modules, scene
    np.random.seed(0)
    torch.manual_seed(0)
    pool = cubicasa.sample(args.distinct, split='all', n_unique=max(args.distinct, 16), seed=1, workers=32, context='subprocess')
    geometries = [pool[i % len(pool)] for i in range(args.envs)]
    results = dict(envs=args.envs, rays_per_env=args.rays, distinct_plans=len(pool), agents=args.agents,
                   repeats=args.repeats, warmup=args.warmup)
    for grid in (True, False):
        sc = scene.scenery(geometries, args.agents, device='cuda', random=np.random.RandomState(0), fast=True, bake=False)
        cuda.bake(sc, wall_grid=grid)
        c = core.Core(sc, res=64, fov=130, fps=10)
        torch.manual_seed(1)                                             # (the same poses in both worlds)
        modules.RandomSpawns(geometries, c, fast=True)(c.agent_full(True))
        for kind, (origins, dirs) in (('scattered', random_rays(sc, args.rays, seed=2)), ('lidar', lidar_rays(c.agents, args.rays))):
            tag = kind + ('_grid' if grid else '_no_grid')
            total = origins.shape[0]*origins.shape[1]
            counter = torch.zeros(1, dtype=torch.int32, device='cuda')
            cuda.raycast(sc, origins, dirs, near=c.agent_radius, grid_rays=counter)
            torch.cuda.synchronize()
            out = cuda.raycast(sc, origins, dirs, near=c.agent_radius)
            t, lo, hi = timed(lambda: cuda.raycast(sc, origins, dirs, near=c.agent_radius, out=out), args.repeats, args.warmup)
            results[f'static_{tag}'] = dict(s=t, min_s=lo, max_s=hi, rays_per_s=total/t, grid_share=int(counter)/total,
                                            hit_share=float((out.indices >= 0).float().mean()))
            out_a = cuda.raycast(sc, origins, dirs, agents=c.agents)
            t, lo, hi = timed(lambda: cuda.raycast(sc, origins, dirs, agents=c.agents, out=out_a), args.repeats, args.warmup)
            results[f'agents_{tag}'] = dict(s=t, min_s=lo, max_s=hi, rays_per_s=total/t)
            for k in ('static', 'agents'):
                v = results[f'{k}_{tag}']
                print(f'{k:8s} {tag:20s} {v["s"]*1e3:8.3f} ms (min {v["min_s"]*1e3:.3f}, max {v["max_s"]*1e3:.3f})  '
                      f'{v["rays_per_s"]/1e9:7.3f} G rays/s' + (f'  grid share {v["grid_share"]:.3f}' if 'grid_share' in v else ''), flush=True)
            del out, out_a
        cuda.physics(sc, c.agents)
        r = cuda.render(sc, c.agents, fields=('distances',))
        t, lo, hi = timed(lambda: cuda.render(sc, c.agents, fields=('distances',), out=r), args.repeats, args.warmup)
        tag = 'grid' if grid else 'no_grid'
        results[f'render_depth_{tag}'] = v = dict(s=t, min_s=lo, max_s=hi, rays_per_s=args.envs*args.agents*64/t)
        print(f'{"render":8s} {"depth_" + tag:20s} {v["s"]*1e3:8.3f} ms (min {v["min_s"]*1e3:.3f}, max {v["max_s"]*1e3:.3f})  '
              f'{v["rays_per_s"]/1e9:7.3f} G rays/s', flush=True)
        del sc, c, r
        torch.cuda.empty_cache()
    for kind in ('scattered', 'lidar'):
        for k in ('static', 'agents'):
            results[f'grid_speedup_{k}_{kind}'] = results[f'{k}_{kind}_grid']['rays_per_s']/results[f'{k}_{kind}_no_grid']['rays_per_s']
    print(json.dumps(results))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
