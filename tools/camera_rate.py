"""What cameras that look from anywhere cost on the MI355X:

    python tools/camera_rate.py [--envs 4096] [--agents 4] [--distinct 1024] [--repeats 20] [--only launches|env] [--json out.json]

  (a) at `--envs` envs x `--agents` agents over `--distinct` distinct synthetic floorplans (the headline's world), agents at their
      spawn poses, each call between two HIP events of its own, `--repeats` calls back to back, the median and the range:
        cuda.render(fields=('screen', 'distances'))                 the yardstick: the agents' own 64-ray fans in one launch
        cuda.look of one plane camera per agent, 64 rays            the same rays as a raycast launch and a shade launch
        cuda.look of one 256-ray ring of 360 degrees per agent      a panorama
        cuda.shade alone on the plane cameras' hits                 with the share of rays that landed on an agent
        cuda.shade alone, the light grid withheld                   the plain light path next to the grid's
  (b) PointGoal(`--envs`, panorama=True).step under random actions, eager and as one HIP graph, next to the plain env's.
`--only` picks one part (for a profiler run of its own).  Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402


def back_to_back(fn, repeats, warmup=5):
    """Seconds per call of `fn`, each between two events of its own: (median, least, most)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b)*1e-3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def us(t):
    return f'{t[0]*1e6:.1f} us [{t[1]*1e6:.1f}, {t[2]*1e6:.1f}]'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--agents', type=int, default=4)
    ap.add_argument('--distinct', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--only', choices=('launches', 'env'))
    ap.add_argument('--json')
    args = ap.parse_args()
    from megastep_amd import arrdict, core, cubicasa, cuda, graphs, scene
    from megastep_amd.demo.envs.pointgoal import PointGoal
    from tests import util

    np.random.seed(0); torch.manual_seed(0)
    pool = cubicasa.sample(args.distinct, split='all', n_unique=args.distinct, workers=16, context='subprocess')
    geoms = [pool[i % len(pool)] for i in range(args.envs)]
    out = dict(envs=args.envs, agents=args.agents, distinct=len(pool))
    want = lambda part: args.only in (None, part)

    if want('launches'):
        c = core.Core(scene.scenery(geoms, args.agents, device='cuda'), res=64, fov=130)
        util.spawn(c, geoms, seed=0)
        sc, ag = c.scenery, c.agents
        fields = ('screen', 'distances')
        r = cuda.render(sc, ag, fields=fields)
        plane = cuda.mounted(ag, [[0., 0., 0.]], c.res, c.fov)
        ring = cuda.mounted(ag, [[0., 0., 0.]], 256, 360., 'ring')
        seen, around = cuda.look(sc, plane, agents=ag, fields=fields), cuda.look(sc, ring, agents=ag, fields=fields)
        same = bool(util.same_bits(seen.screen, r.screen).all()) and bool(util.same_bits(seen.distances, r.distances).all())
        hits = cuda.raycast(sc, plane.origins, plane.directions, agents=ag, fields=('indices', 'locations', 'dots'))
        on_body = float(((hits.indices >= 0) & (hits.indices < args.agents*sc.model.shape[0])).float().mean())
        screen = cuda.shade(sc, hits, agents=ag)
        gridded = bool(sc._as_struct().lg_vals)
        res = dict(
            render=back_to_back(lambda: cuda.render(sc, ag, fields=fields, out=r), args.repeats),
            look_plane_64=back_to_back(lambda: cuda.look(sc, plane, agents=ag, fields=fields, out=seen), args.repeats),
            look_ring_256=back_to_back(lambda: cuda.look(sc, ring, agents=ag, fields=fields, out=around), args.repeats),
            shade_alone=back_to_back(lambda: cuda.shade(sc, hits, agents=ag, out=screen), args.repeats),
            shade_alone_no_grid=back_to_back(lambda: cuda.shade(sc, hits, agents=ag, out=screen, light_grid=False), args.repeats))
        out['launches'] = dict(seconds=res, rays_on_an_agent=on_body, light_grid=gridded, look_is_render=same)
        print(f'(a) {args.envs} x {args.agents}, {len(pool)} plans; light grid: {gridded}; look is the render, as bits: {same}')
        print(f'    cuda.render, 64 rays an agent (the yardstick)   {us(res["render"])}')
        print(f'    cuda.look, a plane camera an agent, 64 rays      {us(res["look_plane_64"])} - {res["look_plane_64"][0]/res["render"][0]:.2f} x the render')
        print(f'    cuda.look, a 256-ray panorama an agent           {us(res["look_ring_256"])}')
        print(f'    cuda.shade alone (rays on an agent: {on_body:.4f})     {us(res["shade_alone"])}')
        print(f'    cuda.shade alone, the light grid withheld        {us(res["shade_alone_no_grid"])}')
        del c, sc, ag, r, seen, around, hits, screen, plane, ring

    if want('env'):
        out['env'] = {}
        for panorama in (False, True):
            for graphed in (False, True):
                np.random.seed(0); torch.manual_seed(0)
                inner = PointGoal(args.envs, geometries=geoms, panorama=panorama)
                env = graphs.GraphedStep(inner) if graphed else inner
                env.reset()
                actions = arrdict.arrdict(actions=torch.randint(0, 7, (args.envs, 1), device='cuda'))
                t = back_to_back(lambda: env.step(actions), args.repeats)
                key = f"{'panorama' if panorama else 'plain'}_{'graphed' if graphed else 'eager'}"
                out['env'][key] = t
                print(f'(b) PointGoal({args.envs}, panorama={panorama}).step, {"one HIP graph" if graphed else "eager"}: {us(t)}')
                del env, inner

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
