"""What flow fields cost, and what they save a crowd, on the MI355X:

    python tools/flow_rate.py [--envs 4096] [--distinct 1024] [--repeats 20] [--only launches|env|crowd] [--json out.json]

HIP events, each call between two of its own, `--repeats` calls back to back, the median with least and most:
  (a) at `--envs` envs over `--distinct` synthetic floorplans (the headline's world), 4 goal fields an env: `flow_fields` next to the
      `distance_fields` launch that feeds it; `FlowFields.at` of 16, 64 and 256 points an env next to `waypoints` of the same points;
      the share of the queries that took the fallback; the LDS tier the plans land in.
  (b) Crowd(`--envs`, n_walkers=P).step for P = 16 and 64, eager and as one HIP graph, with and without `flow`.
  (c) Crowd(64, n_walkers=16), 300 steps of random actions, with and without `flow`: arrivals, and the walkers' speed over their
      preferred speed.
Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from tools.item_rate import back_to_back, us   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--distinct', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--only', choices=('launches', 'env', 'crowd'))
    ap.add_argument('--json')
    args = ap.parse_args()
    from megastep_amd import arrdict, core, cubicasa, cuda, graphs, modules, scene
    from megastep_amd.demo import Crowd
    from tests import util

    np.random.seed(0); torch.manual_seed(0)
    want = lambda part: args.only in (None, part)
    pool = cubicasa.sample(args.distinct, split='all', n_unique=args.distinct, workers=16, context='subprocess')
    geoms = [pool[i % len(pool)] for i in range(args.envs)]
    out = dict(envs=args.envs, distinct=len(pool))

    if want('launches'):
        c = core.Core(scene.scenery(geoms, 4, device='cuda', bake=False), res=64, fov=130)
        util.spawn(c, geoms, seed=0)
        grid = cuda.nav_grid(c.scenery, config=c.config)
        framed = (grid._host_geom[:, 2].astype(np.int64) + 2)*(grid._host_geom[:, 3] + 2)
        tier = int(np.searchsorted(cuda.FLOW_CAPACITY, grid._max_framed))
        print(f'(a) {args.envs} envs, {len(pool)} plans, 4 fields an env: framed cells median {int(np.median(framed))}, most {grid._max_framed}: '
              f'the launch takes tier {tier} of {cuda.FLOW_CAPACITY}')
        out['launches'] = dict(median_framed=int(np.median(framed)), max_framed=grid._max_framed, tier=tier)
        for p in (16, 64, 256):
            crowd = modules.Walkers(c, grid, p)
            for _ in range(10):                          # (off their spawn cells)
                crowd()
            fields, positions, goal = crowd.fields, crowd.positions, crowd.goal
            if p == 16:
                t = back_to_back(lambda: fields.update(), args.repeats)
                print(f'    distance_fields, all {args.envs} x 4 fields: {us(t)}')
                flows = fields.flows()
                t1 = back_to_back(lambda: flows.update(), args.repeats)
                print(f'    flow_fields of them, look-ahead 16: {us(t1)}')
                out['launches'].update(fields=t, flows=t1)
            flows = fields.flows()
            towards = fields.waypoints(positions, goal=goal)
            t = back_to_back(lambda: fields.waypoints(positions, goal=goal, out=towards), args.repeats)
            t1 = back_to_back(lambda: flows.at(positions, goal=goal, out=towards, took=True), args.repeats)
            fallback = float((flows.took == 0).float().sum()/(flows.took >= 0).float().sum().clamp(min=1))
            out['launches'][f'P{p}'] = dict(waypoints=t, at=t1, fallback=fallback)
            print(f'    P = {p}: waypoints {us(t)}; FlowFields.at {us(t1)}; {fallback:.3f} of the answers by the fallback')
            del crowd, flows
        del c

    if want('env'):
        out['env'] = {}
        for p in (16, 64):
            for flow in (False, True):
                for graphed in (False, True):
                    np.random.seed(0); torch.manual_seed(0)
                    inner = Crowd(args.envs, n_walkers=p, geometries=geoms, flow=flow)
                    env = graphs.GraphedStep(inner) if graphed else inner
                    env.reset()
                    actions = arrdict.arrdict(actions=torch.randint(0, 7, (args.envs, 1), device='cuda'))
                    t = back_to_back(lambda: env.step(actions), args.repeats)
                    out['env'][f"P{p}_{'flow' if flow else 'waypoints'}_{'graphed' if graphed else 'eager'}"] = t
                    print(f'(b) Crowd({args.envs}, n_walkers={p}, flow={flow}).step, {"one HIP graph" if graphed else "eager"}: {us(t)}')
                    del env, inner

    if want('crowd'):
        out['crowd'] = {}
        for flow in (False, True):
            np.random.seed(0); torch.manual_seed(0)
            env = Crowd(64, geometries=geoms[:64], flow=flow)
            env.reset()
            arrivals, ratio = 0, []
            for _ in range(300):
                before, goal = env.walkers.positions.clone(), env.walkers.goal.clone()
                env.step(arrdict.arrdict(actions=torch.randint(0, 7, (64, 1), device='cuda')))
                arrivals += int((env.walkers.goal != goal).sum())
                ratio.append(float(((env.walkers.positions - before).norm(dim=-1)*env.core.fps/env.walkers.store.speeds).mean()))
            out['crowd'][f'flow_{flow}'] = dict(arrivals=arrivals, speed=float(np.mean(ratio)))
            print(f'(c) Crowd(64), 300 steps, flow={flow}: the walkers arrived {arrivals} times, at {np.mean(ratio):.3f} of their preferred speed')

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
