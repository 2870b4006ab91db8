"""What projectiles cost on the MI355X:

    python tools/projectile_rate.py [--envs 4096] [--distinct 1024] [--repeats 20] [--only launches|env] [--json out.json]

  (a) at `--envs` envs over `--distinct` distinct synthetic floorplans (the headline's world), 4 agents at their spawn poses, each
      call between two HIP events of its own, `--repeats` calls back to back, the median and the range (the store is put back
      before every call by five small copies, which are inside the events of every row alike):
        cuda.fly at S = 4 with a quarter of the slots in flight and at S = 16 with all of them, bounces 0 and 3
        the route a caller had before, for a single leg: one cuda.raycast of the same sweeps and the torch bookkeeping
        the whole rule in torch ops on 256 envs (the single-leg route run four times), scaled to `--envs`
  (b) Dodge(`--envs`).step under random actions, eager and as one HIP graph, next to Deathmatch(2 `--envs`, 2).step - two agents
      a plan too - in the same run.
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

from tools.item_rate import back_to_back, us   # noqa: E402


def single_leg(cuda, sc, ag, positions, velocities, timers, fps):
    """One leg of every projectile the way a caller had it: a cast of the sweeps against walls and bodies, then the bookkeeping."""
    sweep = velocities/fps
    cast = cuda.raycast(sc, torch.nan_to_num(positions), sweep.contiguous(), agents=ag, near=0., fields=('distances', 'indices'))
    reach = sweep.norm(dim=-1)
    hit = (cast.indices >= 0) & (cast.distances <= reach)
    moved = positions + sweep
    timers = timers - 1
    gone = hit | (timers == 0)
    return torch.where(gone[..., None], torch.full_like(moved, float('nan')), moved), timers, hit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--distinct', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--only', choices=('launches', 'env'))
    ap.add_argument('--json')
    args = ap.parse_args()
    from megastep_amd import arrdict, core, cubicasa, cuda, graphs, scene
    from megastep_amd.demo import Deathmatch, Dodge
    from tests import util

    np.random.seed(0); torch.manual_seed(0)
    want = lambda part: args.only in (None, part)
    out = dict(envs=args.envs)
    pool = cubicasa.sample(args.distinct, split='all', n_unique=args.distinct, workers=16, context='subprocess')
    geoms = [pool[i % len(pool)] for i in range(args.envs)]
    out['distinct'] = len(pool)

    if want('launches'):
        n = args.envs
        c = core.Core(scene.scenery(geoms, 4, device='cuda'), res=64, fov=130)
        util.spawn(c, geoms, seed=0)
        sc, ag = c.scenery, c.agents
        out['launches'] = {}
        print(f'(a) {n} envs x 4 agents, {len(pool)} plans')
        for s, share in ((4, .25), (16, 1.)):
            store = cuda.projectiles(n, 4, s)
            p = 4*s
            heading = torch.rand(n, p, device='cuda')*6.2831853
            start = (ag.positions[:, :, None] + .25*torch.randn(n, 4, s, 2, device='cuda')).reshape(n, p, 2)
            start[torch.rand(n, p, device='cuda') >= share] = float('nan')
            begin = dict(positions=start, velocities=8.*torch.stack([heading.cos(), heading.sin()], -1), owners=store.owners.clone(),
                         timers=torch.full((n, p), 64, dtype=torch.int32, device='cuda'), bounces=None)
            flown = cuda.fly(sc, ag, store)

            def restore(bounces):
                for k, v in begin.items():
                    getattr(store, k).copy_(v) if v is not None else store.bounces.fill_(bounces)

            for bounces in (0, 3):
                def tick():
                    restore(bounces)
                    cuda.fly(sc, ag, store, out=flown)

                t = back_to_back(tick, args.repeats)
                legs = float((flown.ended < 4).float().mean())
                out['launches'][f'fly_S{s}_b{bounces}'] = dict(t=t, in_flight=legs)
                print(f'    S = {s}, {legs:.2f} of the slots in flight, bounces {bounces}: restore + cuda.fly {us(t)}')
            t = back_to_back(lambda: restore(0), args.repeats)
            out['launches'][f'restore_S{s}'] = t
            print(f'    S = {s}: the restore alone {us(t)}')

            def before():
                restore(0)
                single_leg(cuda, sc, ag, store.positions, store.velocities, store.timers, c.fps)

            t = back_to_back(before, args.repeats)
            out['launches'][f'raycast_route_S{s}'] = t
            print(f'    S = {s}: restore + one cuda.raycast and the torch bookkeeping, a single leg, no bounce, no records {us(t)}')
            m = min(256, n)
            small = core.Core(scene.scenery(geoms[:m], 4, device='cuda'), res=64, fov=130)
            util.spawn(small, geoms[:m], seed=0)

            def in_torch():
                pos, tim = begin['positions'][:m].clone(), begin['timers'][:m].clone()
                for _ in range(4):
                    pos, tim, _hit = single_leg(cuda, small.scenery, small.agents, pos, begin['velocities'][:m], tim, c.fps)

            t = back_to_back(in_torch, args.repeats)
            out['launches'][f'torch_rule_S{s}'] = dict(t=t, envs=m, scaled=t[0]*n/m)
            print(f'    S = {s}: four such legs in torch on {m} envs {us(t)}; scaled to {n} envs {t[0]*n/m*1e6:.0f} us')
            del small
        del c

    if want('env'):
        out['env'] = {}
        for name in ('Dodge', 'Deathmatch'):
            for graphed in (False, True):
                np.random.seed(0); torch.manual_seed(0)
                inner = Dodge(args.envs, geometries=geoms) if name == 'Dodge' else Deathmatch(2*args.envs, 2, geometries=geoms)
                env = graphs.GraphedStep(inner) if graphed else inner
                env.reset()
                shape = (args.envs, 2) if name == 'Dodge' else (2*args.envs, 1)
                actions = arrdict.arrdict(actions=torch.randint(0, 8 if name == 'Dodge' else 7, shape, device='cuda'))
                t = back_to_back(lambda: env.step(actions), args.repeats)
                out['env'][f"{name}_{'graphed' if graphed else 'eager'}"] = t
                label = f'Dodge({args.envs})' if name == 'Dodge' else f'Deathmatch({2*args.envs}, 2) on {args.envs} plans'
                print(f'(b) {label}.step, {"one HIP graph" if graphed else "eager"}: {us(t)}')
                del env, inner

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
