"""What items cost on the MI355X:

    python tools/item_rate.py [--envs 4096] [--distinct 1024] [--repeats 20] [--only launches|env] [--json out.json]

  (a) at `--envs` envs over `--distinct` distinct synthetic floorplans (the headline's world), 4 agents at their spawn poses, 256
      rays an agent, 16 and 64 items an env placed on free cells, each call between two HIP events of its own, `--repeats` calls
      back to back, the median and the range:
        cuda.overlay_items on the frame of a cuda.render, next to that cuda.render of the same frame
        cuda.collect_items (reach .3, delay 0, so that taken items are due at once)
        the three-step return: cuda.collect_items, CellDraws.again(mask=due) and the select (cuda.place_items)
  (b) Forage(`--envs`).step under random actions, eager and as one HIP graph, next to PointGoal(`--envs`).step in the same run.
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
    ap.add_argument('--distinct', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--only', choices=('launches', 'env'))
    ap.add_argument('--json')
    args = ap.parse_args()
    from megastep_amd import arrdict, core, cubicasa, cuda, graphs, scene
    from megastep_amd.demo import Forage, PointGoal
    from tests import util

    np.random.seed(0); torch.manual_seed(0)
    want = lambda part: args.only in (None, part)
    out = dict(envs=args.envs)
    pool = cubicasa.sample(args.distinct, split='all', n_unique=args.distinct, workers=16, context='subprocess')
    geoms = [pool[i % len(pool)] for i in range(args.envs)]
    out['distinct'] = len(pool)

    if want('launches'):
        n = args.envs
        c = core.Core(scene.scenery(geoms, 4, device='cuda'), res=256, fov=130)
        util.spawn(c, geoms, seed=0)
        sc, ag = c.scenery, c.agents
        grid = cuda.nav_grid(sc, config=c.config)
        dirs = cuda.camera_rays(ag)
        frame = cuda.render(sc, ag)
        out['launches'] = {}
        print(f'(a) {n} envs x 4 agents x 256 rays, {len(pool)} plans')
        t = back_to_back(lambda: cuda.render(sc, ag, out=frame), args.repeats)
        out['launches']['render'] = t
        print(f'    cuda.render of the frame: {us(t)}')
        for p in (16, 64):
            store = cuda.items(n, p, kinds=torch.arange(p) % 2, colors=torch.rand(p, 3))
            got = cuda.collect_items(sc, ag, store, .3)
            draws = cuda.cell_draws(grid, grid, p, 1, seed=1, mask=got.due)
            cuda.place_items(store, draws, got.due)
            shown = torch.empty((n, 4, 256), dtype=torch.int32, device='cuda')

            def overlay():
                cuda.overlay_items(store, frame, agents=ag, dirs=dirs, out_items=shown)

            cuda.render(sc, ag, out=frame)
            overlay()
            share = float((shown >= 0).float().mean())
            # (the frame is not rendered again between the calls: from the second on no item is nearer than what the planes hold,
            # which changes the stores of a call, not its folds)
            t = back_to_back(overlay, args.repeats)
            out['launches'][f'overlay_{p}'] = dict(t=t, rays_on_an_item=share)
            print(f'    P = {p}: cuda.overlay_items {us(t)}; {share:.4f} of the rays show an item')

            def both():
                cuda.render(sc, ag, out=frame)
                overlay()

            t = back_to_back(both, args.repeats)
            out['launches'][f'render_overlay_{p}'] = t
            print(f'    P = {p}: cuda.render + cuda.overlay_items {us(t)}')
            t = back_to_back(lambda: cuda.collect_items(sc, ag, store, .3, out=got), args.repeats)
            out['launches'][f'collect_{p}'] = t
            print(f'    P = {p}: cuda.collect_items {us(t)}')

            def returns():
                cuda.collect_items(sc, ag, store, .3, out=got)
                cuda.place_items(store, draws, got.due)

            t = back_to_back(returns, args.repeats)
            out['launches'][f'return_{p}'] = t
            print(f'    P = {p}: collect, draw again, place {us(t)}')
        del c, frame

    if want('env'):
        out['env'] = {}
        for name in ('Forage', 'PointGoal'):
            for graphed in (False, True):
                np.random.seed(0); torch.manual_seed(0)
                inner = Forage(args.envs, geometries=geoms) if name == 'Forage' else PointGoal(args.envs, geometries=geoms)
                env = graphs.GraphedStep(inner) if graphed else inner
                env.reset()
                actions = arrdict.arrdict(actions=torch.randint(0, 7, (args.envs, 1), device='cuda'))
                t = back_to_back(lambda: env.step(actions), args.repeats)
                out['env'][f"{name}_{'graphed' if graphed else 'eager'}"] = t
                print(f'(b) {name}({args.envs}).step, {"one HIP graph" if graphed else "eager"}: {us(t)}')
                del env, inner

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
