"""What solid bodies cost on the MI355X, and how solid they are:

    python tools/body_rate.py [--envs 4096] [--distinct 1024] [--repeats 20] [--only launches|env|overlap] [--json out.json]

  (a) cuda.physics(movement=..., bodies=store) next to cuda.physics(movement=...) at `--envs` envs x 4 agents over `--distinct`
      synthetic floorplans, the store a modules.Walkers crowd of P = 16, 64 and 256 ten ticks off its spawn cells, at rest and
      `moving`; and the same with the store EMPTY: what opting in costs when nobody is there.  The agents are restored before every
      launch (a copy of four tensors, timed alone next to it); HIP events round `--repeats` calls back to back, medians with
      [least, most].  The share of agents blocked, and blocked by a body, is stated.
  (b) Crowd(`--envs`, n_walkers=16 / 64, flow=True).step with and without `solid`, eager and as one HIP graph.
  (c) a finding, on the CPU - needs no GPU: the numpy rules (tests/body_rule.py, tests/walker_rule.py) rolled Crowd-like over two
      plans - physics among the bodies, then the walkers' tick - and the largest overlap of an agent's disc and a walker's, float64.
`--only` picks one part.  (a) and (b) need a GPU: there is no CPU fall-back.
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


def overlap(steps=60, n_walkers=8, seed=0):
    """Two plans, two agents each, `n_walkers` walkers: `steps` rounds of body_rule (random actions under MomentumMovement's table)
    then walk_rule towards random points. Returns the largest overlap agent-walker and walker-walker after a round, in metres."""
    from tests import util
    from tests.body_rule import body_rule
    from tests.rollout_rule import world_of
    from tests.walker_rule import random_store, walk_rule
    c, _ = util.plan_world(2, 2, 8, 130., seed=3, device='cpu')
    w = world_of(c)
    R, fps = float(c.agent_radius), float(c.fps)
    rng = np.random.RandomState(seed)
    lo, hi = w['positions'].min(1) - 1.5, w['positions'].max(1) + 1.5
    store, _ = random_store(2, n_walkers, lo, hi, seed)
    table = np.float32([[0, 0, 0], [0, .5, 0], [0, -.5, 0], [.5, 0, 0], [-.5, 0, 0], [0, 0, 18], [0, 0, -18]])
    worst = dict(agent=0., walker=0.)
    for _ in range(steps):
        out = body_rule(w, store['positions'], None, (rng.randint(0, 7, (2, 2)), table, .875), R, fps)
        w = dict(walls=w['walls'], **{k: out[k] for k in ('positions', 'angles', 'velocity', 'angvelocity')})
        towards = (w['positions'][:, rng.randint(0, 2, n_walkers)] + rng.uniform(-.5, .5, (2, n_walkers, 2))).astype(np.float32)
        walked = walk_rule(w['walls'], w['positions'], store, towards, fps=fps, radius=R)
        store = dict(store, positions=walked['positions'], velocities=walked['velocities'])
        p, q = w['positions'].astype(float), store['positions'].astype(float)
        for n in range(2):
            there = np.isfinite(q[n]).all(-1)
            d = np.linalg.norm(p[n][:, None] - q[n][there][None], axis=-1)
            worst['agent'] = max(worst['agent'], float((2*R - d).max(initial=0.)))
            dd = np.linalg.norm(q[n][there][:, None] - q[n][there][None], axis=-1) + 9*np.eye(there.sum())
            worst['walker'] = max(worst['walker'], float((2*R - dd).max(initial=0.)))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--distinct', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--only', choices=('launches', 'env', 'overlap'))
    ap.add_argument('--json')
    args = ap.parse_args()
    want = lambda part: args.only in (None, part)
    out = dict(envs=args.envs)

    if want('overlap'):
        out['overlap'] = overlap()
        print(f"(c) 60 Crowd-like rounds of the numpy rules on two plans, 2 agents and 8 walkers each: the largest overlap of an agent and a "
              f"walker {out['overlap']['agent']:.4f} m, of two walkers {out['overlap']['walker']:.4f} m")

    if want('launches') or want('env'):
        from megastep_amd import arrdict, core, cubicasa, cuda, graphs, modules, scene
        from megastep_amd.demo import Crowd
        from tests import util
        np.random.seed(0); torch.manual_seed(0)
        pool = cubicasa.sample(args.distinct, split='all', n_unique=args.distinct, workers=16, context='subprocess')
        geoms = [pool[i % len(pool)] for i in range(args.envs)]
        out['distinct'] = len(pool)

    if want('launches'):
        n = args.envs
        c = core.Core(scene.scenery(geoms, 4, device='cuda'), res=64, fov=130)
        util.spawn(c, geoms, seed=0)
        util.random_velocities(c, np.random.RandomState(1), speed=1.5, spin=90.)
        sc, a = c.scenery, c.agents
        grid = cuda.nav_grid(sc, config=c.config)
        mover = modules.MomentumMovement(c)
        movement = (torch.randint(0, 7, (n, 4), generator=torch.Generator().manual_seed(2)).cuda(), mover._table, mover.keep)
        start = [t.clone() for t in (a.positions, a.angles, a.velocity, a.angvelocity)]

        def restore():
            for t, s in zip((a.positions, a.angles, a.velocity, a.angvelocity), start):
                t.copy_(s)

        def timed(**kw):
            held = cuda.physics(sc, a, movement=movement, **kw)

            def call():
                restore()
                cuda.physics(sc, a, movement=movement, out=held, **kw)
            return back_to_back(call, args.repeats), held

        out['launches'] = dict(restore=back_to_back(restore, args.repeats))
        print(f'(a) {n} envs x 4 agents, {len(pool)} plans; the restore alone {us(out["launches"]["restore"])}')
        plain, held = timed()
        out['launches']['plain'] = plain
        print(f'    restore + cuda.physics(movement=): {us(plain)}; {float((held.progress < 1).float().mean()):.3f} of the agents blocked')
        for p in (16, 64, 256):
            crowd = modules.Walkers(c, grid, p)
            for _ in range(10):                          # (off their spawn cells, with velocities)
                crowd()
            restore()
            for name, store, moving in (('at rest', crowd.store, False), ('moving', crowd.store, True), ('empty', cuda.walkers(n, p), False)):
                t, held = timed(bodies=dict(store=store, moving=moving))
                shares = dict(blocked=float((held.progress < 1).float().mean()), by_body=float((held.blocker >= 0).float().mean()))
                out['launches'][f'P{p}_{name}'] = dict(t=t, **shares)
                print(f'    P = {p}, {name}: restore + cuda.physics(movement=, bodies=) {us(t)}; {shares["blocked"]:.3f} of the agents blocked, '
                      f'{shares["by_body"]:.3f} by a body')
            del crowd
        del c

    if want('env'):
        out['env'] = {}
        for p in (16, 64):
            for solid in (False, True):
                for graphed in (False, True):
                    np.random.seed(0); torch.manual_seed(0)
                    inner = Crowd(args.envs, n_walkers=p, geometries=geoms, flow=True, solid=solid)
                    env = graphs.GraphedStep(inner) if graphed else inner
                    env.reset()
                    actions = arrdict.arrdict(actions=torch.randint(0, 7, (args.envs, 1), device='cuda'))
                    t = back_to_back(lambda: env.step(actions), args.repeats)
                    out['env'][f'P{p}_{"solid" if solid else "plain"}_{"graph" if graphed else "eager"}'] = t
                    print(f'(b) Crowd({args.envs}, n_walkers={p}, flow=True, solid={solid}).step, {"one HIP graph" if graphed else "eager"}: {us(t)}')
                    del env, inner

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
