"""What walkers cost on the MI355X:

    python tools/walker_rate.py [--envs 4096] [--distinct 1024] [--repeats 20] [--only launches|env|crowd] [--json out.json]

  (a) at `--envs` envs over `--distinct` distinct synthetic floorplans (the headline's world), 4 agents at their spawn poses, each
      call between two HIP events of its own, `--repeats` calls back to back, the median and the range (the store is put back
      before every call by two small copies, which are inside the events of every cuda.walk row alike):
        cuda.walk at P = 16 and 64 (a wavefront an env) and 256 (a workgroup an env), `towards` precomputed, plainly and with slide=True
        the waypoints launch in front of it
        the route a caller had before: the same crowd as P extra agents through cuda.physics with the steering in torch ops, at
        P = 16 and 60, and what those extra agents add to cuda.render at 64 rays
  (b) Crowd(`--envs`).step under random actions, eager and as one HIP graph, next to PointGoal(`--envs`).step in the same run;
      Crowd(`--envs`, n_walkers=16 | 64, flow=True).step as one HIP graph, with and without walk=dict(slide=True).
  (c) Crowd(64), 300 steps under expert(), under random actions and under expert() with sliding walkers: arrivals, bumps a step,
      the walkers' mean speed over their preferred speed, what blocked them and how many a tick left at rest.
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


def steer_in_torch(p, v, towards, speeds, fps, personal=.6, push=1., keep=.5):
    """cuda.walk's steer, keep apart and blend as a caller writes them in torch ops: (N, P, 2) -> the velocities."""
    d = towards - p
    l = d.norm(dim=-1, keepdim=True)
    pref = torch.nan_to_num(d*torch.minimum(speeds[..., None], l*fps)/l)
    r = p[:, :, None] - p[:, None]
    l2 = r.norm(dim=-1, keepdim=True)
    near = (l2 > 0) & (l2 < personal)
    sep = torch.where(near, r*push*(personal - l2)/(personal*l2), torch.zeros_like(r)).sum(2)
    want = pref + sep
    wl = want.norm(dim=-1, keepdim=True)
    want = torch.where(wl > speeds[..., None], want*speeds[..., None]/wl, want)
    return keep*v + (1 - keep)*want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--distinct', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--only', choices=('launches', 'env', 'crowd'))
    ap.add_argument('--json')
    args = ap.parse_args()
    from megastep_amd import arrdict, core, cubicasa, cuda, graphs, modules, scene
    from megastep_amd.demo import Crowd, PointGoal
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
        grid = cuda.nav_grid(sc, config=c.config)
        out['launches'] = {}
        print(f'(a) {n} envs x 4 agents, {len(pool)} plans')
        t = back_to_back(lambda: cuda.render(sc, ag), args.repeats)
        out['launches']['render_A4'] = t
        print(f'    cuda.render, 4 agents x 64 rays: {us(t)}')
        for p in (16, 64, 256):
            crowd = modules.Walkers(c, grid, p)
            for _ in range(10):                          # (off their spawn cells, with velocities)
                crowd()
            store = crowd.store
            begin = store.positions.clone(), store.velocities.clone()
            towards = crowd.fields.waypoints(store.positions, goal=crowd.goal)
            walked = cuda.walk(sc, ag, store, towards)

            def restore():
                store.positions.copy_(begin[0]); store.velocities.copy_(begin[1])

            def tick():
                restore()
                cuda.walk(sc, ag, store, towards, out=walked)

            t, t0 = back_to_back(tick, args.repeats), back_to_back(restore, args.repeats)
            stopped = float((walked.progress < 1).float().mean())
            out['launches'][f'walk_P{p}'] = dict(t=t, restore=t0, stopped=stopped)
            print(f'    P = {p}: restore + cuda.walk {us(t)}; the restore alone {us(t0)}; {stopped:.3f} of the walkers stopped')
            sliding = cuda.walk(sc, ag, store, towards, slide=True)

            def tick_sliding():
                restore()
                cuda.walk(sc, ag, store, towards, out=sliding, slide=True)

            t = back_to_back(tick_sliding, args.repeats)
            slid, dead = float((sliding.slid > 0).float().mean()), float((sliding.stopped == 1).float().mean())
            out['launches'][f'walk_slide_P{p}'] = dict(t=t, slid=slid, stopped=dead)
            print(f'    P = {p}: restore + cuda.walk(slide=True) {us(t)}; {slid:.3f} of the walkers slid, {dead:.3f} were left at rest')
            restore()
            t = back_to_back(lambda: crowd.fields.waypoints(store.positions, goal=crowd.goal, out=towards), args.repeats)
            out['launches'][f'waypoints_P{p}'] = t
            print(f'    P = {p}: the waypoints launch {us(t)}')
            if p == 256:
                continue
            # the route a caller had: the crowd as extra agents (60: the most beside four learners)
            extra = min(p, 60)
            wide = core.Core(scene.scenery(geoms, 4 + extra, device='cuda'), res=64, fov=130)
            wide.agents.positions[:, :4] = ag.positions
            wide.agents.positions[:, 4:] = begin[0][:, :extra]
            wide.agents.velocity[:, 4:] = begin[1][:, :extra]
            goal, speeds, start = crowd.goal[:, :extra].contiguous(), store.speeds[:, :extra].contiguous(), wide.agents.positions.clone()

            def as_agents():
                wide.agents.positions.copy_(start)
                pos = wide.agents.positions[:, 4:].contiguous()
                heads = crowd.fields.waypoints(pos, goal=goal)
                wide.agents.velocity[:, 4:] = steer_in_torch(pos, wide.agents.velocity[:, 4:], heads, speeds, c.fps)
                cuda.physics(wide.scenery, wide.agents)

            t = back_to_back(as_agents, args.repeats)
            out['launches'][f'as_agents_P{extra}'] = t
            print(f'    P = {extra} as extra agents: restore + waypoints + the steering in torch + cuda.physics {us(t)}')
            t = back_to_back(lambda: cuda.render(wide.scenery, wide.agents), args.repeats)
            out['launches'][f'render_A{4 + extra}'] = t
            print(f'    P = {extra} as extra agents: cuda.render, {4 + extra} agents x 64 rays {us(t)}')
            del wide, crowd
        del c

    if want('env'):
        out['env'] = {}
        for name in ('Crowd', 'PointGoal'):
            for graphed in (False, True):
                np.random.seed(0); torch.manual_seed(0)
                inner = (Crowd if name == 'Crowd' else PointGoal)(args.envs, geometries=geoms)
                env = graphs.GraphedStep(inner) if graphed else inner
                env.reset()
                actions = arrdict.arrdict(actions=torch.randint(0, 7, (args.envs, 1), device='cuda'))
                t = back_to_back(lambda: env.step(actions), args.repeats)
                out['env'][f"{name}_{'graphed' if graphed else 'eager'}"] = t
                print(f'(b) {name}({args.envs}).step, {"one HIP graph" if graphed else "eager"}: {us(t)}')
                del env, inner
        for p in (16, 64):
            for slide in (False, True):
                np.random.seed(0); torch.manual_seed(0)
                inner = Crowd(args.envs, n_walkers=p, flow=True, walk=dict(slide=True) if slide else None, geometries=geoms)
                env = graphs.GraphedStep(inner)
                env.reset()
                actions = arrdict.arrdict(actions=torch.randint(0, 7, (args.envs, 1), device='cuda'))
                t = back_to_back(lambda: env.step(actions), args.repeats)
                out['env'][f"Crowd_flow_P{p}_{'slide' if slide else 'plain'}"] = t
                print(f'(b) Crowd({args.envs}, n_walkers={p}, flow=True{", walk=dict(slide=True)" if slide else ""}).step, one HIP graph: {us(t)}')
                del env, inner

    if want('crowd'):
        out['crowd'] = {}
        for policy in ('expert', 'random', 'expert, walkers sliding'):
            np.random.seed(0); torch.manual_seed(0)
            env = Crowd(64, geometries=geoms[:64], walk=dict(slide=True) if 'sliding' in policy else None)
            env.reset()
            arrivals = bumps = close = 0
            ratio, rest = [], []
            for _ in range(300):
                decision = env.expert() if policy != 'random' else arrdict.arrdict(actions=torch.randint(0, 7, (64, 1), device='cuda'))
                before = env.walkers.positions.clone()
                world = env.step(decision)
                arrivals += int((world.reward > .5).sum())
                bumps += int(env.walkers.bumps.sum()); close += int(env.walkers.close.sum())
                ratio.append(float(((env.walkers.positions - before).norm(dim=-1)*env.core.fps/env.walkers.store.speeds).mean()))
                walked = env.walkers.walked                  # (at rest after the tick: blocked and, when sliding, not carried on)
                rest.append([float((walked.blocked == c).float().mean()) for c in (1, 2, 3)]
                            + [float(((walked.progress < 1) if walked.stopped is None else (walked.stopped == 1)).float().mean())])
            blocked = np.mean(rest, 0)
            out['crowd'][policy] = dict(arrivals=arrivals, bumps_a_step=bumps/300/64, close_a_step=close/300/64, speed_ratio=float(np.mean(ratio)),
                                        blocked_by_agent=blocked[0], blocked_by_walker=blocked[1], blocked_by_wall=blocked[2], left_at_rest=blocked[3])
            print(f'(c) Crowd(64), 300 steps, {policy}: {arrivals} arrivals, {bumps/300/64:.4f} bumps and {close/300/64:.4f} close an env-step, '
                  f'the walkers at {np.mean(ratio):.3f} of their preferred speed; blocked a tick by an agent {blocked[0]:.3f}, a walker {blocked[1]:.3f}, '
                  f'a wall {blocked[2]:.3f} of them, left at rest {blocked[3]:.3f}')

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
