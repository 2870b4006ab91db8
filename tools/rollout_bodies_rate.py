"""What rollouts among bodies cost on the MI355X, next to the plain call and to the only other way to the same numbers:

    python tools/rollout_bodies_rate.py [--envs 4096] [--agents 4] [--only call|envs|findings] [--package DIR] [--out FILE]

  (a) one cuda.rollouts call, `--envs` envs x `--agents` agents, K = 49 (cuda.plans(7, 8, 2)) and 64, H = 8, others='rest': without
      bodies; with an empty store of 16 slots; with 16, 64 and 256 walkers an env within 3 m of its agents, at rest and moving. Each
      figure is the median [least, most] of 20 calls, each between two HIP events, back to back. Next to them the sequential route
      the call replaces - per plan the agents restored and H cuda.physics(bodies=) launches - at 256 envs, the median of 3 runs
      after one of warm-up, and scaled by envs/256.
  (b) Crowd(envs, 16, flow=True, solid=True): expert('lookahead') + step() replayed as ONE graph, with the plans rolled among the
      walkers and (the expert made without ``bodies``) not.
  (c) findings, Crowd(64, solid=True) over 300 steps: arrivals and (agent, step) pairs at a dead stop under 'follow', under
      'lookahead' without bodies and with them.
`--package DIR`: import megastep_amd from another checkout (one without ``bodies`` gives (a)'s plain figures only).
Needs a GPU: there is no CPU fall-back."""
import argparse
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def events(fn, calls=20, warmup=5):
    """Seconds of one call: (median, least, most) of `calls` calls back to back, each between two HIP events."""
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    marks[0].record()
    for i in range(calls):
        fn()
        marks[i + 1].record()
    torch.cuda.synchronize()
    t = [marks[i].elapsed_time(marks[i + 1])*1e-3 for i in range(calls)]
    return float(np.median(t)), min(t), max(t)


def us(t):
    return '{:.1f} us [{:.1f}, {:.1f}]'.format(*(1e6*x for x in t))


def world(n, a, geoms):
    import numpy as np
    from megastep_amd import core, modules, scene
    from tests import util
    c = core.Core(scene.scenery(geoms[:n], a, device='cuda'), res=64)
    util.spawn(c, geoms[:n], seed=0)
    util.random_velocities(c, np.random.RandomState(1), speed=1.5, spin=90.)
    return c, modules.MomentumMovement(c)


def crowd_round(c, p, seed):
    """A store of p walkers an env, each within 3 m of one of its env's agents, walking at up to 1.4 m/s."""
    import torch
    from megastep_amd import cuda
    g = torch.Generator(device='cuda').manual_seed(seed)
    n, a = c.agents.angles.shape
    store = cuda.walkers(n, p)
    near = c.agents.positions[:, torch.arange(p, device='cuda') % a]
    store.positions[:] = near + 6*torch.rand((n, p, 2), generator=g, device='cuda') - 3
    store.velocities[:] = 2.8*torch.rand((n, p, 2), generator=g, device='cuda') - 1.4
    return store


def sequential(c, mover, plans, bodies):
    """The route the call replaces: per plan the agents restored and H cuda.physics(bodies=) launches (the store left where it is)."""
    from megastep_amd import cuda
    a = c.agents
    start = [a.positions.clone(), a.angles.clone(), a.velocity.clone(), a.angvelocity.clone()]
    acts = [[plans[k, h].expand(*a.angles.shape).contiguous() for h in range(plans.shape[1])] for k in range(plans.shape[0])]
    out = cuda.physics(c.scenery, a, bodies=bodies)

    def run():
        for row in acts:
            a.positions.copy_(start[0]); a.angles.copy_(start[1]); a.velocity.copy_(start[2]); a.angvelocity.copy_(start[3])
            for act in row:
                cuda.physics(c.scenery, a, movement=(act, mover._table, mover.keep), bodies=bodies, out=out)
    return run


class ExpertStep:
    def __init__(self, env):
        self.env = env

    def step(self):
        return self.env.step(self.env.expert('lookahead'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--agents', type=int, default=4)
    ap.add_argument('--only', choices=('call', 'envs', 'findings'))
    ap.add_argument('--package', default=ROOT)
    ap.add_argument('--out')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    import numpy as np
    import torch
    from megastep_amd import cubicasa, cuda, modules
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    among = 'bodies' in inspect.signature(cuda.rollouts).parameters
    say(f"package: {'this tree' if os.path.abspath(args.package) == ROOT else 'another checkout'}; rollouts take bodies: {among}")
    np.random.seed(0); torch.manual_seed(0)
    pool = cubicasa.sample(1024, split='all', n_unique=1024, workers=16, context='subprocess')
    geoms = [pool[i % len(pool)] for i in range(args.envs)]
    want = lambda part: args.only in (None, part)

    if want('call'):
        c, mover = world(args.envs, args.agents, geoms)
        small, small_mover = world(256, args.agents, geoms) if among else (None, None)
        for K in (49, 64):
            plans = cuda.plans(7, 8, 2, device='cuda') if K == 49 else torch.randint(0, 7, (64, 8), generator=torch.Generator().manual_seed(2)).cuda()
            shape = f'{args.envs} x {args.agents} x {K} x 8'
            rolled = mover.rollouts(plans, others='rest')
            say(f'(a) {shape} without bodies: {us(events(lambda: mover.rollouts(plans, others="rest", out=rolled)))}')
            if not among:
                continue
            for p, filled in ((16, False), (16, True), (64, True), (256, True)):
                store = crowd_round(c, p, p) if filled else cuda.walkers(args.envs, p)
                for moving in ((False, True) if filled else (False,)):
                    bodies = dict(store=store, moving=moving)
                    r = mover.rollouts(plans, others='rest', bodies=bodies)
                    t = events(lambda: mover.rollouts(plans, others='rest', bodies=bodies, out=r))
                    say(f'(a) {shape} {"among " + str(p) + " walkers" if filled else "with an empty store of 16"}, {"moving" if moving else "at rest"}: {us(t)}; '
                        f'candidates a body stopped: {float((r.body_stops > 0).float().mean()):.3f}')
            bodies = dict(store=crowd_round(small, 64, 64), moving=True)
            t = events(sequential(small, small_mover, plans, bodies), calls=3, warmup=1)
            say(f'(a) the sequential route at 256 envs, {K} x 8 = {K*8} cuda.physics(bodies=) launches among 64 walkers: {t[0]*1e3:.2f} ms '
                f'[{t[1]*1e3:.2f}, {t[2]*1e3:.2f}]; scaled by {args.envs}/256: {t[0]*1e3*args.envs/256:.1f} ms')
        del c, small

    if want('envs') and among:
        from megastep_amd.demo import Crowd
        for with_bodies in (True, False):
            np.random.seed(0); torch.manual_seed(0)
            env = Crowd(args.envs, 16, geometries=geoms, max_lifespan=10**6, flow=True, solid=True)
            env.reset()
            if not with_bodies:
                source = env._goals if env._routes is None else env._routes
                env._lookahead = modules.LookAhead(env.core, source, env._mover, fallback=modules.PathFollower(env.core, source, cone=15.))
            step = ExpertStep(env).step
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(5):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            t = events(g.replay)
            say(f"(b) Crowd({args.envs}, 16, flow=True, solid=True).step(expert('lookahead')) as one graph, the plans rolled "
                f"{'among the walkers' if with_bodies else 'without bodies'}: {t[0]*1e3:.3f} ms [{t[1]*1e3:.3f}, {t[2]*1e3:.3f}]")
            del env, g

    if want('findings') and among:
        from megastep_amd.demo import Crowd
        for name in ('follow', 'lookahead without bodies', 'lookahead among the walkers'):
            np.random.seed(0); torch.manual_seed(0)
            env = Crowd(64, geometries=pool[:64], solid=True)
            env.reset()
            if name == 'lookahead without bodies':
                source = env._goals if env._routes is None else env._routes
                env._lookahead = modules.LookAhead(env.core, source, env._mover, fallback=modules.PathFollower(env.core, source, cone=15.))
            arrivals = stops = 0
            for _ in range(300):
                env.step(env.expert('follow' if name == 'follow' else 'lookahead'))
                a = env.core.agents
                arrivals += int(((env._distance < env.arrive) & ~env._goals.stranded).sum())
                stops += int(((a.velocity == 0).all(-1) & (a.angvelocity == 0)).sum())
            say(f'(c) Crowd(64, solid=True), 300 steps under {name}: {arrivals} arrivals, {stops} (agent, step) pairs at a dead stop')

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
