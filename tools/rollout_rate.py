"""What the rollouts cost on the MI355X, next to the only other way to get the same numbers - stepping restored agents:

    python tools/rollout_rate.py [--envs 4096] [--distinct 1024] [--repeats 7] [--only call|envs|findings] [--json out.json]

The world is the headline's: `--envs` envs over `--distinct` distinct synthetic floorplans, one agent each, at their spawn poses with
a walking velocity, under MomentumMovement's table and keep.
  (a) one cuda.rollouts call (ms_rollouts) of K x H = 49 x 8 (cuda.plans(7, 8, 2): LookAhead's), 7 x 8 and 256 x 16 - timed as 20
      calls back to back between two HIP events, the median of `--repeats` such runs - next to the launch loop it replaces: for
      every candidate the agents restored (four copies) and H cuda.physics(movement=...) launches, K H launches in all, timed
      between two events around the whole loop (the median of 3 loops; one for 256 x 16).  The loop's end poses, progress and stops are
      held against the call's as bits while it is at it.  Next to both, the call pinned to either scheme (ms_debug_rollout_scheme: a
      lane a candidate; a lane a wall, the candidates one after another), the outputs held against the library's as bits.
  (b) PointGoal(envs): expert('lookahead') + step() eager and replayed as a HIP graph, next to expert() + step().
  (c) findings, from PointGoal(64, spl=True), 300 steps under either expert: arrivals, the (agent, step) pairs at a dead stop (no
      velocity and no spin after the step), and the mean SPL of the episodes that ended.
`--only` picks one part (for a profiler run of its own).  Needs a GPU: there is no CPU fall-back.
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


def back_to_back(fn, calls, repeats, warmup=3):
    """Seconds per call: `calls` calls between two events, the median (and the range) of `repeats` such runs."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b)*1e-3/calls)
    return float(np.median(times)), float(min(times)), float(max(times))


def launch_loop(c, mover, plans):
    """The parent's way to the same numbers: per candidate the agents restored and H physics launches. Returns run() -> (end
    positions, least progress, stops), each (N, 1, K[, 2])."""
    from megastep_amd import cuda
    a = c.agents
    start = [a.positions.clone(), a.angles.clone(), a.velocity.clone(), a.angvelocity.clone()]
    N = a.angles.shape[0]
    K, H = plans.shape
    acts = [[plans[k, h].expand(N, 1).contiguous() for h in range(H)] for k in range(K)]
    ends = torch.empty((N, 1, K, 2), device='cuda')
    least = torch.empty((N, 1, K), device='cuda')
    stops = torch.empty((N, 1, K), dtype=torch.int32, device='cuda')
    out = cuda.physics(c.scenery, a)

    def restore():
        a.positions.copy_(start[0]); a.angles.copy_(start[1]); a.velocity.copy_(start[2]); a.angvelocity.copy_(start[3])

    def run(check=False):
        """(timed lean: the restores and the launches alone; ``check`` also gathers what the call returns)"""
        for k in range(K):
            restore()
            low, count = None, None
            for h in range(H):
                p = cuda.physics(c.scenery, a, movement=(acts[k][h], mover._table, mover.keep), out=out).progress
                if check:
                    low = p.clone() if low is None else torch.minimum(low, p)
                    count = (p < 1).int() if count is None else count + (p < 1).int()
            if check:
                ends[:, :, k], least[:, :, k], stops[:, :, k] = a.positions, low, count
        restore()
        return ends, least, stops
    restore()
    return run


class ExpertStep:
    """An env whose step is the expert's own: expert() + step(), the decision handed in ignored."""

    def __init__(self, env, *kind):
        self.env, self.action_space, self.kind = env, env.action_space, kind

    def reset(self):
        return self.env.reset()

    def step(self, decision):
        return self.env.step(self.env.expert(*self.kind))


def env_rates(env, n, steps, warm):
    from megastep_amd import arrdict
    env.reset()
    decision = arrdict.arrdict(actions=torch.zeros((n, 1), dtype=torch.long, device='cuda'))
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
        g.replay()
    torch.cuda.synchronize()
    return eager, (time.perf_counter() - t)/steps


def expert_score(env, steps, *kind):
    """`steps` steps of a PointGoal(spl=True) under an expert: arrivals, the (agent, step) pairs at a dead stop, the episodes that
    ended and their mean SPL."""
    env.reset()
    arrivals = stops = 0
    scores = []
    for _ in range(steps):
        world = env.step(env.expert(*kind))
        a = env.core.agents
        arrivals += int(((env._distance < env.arrive) & ~env._goals.stranded).sum())
        stops += int(((a.velocity == 0).all(-1) & (a.angvelocity == 0)).sum())
        scores += world.spl[~torch.isnan(world.spl)].tolist()
    return dict(arrivals=arrivals, dead_stops=stops, episodes_scored=len(scores), mean_spl=float(np.mean(scores)) if scores else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--distinct', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--only', choices=('call', 'envs', 'findings'))
    ap.add_argument('--json')
    args = ap.parse_args()
    from megastep_amd import core, cubicasa, cuda, modules, scene
    from megastep_amd.demo import PointGoal
    from tests import util

    np.random.seed(0); torch.manual_seed(0)
    pool = cubicasa.sample(args.distinct, split='all', n_unique=args.distinct, workers=16, context='subprocess')
    geoms = [pool[i % len(pool)] for i in range(args.envs)]
    out = dict(envs=args.envs, distinct=len(pool))
    want = lambda part: args.only in (None, part)

    if want('call'):
        sc = scene.scenery(geoms, 1, device='cuda')
        c = core.Core(sc, res=64)
        util.spawn(c, geoms, seed=0)
        util.random_velocities(c, np.random.RandomState(1), speed=1.5, spin=90.)
        mover = modules.MomentumMovement(c)
        g = torch.Generator().manual_seed(2)
        out['call'] = {}
        for name, plans in (('49x8', cuda.plans(7, 8, 2, device='cuda')), ('7x8', cuda.plans(7, 8, device='cuda')),
                            ('256x16', torch.randint(0, 7, (256, 16), generator=g).cuda())):
            K, H = plans.shape
            rolled = mover.rollouts(plans)
            med, lo, hi = back_to_back(lambda: mover.rollouts(plans, out=rolled), 20, args.repeats)
            loop = launch_loop(c, mover, plans)
            ends, least, stops = loop(check=True)
            same = bool(util.same_bits(ends, rolled.positions).all() and util.same_bits(least, rolled.progress).all() and
                        util.same_bits(stops, rolled.stops).all())
            lmed, llo, lhi = back_to_back(loop, 1, 1 if K*H > 1000 else 3, warmup=0 if K*H > 1000 else 1)
            from megastep_amd import _lib
            pinned = {}
            for scheme in (0, 1):                                        # a lane a candidate; a lane a wall, the candidates one after another
                _lib.lib().ms_debug_rollout_scheme(scheme)
                try:
                    other = mover.rollouts(plans)
                    pinned[scheme] = back_to_back(lambda: mover.rollouts(plans, out=other), 20, args.repeats)
                finally:
                    _lib.lib().ms_debug_rollout_scheme(-1)
                same = same and all(bool(util.same_bits(getattr(other, f), getattr(rolled, f)).all())
                                    for f in ('positions', 'angles', 'velocity', 'angvelocity', 'progress', 'stops', 'first_stop'))
            print('    pinned (ms_debug_rollout_scheme): a lane a candidate {:.1f} us [{:.1f}, {:.1f}], a lane a wall {:.1f} us [{:.1f}, {:.1f}]'.format(
                *(1e6*x for x in pinned[0] + pinned[1])))
            out['call'][name] = dict(lane_a_candidate_seconds=pinned[0], lane_a_wall_seconds=pinned[1], **dict(K=K, H=H, seconds=med, min=lo, max=hi, loop_seconds=lmed, loop_min=llo, loop_max=lhi, launches=K*H,
                                     equal_bits=same, stopped_share=float((rolled.stops > 0).float().mean())))
            print(f'(a) rollouts {args.envs} x 1 x {K} x {H}: {med*1e6:.1f} us [{lo*1e6:.1f}, {hi*1e6:.1f}]; the loop of {K*H} physics launches: '
                  f'{lmed*1e3:.2f} ms [{llo*1e3:.2f}, {lhi*1e3:.2f}] - {lmed/med:.0f} x; equal bits: {same}; '
                  f"candidates stopped at least once: {out['call'][name]['stopped_share']:.3f}")
            assert same and med < lmed
        del c, sc

    if want('envs'):
        out['envs'] = {}
        for name, kind in (('follow', ()), ('lookahead', ('lookahead',))):
            np.random.seed(0); torch.manual_seed(0)
            env = PointGoal(args.envs, geometries=geoms, max_lifespan=10**6)
            env.reset()
            env.expert(*kind)
            eager, graph = env_rates(ExpertStep(env, *kind), args.envs, 50, 5)
            out['envs'][name] = dict(eager_seconds=eager, graph_seconds=graph)
            print(f"(b) PointGoal({args.envs}): expert({', '.join(map(repr, kind))}) + step(): eager {eager*1e3:.3f} ms, graph {graph*1e3:.3f} ms")
            del env

    if want('findings'):
        out['findings'] = {}
        for name, kind in (('follow', ()), ('lookahead', ('lookahead',))):
            np.random.seed(0); torch.manual_seed(0)
            env = PointGoal(64, geometries=pool[:64], spl=True)
            out['findings'][name] = expert_score(env, 300, *kind)
            print(f"(c) PointGoal(64, spl=True), 300 steps under expert({', '.join(map(repr, kind))}): {out['findings'][name]}")

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
