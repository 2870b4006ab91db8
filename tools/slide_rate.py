"""What sliding contacts cost on the MI355X, and what they change for the experts:

    python tools/slide_rate.py [--distinct 1024] [--repeats 20] [--only launch|findings] [--json out.json]

  (a) the sliding launch, cuda.physics(movement=..., slide=True), next to the plain one, cuda.physics(movement=...), at 4096 envs x 4
      agents and at 32 768 x 1 over `--distinct` distinct synthetic floorplans: the agents at their spawn poses with a walking velocity
      under MomentumMovement's table and keep, restored before every timed launch (a copy of four tensors, outside the events);
      the two launches in turn, each between two HIP events of its own, the median and the range of `--repeats` rounds.  The share of agents the step
      blocks, slides and stops dead is stated with it: phase B and the contact's pass cost a wave something only where one of its
      agents is blocked.
  (b) findings, from PointGoal(64, spl=True), 300 steps under expert() and expert('lookahead'), with and without slide: arrivals,
      the (agent, step) pairs at a dead stop (no velocity and no spin after the step), and the mean SPL of the episodes that ended.
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


def alternating(fns, restore, repeats, warmup=5):
    """Seconds per launch of each of `fns`, taken in turn: `restore()` then the launch between two events of its own, `repeats`
    rounds. Returns (median, least, most) per function."""
    for _ in range(warmup):
        for fn in fns:
            restore(); fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for fn, ts in zip(fns, times):
            restore()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b)*1e-3)
    return [(float(np.median(ts)), float(min(ts)), float(max(ts))) for ts in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--distinct', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--only', choices=('launch', 'findings'))
    ap.add_argument('--json')
    args = ap.parse_args()
    from megastep_amd import core, cubicasa, cuda, modules, scene
    from megastep_amd.demo import PointGoal
    from tests import util
    from tools.rollout_rate import expert_score

    np.random.seed(0); torch.manual_seed(0)
    pool = cubicasa.sample(args.distinct, split='all', n_unique=args.distinct, workers=16, context='subprocess')
    out = dict(distinct=len(pool))
    want = lambda part: args.only in (None, part)

    if want('launch'):
        out['launch'] = {}
        for envs, agents in ((4096, 4), (32768, 1)):
            geoms = [pool[i % len(pool)] for i in range(envs)]
            c = core.Core(scene.scenery(geoms, agents, device='cuda'), res=64)
            util.spawn(c, geoms, seed=0)
            util.random_velocities(c, np.random.RandomState(1), speed=1.5, spin=90.)
            mover = modules.MomentumMovement(c)
            a = c.agents
            start = [t.clone() for t in (a.positions, a.angles, a.velocity, a.angvelocity)]
            actions = torch.randint(0, 7, (envs, agents), generator=torch.Generator().manual_seed(2)).cuda()
            movement = (actions, mover._table, mover.keep)

            def restore():
                for t, s in zip((a.positions, a.angles, a.velocity, a.angvelocity), start):
                    t.copy_(s)
            plain_out, slide_out = cuda.physics(c.scenery, a, movement=movement), cuda.physics(c.scenery, a, movement=movement, slide=True)
            plain, slide = alternating([lambda: cuda.physics(c.scenery, a, movement=movement, out=plain_out),
                                        lambda: cuda.physics(c.scenery, a, movement=movement, slide=True, out=slide_out)], restore, args.repeats)
            same = bool(util.same_bits(plain_out.progress, slide_out.progress).all())
            shares = dict(blocked=float((slide_out.progress < 1).float().mean()), slid=float((slide_out.slid > 0).float().mean()),
                          stopped=float((slide_out.stopped > 0).float().mean()))
            out['launch'][f'{envs}x{agents}'] = dict(plain_seconds=plain, slide_seconds=slide, ratio=slide[0]/plain[0], same_progress=same, **shares)
            print(f'(a) {envs} x {agents}: plain {plain[0]*1e6:.1f} us [{plain[1]*1e6:.1f}, {plain[2]*1e6:.1f}], slide {slide[0]*1e6:.1f} us '
                  f'[{slide[1]*1e6:.1f}, {slide[2]*1e6:.1f}] - {slide[0]/plain[0]:.2f} x; agents blocked {shares["blocked"]:.3f}, '
                  f'slid {shares["slid"]:.3f}, stopped dead {shares["stopped"]:.3f}; the same progress: {same}')
            assert same
            del c

    if want('findings'):
        out['findings'] = {}
        for slide in (False, True):
            for name, kind in (('follow', ()), ('lookahead', ('lookahead',))):
                np.random.seed(0); torch.manual_seed(0)
                env = PointGoal(64, geometries=pool[:64], spl=True, slide=slide)
                key = f"{name}{'+slide' if slide else ''}"
                out['findings'][key] = expert_score(env, 300, *kind)
                print(f"(b) PointGoal(64, spl=True, slide={slide}), 300 steps under expert({', '.join(map(repr, kind))}): {out['findings'][key]}")

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
