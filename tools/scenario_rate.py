"""What the scenarios cost on the MI355X, next to the two yardsticks there are:

    python tools/scenario_rate.py [--envs 4096] [--distinct 1024] [--agents 4] [--repeats 7] [--only call|findings] [--json out.json]

The world is the headline's: `--envs` envs over `--distinct` distinct synthetic floorplans, `--agents` agents each, at their spawn
poses with a walking velocity, under MomentumMovement's table and keep.
  (a) one call of the scenario kernel (ms_scenarios) - focal K x H = 49 x 8 (cuda.plans(7, 8, 2): LookAhead's) and 7 x 8 through
      cuda.rollouts(others=base), joint S = 64, H = 8 through cuda.scenarios - timed as 20 calls back to back between two HIP
      events, the median of `--repeats` such runs with [least, most].  Next to each: cuda.rollouts(others='rest') at the same
      K x H (the others frozen: A lanes fewer a candidate), and the launch loop the call replaces - for every scenario the agents
      restored (four copies) and H cuda.physics(movement=...) launches, S H launches in all (focal: A K H), timed between two events
      around the whole loop (the median of 3 loops).  The loop's end states are held against the call's as bits while at it.
  (b) findings, from PointGoal(64, n_agents=4, spl=True), 300 steps under expert('lookahead') and expert('anticipate'): arrivals,
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

from tools.rollout_rate import back_to_back, expert_score   # noqa: E402


def launch_loop(c, mover, scenarios):
    """The parent's way to the same numbers: `scenarios` is a list of (N, A, H) plans - per scenario the agents restored and H
    physics launches. Returns run(check) -> the end states (positions, angles, velocity, angvelocity), each (N, len, A[, 2])."""
    from megastep_amd import cuda
    a = c.agents
    start = [a.positions.clone(), a.angles.clone(), a.velocity.clone(), a.angvelocity.clone()]
    N, A = a.angles.shape
    H = scenarios[0].shape[-1]
    acts = [[plan[:, :, h].contiguous() for h in range(H)] for plan in scenarios]
    ends = [torch.empty((N, len(scenarios), A, 2), device='cuda'), torch.empty((N, len(scenarios), A), device='cuda'),
            torch.empty((N, len(scenarios), A, 2), device='cuda'), torch.empty((N, len(scenarios), A), device='cuda')]
    out = cuda.physics(c.scenery, a)

    def restore():
        a.positions.copy_(start[0]); a.angles.copy_(start[1]); a.velocity.copy_(start[2]); a.angvelocity.copy_(start[3])

    def run(check=False):
        """(timed lean: the restores and the launches alone; ``check`` also gathers the end states)"""
        for s in range(len(acts)):
            restore()
            for h in range(H):
                cuda.physics(c.scenery, a, movement=(acts[s][h], mover._table, mover.keep), out=out)
            if check:
                ends[0][:, s], ends[1][:, s], ends[2][:, s], ends[3][:, s] = a.positions, a.angles, a.velocity, a.angvelocity
        restore()
        return ends
    restore()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--distinct', type=int, default=1024)
    ap.add_argument('--agents', type=int, default=4)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--only', choices=('call', 'findings'))
    ap.add_argument('--json')
    args = ap.parse_args()
    from megastep_amd import core, cubicasa, cuda, modules, scene
    from megastep_amd.demo import PointGoal
    from tests import util

    np.random.seed(0); torch.manual_seed(0)
    pool = cubicasa.sample(args.distinct, split='all', n_unique=args.distinct, workers=16, context='subprocess')
    geoms = [pool[i % len(pool)] for i in range(args.envs)]
    N, A = args.envs, args.agents
    out = dict(envs=N, distinct=len(pool), agents=A)
    want = lambda part: args.only in (None, part)
    STATE = ('positions', 'angles', 'velocity', 'angvelocity')
    us = lambda t: '{:.1f} us [{:.1f}, {:.1f}]'.format(*(1e6*x for x in t))

    if want('call'):
        sc = scene.scenery(geoms, A, device='cuda')
        c = core.Core(sc, res=64)
        util.spawn(c, geoms, seed=0)
        util.random_velocities(c, np.random.RandomState(1), speed=1.5, spin=90.)
        mover = modules.MomentumMovement(c)
        g = torch.Generator().manual_seed(2)
        out['call'] = {}
        base = torch.randint(0, 7, (N, A, 8), generator=g).cuda()
        for name, plans in (('focal 49x8', cuda.plans(7, 8, 2, device='cuda')), ('focal 7x8', cuda.plans(7, 8, device='cuda'))):
            K, H = plans.shape
            rolled = mover.rollouts(plans, others=base)
            call = back_to_back(lambda: mover.rollouts(plans, others=base, out=rolled), 20, args.repeats)
            rest = mover.rollouts(plans, others='rest')
            frozen = back_to_back(lambda: mover.rollouts(plans, others='rest', out=rest), 20, args.repeats)
            scenarios = []
            for f in range(A):
                for k in range(K):
                    plan = base.clone()
                    plan[:, f] = plans[k]
                    scenarios.append(plan)
            loop = launch_loop(c, mover, scenarios)
            ends = loop(check=True)
            same = all(bool(util.same_bits(torch.stack([torch.stack([e[:, f*K + k, f] for k in range(K)], 1) for f in range(A)], 1),
                                           getattr(rolled, field)).all()) for e, field in zip(ends, STATE))
            looped = back_to_back(loop, 1, 3, warmup=1)
            out['call'][name] = dict(K=K, H=H, seconds=call, others_rest_seconds=frozen, loop_seconds=looped, launches=A*K*H, equal_bits=same,
                                     stopped_share=float((rolled.stops > 0).float().mean()), stopped_share_rest=float((rest.stops > 0).float().mean()))
            print(f"(a) {name}, {N} x {A}: rollouts(others=base) {us(call)}; rollouts(others='rest') {us(frozen)} - {call[0]/frozen[0]:.2f} x; "
                  f'the loop of {A*K*H} physics launches {looped[0]*1e3:.2f} ms [{looped[1]*1e3:.2f}, {looped[2]*1e3:.2f}] - {looped[0]/call[0]:.0f} x; '
                  f"equal bits: {same}; candidates stopped at least once: {out['call'][name]['stopped_share']:.3f} (others at rest: "
                  f"{out['call'][name]['stopped_share_rest']:.3f})")
            assert same
        S, H = 64, 8
        actions = torch.randint(0, 7, (N, S, A, H), generator=g).cuda()
        rolled = mover.scenarios(actions)
        call = back_to_back(lambda: mover.scenarios(actions, out=rolled), 20, args.repeats)
        per_agent = actions.transpose(1, 2).contiguous()
        rest = mover.rollouts(per_agent, others='rest')
        frozen = back_to_back(lambda: mover.rollouts(per_agent, others='rest', out=rest), 20, args.repeats)
        loop = launch_loop(c, mover, [actions[:, s] for s in range(S)])
        ends = loop(check=True)
        same = all(bool(util.same_bits(e, getattr(rolled, field)).all()) for e, field in zip(ends, STATE))
        looped = back_to_back(loop, 1, 3, warmup=1)
        out['call']['joint 64x8'] = dict(S=S, H=H, seconds=call, others_rest_seconds=frozen, loop_seconds=looped, launches=S*H, equal_bits=same,
                                         stopped_share=float((rolled.stops > 0).float().mean()))
        print(f"(a) joint S x H = {S} x {H}, {N} x {A}: scenarios {us(call)}; rollouts(others='rest') at K = {S} {us(frozen)} - {call[0]/frozen[0]:.2f} x; "
              f'the loop of {S*H} physics launches {looped[0]*1e3:.2f} ms [{looped[1]*1e3:.2f}, {looped[2]*1e3:.2f}] - {looped[0]/call[0]:.0f} x; '
              f"equal bits: {same}; agents stopped at least once: {out['call']['joint 64x8']['stopped_share']:.3f}")
        assert same
        del c, sc

    if want('findings'):
        out['findings'] = {}
        for kind in ('lookahead', 'anticipate'):
            np.random.seed(0); torch.manual_seed(0)
            env = PointGoal(64, n_agents=4, geometries=pool[:64], spl=True)
            out['findings'][kind] = expert_score(env, 300, kind)
            print(f"(b) PointGoal(64, n_agents=4, spl=True), 300 steps under expert({kind!r}): {out['findings'][kind]}")

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
