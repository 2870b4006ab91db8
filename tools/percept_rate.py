"""What percepts cost on the MI355X:

    python tools/percept_rate.py [--envs 4096] [--distinct 1024] [--repeats 20] [--only launches|env|play] [--json out.json]

  (a) at `--envs` envs over `--distinct` distinct synthetic floorplans (the headline's world), agents at their spawn poses, each call
      between two HIP events of its own, `--repeats` calls back to back, the median and the range:
        cuda.percepts in agents form, A = 4, K = 3, a cone of 130 degrees
        cuda.percepts of E = 4 eyes on P = 64 and on P = 1024 random points at R = 10
      and next to each
        the route a caller had before: one cuda.raycast of the same pairs as rays, then torch's where / sort / gather for the nearest
        K.  It is another rule (a near plane, first-hit order), so only the time compares; the share of pairs on which the two
        disagree is printed.
        the torch formulation of this rule - padded walls, a loop over the wall index - on 256 envs, its outputs equal to the
        kernel's, its time scaled to `--envs`.
  (b) Tag(`--envs`, 2, 2).step under random actions, eager and as one HIP graph, next to Deathmatch(`--envs`, 4).step in the same run.
  (c) as a finding: Tag(64, 1, 1) for 300 steps under env.expert() and under random actions - the tags, and the share of steps a
      hider spent out of every seeker's sight.
`--only` picks one part (for a profiler run of its own).  Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import math
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


def us(t, scale=1.):
    return f'{t[0]*scale*1e6:.1f} us [{t[1]*scale*1e6:.1f}, {t[2]*scale*1e6:.1f}]'


def nearest_of(visible, squares, k):
    """torch's where / sort / gather: (nearest (N, E, K) int64, -1 beyond the visible ones; their squares)."""
    p = visible.shape[-1]
    keys = torch.where(visible, squares, torch.full_like(squares, float('inf')))
    order = keys.sort(dim=-1, stable=True)
    index, rr = order.indices[..., :k], order.values[..., :k]
    if k > p:
        index, rr = torch.nn.functional.pad(index, (0, k - p), value=-1), torch.nn.functional.pad(rr, (0, k - p), value=float('inf'))
    return torch.where(torch.isfinite(rr), index, torch.full_like(index, -1)), rr


def by_raycast(cuda, scenery, eyes, points, R, k, headings=None, cos_half=0., pairs=None, out=None):
    """The route a caller had before: a ray from every eye towards every point, seen when nothing is hit nearer than the point."""
    n, e, p = eyes.shape[0], eyes.shape[1], points.shape[1]
    offsets = points[:, None] - eyes[:, :, None]                        # (N, E, P, 2)
    origins = eyes[:, :, None].expand(n, e, p, 2).reshape(n, e*p, 2).contiguous()
    hit = cuda.raycast(scenery, origins, offsets.reshape(n, e*p, 2).contiguous(), near=0., fields=('distances',), out=out)
    squares = (offsets*offsets).sum(-1)
    span = squares.sqrt()
    visible = (hit.distances.reshape(n, e, p) >= span) & (squares <= R*R)
    if headings is not None:
        hlen = (headings*headings).sum(-1).sqrt()[..., None]
        visible &= (headings[:, :, None]*offsets).sum(-1) >= cos_half*span*hlen
    if pairs is not None:
        visible &= pairs.bool()
    return visible, squares, nearest_of(visible, squares, k)[0], hit


def by_torch(walls, eyes, points, R, k, headings=None, cos_half=0., pairs=None):
    """This rule in torch: `walls` (N, L, 4) padded with NaN rows (they block nothing), a loop over the wall index, every statement
    one binary32 operation in the header's order."""
    px, py = eyes[:, :, None, 0], eyes[:, :, None, 1]
    x, y = points[:, None, :, 0], points[:, None, :, 1]
    rx, ry = x - px, y - py
    rr = rx*rx + ry*ry
    live = torch.isfinite(px) & torch.isfinite(py)
    ok = live & (rr <= R*R)
    if headings is not None:
        hx, hy = headings[:, :, None, 0], headings[:, :, None, 1]
        hlen = (hx*hx + hy*hy).sqrt()
        ok &= torch.isfinite(hlen) & (hlen > 0) & (hx*rx + hy*ry >= (cos_half*rr.sqrt())*hlen)
    if pairs is not None:
        ok &= pairs.bool()
    sx0, sx1, sy0, sy1 = torch.minimum(px, x), torch.maximum(px, x), torch.minimum(py, y), torch.maximum(py, y)
    blocked = torch.zeros_like(ok)
    for l in range(walls.shape[1]):
        ax, ay, bx, by = (walls[:, l, i][:, None, None] for i in range(4))
        meets = (torch.minimum(ax, bx) <= sx1) & (torch.maximum(ax, bx) >= sx0) & (torch.minimum(ay, by) <= sy1) & (torch.maximum(ay, by) >= sy0)
        vx, vy = bx - ax, by - ay
        o1 = vx*(py - ay) - vy*(px - ax)
        o2 = vx*(y - ay) - vy*(x - ax)
        apart = ((o1 < 0) & (o2 > 0)) | ((o1 > 0) & (o2 < 0))
        o3 = rx*(ay - py) - ry*(ax - px)
        o4 = rx*(by - py) - ry*(bx - px)
        across = ((o3 <= 0) & (o4 >= 0)) | ((o3 >= 0) & (o4 <= 0))
        blocked |= meets & apart & across
    visible = ok & ~blocked
    return visible, rr, nearest_of(visible, rr, k)[0]


def padded_walls(scenery, envs):
    """(envs, L, 4): the static rows of the first `envs` envs, padded with NaN rows."""
    lines = scenery.lines
    af = scenery.n_agents*scenery.model.shape[0]
    starts, widths = lines.starts[:envs].long(), lines.widths[:envs].long()
    most = int((widths - af).max())
    index = torch.arange(most, device=starts.device)[None]
    rows = lines.vals.reshape(-1, 4)[(starts[:, None] + af + index).clamp(max=lines.vals.shape[0] - 1)]
    return torch.where((index < (widths - af)[:, None])[..., None], rows, torch.full_like(rows, float('nan'))).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--distinct', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--only', choices=('launches', 'env', 'play'))
    ap.add_argument('--json')
    args = ap.parse_args()
    from megastep_amd import arrdict, core, cubicasa, cuda, graphs, scene
    from megastep_amd.demo import Deathmatch, Tag
    from megastep_amd.nav import _static_boxes
    from tests import util

    np.random.seed(0); torch.manual_seed(0)
    want = lambda part: args.only in (None, part)
    out = dict(envs=args.envs)
    if want('launches') or want('env'):
        pool = cubicasa.sample(args.distinct, split='all', n_unique=args.distinct, workers=16, context='subprocess')
        geoms = [pool[i % len(pool)] for i in range(args.envs)]
        out['distinct'] = len(pool)

    if want('launches'):
        n, sub = args.envs, min(256, args.envs)
        c = core.Core(scene.scenery(geoms, 4, device='cuda'), res=64, fov=130)
        util.spawn(c, geoms, seed=0)
        sc, ag = c.scenery, c.agents
        walls = padded_walls(sc, sub)
        cos_half = math.cos(math.radians(130.)/2.)
        res = {}
        print(f'(a) {n} envs, {len(pool)} plans; at most {walls.shape[1]} static walls an env among the first {sub}')
        # the agents look at each other
        seen = cuda.percepts(sc, agents=ag, fov=130., k=3)
        others = (1 - torch.eye(4, dtype=torch.uint8, device='cuda'))
        eyes = ag.positions
        vis, _, near, hit = by_raycast(cuda, sc, eyes, eyes, 10., 3, seen.headings, cos_half, others)
        t_vis, _, t_near = by_torch(walls, eyes[:sub], eyes[:sub], 10., 3, seen.headings[:sub], cos_half, others)
        equal = bool(torch.equal(t_vis, seen.visible[:sub].bool())) and bool(torch.equal(t_near, seen.nearest[:sub].long()))
        differ = float((vis != seen.visible.bool())[:, others.bool()].float().mean())
        res['agents'] = dict(
            percepts=back_to_back(lambda: cuda.percepts(sc, agents=ag, fov=130., k=3, out=seen), args.repeats),
            raycast_route=back_to_back(lambda: by_raycast(cuda, sc, eyes, eyes, 10., 3, seen.headings, cos_half, others, hit), args.repeats),
            torch_rule_256=back_to_back(lambda: by_torch(walls, eyes[:sub], eyes[:sub], 10., 3, seen.headings[:sub], cos_half, others), max(args.repeats//4, 3), 1),
            torch_equal=equal, raycast_disagrees=differ, visible=float(seen.visible.float().sum()/(n*12)))
        r = res['agents']
        print(f'    agents form, A = 4, K = 3, 130 degrees: visible share of the pairs {r["visible"]:.3f}')
        print(f'      cuda.percepts                                  {us(r["percepts"])}')
        print(f'      raycast + where/sort/gather                    {us(r["raycast_route"])} (disagrees on {differ:.4f} of the pairs)')
        print(f'      the rule in torch, {sub} envs scaled to {n}     {us(r["torch_rule_256"], n/sub)} (outputs equal: {equal})')
        # eyes on random points
        lo, hi = _static_boxes(sc)
        for p in (64, 1024):
            points = (lo[:, None] + torch.rand((n, p, 2), device='cuda')*(hi - lo)[:, None]).contiguous()
            seen = cuda.percepts(sc, points, eyes=eyes, max_range=10., k=4)
            vis, _, near, hit = by_raycast(cuda, sc, eyes, points, 10., 4)
            t_vis, _, t_near = by_torch(walls, eyes[:sub], points[:sub], 10., 4)
            equal = bool(torch.equal(t_vis, seen.visible[:sub].bool())) and bool(torch.equal(t_near, seen.nearest[:sub].long()))
            differ = float((vis != seen.visible.bool()).float().mean())
            r = res[f'points_{p}'] = dict(
                percepts=back_to_back(lambda: cuda.percepts(sc, points, eyes=eyes, max_range=10., k=4, out=seen), args.repeats),
                raycast_route=back_to_back(lambda: by_raycast(cuda, sc, eyes, points, 10., 4, out=hit), args.repeats),
                torch_rule_256=back_to_back(lambda: by_torch(walls, eyes[:sub], points[:sub], 10., 4), max(args.repeats//4, 3), 1),
                torch_equal=equal, raycast_disagrees=differ, visible=float(seen.visible.float().mean()))
            print(f'    E = 4 eyes on P = {p} random points, R = 10, K = 4: visible share of the pairs {r["visible"]:.3f}')
            print(f'      cuda.percepts                                  {us(r["percepts"])}')
            print(f'      raycast + where/sort/gather                    {us(r["raycast_route"])} (disagrees on {differ:.4f} of the pairs)')
            print(f'      the rule in torch, {sub} envs scaled to {n}     {us(r["torch_rule_256"], n/sub)} (outputs equal: {equal})')
            del points, seen, vis, near, hit
        out['launches'] = res
        del c, sc, ag, walls

    if want('env'):
        out['env'] = {}
        for name in ('Tag', 'Deathmatch'):
            for graphed in (False, True):
                np.random.seed(0); torch.manual_seed(0)
                inner = Tag(args.envs, 2, 2, geometries=geoms) if name == 'Tag' else Deathmatch(4*args.envs, 4, geometries=geoms)
                env = graphs.GraphedStep(inner) if graphed else inner
                env.reset()
                shape = (args.envs, 4) if name == 'Tag' else (4*args.envs, 1)
                actions = arrdict.arrdict(actions=torch.randint(0, 7, shape, device='cuda'))
                t = back_to_back(lambda: env.step(actions), args.repeats)
                out['env'][f"{name}_{'graphed' if graphed else 'eager'}"] = t
                label = f'Tag({args.envs}, 2, 2)' if name == 'Tag' else f'Deathmatch({4*args.envs}, 4) on {args.envs} plans'
                print(f'(b) {label}.step, {"one HIP graph" if graphed else "eager"}: {us(t)}')
                del env, inner

    if want('play'):
        out['play'] = {}
        from tests.test_navfield_host import plans
        for policy in ('expert', 'random'):
            np.random.seed(1); torch.manual_seed(1)
            env = Tag(64, 1, 1, geometries=plans(64))
            env.reset()
            rng = np.random.RandomState(2)
            tags = unseen = 0
            for _ in range(300):
                decision = env.expert() if policy == 'expert' else arrdict.arrdict(actions=torch.as_tensor(rng.randint(0, 7, (64, 2)), device='cuda'))
                world = env.step(decision)
                tags += int(env._tagged.sum())
                unseen += int((world.reward[:, 1] == env.hide_bonus).sum())
            out['play'][policy] = dict(tags=tags, unseen_share=unseen/(300*64))
            print(f'(c) Tag(64, 1, 1), 300 steps, {policy}: {tags} tags; the hider out of sight on {unseen/(300*64):.3f} of its steps')

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
