"""What scent fields cost on the MI355X:

    python tools/scent_rate.py [--envs 4096] [--distinct 1024] [--repeats 20] [--torch-envs 256] [--json out.json]

At `--envs` envs over `--distinct` distinct synthetic floorplans (the headline's world), 4 agents at their spawn poses, one deposit
an agent, each call between two HIP events of its own, `--repeats` calls back to back, the median and the range:
    ScentFields.step at T = 1, 4 and 16 sub-steps (one shared store an env)
    ScentFields.sniff of `--envs` x 4 points
    modules.Scent - a deposit, a tick and the observation - eager and as one HIP graph
    the torch formulation of the same rule (grids padded to the largest, four shifted differences) at `--torch-envs` envs, T = 4,
    next to the kernel on the same envs - after a check that the two leave the same bits
and the LDS tier the plans land in.  Needs a GPU: there is no CPU fall-back.
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


class TorchScent:
    """The rule of MsNavScent in torch, one store an env: every env's grid padded to (H + 2, W + 2), closed and padding cells 0."""

    def __init__(self, grid, rate, keep, floor):
        geom = grid._host_geom
        n, H, W = len(geom), int(geom[:, 3].max()), int(geom[:, 2].max())
        self.open = torch.zeros((n, H + 2, W + 2), dtype=torch.bool, device='cuda')
        for e in range(n):
            _, ny, nx = grid.cells(e)
            self.open[e, 1:ny + 1, 1:nx + 1] = grid.image(e)
        self.V = torch.zeros((n, H + 2, W + 2), dtype=torch.float32, device='cuda')
        self.grid, self.rate, self.keep, self.floor = grid, rate, keep, floor
        self.origin = torch.as_tensor(geom[:, :2].copy(), device='cuda')
        self.side = [(0, -1), (0, 1), (-1, 0), (1, 0)]                  # west, east, south, north

    def step(self, points, amounts, T):
        """(A deposit per source by index_put: sources of one env on one cell would add in no fixed order - the tool's world has none.)"""
        cell = torch.floor(points/self.grid.cell).long() - self.origin[:, None]
        e = torch.arange(len(points), device='cuda')[:, None].expand(cell.shape[:2])
        i, j = cell[..., 1] + 1, cell[..., 0] + 1
        ok = self.open[e, i.clamp(0, self.V.shape[1] - 1), j.clamp(0, self.V.shape[2] - 1)] & (amounts > 0)
        self.V.index_put_((e[ok], i[ok], j[ok]), amounts[ok], accumulate=True)
        x, inner = self.V, self.open[:, 1:-1, 1:-1]
        H, W = inner.shape[1:]
        for _ in range(T):
            own, s = x[:, 1:-1, 1:-1], torch.zeros_like(inner, dtype=torch.float32)
            for di, dj in self.side:
                there = (slice(None), slice(1 + di, 1 + di + H), slice(1 + dj, 1 + dj + W))
                s = torch.where(self.open[there], s + (x[there] - own), s)
            v = (own + self.rate*s)*self.keep
            x = torch.nn.functional.pad(torch.where(inner & (v >= self.floor), v, torch.zeros_like(v)), (1, 1, 1, 1))
        self.V = x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--distinct', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--torch-envs', type=int, default=256)
    ap.add_argument('--json')
    args = ap.parse_args()
    from megastep_amd import core, cubicasa, cuda, modules, scene
    from tests import util

    np.random.seed(0); torch.manual_seed(0)
    pool = cubicasa.sample(args.distinct, split='all', n_unique=args.distinct, workers=16, context='subprocess')
    geoms = [pool[i % len(pool)] for i in range(args.envs)]
    c = core.Core(scene.scenery(geoms, 4, device='cuda', bake=False), res=64, fov=130)
    util.spawn(c, geoms, seed=0)
    grid = cuda.nav_grid(c.scenery, config=c.config)
    points, amounts = c.agents.positions, torch.ones((args.envs, 4), device='cuda')
    framed = np.sort((grid._host_geom[:, 2].astype(np.int64) + 2)*(grid._host_geom[:, 3] + 2))
    tier = int(np.searchsorted(cuda.SCENT_CAPACITY, grid._max_framed))
    out = dict(envs=args.envs, distinct=len(pool), median_framed=int(np.median(framed)), max_framed=grid._max_framed, tier=tier)
    print(f'{args.envs} envs x 4 agents, {len(pool)} plans: framed cells median {out["median_framed"]}, most {grid._max_framed}: the launch '
          f'takes tier {tier} of {cuda.SCENT_CAPACITY}' + (' (the global path for the largest)' if tier > 2 else ''))

    for T in (1, 4, 16):
        fields = cuda.scent_fields(grid, substeps=T)
        out[f'step_T{T}'] = t = back_to_back(lambda: fields.step(points, amounts), args.repeats)
        print(f'    ScentFields.step, T = {T:2d}: {us(t)}')
    fields = cuda.scent_fields(grid)
    fields.step(points, amounts)
    sniffed = fields.sniff(points)
    out['sniff'] = t = back_to_back(lambda: fields.sniff(points, out=sniffed), args.repeats)
    print(f'    ScentFields.sniff of {args.envs} x 4 points: {us(t)}')

    module = modules.Scent(c, grid)

    def act():
        module()
        return module.observation()

    out['module_eager'] = t = back_to_back(act, args.repeats)
    print(f'    modules.Scent, a tick and the observation, eager: {us(t)}')
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        act()
    out['module_graphed'] = t = back_to_back(graph.replay, args.repeats)
    print(f'    ... as one HIP graph: {us(t)}')

    m = min(args.torch_envs, args.envs)
    small = core.Core(scene.scenery(geoms[:m], 4, device='cuda', bake=False), res=64, fov=130)
    util.spawn(small, geoms[:m], seed=0)
    small_grid = cuda.nav_grid(small.scenery, config=small.config)
    ours, theirs = cuda.scent_fields(small_grid), TorchScent(small_grid, torch.tensor(.2).item(), torch.tensor(.98).item(), torch.tensor(1e-6).item())
    cells = torch.floor(small.agents.positions/small_grid.cell).long() + 2**20*torch.arange(m, device='cuda')[:, None, None]
    assert len(torch.unique(cells.view(-1, 2), dim=0)) == 4*m, 'two agents of an env share a cell: index_put has no order'
    for _ in range(3):
        ours.step(small.agents.positions, amounts[:m])
        theirs.step(small.agents.positions, amounts[:m], 4)
    for e in range(m):
        _, ny, nx = small_grid.cells(e)
        assert torch.equal(ours.image(e).view(torch.int32), theirs.V[e, 1:ny + 1, 1:nx + 1].view(torch.int32)), e
    out['kernel_small'] = t = back_to_back(lambda: ours.step(small.agents.positions, amounts[:m]), args.repeats)
    print(f'    {m} envs, T = 4, equal bits: the kernel {us(t)}')
    out['torch_small'] = t = back_to_back(lambda: theirs.step(small.agents.positions, amounts[:m], 4), args.repeats)
    print(f'    {m} envs, T = 4: the torch formulation {us(t)}')

    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
