"""Pixels per second of cuda.overhead (ms_overhead) on the MI355X, with the tile cull and without it:

    python tools/overhead_rate.py [--envs 4096] [--distinct 1024] [--agents 4] [--repeats 20] [--warmup 5] [--json out.json]
                                  [--only plan|agents] [--cull on|off]

The world is the headline's: `--envs` envs over `--distinct` distinct synthetic floorplans, four agents each.  Two workloads:
'plan' - one plan view of every env at 256 x 256 (cuda.plan_views, as scene.display frames it) - and 'agents' - what
modules.Overhead asks for, a 32 x 32 map of 4 m radius around every agent.  Each is timed with the cull on and with
ms_debug_overhead_cull(0), which keeps every line in every tile.  Times are HIP events around single calls after a warm-up;
the median of the repeats is reported (and the spread).  `--only` / `--cull` pick one workload and one setting (for a
profiler run of its own: `rocprofv3 --kernel-trace --stats -- python tools/overhead_rate.py --only agents --cull on`).
Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b)*1e-3)
    times = np.array(times)
    return float(np.median(times)), float(times.min()), float(times.max())


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--envs', type=int, default=4096)
    p.add_argument('--distinct', type=int, default=1024)
    p.add_argument('--agents', type=int, default=4)
    p.add_argument('--repeats', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--only', choices=('plan', 'agents'), default=None)
    p.add_argument('--cull', choices=('on', 'off'), default=None)
    p.add_argument('--json', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('overhead_rate.py needs a GPU')
    from megastep_amd import _lib, core, cubicasa, cuda, modules, scene
    np.random.seed(0)
    torch.manual_seed(0)
    pool = cubicasa.sample(args.distinct, split='all', n_unique=max(args.distinct, 16), seed=1, workers=32, context='subprocess')
    geometries = [pool[i % len(pool)] for i in range(args.envs)]
    sc = scene.scenery(geometries, args.agents, device='cuda', random=np.random.RandomState(0), fast=True)
    c = core.Core(sc, res=64, fov=130, fps=10)
    modules.RandomSpawns(geometries, c, fast=True)(c.agent_full(True))
    module = modules.Overhead(c, size=32, radius=4.)
    workloads = dict(plan=(cuda.plan_views(sc, 256), 256, scene.line_half_width(0.)),
                     agents=(module.views(), 32, module.half_width))
    results = dict(envs=args.envs, distinct_plans=len(pool), agents=args.agents, repeats=args.repeats, warmup=args.warmup)
    handle = _lib.lib()
    for kind, (views, size, half_width) in workloads.items():
        if args.only not in (None, kind):
            continue
        pixels = views.shape[0]*views.shape[1]*size*size
        out = cuda.overhead(sc, views, size, agents=c.agents, half_width=half_width, fields=('rgb',))
        for cull in ('on', 'off'):
            if args.cull not in (None, cull):
                continue
            handle.ms_debug_overhead_cull(1 if cull == 'on' else 0)
            try:
                t, lo, hi = timed(lambda: cuda.overhead(sc, views, size, agents=c.agents, half_width=half_width, fields=('rgb',), out=out),
                                  args.repeats, args.warmup)
            finally:
                handle.ms_debug_overhead_cull(1)
            results[f'{kind}_cull_{cull}'] = v = dict(s=t, min_s=lo, max_s=hi, pixels=pixels, pixels_per_s=pixels/t,
                                                      size=size, half_width=half_width)
            print(f'{kind:7s} cull {cull:3s} {pixels/1e6:7.1f} M px  {t*1e6:9.1f} us (min {lo*1e6:.1f}, max {hi*1e6:.1f})  '
                  f'{pixels/t/1e9:7.2f} G px/s', flush=True)
        if f'{kind}_cull_on' in results and f'{kind}_cull_off' in results:
            results[f'{kind}_cull_speedup'] = results[f'{kind}_cull_off']['s']/results[f'{kind}_cull_on']['s']
        del out
    print(json.dumps(results))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
