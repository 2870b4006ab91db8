"""Top-down pictures (`ms_overhead` / `cuda.overhead`, `cuda.plan_views`, `cuda.agent_views`) on the CPU: the C-ABI declares
and binds them, bad arguments are refused before any launch, the binary32 numpy rule the GPU tests (tests/test_gpu_overhead.py)
hold the kernel to agrees with a float64 statement of it, and the kernel's tile cull never drops a line that covers a pixel
of its tile."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols

F = np.float32
NONE = np.iinfo(np.int32).max


def pixel_centres(g, height, width):
    """(x, y), each (H, W) float32: the world point of every pixel centre under view g, as the kernel forms it."""
    g = np.asarray(g, F)
    u = (np.arange(width).astype(F) + F(.5))[None, :]
    w = (np.arange(height).astype(F) + F(.5))[:, None]
    return (g[0]*u + g[1]*w) + g[2], (g[3]*u + g[4]*w) + g[5]


def line_d2(x, y, line):
    """The rule's (d2, t) of one line (ax, ay, bx, by) at pixel centres (x, y), every operation in binary32."""
    ax, ay, bx, by = (F(c) for c in np.asarray(line, F).reshape(4))
    vx, vy = bx - ax, by - ay
    px, py = x - ax, y - ay
    vv = vx*vx + vy*vy
    with np.errstate(all='ignore'):
        t = ((px*vx + py*vy)/vv).astype(F) if vv > 0 else np.zeros_like(x)
        t = np.where(t < 0, F(0), np.where(t > 1, F(1), t)).astype(F)
        dx, dy = px - t*vx, py - t*vy
        d2 = dx*dx + dy*dy
    return d2, t


def overhead_rule(lines, g, height, width, half_width, af=0, textures=None, lit=True, background=(0., 0., 0.)):
    """The overhead rule (include/megastep_hip.h, MsOverhead) in binary32 numpy for one view of one env: `lines` (L, 2, 2)
    env-local in line order, the first `af` of them the agents'.  `textures`: (widths (L,), starts (L,), texels (T, 3),
    baked (T,)) - starts index into texels and baked - or None for indices alone.  Returns (rgb (3, H, W), indices (H, W))."""
    x, y = pixel_centres(g, height, width)
    h2 = F(half_width)*F(half_width)
    bd = np.full(x.shape, np.inf, F)
    bi = np.full(x.shape, NONE, np.int64)
    bt = np.zeros(x.shape, F)
    for l, line in enumerate(np.asarray(lines, F).reshape(-1, 4)):
        d2, t = line_d2(x, y, line)
        with np.errstate(invalid='ignore'):
            take = (d2 <= h2) & ((d2 < bd) | ((d2 == bd) & (l < bi)))
        bd, bi, bt = np.where(take, d2, bd), np.where(take, l, bi), np.where(take, t, bt)
    indices = np.where(bi == NONE, -1, bi).astype(np.int32)
    rgb = np.empty((3,) + x.shape, F)
    rgb[:] = np.asarray(background, F)[:, None, None]
    if textures is not None:
        widths, starts, texels, baked = (np.asarray(a) for a in textures)
        i, j = np.nonzero(indices >= 0)
        l = indices[i, j]
        wl = widths[l].astype(np.int64)
        q = np.minimum((bt[i, j]*wl.astype(F)).astype(np.int64), wl - 1)
        tex = np.where(wl > 0, starts[l].astype(np.int64) + q, 0)
        c = np.asarray(texels, F)[tex]
        bk = np.where(lit & (l >= af), np.asarray(baked, F)[tex], F(1))
        c = np.where((lit & (l >= af))[:, None], c*bk[:, None], c)
        rgb[:, i, j] = np.where((wl > 0)[:, None], c, F(0)).T
    return rgb, indices


def test_the_header_declares_overhead_and_the_loader_binds_it():
    from megastep_amd import _lib
    public = declared_symbols(('megastep_hip.h',))
    assert 'ms_overhead' in public
    assert not {'ms_host_overhead_keeps', 'ms_debug_overhead_cull'} & set(public)
    assert {'ms_host_overhead_keeps', 'ms_debug_overhead_cull'} <= set(declared_symbols(('megastep_hip_test.h',)))
    assert {'ms_overhead', 'ms_host_overhead_keeps', 'ms_debug_overhead_cull'} <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert hasattr(handle, 'ms_overhead') and handle.ms_abi_version() == 17


def test_msoverhead_mirror_has_the_c_layout():
    import subprocess
    import tempfile
    from megastep_amd import _lib
    fields = ('n_views', 'height', 'width', 'envs', 'views', 'half_width', 'lit', 'background', 'rgb', 'indices')
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "megastep_hip.h"\nint main(){printf("%zu", sizeof(MsOverhead));' +
           ''.join(f'printf(" %zu", offsetof(MsOverhead, {f}));' for f in fields) + '}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')])
        got = list(map(int, subprocess.check_output([os.path.join(d, 't')]).split()))
    assert got == [ctypes.sizeof(_lib.MsOverhead)] + [getattr(_lib.MsOverhead, f).offset for f in fields]


def test_bad_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    bg = (ctypes.c_float*3)(0, 0, 0)
    fake = ctypes.c_void_p(64)                      # (never dereferenced: every call below fails its checks first)
    ok = dict(n_images=1, n_views=1, height=8, width=8, envs=None, views=fake, half_width=.05, lit=1, background=bg,
              rgb=fake, indices=fake)
    assert h.ms_overhead(None, None, ctypes.byref(_lib.MsOverhead(**ok)), None) == -1
    assert h.ms_overhead(None, None, None, None) == -1
    sc = _lib.MsScenery(n_envs=1, n_agents=1, n_model=8, lines_vals=64, lines_widths=64, lines_starts=64, model=64,
                        textures_vals=64, textures_widths=64, textures_starts=64, baked_vals=64)
    assert h.ms_overhead(ctypes.byref(sc), None, None, None) == -1
    for bad in (dict(n_images=0), dict(n_views=0), dict(height=0), dict(width=-3), dict(views=None), dict(rgb=None, indices=None),
                dict(half_width=-1.), dict(half_width=float('nan')), dict(half_width=float('inf'))):
        assert h.ms_overhead(ctypes.byref(sc), None, ctypes.byref(_lib.MsOverhead(**{**ok, **bad})), None) == -1, bad
    ag = _lib.MsAgents(None, None, None, None, None)
    assert h.ms_overhead(ctypes.byref(sc), ctypes.byref(ag), ctypes.byref(_lib.MsOverhead(**ok)), None) == -1


def _cpu_world(n_envs=2, n_agents=2):
    from megastep_amd import core, cubicasa, scene
    from tests import util
    np.random.seed(0)
    geoms = cubicasa.sample(n_envs, n_unique=16)
    sc = scene.scenery(geoms, n_agents, device='cpu', random=np.random.RandomState(0), bake=False)
    c = core.Core(sc, res=16, fov=90)
    util.spawn(c, geoms, seed=1)
    return c


def test_overhead_refuses_cpu_tensors_and_bad_shapes():
    from megastep_amd import cuda
    c = _cpu_world()
    n = len(c.scenery.lines)
    views = torch.zeros(n, 1, 6)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.overhead(c.scenery, views, 16)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.overhead(c.scenery, views, 16, agents=c.agents)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.overhead(c.scenery, views, 16, envs=torch.zeros(n, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='views'):
        cuda.overhead(c.scenery, torch.zeros(n, 1, 5), 16)
    with pytest.raises(RuntimeError, match='views'):
        cuda.overhead(c.scenery, torch.zeros(n + 1, 1, 6), 16)             # one row per env without envs
    with pytest.raises(RuntimeError, match='envs'):
        cuda.overhead(c.scenery, views, 16, envs=torch.zeros(n + 1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='dtype'):
        cuda.overhead(c.scenery, views.double(), 16)
    with pytest.raises(RuntimeError, match='size'):
        cuda.overhead(c.scenery, views, (0, 16))
    with pytest.raises(RuntimeError, match='fields'):
        cuda.overhead(c.scenery, views, 16, fields=('screen',))
    with pytest.raises(RuntimeError, match='half_width'):
        cuda.overhead(c.scenery, views, 16, half_width=-1.)


def test_the_numpy_rule_is_its_float64_statement_away_from_the_boundaries():
    """On pixels whose centre is more than a millimetre from every coverage boundary (|distance - h|) and whose two nearest
    covering lines differ by more than a millimetre, the binary32 rule picks the line float64 geometry picks."""
    from megastep_amd import cubicasa
    geoms = cubicasa.sample(3, n_unique=16, seed=5)
    rng = np.random.RandomState(0)
    checked = 0
    for geom in geoms:
        walls = np.asarray(geom['walls'], np.float64).reshape(-1, 2, 2)
        lo, hi = walls.reshape(-1, 2).min(0), walls.reshape(-1, 2).max(0)
        for _ in range(2):
            a = rng.uniform(0, 2*np.pi)
            s = rng.uniform(.02, .1)*rng.choice([-1, 1])
            c = lo + rng.uniform(0, 1, 2)*(hi - lo)
            H, W = 41, 29
            g = np.array([s*np.cos(a), -s*np.sin(a), 0, s*np.sin(a), s*np.cos(a), 0])
            g[2] = c[0] - g[0]*W/2 - g[1]*H/2
            g[5] = c[1] - g[3]*W/2 - g[4]*H/2
            g = g.astype(F)
            h = .08
            _, got = overhead_rule(walls, g, H, W, h)
            x, y = (v.astype(np.float64) for v in pixel_centres(g, H, W))
            a_, b_ = walls[:, 0][:, None, None], walls[:, 1][:, None, None]
            v = b_ - a_
            px, py = x[None] - a_[..., 0], y[None] - a_[..., 1]
            vv = v[..., 0]**2 + v[..., 1]**2
            t = np.clip(np.where(vv > 0, (px*v[..., 0] + py*v[..., 1])/np.where(vv > 0, vv, 1), 0), 0, 1)
            d = np.hypot(px - t*v[..., 0], py - t*v[..., 1])                  # (L, H, W)
            covering = np.where(d <= h, d, np.inf)
            order = np.sort(covering, 0)
            want = np.where(np.isfinite(order[0]), np.argmin(covering, 0), -1)
            with np.errstate(invalid="ignore"):
                clear = (np.abs(d - h) > 1e-3).all(0) & ((order[1] - order[0] > 1e-3) | ~np.isfinite(order[1]))
            assert np.array_equal(got[clear], want[clear])
            checked += int(clear.sum())
            assert (want[clear] >= 0).any()
    assert checked > 1000


def _keeps(g, H, W, ty, tx, h, line):
    from megastep_amd import _lib
    gp = np.ascontiguousarray(g, F)
    lp = np.ascontiguousarray(line, F)
    f32p = ctypes.POINTER(ctypes.c_float)
    return _lib.lib().ms_host_overhead_keeps(gp.ctypes.data_as(f32p), H, W, ty, tx, F(h), lp.ctypes.data_as(f32p))


def test_the_tile_cull_never_drops_a_line_that_covers_a_pixel_of_the_tile():
    """Thousands of random tiles and segments - rotated, scaled and mirrored views, half widths from 1 mm to 1 m, zero-length
    and very long segments, coordinates up to 10^4 m, many laid right at the coverage boundary of one of the tile's pixel
    centres: whenever the binary32 rule has the line cover any pixel of the tile, ms_host_overhead_keeps keeps it."""
    rng = np.random.RandomState(1)
    covering = dropped = 0
    for trial in range(4000):
        H, W = rng.randint(1, 80, 2)
        ty, tx = rng.randint(0, (H + 15)//16), rng.randint(0, (W + 15)//16)
        s = 10**rng.uniform(-3, 1)
        a = rng.uniform(0, 2*np.pi)
        m = rng.choice([-1, 1])
        origin = rng.uniform(-1, 1, 2)*10**rng.uniform(0, 4)
        g = np.array([s*np.cos(a), -m*s*np.sin(a), origin[0], s*np.sin(a), m*s*np.cos(a), origin[1]], F)
        h = F(10**rng.uniform(-3, 0))
        i0, j0 = 16*ty, 16*tx
        i1, j1 = min(i0 + 16, H), min(j0 + 16, W)
        x, y = pixel_centres(g, H, W)
        x, y = x[i0:i1, j0:j1], y[i0:i1, j0:j1]
        kind = trial % 4
        pi, pj = rng.randint(0, i1 - i0), rng.randint(0, j1 - j0)
        P = np.array([x[pi, pj], y[pi, pj]], np.float64)
        if kind == 0:                                   # a segment whose nearest point to a pixel centre is at about h
            d = rng.normal(size=2)
            d /= np.linalg.norm(d)
            n = np.array([-d[1], d[0]])
            foot = P + n*float(h)*(1 + rng.uniform(-1e-6, 1e-6))
            length = 10**rng.uniform(-3, 4)
            t0 = rng.uniform(-1, 0)
            line = np.concatenate([foot + d*length*t0, foot + d*length*(1 + t0)])
        elif kind == 1:                                 # an endpoint at about h from a pixel centre
            d = rng.normal(size=2)
            d /= np.linalg.norm(d)
            end = P + d*float(h)*(1 + rng.uniform(-1e-6, 1e-6))
            line = np.concatenate([end, end + d*10**rng.uniform(-3, 4)])
        elif kind == 2:                                 # a zero-length segment near a pixel centre
            end = P + rng.normal(size=2)*float(h)
            line = np.concatenate([end, end])
        else:                                           # anywhere around the tile
            line = np.concatenate([P + rng.normal(size=2)*10**rng.uniform(-2, 4), P + rng.normal(size=2)*10**rng.uniform(-2, 4)])
        line = line.astype(F)
        d2, _ = line_d2(x, y, line)
        covers = bool((d2 <= h*h).any())
        keep = _keeps(g, H, W, ty, tx, h, line)
        assert keep in (0, 1)
        if covers:
            covering += 1
            assert keep == 1, (trial, g, H, W, ty, tx, h, line)
        dropped += keep == 0
    assert covering > 1000 and dropped > 500                 # (the boundary cases are exercised, and the cull does cull)
    g = np.array([np.nan, 0, 0, 0, 1, 0], F)                 # a view that is not finite keeps everything
    assert _keeps(g, 32, 32, 0, 0, F(.05), np.array([1e6, 1e6, 1e6 + 1, 1e6], F)) == 1
    g = np.array([np.inf, 0, 0, 0, 1, 0], F)
    assert _keeps(g, 32, 32, 1, 1, F(.05), np.array([-1e6, 1e6, -1e6 + 1, 1e6], F)) == 1


def test_plan_views_and_agent_views_on_cpu_tensors():
    """agent_views: the agent at the image centre, a point ahead of it above the centre, one to its right to the right;
    plan_views: the static lines' bounding box (grown by the margin) inside the image, north up."""
    from megastep_amd import cuda
    c = _cpu_world(3, 2)
    size = 32
    g = cuda.agent_views(c.agents, size, 4.).numpy().astype(np.float64)
    assert g.shape == (3, 2, 6)
    pos, ang = c.agents.positions.numpy().astype(np.float64), np.radians(c.agents.angles.numpy().astype(np.float64))
    inv = lambda g, p: np.linalg.solve(np.array([[g[0], g[1]], [g[3], g[4]]]), np.asarray(p) - np.array([g[2], g[5]]))
    for e in range(3):
        for a in range(2):
            np.testing.assert_allclose(inv(g[e, a], pos[e, a]), [size/2, size/2], atol=1e-3)
            fwd = np.array([np.cos(ang[e, a]), np.sin(ang[e, a])])
            u, w = inv(g[e, a], pos[e, a] + 2*fwd)
            assert abs(u - size/2) < 1e-3 and w < size/2 - 5
            u, w = inv(g[e, a], pos[e, a] + 2*np.array([fwd[1], -fwd[0]]))
            assert u > size/2 + 5 and abs(w - size/2) < 1e-3
            assert abs(np.hypot(g[e, a, 0], g[e, a, 3]) - 8/size) < 1e-6
    views = cuda.plan_views(c.scenery, (48, 64), margin=1.)
    assert views.shape == (3, 1, 6) and views.dtype == torch.float32
    af = c.scenery.n_agents*c.scenery.model.shape[0]
    for e in range(3):
        walls = c.scenery.lines[e][af:].numpy().reshape(-1, 2).astype(np.float64)
        gv = views[e, 0].numpy().astype(np.float64)
        assert gv[0] > 0 and gv[4] < 0 and gv[1] == 0 and gv[3] == 0      # north up
        for corner in ([walls[:, 0].min() - 1, walls[:, 1].min() - 1], [walls[:, 0].max() + 1, walls[:, 1].max() + 1]):
            u, w = inv(gv, corner)
            assert -1e-3 <= u <= 64 + 1e-3 and -1e-3 <= w <= 48 + 1e-3
    sub = cuda.plan_views(c.scenery, 16, envs=[2, 0])
    full = cuda.plan_views(c.scenery, 16)
    assert torch.equal(sub, full[[2, 0]])
