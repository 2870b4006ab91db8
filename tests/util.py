"""Shared helpers for the parity tests: moving a product-side Core into the oracle's numpy world and comparing."""
import numpy as np
import torch
from oracle import oracle as O


def scene_dict(scenery):
    """cuda.Scenery -> the oracle's scene dict (numpy copies)."""
    n = lambda t: t.detach().cpu().numpy().copy()
    return dict(
        n_agents=scenery.n_agents, model=n(scenery.model),
        lights_vals=n(scenery.lights.vals), lights_widths=n(scenery.lights.widths),
        lines_vals=n(scenery.lines.vals), lines_widths=n(scenery.lines.widths),
        textures_vals=n(scenery.textures.vals), textures_widths=n(scenery.textures.widths),
        baked_vals=n(scenery.baked.vals))


def agents_dict(agents):
    n = lambda t: t.detach().cpu().numpy().copy()
    return dict(angles=n(agents.angles), positions=n(agents.positions),
                angvelocity=n(agents.angvelocity), velocity=n(agents.velocity))


class OracleWorld:
    """The oracle's copy of a Core: same scene, same config, agents pulled on demand."""

    def __init__(self, core):
        self.scene = O.Scene(scene_dict(core.scenery))
        self.cfg = O.config(core.agent_radius, core.res, core.fov, core.fps)
        self.agents = agents_dict(core.agents)

    def pull_agents(self, core):
        self.agents = agents_dict(core.agents)

    def pull_baked(self, core):
        self.scene.baked_vals[:] = core.scenery.baked.vals.cpu().numpy()

    def bake(self):
        return O.bake(self.scene, self.cfg).copy()

    def physics(self):
        progress, self.agents = O.physics(self.scene, self.agents, self.cfg)
        return progress, self.agents

    def render(self):
        return O.render(self.scene, self.agents, self.cfg)


def spawn(core, geometries, seed=0):
    """Puts every agent on a random free cell of its geometry with a random heading."""
    rng = np.random.RandomState(seed)
    from megastep_amd import geometry
    pos = np.zeros((core.n_envs, core.n_agents, 2), np.float32)
    for e, g in enumerate(geometries):
        free = np.stack((g['masks'] > 0).nonzero(), -1)
        pick = free[rng.choice(len(free), core.n_agents)]
        pos[e] = geometry.centers(pick, g['masks'].shape, g['res'])
    core.agents.positions[:] = torch.as_tensor(pos, device=core.device)
    core.agents.angles[:] = torch.as_tensor(rng.uniform(-180, 180, (core.n_envs, core.n_agents)).astype(np.float32), device=core.device)


def random_velocities(core, rng, speed=3., spin=180.):
    shape = (core.n_envs, core.n_agents)
    core.agents.velocity[:] = torch.as_tensor(rng.uniform(-speed, speed, shape + (2,)).astype(np.float32), device=core.device)
    core.agents.angvelocity[:] = torch.as_tensor(rng.uniform(-spin, spin, shape).astype(np.float32), device=core.device)


def _np(t):
    return t.detach().cpu().numpy()


def assert_physics_matches(core, p, progress_ref, agents_ref, atol=1e-5):
    """Bit-exact collision masks; float state within the north-star tolerance (1e-5)."""
    progress = _np(p.progress)
    np.testing.assert_array_equal(progress < 1, progress_ref < 1, err_msg='collision masks differ')
    np.testing.assert_allclose(progress, progress_ref, rtol=0, atol=atol)
    for k in ('positions', 'velocity', 'angvelocity'):
        np.testing.assert_allclose(_np(getattr(core.agents, k)), agents_ref[k], rtol=0, atol=atol, err_msg=k)
    # angles live in [-180, 180): one binary32 ulp there is 1.5e-5, so compare modulo that
    np.testing.assert_allclose(_np(core.agents.angles), agents_ref['angles'], rtol=0, atol=2e-5, err_msg='angles')


def assert_render_matches(core, r, ref, atol=1e-5):
    """Bit-exact hit indices (and miss sentinels); floats within 1e-5."""
    idx = _np(r.indices)
    np.testing.assert_array_equal(idx, ref['indices'], err_msg='hit indices differ')
    hit = idx >= 0
    for k in ('locations', 'dots', 'distances'):
        got, want = _np(getattr(r, k)), ref[k]
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=k)
        np.testing.assert_array_equal(np.isinf(got), np.isinf(want), err_msg=k)
        np.testing.assert_allclose(got[hit], want[hit], rtol=0, atol=atol, err_msg=k)
    np.testing.assert_allclose(_np(r.screen), ref['screen'], rtol=0, atol=atol, err_msg='screen')


# ---- bits: the product is defined as the oracle's binary32 results, so the GPU comparisons hold every float to its
# 32-bit pattern. Any NaN equals any NaN (DESIGN 5's convention); -0. differs from +0.; integers compare by ==.

def _arr(t):
    return _np(t) if isinstance(t, torch.Tensor) else np.asarray(t)


def _same_kind(got, want, what='arrays'):
    assert got.shape == want.shape, f'{what}: shapes differ: {got.shape} vs {want.shape}'
    assert got.dtype == want.dtype, f'{what}: dtypes differ: {got.dtype} vs {want.dtype}'
    assert got.dtype == np.float32 or got.dtype.kind in 'iub', f'{what}: binary32 or integers, not {got.dtype}'


def same_bits(got, want):
    """Elementwise, for two arrays of one shape and dtype: binary32 values are the same when their 32-bit patterns are, or when
    both are NaN (of whatever payload); integers and booleans when they are =="""
    got, want = _arr(got), _arr(want)
    _same_kind(got, want)
    if got.dtype != np.float32:
        return got == want
    return (np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def _on_the_line(x):
    """Binary32 patterns (sign and magnitude) as int64 points of one monotone line: -0. and +0. both at 0, the smallest
    denormals at -1 and +1, the infinities at -/+ 0x7f800000, NaNs beyond them."""
    b = np.ascontiguousarray(x).view(np.uint32).astype(np.int64)
    mag = b & 0x7fffffff
    return np.where(b >> 31 != 0, -mag, mag)


def ulp_distance(got, want):
    """How many binary32 values lie between two floats (elementwise, int64), across zero too."""
    return np.abs(_on_the_line(np.asarray(got, np.float32)) - _on_the_line(np.asarray(want, np.float32)))


def assert_bits(got, want, what='values'):
    """Fails unless same_bits() holds everywhere, saying how many elements differ, where the first five are and what they hold
    (as float.hex), the largest distance in ulps and the largest absolute difference."""
    got, want = _arr(got), _arr(want)
    _same_kind(got, want, what)
    bad = ~same_bits(got, want)
    if not bad.any():
        return
    where = np.argwhere(bad)
    show = (lambda v: float(v).hex()) if got.dtype == np.float32 else (lambda v: repr(v.item()))
    first = '; '.join(f'{tuple(int(i) for i in ix)}: got {show(got[tuple(ix)])}, want {show(want[tuple(ix)])}' for ix in where[:5])
    msg = f'{what}: {int(bad.sum())} of {bad.size} elements differ in their bits. First: {first}.'
    if got.dtype == np.float32:
        g, w = got[bad], want[bad]
        with np.errstate(invalid='ignore', over='ignore'):
            diff = np.abs(g.astype(np.float64) - w.astype(np.float64))
        diff = diff[~np.isnan(diff)]                    # (a NaN against a number, inf against inf of the other sign...: no difference to name)
        largest = f'{diff.max():.3g}' if diff.size else 'nan'
        msg += f' Largest distance: {int(ulp_distance(g, w).max())} ulp; largest absolute difference: {largest}.'
    raise AssertionError(msg)


def assert_physics_bits(core, p, progress_ref, agents_ref):
    """The collision masks first (their message says most), then progress and the agents' state, bit for bit."""
    progress = _np(p.progress)
    np.testing.assert_array_equal(progress < 1, progress_ref < 1, err_msg='collision masks differ')
    assert_bits(progress, progress_ref, 'progress')
    for k in ('positions', 'velocity', 'angvelocity', 'angles'):
        assert_bits(getattr(core.agents, k), agents_ref[k], k)


def assert_render_bits(core, r, ref):
    """Hit indices (and miss sentinels) equal; the four float planes bit for bit, everywhere - also where a ray missed."""
    np.testing.assert_array_equal(_np(r.indices), ref['indices'], err_msg='hit indices differ')
    for k in ('locations', 'dots', 'distances', 'screen'):
        assert_bits(getattr(r, k), ref[k], k)


def pooled_rule(screen, distances, agent_radius, max_depth, sub):
    """The pooled observations' rule (render.h, "pooled observations") in numpy's binary32, on full-resolution
    planes - screen (N, A, R, 3) and distances (N, A, R) - giving rgb (N, A, 3, R/sub) and depth (N, A, R/sub). Per ray the depth
    1 - clamp((d - agent_radius)*(1.f/max_depth), 0, 1), a ray that missed (+inf) giving 0; then, for depth and each colour, the
    sum of `sub` adjacent rays as a pairwise tree - (x0 + x1) + (x2 + x3), ... - times 2^-log2(sub)."""
    f = np.float32
    assert sub >= 1 and sub & (sub - 1) == 0 and distances.shape[-1] % sub == 0
    screen, distances = np.asarray(screen, f), np.asarray(distances, f)
    depth = f(1) - np.minimum(np.maximum((distances - f(agent_radius))*(f(1)/f(max_depth)), f(0)), f(1))

    def pool(x):
        x = x.reshape(x.shape[:-1] + (x.shape[-1]//sub, sub))
        while x.shape[-1] > 1:
            x = x[..., 0::2] + x[..., 1::2]
        return x[..., 0]*f(1./sub)
    rgb = pool(np.moveaxis(screen, -1, -2))
    assert rgb.dtype == f and depth.dtype == f
    return rgb, pool(depth)


def scenery_by_the_book(geometries, n_agents, random=np.random):
    """The reference's assembly loop (scene.py:75-100) over the product's per-env helpers - repeat, gamma-decode and
    concatenate, one geometry at a time. Slow and obviously right: what scene.scenery's vectorised build is checked
    against. Returns numpy arrays (float32 / int32, as arrdict.torchify would make them)."""
    from megastep_amd import scene
    model = scene.agent_model()
    agentlines, agentcolors = np.tile(model, (n_agents, 1, 1)), np.tile(scene.agent_colors(), (n_agents, 1))
    lights, lines, texels, counts = [], [], [], []
    for g in geometries:
        lights.append(scene.random_lights(g['lights']))
        tex, cnt = scene.init_textures(agentlines, agentcolors, g['walls'], random)
        lines.append(np.concatenate([agentlines, g['walls']]))
        texels.append(tex)
        counts.append(cnt)
    return dict(
        lights_vals=np.concatenate(lights).astype(np.float32), lights_widths=np.array([len(x) for x in lights], np.int32),
        lines_vals=np.concatenate(lines).astype(np.float32), lines_widths=np.array([len(x) for x in lines], np.int32),
        textures_vals=np.concatenate(texels).astype(np.float32), textures_widths=np.concatenate(counts).astype(np.int32))


class OracleSubset:
    """The oracle's copy of a few envs of a (large) Core: what the full-size tests compare a sample against."""

    def __init__(self, core, envs):
        sc = core.scenery
        self.envs = np.asarray(envs)
        e = torch.as_tensor(self.envs, device=core.device)
        ln, li, tx = sc.lines, sc.lights, sc.textures
        rows = lambda r, which: torch.cat([torch.arange(int(r.starts[i]), int(r.ends[i]), device=core.device) for i in which]) \
            if len(which) else torch.zeros(0, dtype=torch.long, device=core.device)
        self.line_rows = rows(ln, self.envs)
        light_rows = rows(li, self.envs)
        tstart, tend = tx.starts.long()[self.line_rows], tx.ends.long()[self.line_rows]
        self.texel_rows = torch.cat([torch.arange(int(a), int(b), device=core.device) for a, b in
                                     zip(tx.starts.long()[ln.starts.long()[e]].tolist(), tx.ends.long()[ln.ends.long()[e] - 1].tolist())])
        assert int((tend - tstart).sum()) == len(self.texel_rows)
        n = lambda t: t.detach().cpu().numpy().copy()
        self.scene = O.Scene(dict(
            n_agents=sc.n_agents, model=n(sc.model),
            lights_vals=n(li.vals[light_rows]), lights_widths=n(li.widths[e]),
            lines_vals=n(ln.vals[self.line_rows]), lines_widths=n(ln.widths[e]),
            textures_vals=n(tx.vals[self.texel_rows]), textures_widths=n(tx.widths[self.line_rows]),
            baked_vals=n(sc.baked.vals[self.texel_rows])))
        self.cfg = O.config(core.agent_radius, core.res, core.fov, core.fps)
        self.pull_agents(core)

    def pull_agents(self, core):
        self.agents = {k: v[self.envs] for k, v in agents_dict(core.agents).items()}

    def bake(self):
        return O.bake(self.scene, self.cfg).copy()

    def physics(self):
        progress, self.agents = O.physics(self.scene, self.agents, self.cfg)
        return progress, self.agents

    def render(self):
        return O.render(self.scene, self.agents, self.cfg)


class _Rows:
    """A Core-like view of a few envs of a step's results, for the assert_* helpers above."""

    def __init__(self, core, envs):
        class A:
            pass
        self.agents = A()
        for k in ('angles', 'positions', 'angvelocity', 'velocity'):
            setattr(self.agents, k, getattr(core.agents, k)[envs])


def assert_subset_matches(core, sub, p, r):
    """Physics and render results of the full batch, at the sampled envs, against the oracle."""
    e = torch.as_tensor(sub.envs, device=core.device)
    prog_ref, agents_ref = sub.physics()

    class P:
        progress = p.progress[e]
    assert_physics_matches(_Rows(core, e), P, prog_ref, agents_ref)

    class R:
        pass
    for k in ('indices', 'locations', 'dots', 'distances', 'screen'):
        setattr(R, k, getattr(r, k)[e])
    assert_render_matches(None, R, sub.render())


def assert_subset_bits(core, sub, p, r):
    """assert_subset_matches, to the bit."""
    e = torch.as_tensor(sub.envs, device=core.device)
    prog_ref, agents_ref = sub.physics()

    class P:
        progress = p.progress[e]
    assert_physics_bits(_Rows(core, e), P, prog_ref, agents_ref)

    class R:
        pass
    for k in ('indices', 'locations', 'dots', 'distances', 'screen'):
        setattr(R, k, getattr(r, k)[e])
    assert_render_bits(None, R, sub.render())


def obstructed_pairs(I, U, a, v):
    """obstructed() of kernels.cu:253-257 in float32 numpy, pair by pair: does the wall (a, a + v) stand between the light I and
    the point I + U? Arrays (..., 2) of float32 that broadcast against each other; booleans of the broadcast shape."""
    f = np.float32
    with np.errstate(all='ignore'):
        d = U[..., 0]*v[..., 1] - U[..., 1]*v[..., 0]
        PQ = a - I
        s =(PQ[..., 0]*v[..., 1] - PQ[..., 1]*v[..., 0])/d
        t = (PQ[..., 0]*U[..., 1] - PQ[..., 1]*U[..., 0])/d
        return (np.abs(d) >= f(1e-3)) & (t > 0) & (t < 1) & (s > 0) & (s < f(.999))


def obstructed(I, C, walls):
    """... of n_points points C from one light I against n_walls walls: (n_points, n_walls) booleans."""
    return obstructed_pairs(I, (C - I)[:, None], walls[None, :, 0], (walls[:, 1] - walls[:, 0])[None])


# ---- worlds that the GPU suite and the reference pin (tests/test_reference_pin.py) both run ---------------------------
# Each returns a Core on `device`. On the CPU nothing can bake: the scenery is left unbaked there (baked == 1) and its
# user bakes it with whatever it is checking.

def _bakes(device):
    return torch.device(device).type != 'cpu'


def plan_world(n_envs, n_agents, res, fov, seed=0, large=False, toy=None, device='cuda'):
    """Seeded floorplans (or n_envs copies of a toy), agents spawned on free cells: (core, geometries)."""
    from megastep_amd import core, cubicasa, scene, toys
    np.random.seed(seed)
    if toy is not None:
        geometries = n_envs*[getattr(toys, toy)()]
    else:
        geometries = cubicasa.sample(n_envs, n_unique=64, seed=seed + 1, large=large)
    scenery = scene.scenery(geometries, n_agents, device=device, random=np.random.RandomState(seed), bake=_bakes(device))
    c = core.Core(scenery, res=res, fov=fov, fps=10)
    spawn(c, geometries, seed=seed)
    return c, geometries


def oblique_world(n_envs, n_agents, res, fov, large, device='cuda'):
    """Floorplans turned by seeded angles, with diagonal partitions: (core, geometries)."""
    from megastep_amd import core, cubicasa, scene
    np.random.seed(11)
    geometries = cubicasa.sample(n_envs, n_unique=16, seed=12, large=large, oblique=True)
    scenery = scene.scenery(geometries, n_agents, device=device, random=np.random.RandomState(11), bake=_bakes(device))
    c = core.Core(scenery, res=res, fov=fov, fps=10)
    spawn(c, geometries, seed=11)
    return c, geometries


def custom_world(walls_per_env, n_agents, res, fov, positions, angles, lights=None, device='cuda'):
    """A Core over hand-made wall sets (one (W, 2, 2) array per env), agents placed explicitly."""
    from megastep_amd import core, scene, arrdict
    geoms = [arrdict.arrdict(walls=np.asarray(w, float), lights=np.array([[2., 2.]]) if lights is None else lights,
                             masks=np.ones((4, 4), np.int16), res=.2) for w in walls_per_env]
    np.random.seed(0)
    scenery = scene.scenery(geoms, n_agents, device=device, random=np.random.RandomState(0), bake=_bakes(device))
    c = core.Core(scenery, res=res, fov=fov, fps=10)
    c.agents.positions[:] = torch.as_tensor(np.asarray(positions, np.float32), device=c.device)
    c.agents.angles[:] = torch.as_tensor(np.asarray(angles, np.float32), device=c.device)
    return c


def hysteresis_band_world(device='cuda'):
    """Stacks of (nearly) coincident walls in shuffled order: the 1e-4 z-fight rule (kernels.cu:369) makes the
    winner depend on line order. Offsets straddle the band: 0, 2e-5, 5e-5, 9e-5, 1e-4, 1.1e-4, 2e-4, 1e-3."""
    rng = np.random.RandomState(3)
    offsets = np.array([0., 0., 2e-5, 5e-5, 9e-5, 1e-4, 1.1e-4, 2e-4, 3e-4, 1e-3])
    envs, pos, ang = [], [], []
    for e in range(48):
        k = rng.randint(2, 9)
        xs = 4. + rng.choice(offsets, k)*rng.choice([1, 1, -1], k) + rng.choice([0., 0., .5], k)
        walls = [[[x, 1. + rng.uniform(-.2, .2)], [x, 3. + rng.uniform(-.2, .2)]] for x in xs]
        if e % 3 == 0:      # an enclosing corner so that rays through shared vertices occur too
            walls += [[[4., 3.], [2., 3.]], [[2., 3.], [2., 1.]], [[2., 1.], [4., 1.]]]
        if e % 4 == 0:      # duplicates and reversed duplicates
            walls += [walls[0], [walls[1][1], walls[1][0]]]
        order = rng.permutation(len(walls))
        envs.append(np.array(walls)[order])
        pos.append([[rng.uniform(2.2, 3.9), rng.uniform(1.5, 2.5)]])
        ang.append([rng.uniform(-30, 30)])
    # pad every env to its own length is fine: Ragged
    return custom_world(envs, 1, 64, 100, pos, ang, device=device)


def wedged_agent_world(device='cuda'):
    """An agent 0.11 m from a wall that is doubled by a flush pillar face: most of its rays tie."""
    wall = [[[2., 1.], [2., 2.2]], [[2., 2.2], [2., 4.]]]
    pillar = [[[2., 2.], [2.3, 2.]], [[2.3, 2.], [2.3, 2.4]], [[2.3, 2.4], [2., 2.4]], [[2., 2.4], [2., 2.]]]
    triple = pillar + [[[2., 2.05], [2., 2.35]]]
    box = [[[1., 1.], [4., 1.]], [[4., 1.], [4., 4.]], [[4., 4.], [1., 4.]], [[1., 4.], [1., 1.]]]
    envs = [np.array(wall + pillar + box), np.array(pillar + wall + box), np.array(wall + triple + box),
            np.array(triple[::-1] + wall + box)]
    return custom_world(envs, 1, 64, 130, [[[2.11, 2.2]]]*4, [[180.], [170.], [-175.], [180.]], device=device)


def coincident_stacks_world(device='cuda'):
    """Views full of walls within the 1e-4 band of each other (kernels.cu:369), in shuffled line order, 512 rays over 40
    degrees; one env with 150 such walls, one with 70."""
    rng = np.random.RandomState(5)
    offsets = np.array([0., 0., 2e-5, 5e-5, 9e-5, 1e-4, 1.1e-4, 2e-4, 3e-4, 1e-3])
    envs, pos, ang = [], [], []
    for e in range(24):
        k = 150 if e == 0 else 70 if e == 1 else rng.randint(2, 9)
        xs = 4. + rng.choice(offsets, k)*rng.choice([1, 1, -1], k) + rng.choice([0., 0., .5], k)
        walls = [[[x, 1. + rng.uniform(-.2, .2)], [x, 3. + rng.uniform(-.2, .2)]] for x in xs]
        if e % 3 == 0:
            walls += [[[4., 3.], [2., 3.]], [[2., 3.], [2., 1.]], [[2., 1.], [4., 1.]]]
        if e % 4 == 0:
            walls += [walls[0], [walls[1][1], walls[1][0]]]
        envs.append(np.array(walls)[rng.permutation(len(walls))])
        pos.append([[rng.uniform(2.2, 3.9), rng.uniform(1.5, 2.5)]])
        ang.append([rng.uniform(-20, 20)])
    return custom_world(envs, 1, 512, 40, pos, ang, device=device)


def crawling_agents_world(device='cuda'):
    """project() divides by (|v| + 1e-6) (kernels.cu:91-107): for |v| below ~1e-6 per step its distances shrink until
    endpoints metres away pass `d < r` and the reference stops the agent. Env 0 is ADVICE r1's case."""
    from megastep_amd import core, scene, toys
    sc = scene.scenery(64*[toys.box()], 1, device=device, bake=_bakes(device))
    c = core.Core(sc, res=8, fps=10)
    rng = np.random.RandomState(0)
    pos = rng.uniform(1.5, 5.5, (64, 1, 2)).astype(np.float32)
    pos[0] = [5., 5.]
    speed = 10.**rng.uniform(-9, -2, (64, 1, 1))
    ang = rng.uniform(0, 2*np.pi, (64, 1, 1))
    vel = (10*speed*np.concatenate([np.cos(ang), np.sin(ang)], -1)).astype(np.float32)      # v/fps = speed
    vel[0] = [1e-6, 0.]
    c.agents.positions[:] = torch.as_tensor(pos, device=device)
    c.agents.velocity[:] = torch.as_tensor(vel, device=device)
    return c


def agents_meeting_agents_world(n_agents, device='cuda'):
    """Pairs at every distance around the threshold, relative velocities from a brisk walk down to 1e-9 a step (project()'s
    `+ 1e-6` stretches the reach of a pair that moves almost in step, kernels.cu:91-107), pairs in perfect step, pairs with
    a NaN or an infinity in their state."""
    from megastep_amd import core, scene, toys
    E = 512
    sc = scene.scenery(E*[toys.box()], n_agents, device=device, bake=_bakes(device))
    c = core.Core(sc, res=8, fps=10)
    rng = np.random.RandomState(3)
    base = rng.uniform(2.5, 3.5, (E, 1, 2))
    gap = 10.**rng.uniform(-2.5, .7, (E, n_agents, 1))                    # 3 mm .. 5 m from the first agent
    ang = rng.uniform(0, 2*np.pi, (E, n_agents, 1))
    pos = (base + gap*np.concatenate([np.cos(ang), np.sin(ang)], -1)).astype(np.float32)
    pos[:, 0] = base[:, 0]
    common = rng.uniform(-3, 3, (E, 1, 2))*(rng.rand(E, 1, 1) < .8)       # a fifth of the envs: no common drift
    rel = 10.**rng.uniform(-8, .5, (E, n_agents, 1))                      # 10 x the relative velocity per step
    rang = rng.uniform(0, 2*np.pi, (E, n_agents, 1))
    vel = (common + rel*np.concatenate([np.cos(rang), np.sin(rang)], -1)).astype(np.float32)
    vel[::7, 1] = vel[::7, 0]                                             # in perfect step
    vel[5::31, 1, 0] = np.nan
    vel[11::37, 0, 1] = np.inf
    pos[17::41, 1, 0] = np.nan
    c.agents.positions[:] = torch.as_tensor(pos, device=device)
    c.agents.velocity[:] = torch.as_tensor(vel, device=device)
    return c


def non_finite_walls_world(n_agents, device='cuda'):
    """A NaN or an infinity among a wall's coordinates, in 47 of 48 boxes (env 0 stays clean); agents at random, moving."""
    from megastep_amd import core, cuda, scene, toys
    sc = scene.scenery([toys.box() for _ in range(48)], n_agents, device=device, bake=_bakes(device))     # (48 floorplans of their own: their walls are about to differ)
    c = core.Core(sc, res=8, fps=10)
    rng = np.random.RandomState(1)
    AF = n_agents*sc.model.shape[0]
    lines = sc.lines.vals.reshape(48, -1, 4)                  # (env, line, xyxy): the box's four walls follow the agents' lines
    assert lines.shape[1] == AF + 4
    bad = [np.nan, np.inf, -np.inf]
    for e in range(1, 48):                                    # env 0 stays clean
        wall, coord = AF + rng.randint(4), rng.randint(4)
        lines[e, wall, coord] = bad[e % 3]
        if e % 5 == 0:
            lines[e, wall, (coord + 2) % 4] = bad[(e + 1) % 3]
    if _bakes(device):
        cuda.bake(sc)                                         # walls were moved: the wall grid (and the baked light) start over
    c.agents.positions[:] = torch.as_tensor(rng.uniform(1.2, 4.8, (48, n_agents, 2)).astype(np.float32), device=device)
    random_velocities(c, rng, speed=6.)
    return c


def many_lights_geometries(rng):
    """A box with six pillars under 70, 9, 150 and 64 lights: more than the light grid holds per env, and fewer."""
    from megastep_amd import arrdict, toys
    box = toys.box()
    pillars = np.concatenate([np.array([[[x, y], [x + .2, y]], [[x + .2, y], [x + .2, y + .2]], [[x + .2, y + .2], [x, y + .2]],
                                        [[x, y + .2], [x, y]]]) for x, y in rng.uniform(1.5, 5.3, (6, 2))])
    walls = np.concatenate([box.walls, pillars])
    return [arrdict.arrdict(walls=walls, lights=rng.uniform(1.2, 5.8, (k, 2)), masks=box.masks, res=.2) for k in (70, 9, 150, 64)]


def many_lights_world(geoms, rng, device='cuda'):
    """Three agents in a triangle, looking at each other, in each of many_lights_geometries()."""
    from megastep_amd import core, scene
    np.random.seed(0)
    sc = scene.scenery(geoms, 3, device=device, random=np.random.RandomState(0), bake=_bakes(device))
    c = core.Core(sc, res=64, fov=130)
    spots = np.array([[3., 3.], [4., 3.1], [3.5, 4.]], np.float32) + rng.uniform(-.2, .2, (4, 3, 2)).astype(np.float32)
    c.agents.positions[:] = torch.as_tensor(spots, device=c.device)     # a triangle of agents looking at each other
    c.agents.angles[:] = torch.as_tensor(np.array([30., 150., -90.], np.float32) + rng.uniform(-10, 10, (4, 3)).astype(np.float32), device=c.device)
    return c


def crowd_world(rng, device='cuda'):
    """66 agents in one 8 m box: past 64 agents per env."""
    from megastep_amd import core, scene, toys
    crowd = scene.scenery([toys.box(8)], 66, device=device, random=np.random.RandomState(0), bake=_bakes(device))
    c = core.Core(crowd, res=16, fov=130)
    c.agents.positions[:] = torch.as_tensor(rng.uniform(1.5, 8.5, (1, 66, 2)).astype(np.float32), device=c.device)
    c.agents.angles[:] = torch.as_tensor(rng.uniform(-180, 180, (1, 66)).astype(np.float32), device=c.device)
    return c


def ragged_edge_world(rng, device='cuda', many_walls=True):
    """An env without lights, an env with a single wall, (with `many_walls`) an env with more walls than one LDS staging pass
    of the bake kernels holds (2048), side by side with a normal one."""
    from megastep_amd import toys, arrdict
    box = toys.box()
    many = np.concatenate([box.walls] + [np.array([[[x, y], [x + .03, y + .02]]]) for x in np.linspace(1.5, 5.5, 50) for y in np.linspace(1.5, 5.5, 44)])
    assert len(many) > 2048
    geoms = [
        arrdict.arrdict(walls=box.walls, lights=np.zeros((0, 2)), masks=box.masks, res=.2),          # dark room
        arrdict.arrdict(walls=box.walls[:1], lights=box.lights, masks=box.masks, res=.2),            # one wall
        arrdict.arrdict(walls=many, lights=np.array([[3.5, 3.5], [2., 5.]]), masks=box.masks, res=.2),
        box]
    if not many_walls:
        geoms = geoms[:2] + geoms[3:]
    from megastep_amd import core, scene
    np.random.seed(0)
    scenery = scene.scenery(geoms, 2, device=device, random=np.random.RandomState(0), bake=_bakes(device))
    c = core.Core(scenery, res=64, fov=130)
    c.agents.positions[:] = torch.as_tensor(rng.uniform(2, 5, (len(geoms), 2, 2)).astype(np.float32), device=c.device)
    c.agents.angles[:] = torch.as_tensor(rng.uniform(-180, 180, (len(geoms), 2)).astype(np.float32), device=c.device)
    return c


# ---- cases: a world as plain arrays, for the reference pin and the recorded goldens ------------------------------------
# A case is dict(scene=<the oracle's scene dict, unbaked>, config=(agent_radius, res, fov, fps), agents=<agents dict>,
# moves=[(velocity, angvelocity), ...]): one (N, A, 2) / (N, A) pair per step, set before that step's physics.

def case_of(core, moves):
    """A Core (on any device) as a case."""
    scene = scene_dict(core.scenery)
    scene['baked_vals'] = None
    return dict(scene=scene, config=(core.agent_radius, core.res, core.fov, core.fps), agents=agents_dict(core.agents),
                moves=[(np.asarray(v, np.float32), np.asarray(w, np.float32)) for v, w in moves])


def random_moves(shape, rng, speeds, spin=180.):
    """What random_velocities() draws, one step per entry of `speeds`."""
    return [(rng.uniform(-s, s, shape + (2,)).astype(np.float32), rng.uniform(-spin, spin, shape).astype(np.float32)) for s in speeds]


def still(case):
    return [(case['agents']['velocity'], case['agents']['angvelocity'])]


def hand_case(envs, positions, angles, res, fov, n_agents=1, seed=0, moves=None, fps=10.):
    """A case assembled by hand: `envs` is a list of dict(walls (W, 2, 2), lights (I, 3) = x, y, intensity, widths (W,) texels
    per wall or None for scene.resolutions'). Texel colours are seeded uniform noise, so that the filter's two taps differ."""
    from megastep_amd import scene
    rng = np.random.RandomState(seed)
    model = scene.agent_model().astype(np.float32)
    agentlines = np.tile(model, (n_agents, 1, 1))
    lights, lines, widths = [], [], []
    for env in envs:
        walls = np.asarray(env['walls'], np.float32).reshape(-1, 2, 2)
        w = scene.resolutions(walls.astype(float)) if env.get('widths') is None else np.asarray(env['widths'])
        assert len(w) == len(walls) and (w >= 1).all()
        lights.append(np.asarray(env['lights'], np.float32).reshape(-1, 3))
        lines.append(np.concatenate([agentlines, walls]))
        widths.append(np.concatenate([scene.resolutions(agentlines.astype(float)), w]))
    textures_widths = np.concatenate(widths).astype(np.int32)
    sc = dict(n_agents=n_agents, model=model, baked_vals=None,
              lights_vals=np.concatenate(lights).astype(np.float32), lights_widths=np.array([len(x) for x in lights], np.int32),
              lines_vals=np.concatenate(lines).astype(np.float32), lines_widths=np.array([len(x) for x in lines], np.int32),
              textures_vals=rng.uniform(.05, 1., (int(textures_widths.sum()), 3)).astype(np.float32), textures_widths=textures_widths)
    N = len(envs)
    agents = dict(angles=np.asarray(angles, np.float32).reshape(N, n_agents), positions=np.asarray(positions, np.float32).reshape(N, n_agents, 2),
                  angvelocity=np.zeros((N, n_agents), np.float32), velocity=np.zeros((N, n_agents, 2), np.float32))
    from megastep_amd import core
    case = dict(scene=sc, config=(core.AGENT_RADIUS, res, float(fov), float(fps)), agents=agents)
    case['moves'] = still(case) if moves is None else moves
    return case


def _turned(points, quarter_turns, about):
    """Points turned by a multiple of 90 degrees about a point with integer coordinates: exact for integer-valued inputs."""
    p = np.asarray(points, float) - about
    for _ in range(quarter_turns % 4):
        p = np.stack([-p[..., 1], p[..., 0]], -1)
    return p + about


def endpoint_case():
    """Rays that pass exactly through wall endpoints and shared corners (kernels.cu:367, `0 <= q.t <= 1`), and hits at the
    texture filter's clamps (kernels.cu:394-405: loc 0 and 1, x*(w+1) on an integer), on walls of 1, 2, 3 and 7 texels.

    One agent on a grid point, heading along an axis, ONE ray (res 1: ray_y = 0, the ray is the heading itself, and
    sin/cos of a quarter turn are exact), walls on grid points: q.t is exactly 0, 1/4, 1/2, 3/4 or 1. Behind every wall under
    test a backstop: a rule that lets the ray through the endpoint shows as another index. The agent then walks along its ray,
    which puts `mid.t` of the collision test (kernels.cu:144) on the same exact values."""
    backstop = [[[6, -4], [6, 4]]]
    variants = [
        [[[4, 0], [4, 2]]],                                   # q.t == 0
        [[[4, -2], [4, 0]]],                                  # q.t == 1
        [[[4, 0], [4, 2]], [[4, -2], [4, 0]]],                # a shared endpoint: both hit, the first stays (z-fight rule)
        [[[4, -2], [4, 0]], [[4, 0], [4, 2]]],
        [[[4, 0], [5, 1]], [[4, 0], [5, -1]]],                # a corner pointing at the agent
        [[[5, 1], [4, 0]], [[5, -1], [4, 0]]],                # ... with q.t == 1
        [[[4, -1], [4, 3]]],                                  # q.t == 1/4
        [[[4, -2], [4, 2]]],                                  # q.t == 1/2
        [[[4, -3], [4, 1]]],                                  # q.t == 3/4
        [[[4, 0], [4, 8]]],                                   # q.t == 0 on a long wall
        [[[4, -1], [4, 7]]],                                  # q.t == 1/8
        [[[4, -7], [4, 1]]],                                  # q.t == 7/8
    ]
    envs, pos, ang = [], [], []
    about = np.array([8., 8.])
    for v, walls in enumerate(variants):
        for turns in range(4):
            for w in (1, 2, 3, 7):
                if w != 3 and turns != v % 4:     # every width on one heading per variant, 3 texels on all four
                    continue
                ws = np.array(walls + backstop, float) + about
                envs.append(dict(walls=_turned(ws, turns, about), lights=[[8.5 + turns, 8.25, 1.]], widths=[w]*len(walls) + [5]))
                pos.append(about)
                ang.append([0., 90., 180., -90.][turns])
    N = len(envs)
    head = np.stack([_turned([1., 0.], int(round(a/90)) % 4, 0.) for a in ang]).astype(np.float32).reshape(N, 1, 2)
    moves = [(np.zeros((N, 1, 2), np.float32), np.zeros((N, 1), np.float32)), (45*head, np.zeros((N, 1), np.float32))]
    return hand_case(envs, pos, ang, res=1, fov=90, moves=moves, seed=1)


def corner_fan_case():
    """As endpoint_case, seen through a fan: 3 rays at fov 90 (the outer two within an ulp of the diagonals) and 5 at fov 130,
    from grid points inside a lattice of unit pillars whose corners lie on the axes and diagonals through the agent."""
    pillars = []
    for x in range(0, 9, 2):
        for y in range(0, 9, 2):
            c = [[x, y], [x + 1, y], [x + 1, y + 1], [x, y + 1]]
            pillars += [[c[i], c[(i + 1) % 4]] for i in range(4)]
    room = [[[-2, -2], [11, -2]], [[11, -2], [11, 11]], [[11, 11], [-2, 11]], [[-2, 11], [-2, -2]]]
    walls = np.array(pillars + room, float)
    envs, pos, ang = [], [], []
    for k, (p, a) in enumerate([([5, 1.5], 90), ([1.5, 5], 0), ([5, 5.5], 45), ([3.5, 3.5], -135), ([7, 1.5], 180), ([1.5, 3], -90),
                                ([5.5, 5.5], 135), ([3.5, 7], -45)]):
        envs.append(dict(walls=walls, lights=[[5.5, 5.5, 1.5], [1.5, 1.5, .7]], widths=None))
        pos.append(p); ang.append(a)
    return hand_case(envs, pos, ang, res=3, fov=90, seed=2), hand_case(envs, pos, ang, res=5, fov=130, seed=2)


def near_parallel_case():
    """Rays nearly parallel to a wall, on both sides of intersect()'s `distant` threshold (kernels.cu:77, |U x V| < 1e-3):
    one ray along +x (res 1), a 2 m wall across it that rises by exactly the cross product, from a tenth of the threshold to
    twice it, the threshold itself and its two neighbours in binary32 included; both slopes; a backstop behind."""
    f = np.float32
    t = f(1e-3)
    crosses = [f(1e-4), f(2e-4), f(5e-4), f(9.9e-4), np.nextafter(t, f(0)), t, np.nextafter(t, f(1)), f(1.01e-3), f(1.5e-3), f(2e-3)]
    envs, pos, ang = [], [], []
    for c in crosses:
        for sign in (1, -1):
            h = float(c)/2*sign                  # the wall runs from (3, -h) to (5, +h): V = (2, 2h), U = (1, 0), U x V = 2h exactly
            envs.append(dict(walls=[[[3., -h], [5., h]], [[7., -3.], [7., 3.]]], lights=[[1., 1., 1.]], widths=[4, 6]))
            pos.append([0., 0.]); ang.append(0.)
    N = len(envs)
    moves = [(np.zeros((N, 1, 2), np.float32), np.zeros((N, 1), np.float32)), (np.tile(f([38., 0.]), (N, 1, 1)), np.zeros((N, 1), np.float32))]
    return hand_case(envs, pos, ang, res=1, fov=90, moves=moves, seed=3)


def grazing_light_case():
    """Texels whose light path grazes a wall's end just in front of them: light_intensity() counts a wall as in the way up to
    s < .999 of the path (kernels.cu:255-257). A lit wall of 4 texels, one light, and a 2 cm fence across the path to texel
    1's centre at s = .9975 ... .99995 of it (and the binary32 neighbours of .999 as nearly as the coordinates allow); the agent
    looks at the lit wall with 16 rays, so the baked value is seen through the filter too."""
    envs, pos, ang = [], [], []
    I, a, b = np.array([2., 4.]), np.array([1., 1.]), np.array([5., 1.])
    C = a + (b - a)*(1.5/4)
    d = (C - I)/np.linalg.norm(C - I)
    n = np.array([-d[1], d[0]])
    for s in (.9975, .998, .9985, .9989, .99895, .99899, .999, .99901, .99905, .9991, .9995, .9999, .99995):
        for tilt in (0., .3):
            m = I + s*(C - I)
            across = n + tilt*d
            envs.append(dict(walls=[[a, b], [m - .01*across, m + .01*across], [[1., 5.], [1., 1.]]], lights=[[2., 4., 1.2]], widths=[4, 1, 8]))
            pos.append([3., 3.]); ang.append(-90.)
    return hand_case(envs, pos, ang, res=16, fov=100, seed=4)


def narrow_textures_case():
    """Walls of 1 and 2 texels (and 3) all round an agent that turns on the spot: the filter (kernels.cu:394-405) with w - 1 = 0
    and 1, across a 64-ray fan."""
    envs, pos, ang = [], [], []
    box = [[[1., 1.], [4., 1.]], [[4., 1.], [4., 4.]], [[4., 4.], [1., 4.]], [[1., 4.], [1., 1.]], [[2., 3.], [3., 3.5]]]
    for k, widths in enumerate([[1]*5, [2]*5, [1, 2, 3, 1, 2], [2, 1, 1, 3, 1]]):
        envs.append(dict(walls=box, lights=[[2.5, 2.5, 1.], [3.5, 1.5, .6]], widths=widths))
        pos.append([2.2 + .1*k, 2.1]); ang.append(40.*k - 70)
    N = len(envs)
    moves = [(np.zeros((N, 1, 2), np.float32), np.full((N, 1), w, np.float32)) for w in (0., 900., -1700.)]
    return hand_case(envs, pos, ang, res=64, fov=130, moves=moves, seed=5)


def take_envs(case, envs):
    """The case made of a few envs of a case."""
    sc = case['scene']
    envs = list(envs)
    line_ends, light_ends = np.cumsum(sc['lines_widths']), np.cumsum(sc['lights_widths'])
    texel_ends = np.concatenate([[0], np.cumsum(sc['textures_widths'])])
    lines = [np.arange(line_ends[e] - sc['lines_widths'][e], line_ends[e]) for e in envs]
    lights = np.concatenate([np.arange(light_ends[e] - sc['lights_widths'][e], light_ends[e]) for e in envs]).astype(int)
    texels = np.concatenate([np.arange(texel_ends[l[0]], texel_ends[l[-1] + 1]) for l in lines]).astype(int)
    lines = np.concatenate(lines).astype(int)
    scene = dict(sc, lights_vals=sc['lights_vals'][lights], lights_widths=sc['lights_widths'][envs],
                 lines_vals=sc['lines_vals'][lines], lines_widths=sc['lines_widths'][envs],
                 textures_vals=sc['textures_vals'][texels], textures_widths=sc['textures_widths'][lines], baked_vals=None)
    return dict(scene=scene, config=case['config'], agents={k: v[envs] for k, v in case['agents'].items()},
                moves=[(v[envs], w[envs]) for v, w in case['moves']])


def crop_case(case, radius):
    """Keeps, in every env, the agents' lines and the walls that come within `radius` of the env's first agent (and every
    light): a floorplan cut down to the room around the agents, for cases that are stored."""
    sc = case['scene']
    AF = int(sc['n_agents'])*len(sc['model'])
    line_ends = np.cumsum(sc['lines_widths'])
    texel_ends = np.concatenate([[0], np.cumsum(sc['textures_widths'])])
    keep_lines, widths = [], []
    for e, (end, w) in enumerate(zip(line_ends, sc['lines_widths'])):
        rows = np.arange(end - w, end)
        seg = sc['lines_vals'][rows].astype(float)
        p = case['agents']['positions'][e, 0].astype(float)
        a, d = seg[:, 0], seg[:, 1] - seg[:, 0]
        t = np.clip(((p - a)*d).sum(1)/np.maximum((d*d).sum(1), 1e-12), 0, 1)
        near = np.linalg.norm(a + t[:, None]*d - p, axis=1) <= radius
        near[:AF] = True
        keep_lines.append(rows[near]); widths.append(int(near.sum()))
    lines = np.concatenate(keep_lines)
    texels = np.concatenate([np.arange(texel_ends[l], texel_ends[l + 1]) for l in lines]).astype(int)
    scene = dict(sc, lines_vals=sc['lines_vals'][lines], lines_widths=np.array(widths, np.int32),
                 textures_vals=sc['textures_vals'][texels], textures_widths=sc['textures_widths'][lines], baked_vals=None)
    return dict(case, scene=scene)


def pack_cases(records):
    """{case: {field: array}} as a few flat arrays for one npz: per field the cases' arrays raveled end to end, and their
    shapes (padded with -1); 'names' lists the cases. A zip member per array of every case would cost more than the data."""
    names = list(records)
    fields = list(records[names[0]])
    assert all(list(r) == fields for r in records.values())
    out = dict(names=np.array(names))
    for k in fields:
        arrs = [records[n][k] for n in names]
        assert len({a.dtype for a in arrs}) == 1 and all(a.ndim <= 4 for a in arrs), k
        out[k] = np.concatenate([a.ravel() for a in arrs])
        out[k + '.shape'] = np.array([list(a.shape) + [-1]*(4 - a.ndim) for a in arrs], np.int32)
    return out


def load_cases(path):
    """What pack_cases packed, from an npz: {case: {field: array}}."""
    z = np.load(path)
    names = [str(n) for n in z['names']]
    out = {n: {} for n in names}
    for k in z.files:
        if k == 'names' or k.endswith('.shape'):
            continue
        flat, at = z[k], 0
        for n, shape in zip(names, z[k + '.shape']):
            shape = tuple(int(d) for d in shape if d >= 0)
            size = int(np.prod(shape))
            out[n][k] = flat[at:at + size].reshape(shape).copy()
            at += size
        assert at == len(flat), k
    return out
