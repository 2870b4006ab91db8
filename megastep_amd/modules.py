"""Chunks of functionality that turn up in most environments (reference: megastep/modules.py:10-381).

These are the direct callers of the hot path: the movement modules end in :func:`cuda.physics`, :func:`render` wraps
:func:`cuda.render`. Everything here is thin torch glue over the tensors the kernels own."""
import numpy as np
import torch
from . import spaces, geometry, cuda, arrdict


def _sincos_deg(angles):
    a = np.pi/180*angles
    return torch.sin(a), torch.cos(a)


def to_local_frame(angles, p):
    """Global-frame vectors -> the agents' local frames."""
    s, c = _sincos_deg(angles)
    x, y = p[..., 0], p[..., 1]
    return torch.stack([c*x + s*y, -s*x + c*y], -1)


def to_global_frame(angles, p):
    """Agent-local vectors -> the global frame."""
    s, c = _sincos_deg(angles)
    x, y = p[..., 0], p[..., 1]
    return torch.stack([c*x - s*y, s*x + c*y], -1)


def _actionset(core, linear, angular):
    # noop, forward/backward, strafe left/right, turn left/right
    velocity = torch.tensor([[0., 0.], [0., 1.], [0., -1.], [1., 0.], [-1., 0.], [0., 0.], [0., 0.]])
    angvelocity = torch.tensor([0., 0., 0., 0., 0., +1., -1.])
    return arrdict.arrdict(velocity=linear/core.fps*velocity, angvelocity=angular/core.fps*angvelocity).to(core.device)


def _table(actionset):
    """The action table as cuda.physics' ``movement`` wants it: one (dx, dy, dangle) row per action."""
    return torch.cat([actionset.velocity, actionset.angvelocity[:, None]], 1).contiguous()


def _move(core, actionset, actions, keep, respawn=None, imu=None, table=None, slide=None):
    """The velocity update of both movement modules, then physics. On the GPU it is part of the physics launch
    (cuda.physics' ``movement``) - as are, when the env hands them over, the respawn of the agents it wants respawned
    (``respawn``: :meth:`RandomSpawns.draw`) and the IMU observation of the new state (``imu``: the :class:`IMU`
    module, which then returns it from its next call). The tensor ops below are the same arithmetic, and what the
    reference runs. ``slide``: cuda.physics' sliding contacts - a second phase of the launch, which the tensor ops do not have."""
    agents = core.agents
    if agents.angles.is_cuda:
        table = _table(actionset) if table is None else table
        reading = None if imu is None else (torch.empty(agents.angles.shape + (3,), device=core.device), imu.ang_scale, imu.speed_scale)
        result = cuda.physics(core.scenery, agents, movement=(actions.long().contiguous(), table, keep), respawn=respawn, imu=reading,
                              slide=slide)
        if imu is not None:
            imu._pending = (reading[0], agents._epoch)          # valid until somebody else touches the agents
        return result
    if slide:
        raise RuntimeError('sliding contacts are part of the physics launch: they need the agents on a GPU')
    if respawn is not None and not respawn['after']:
        _respawn(agents, respawn)
    delta = actionset[actions.long()]
    if keep == 0:
        agents.angvelocity[:] = delta.angvelocity
        agents.velocity[:] = to_global_frame(agents.angles, delta.velocity)
    else:
        agents.angvelocity[:] = keep*agents.angvelocity + delta.angvelocity
        agents.velocity[:] = keep*agents.velocity + to_global_frame(agents.angles, delta.velocity)
    result = cuda.physics(core.scenery, agents)
    if respawn is not None and respawn['after']:
        _respawn(agents, respawn)
    return result


def _respawn(agents, request):
    """Applies a :meth:`RandomSpawns.draw` request with tensor ops (what the kernel does inside the physics launch)."""
    reset, choices = request['mask'], request['choices']
    angles = request['angles'].gather(2, choices[..., None]).squeeze(2)
    positions = request['positions'].gather(2, choices[..., None, None].expand(-1, -1, 1, 2)).squeeze(2)
    agents.angles[:] = torch.where(reset, angles, agents.angles)
    agents.positions[:] = torch.where(reset[..., None], positions, agents.positions)
    agents.velocity[:] = torch.where(reset[..., None], torch.zeros_like(agents.velocity), agents.velocity)
    agents.angvelocity[:] = torch.where(reset, torch.zeros_like(agents.angvelocity), agents.angvelocity)
    agents._epoch += 1                  # (a reading an IMU module holds of the state before this is stale now)


class SimpleMovement:

    def __init__(self, core, speed=10, ang_speed=180, n_agents=None, slide=None):
        """Movement without momentum: seven actions - nothing, forward/backward, strafe left/right, turn left/right
        (reference: modules.py:24-66). ``slide``: cuda.physics' sliding contacts (True, or dict(bounce=.05)) for every step."""
        self.core = core
        self.slide = slide
        self._actionset = _actionset(core, speed, ang_speed)
        self._table = _table(self._actionset)
        self.keep = 0.                           # (of the old velocity: none - see cuda.physics' ``movement``)
        self.space = spaces.MultiDiscrete(n_agents or core.n_agents, 7)

    def __call__(self, decision, respawn=None, imu=None):
        """Sets the agents' velocities from ``decision.actions`` ((n_env, n_agent) ints in 0..6), then steps physics.
        ``respawn`` / ``imu``: see :func:`_move`."""
        return _move(self.core, self._actionset, decision.actions, 0., respawn, imu, self._table, self.slide)

    def rollouts(self, actions, **kw):
        """:func:`cuda.rollouts` of ``actions`` ((n_env, n_agent, K, H) or (K, H) int64) under this module's table and ``keep``:
        where each plan would take every agent as it stands, without moving anybody - sliding, where the module's steps slide.
        ``kw``: ``others``, ``trail``, ``mask``, ``out``."""
        if self.slide:
            kw.setdefault('slide', self.slide)
        return cuda.rollouts(self.core.scenery, self.core.agents, actions, self._table, keep=self.keep, **kw)

    def scenarios(self, actions, **kw):
        """:func:`cuda.scenarios` of ``actions`` ((n_env, S, n_agent, H) or (S, n_agent, H) int64) under this module's table and
        ``keep``: where every agent of every env would end up if all of them took the plans of scenario ``s`` together, without
        moving anybody. Scenarios take plain steps: a module whose steps slide refuses. ``kw``: ``trail``, ``mask``, ``out``."""
        if self.slide:
            raise RuntimeError('scenarios take plain steps: sliding steps are not part of a scenario')
        return cuda.scenarios(self.core.scenery, self.core.agents, actions, self._table, keep=self.keep, **kw)


class MomentumMovement:

    def __init__(self, core, accel=5, ang_accel=180, decay=.125, n_agents=None, slide=None):
        """Movement with momentum: the seven actions accelerate rather than move, and velocity decays by ``decay``
        each step (reference: modules.py:68-118). ``slide``: as SimpleMovement's."""
        self.core = core
        self.slide = slide
        self._actionset = _actionset(core, accel, ang_accel)
        self._table = _table(self._actionset)
        self.decay = decay
        self.space = spaces.MultiDiscrete(n_agents or core.n_agents, 7)

    #: the share of the old velocity a step keeps (see cuda.physics' ``movement``)
    keep = property(lambda self: 1 - self.decay)

    def __call__(self, decision, respawn=None, imu=None):
        return _move(self.core, self._actionset, decision.actions, self.keep, respawn, imu, self._table, self.slide)

    rollouts = SimpleMovement.rollouts
    scenarios = SimpleMovement.scenarios


def unpack(d):
    """``cuda`` result objects -> arrdicts with the same attributes (reference: modules.py:120-124)."""
    if isinstance(d, torch.Tensor):
        return d
    return arrdict.arrdict({k: unpack(getattr(d, k)) for k in dir(d) if not k.startswith('_')})


def render(core, observers=None, fields=None, centre=False, seen=None):
    """Calls :func:`cuda.render` and reshapes for torch convs: every field gets a height-1 axis, ``screen`` becomes
    (n_env, n_agent, 3, 1, res) (reference: modules.py:126-136).

    Beyond the reference: pass the :class:`RGB` / :class:`Depth` modules that will consume the result as ``observers``
    and their mean-pooled observations come straight out of the render kernel (they pick them up from the result
    instead of running a chain of tensor ops over the full-resolution outputs), and name in ``fields`` the
    full-resolution outputs that are still needed (default: all five) - the others are not even written.
    ``centre=True`` adds ``centre`` (n_env, n_agent, 2): the agent in each of the two central observation pixels, or -1
    (needs observers); ``seen`` is passed on to :func:`cuda.render` (first-sight texel bookkeeping)."""
    pooled = None
    if observers:
        pooled = _pooling(tuple(observers), bool(centre))
    raw = cuda.render(core.scenery, core.agents, fields=fields, pooled=pooled, seen=seen)
    return _frame(raw, pooled)


def move_render(core, mover, decision, observers=None, fields=None, centre=False, seen=None, respawn=None, imu=None):
    """A movement module's step and :func:`render` as ONE call - ``mover(decision, respawn=, imu=)`` then ``render(core, ...)``, same
    arguments, same result - through :func:`cuda.step_render`: for a single-agent world of up to 64 rays (the reference's tutorial
    env, demo/envs/minimal.py) a whole ``env.step()`` is then one launch; any other shape is the two launches it always was."""
    agents = core.agents
    pooled = _pooling(tuple(observers), bool(centre)) if observers else None
    reading = None if imu is None else (torch.empty(agents.angles.shape + (3,), device=core.device), imu.ang_scale, imu.speed_scale)
    _, raw = cuda.step_render(core.scenery, agents, fields=fields, pooled=pooled, seen=seen,
                              movement=(decision.actions.long().contiguous(), mover._table, mover.keep), respawn=respawn, imu=reading,
                              slide=mover.slide)
    if imu is not None:
        imu._pending = (reading[0], agents._epoch)
    return _frame(raw, pooled)


def _frame(raw, pooled):
    """A :class:`cuda.Render` as the arrdict the observation modules read (see :func:`render`)."""
    r = arrdict.arrdict({k: getattr(raw, k).unsqueeze(2) for k in cuda.FIELDS if getattr(raw, k) is not None})
    if 'screen' in r:
        r['screen'] = r.screen.permute(0, 1, 4, 2, 3)
    if pooled is not None:
        r['pooled_subsample'] = pooled['subsample']
        if raw.obs_rgb is not None:
            r['pooled_rgb'] = raw.obs_rgb.unsqueeze(3)                       # (n_env, n_agent, 3, 1, res/subsample)
        if raw.obs_depth is not None:
            r['pooled_depth'] = raw.obs_depth.unsqueeze(2).unsqueeze(3)      # (n_env, n_agent, 1, 1, res/subsample)
            r['pooled_max_depth'] = pooled['max_depth']
        if raw.obs_centre is not None:
            r['centre'] = raw.obs_centre
    return r


_poolings = {}


def _pooling(observers, centre):
    """What :func:`cuda.render` is asked to pool for these observers - worked out once per set of them (an env hands over the
    same modules every step)."""
    key = (tuple((id(o), o.subsample, getattr(o, 'max_depth', None)) for o in observers), centre)
    pooled = _poolings.get(key)
    if pooled is None:
        subs = {o.subsample for o in observers}
        depth = [o for o in observers if isinstance(o, Depth)]
        if len(subs) != 1 or len({o.max_depth for o in depth}) > 1:
            raise ValueError('observers of one render must share their subsample and max_depth')
        pooled = dict(subsample=subs.pop(), max_depth=depth[0].max_depth if depth else 10.,
                      rgb=any(isinstance(o, RGB) for o in observers), depth=bool(depth), centre=centre)
        if len(_poolings) > 256:
            _poolings.clear()
        _poolings[key] = pooled
    return pooled


def downsample(screen, subsample):
    """(..., W) -> (..., W/subsample, subsample); chase it with a mean/min/max over the last axis
    (reference: modules.py:138-145)."""
    return screen.view(*screen.shape[:-1], screen.shape[-1]//subsample, subsample)


class Depth:

    def __init__(self, core, n_agents=None, subsample=1, max_depth=10):
        """Depth observations in [0, 1]: one at the near plane, zero at ``max_depth`` metres
        (reference: modules.py:147-189)."""
        self.core = core
        self.space = spaces.MultiImage(n_agents or core.n_agents, 1, 1, core.res//subsample)
        self.max_depth = max_depth
        self.subsample = subsample

    def __call__(self, r=None):
        r = render(self.core) if r is None else r
        if 'pooled_depth' in r and r.pooled_subsample == self.subsample and r.pooled_max_depth == self.max_depth:
            self._last_obs = r.pooled_depth                  # the render kernel has done it (see render())
            return self._last_obs
        depth = 1 - ((r.distances - self.core.agent_radius)/self.max_depth).clamp(0, 1)
        self._last_obs = downsample(depth, self.subsample).mean(-1).unsqueeze(3)
        return self._last_obs

    def state(self, e=0):
        return self._last_obs[e].clone()


class RGB:

    def __init__(self, core, n_agents=None, subsample=1):
        """Linear-RGB observations, (n_env, n_agent, 3, 1, res/subsample) (reference: modules.py:191-238)."""
        self.core = core
        self.space = spaces.MultiImage(n_agents or core.n_agents, 3, 1, core.res//subsample)
        self.subsample = subsample

    def __call__(self, r=None):
        r = render(self.core) if r is None else r
        if 'pooled_rgb' in r and r.pooled_subsample == self.subsample:
            self._last_obs = r.pooled_rgb                    # the render kernel has done it (see render())
            return self._last_obs
        self._last_obs = downsample(r.screen, self.subsample).mean(-1)
        return self._last_obs

    def state(self, e=0):
        return self._last_obs[e].clone()


class Cameras:

    def __init__(self, core, mounts, res, fov, projection='plane', subsample=1, max_depth=10, n_agents=None):
        """Cameras mounted on every agent (:func:`cuda.mounted`: ``mounts`` (C, 3) - x, y in the agent's frame, turn in degrees)
        of ``res`` rays each, as observations: a call returns ``arrdict(rgb=(n_env, n_agent, 3, C, res/subsample),
        d=(n_env, n_agent, 1, C, res/subsample))`` - the cameras are the image's rows - colour mean-pooled as :class:`RGB`'s and
        depth by :class:`Depth`'s formula, from one :func:`cuda.look` (a raycast launch and a shade launch; no counterpart in
        the reference, whose agents have one camera each). ``projection='ring'`` takes fields of view up to 360 degrees.
        Nothing is allocated after the first call and nothing waits for the host: it sits in a graphed step."""
        if res % subsample:
            raise ValueError('res must be a multiple of subsample')
        self.core = core
        self.subsample, self.max_depth = subsample, max_depth
        self.cameras = cuda.mounted(core.agents, mounts, res, fov, projection)
        self.n_mounts = self.cameras.n_cameras//core.n_agents
        self.space = spaces.MultiImage(n_agents or core.n_agents, 3, self.n_mounts, res//subsample)
        self.depth_space = spaces.MultiImage(n_agents or core.n_agents, 1, self.n_mounts, res//subsample)
        self._look = None

    def __call__(self):
        c = self.core
        self.cameras.update()
        self._look = cuda.look(c.scenery, self.cameras, agents=c.agents, fields=('screen', 'distances'), out=self._look)
        shape = (c.n_envs, c.n_agents, self.n_mounts, self.cameras.res)
        screen = self._look.screen.view(*shape, 3).permute(0, 1, 4, 2, 3)
        depth = 1 - ((self._look.distances.view(*shape) - c.agent_radius)/self.max_depth).clamp(0, 1)
        self._last_obs = arrdict.arrdict(rgb=downsample(screen, self.subsample).mean(-1),
                                         d=downsample(depth, self.subsample).mean(-1).unsqueeze(2))
        return self._last_obs

    def state(self, e=0):
        return self._last_obs[e].clone()


class Panorama(Cameras):

    def __init__(self, core, res=256, subsample=4, max_depth=10, n_agents=None):
        """One ring camera of 360 degrees at every agent's centre, looking along its heading - ray 0 just left of straight
        behind, the middle of the image straight ahead: what no plane projection can show. See :class:`Cameras`."""
        super().__init__(core, [[0., 0., 0.]], res, 360., 'ring', subsample, max_depth, n_agents)


class Overhead:

    def __init__(self, core, size=32, radius=4., n_agents=None, half_width=None):
        """Egocentric top-down maps, (n_env, n_agent, 3, size, size) linear RGB: each agent at the centre of its own
        ``2*radius`` metre square, its heading up, the walls in their baked light and the agents at their current poses
        (:func:`cuda.agent_views`, :func:`cuda.overhead`; no counterpart in the reference). Lines are drawn
        ``half_width`` metres either side (default: ``scene.line_half_width`` of the pixel size). The tensor a call returns is
        written again by the next call (the module keeps its buffers): clone it to keep it."""
        from . import scene
        self.core = core
        self.size, self.radius = int(size), float(radius)
        self.half_width = scene.line_half_width(2*self.radius/self.size) if half_width is None else float(half_width)
        self.space = spaces.MultiImage(n_agents or core.n_agents, 3, self.size, self.size)
        self._out = None

    def views(self):
        """(n_env, n_agent, 6): the views of the agents' maps as they stand now."""
        return cuda.agent_views(self.core.agents, self.size, self.radius)

    def __call__(self):
        self._out = cuda.overhead(self.core.scenery, self.views(), self.size, agents=self.core.agents,
                                  half_width=self.half_width, fields=('rgb',), out=self._out)
        self._last_obs = self._out.rgb
        return self._last_obs

    def state(self, e=0):
        return self._last_obs[e].clone()


class IMU:

    def __init__(self, core, speed_scale=10., ang_scale=360., n_agents=None):
        """(angular, medial, lateral) velocity observations, (n_env, n_agent, 3) (reference: modules.py:240-270)."""
        self.core = core
        self.space = spaces.MultiVector(n_agents or core.n_agents, 3)
        self.speed_scale = speed_scale
        self.ang_scale = ang_scale
        # a reading the physics launch has already taken (see _move), with the agents' epoch at that moment: every
        # physics call and every respawn through this module's helpers moves the epoch on, and a reading from an earlier
        # epoch is dropped (state changed behind the modules' back - writes straight into the tensors - is not seen)
        self._pending = None

    def __call__(self):
        agents = self.core.agents
        if self._pending is not None:
            (reading, epoch), self._pending = self._pending, None
            if epoch == agents._epoch:
                return reading
        return torch.cat([
            agents.angvelocity[..., None]/self.ang_scale,
            to_local_frame(agents.angles, agents.velocity)/self.speed_scale], -1)


class Proximity:

    def __init__(self, core, max_range=2., others=True):
        """How near the nearest thing is, and which way, (n_env, n_agent, 3) (:func:`cuda.clearance`; no counterpart in the
        reference): element 0 is ``min(d/max_range, 1)`` with ``d`` the distance from the agent's centre to the nearest line within
        ``max_range`` metres - 1 when nothing is in range - and elements 1, 2 the unit vector towards it in the agent's frame
        (:func:`to_local_frame`: the frame :class:`IMU` and :meth:`Goals.observation` use), (0, 0) when nothing is in range. With
        ``others`` the other agents' bodies count, at their current poses, and the agent's own are passed over; without, only the
        building's walls. The input of a wall-hugging penalty or a safety reward. One launch and a few elementwise ops; the module
        keeps the launch's buffers, nothing waits for the host: a call can sit in a HIP graph."""
        self.core = core
        self.max_range, self.others = float(max_range), bool(others)
        self.space = spaces.MultiVector(core.n_agents, 3)
        n, a = core.n_envs, core.n_agents
        self._skip = torch.arange(a, dtype=torch.int32, device=core.device).expand(n, a).contiguous() if self.others else None
        self._reading = None

    #: the :class:`cuda.Clearance` of the last call (None before the first)
    reading = property(lambda self: self._reading)

    @staticmethod
    def observation(distances, towards, angles, max_range):
        """The rule, a pure function: ``distances`` (N, A), ``towards`` (N, A, 2) in the world frame, ``angles`` (N, A) degrees ->
        (N, A, 3)."""
        near = (distances/max_range).clamp(max=1.)
        return torch.cat([near[..., None], to_local_frame(angles, towards)], -1)

    def __call__(self):
        agents = self.core.agents
        self._reading = cuda.clearance(self.core.scenery, agents.positions, self.max_range, agents=agents if self.others else None,
                                       skip=self._skip, out=self._reading)
        return self.observation(self._reading.distances, self._reading.towards, agents.angles, self.max_range)


class Percepts:

    def __init__(self, core, points=None, max_range=10., fov=None, k=4, pairs=None):
        """The nearest things each agent SEES, (n_env, n_agent, k, 4) (:func:`cuda.percepts`; no counterpart in the reference): row j
        is ``[1, forward/max_range, left/max_range, distance/max_range]`` for the j-th nearest of the points in sight of the agent -
        the point's offset turned into the agent's frame by :func:`to_local_frame`'s arithmetic, whose first axis is the camera's -
        and zeros beyond the ones it sees: the entity observation behind a visibility mask of tag, hide-and-seek and foraging
        tasks. ``points``: an (n_env, P, 2) float32 tensor kept by reference - pickups, goal objects; move them in place - or None:
        the other agents. In sight: no further than ``max_range`` metres, within ``fov`` degrees round the agent's heading when
        ``fov`` is given, no static wall in between; the agents' bodies do not occlude. ``pairs``: :func:`cuda.percepts`'. One
        launch and a few elementwise ops; the module keeps the launch's buffers, nothing waits for the host: a call can sit in a
        HIP graph."""
        self.core = core
        self.points, self.max_range, self.fov, self.k, self.pairs = points, float(max_range), fov, int(k), pairs
        self.space = spaces.MultiRows(core.n_agents, self.k, 4)
        self._reading = None

    #: the :class:`cuda.Percepts` of the last call (None before the first)
    reading = property(lambda self: self._reading)

    @staticmethod
    def pack(counts, near_offsets, near_distances, angles, max_range):
        """The rule, a pure function: ``counts`` (N, A) integers, ``near_offsets`` (N, A, K, 2) in the world frame, ``near_distances``
        (N, A, K), ``angles`` (N, A) degrees -> (N, A, K, 4)."""
        k = near_distances.shape[-1]
        listed = torch.arange(k, device=counts.device) < counts[..., None]
        local = to_local_frame(angles[..., None], near_offsets)
        rows = torch.cat([torch.ones_like(near_distances)[..., None], local/max_range, (near_distances/max_range)[..., None]], -1)
        return torch.where(listed[..., None], rows, torch.zeros_like(rows))

    def __call__(self):
        agents = self.core.agents
        self._reading = cuda.percepts(self.core.scenery, self.points, agents=agents, max_range=self.max_range, fov=self.fov, k=self.k,
                                      pairs=self.pairs, fields=('counts', 'near_offsets', 'near_distances'), out=self._reading)
        r = self._reading
        self._last_obs = self.pack(r.counts, r.near_offsets, r.near_distances, agents.angles, self.max_range)
        return self._last_obs

    def state(self, e=0):
        return self._last_obs[e].clone()


class Items:

    def __init__(self, core, grid, n_items, values=(1.,), colors=None, radius=.1, reach=None, delay=32, source=None, gate=None, seed=0,
                 kinds=None):
        """Things the agents see, touch and collect (:func:`cuda.collect_items`, :func:`cuda.overlay_items`; no counterpart in the
        reference): ``n_items`` items an env of ``len(values)`` kinds - item k is of kind ``k % len(values)`` unless ``kinds``
        ((P,) or (n_env, P) integers) says otherwise - worth ``values[kind]`` to the agent that takes one. An agent takes an item by
        coming within ``reach`` metres of it (default ``agent_radius + radius``) with no wall in between; the item is gone then and
        returns ``delay`` steps later (negative: never) on a cell drawn by :func:`cuda.cell_draws` from ``source`` (default: the
        free cells of ``grid``; a float32 layer is drawn where it is finite) through ``gate``. ``colors``: (3,), (P, 3) or
        (n_env, P, 3) linear RGB, default white; ``radius``: half the width an item shows in a camera. All items start absent
        and due: the first call puts them down.

        ``positions`` - (n_env, P, 2), NaN where an item is absent - goes to ``Percepts(core, points=items.positions)`` and to
        :func:`cuda.point_marks` as it is. A call is three launches and a select, keeps its buffers and never waits for the host:
        it can sit in a HIP graph, and every replay draws afresh."""
        self.core, self.grid = core, grid
        self.values = torch.as_tensor(values, dtype=torch.float32, device=core.device).reshape(-1)
        k = len(self.values)
        if kinds is None:
            kinds = torch.arange(int(n_items)) % k
        self.store = cuda.items(core.n_envs, int(n_items), kinds=kinds, colors=colors, n_kinds=k, device=core.device)
        self.radius = float(radius)
        self.reach = float(core.agent_radius + radius if reach is None else reach)
        self.delay, self.seed = int(delay), int(seed)
        self._source, self._gate = grid if source is None else source, gate
        self._collected = self._draws = self._dirs = self._shown = None

    #: (n_env, P, 2) float32: where the items are, NaN for an absent one; the store's own tensor
    positions = property(lambda self: self.store.positions)
    #: the :class:`cuda.Collected` of the last call (None before the first)
    collected = property(lambda self: self._collected)
    space = property(lambda self: spaces.MultiVector(self.core.n_agents, 1))

    @staticmethod
    def reward(counts, values):
        """The rule, a pure function: ``counts`` (N, A, K) integers, ``values`` (K,) -> (N, A) float32, ``counts.float() @ values``."""
        return counts.float() @ values

    def __call__(self, reset=None):
        """Collect, draw, place: ``reset`` (n_env,) bool - the envs whose items are all drawn anew. Returns the (n_env, n_agent)
        reward of this step."""
        c = self.core
        self._collected = cuda.collect_items(c.scenery, c.agents, self.store, self.reach, delay=self.delay, reset=reset, out=self._collected)
        due = self._collected.due
        if self._draws is None:
            gate = {} if self._gate is None else dict(gate=self._gate)
            band = dict(lo=-float('inf'), hi=torch.finfo(torch.float32).max) if cuda.cell_layer(self._source).is_float else {}
            self._draws = cuda.cell_draws(self.grid, self._source, self.store.n_items, 1, seed=self.seed, mask=due, **band, **gate)
            torch.where(due[:, :, None], self._draws.points[:, :, 0], self.store.positions, out=self.store.positions)
        else:
            cuda.place_items(self.store, self._draws, due)
        return self.reward(self._collected.counts, self.values)

    def draw(self, frame):
        """Draws the items into ``frame`` - the :class:`cuda.Render` of the agents as they stand - in place
        (:func:`cuda.overlay_items`); the frame gains ``.items``."""
        agents = self.core.agents
        if self._dirs is None:
            self._dirs = torch.empty(agents.angles.shape + (self.core.res, 2), dtype=torch.float32, device=self.core.device)
        cuda.camera_rays(agents, out=self._dirs)
        if self._shown is None or self._shown.shape != frame.distances.shape:
            self._shown = torch.empty(frame.distances.shape, dtype=torch.int32, device=self.core.device)
        return cuda.overlay_items(self.store, frame, agents=agents, dirs=self._dirs, radius=self.radius, out_items=self._shown,
                                  scenery=self.core.scenery)

    def state(self, e=0):
        return arrdict.arrdict(positions=self.store.positions[e].clone(), timers=self.store.timers[e].clone(), kinds=self.store.kinds[e].clone())


def random_empty_positions(geometries, n_agents, n_points):
    """(n_geometries, n_agents, n_points, 2) randomly chosen free-cell centres, precomputed so respawns are cheap
    (reference: modules.py:272-296; consumes the global ``np.random`` in the same order, env by env). The free cells of
    a geometry that turns up many times are looked up once."""
    free_cells = {}
    points = np.empty((len(geometries), n_agents, n_points, 2))
    for e, g in enumerate(geometries):
        free = free_cells.get(id(g))
        if free is None:
            free = free_cells[id(g)] = np.argwhere(g['masks'] > 0)           # (row, col) of every free cell
        # two draws from the global stream per env, as the reference makes them: which cells (one row of the table per
        # agent-tuple, at most as many rows as the plan has room for), then the order the table is served in
        rows = max(min(len(free)//n_agents, n_points), 0)
        picks = np.random.choice(np.arange(len(free)), (rows, n_agents), replace=True)
        # a plan too small for n_points distinct rows repeats its table; the last n_points rows are the ones kept
        repeats = int(n_points/rows + 1)
        table = np.tile(free[picks], (repeats, 1, 1))[-n_points:]
        table = table[np.random.permutation(len(table))]
        points[e] = np.swapaxes(geometry.centers(table, g['masks'].shape, g['res']), 0, 1)
    return points


def _device_empty_positions(geometries, n_agents, n_points, device):
    """:func:`random_empty_positions` drawn on the device: every spawn point an independent uniform pick among its
    geometry's free cells (what the reference's choice-then-permute amounts to whenever a geometry has at least
    ``n_agents*n_points`` free cells), from torch's generator instead of ``np.random``."""
    tables, which = {}, np.empty(len(geometries), np.int64)
    for e, g in enumerate(geometries):
        if id(g) not in tables:
            free = np.stack((g['masks'] > 0).nonzero(), -1)
            tables[id(g)] = (len(tables), geometry.centers(free, g['masks'].shape, g['res']))
        which[e] = tables[id(g)][0]
    centres = [c for _, c in tables.values()]
    counts = torch.as_tensor([len(c) for c in centres], device=device)
    starts = (counts.cumsum(0) - counts)[torch.as_tensor(which, device=device)]
    counts = counts[torch.as_tensor(which, device=device)]
    pick = (torch.rand((len(geometries), n_agents, n_points), device=device, dtype=torch.float64)*counts[:, None, None]).long()
    pick = torch.minimum(pick, counts[:, None, None] - 1) + starts[:, None, None]
    return torch.as_tensor(np.concatenate(centres), device=device).float()[pick]


class RandomSpawns:

    def __init__(self, geometries, core, n_spawns=100, fast=False):
        """Respawns agents at random free points of their geometry (reference: modules.py:298-326). ``fast=True``
        draws the spawn tables on the device (same distribution, torch's random stream instead of numpy's) - for
        worlds of 10^4 envs and up, where the reference's per-env loop takes seconds."""
        self.core = core
        if fast:
            positions = _device_empty_positions(geometries, core.n_agents, n_spawns, core.device)
            angles = torch.empty(positions.shape[:3], device=core.device).uniform_(-180, 180)
            self._spawns = arrdict.arrdict(positions=positions, angles=angles)
            return
        positions = random_empty_positions(geometries, core.n_agents, n_spawns)
        angles = core.random.uniform(-180, +180, (len(geometries), core.n_agents, n_spawns))
        self._spawns = arrdict.torchify(arrdict.arrdict(positions=positions, angles=angles)).to(core.device)

    def draw(self, reset, after=False):
        """The respawn of the agents marked in the (n_env, n_agent) bool mask ``reset`` as a request that
        :func:`cuda.physics` (through the movement modules' ``respawn=``) carries out inside its launch - before the
        step, or after it with ``after=True``. Same draw as :meth:`__call__`."""
        return dict(mask=reset.contiguous(), choices=self._choices(reset), positions=self._spawns.positions, angles=self._spawns.angles, after=after)

    #: steps' worth of spawn choices drawn per torch.randint call (see _choices)
    DRAW_AHEAD = 64

    def _choices(self, reset):
        """This step's spawn choice for every agent: uniform among the first ``spawns.shape[1]`` spawn points, from torch's
        generator - drawn DRAW_AHEAD steps at a time and handed out a step's slice per call: on (4096, 1) tensors the draw is a
        launch of its own that lasts as long as the env's whole bookkeeping kernel, every step, for numbers that a handful of
        agents in thousands ever look at. Inside a stream capture the draw stays in the step (a captured slice would be the
        same numbers at every replay; torch.randint is graph-safe)."""
        n = self._spawns.angles.shape[1]
        if reset.is_cuda and not torch.cuda.is_current_stream_capturing():
            ahead = getattr(self, '_ahead', None)
            if ahead is None or self._ahead_at >= len(ahead) or ahead.shape[1:] != reset.shape:
                ahead = self._ahead = torch.randint(0, n, (self.DRAW_AHEAD,) + tuple(reset.shape), device=reset.device)
                self._ahead_at = 0
            self._ahead_at += 1
            return ahead[self._ahead_at - 1]
        return torch.randint(0, n, reset.shape, device=reset.device)

    def __call__(self, reset):
        """``reset`` is an (n_env, n_agent) bool mask; the marked agents get a new pose and zero velocity.

        Same draw as the reference (a uniform choice among the first ``spawns.shape[1]`` spawn points), but made for
        every agent and applied through the mask, so the step needs no ``nonzero`` and with it no host sync."""
        _respawn(self.core.agents, self.draw(reset))


class RandomLifespans:

    def __init__(self, core, max_lifespan, min_lifespan=None):
        """Flags agents that outlive a randomly drawn lifespan, so synchronous envs drift apart
        (reference: modules.py:328-381)."""
        self.min_lifespan = max_lifespan//2 if min_lifespan is None else min_lifespan
        self.max_lifespan = max_lifespan
        self._max_lifespans = torch.zeros((core.n_envs, core.n_agents), dtype=torch.int, device=core.device)
        self._lifespans = torch.zeros_like(self._max_lifespans)
        self._reset(core.agent_full(True))

    def _reset(self, reset):
        self._lifespans.masked_fill_(reset, 0)
        fresh = torch.randint_like(self._max_lifespans, self.min_lifespan, self.max_lifespan)
        self._max_lifespans[:] = torch.where(reset, fresh, self._max_lifespans)

    def __call__(self, reset=None):
        self._lifespans += 1
        reset = torch.zeros_like(self._lifespans, dtype=torch.bool) if reset is None else reset
        reset = (self._lifespans >= self._max_lifespans) | reset
        self._reset(reset)
        return reset

    def state(self, e):
        return arrdict.arrdict(lifespan=self._lifespans[e], max_lifespans=self._max_lifespans[e]).clone()


class Goals:

    def __init__(self, geometries, core, grid, candidates=8, min_distance=0., table=None, n_spawns=100):
        """A goal per agent, and how far the agent has to walk to it (no counterpart in the reference).

        ``grid`` is the scenery's :func:`cuda.nav_grid`. Goals come from a table of free points per agent - ``table``
        (n_env, n_agent, S, 2), for instance a :class:`RandomSpawns`' own; default: ``n_spawns`` points drawn as it draws
        them. A floorplan is not one connected space (closets without a door, pillars), so a goal picked blindly is, for a
        fair share of agents, one that cannot be reached. The rule here: the agent's next ``candidates`` table entries (each
        agent walks its table cyclically, ``candidates`` entries per draw - the table is in random order, and no random
        numbers are drawn per step) are measured from where the agent stands, and the first whose walking distance is finite
        and at least ``min_distance`` is the goal. An agent that found none is flagged in :attr:`stranded` and its goal is the
        spot it stands on. Nothing waits for the host: a draw is two masked :func:`cuda.distance_fields` launches (the field
        round the agent, to measure the candidates; the field of the goal) and a :meth:`cuda.DistanceFields.at`."""
        self.core = core
        self.grid = grid
        self.candidates, self.min_distance = int(candidates), float(min_distance)
        if table is None:
            table = torch.as_tensor(random_empty_positions(geometries, core.n_agents, n_spawns), dtype=torch.float32)
        self._table = table.to(core.device).float().contiguous()
        n, a, s = self._table.shape[:3]
        if (n, a) != (core.n_envs, core.n_agents) or self._table.shape[3:] != (2,):
            raise RuntimeError(f'table must be ({core.n_envs}, {core.n_agents}, S, 2); got {tuple(self._table.shape)}')
        self.space = spaces.MultiVector(core.n_agents, 3)
        self.stranded = core.agent_full(False)
        self._draws = torch.zeros((n, a), dtype=torch.long, device=core.device)
        self._step = (s//2 + torch.arange(self.candidates, device=core.device))[None, None, :]
        self._agent = torch.arange(a, dtype=torch.int32, device=core.device)[None, :, None].expand(n, a, self.candidates).reshape(n, -1).contiguous()
        self._around = self._fields = None

    #: (n_env, n_agent, 2): every agent's goal
    goals = property(lambda self: self._fields.goals)
    #: the :class:`cuda.DistanceFields` of the goals
    fields = property(lambda self: self._fields)

    @staticmethod
    def choose(distances, candidates, here, min_distance=0.):
        """The rule: ``distances`` (N, A, K) from each agent to its K ``candidates`` (N, A, K, 2) -> ((N, A, 2) goals: the first
        candidate whose distance is finite and at least ``min_distance``; (N, A) bool: there was none, and the goal is ``here``)."""
        good = torch.isfinite(distances) & (distances >= min_distance)
        first = good.int().argmax(-1)                                   # (the first of the largest: the first True)
        stranded = ~good.any(-1)
        goal = candidates.gather(2, first[..., None, None].expand(-1, -1, 1, 2)).squeeze(2)
        return torch.where(stranded[..., None], here, goal), stranded

    def __call__(self, reset):
        """Agents marked in the (n_env, n_agent) bool ``reset`` get a new goal, reachable from where they stand now."""
        n, a, s = self._table.shape[:3]
        reset = reset.contiguous()
        here = self.core.agents.positions
        index = (self._draws[..., None]*self.candidates + self._step) % s
        self._draws += reset
        candidates = self._table.gather(2, index[..., None].expand(-1, -1, -1, 2))
        self._around = cuda.distance_fields(self.grid, here, mask=reset, out=self._around)
        distances = self._around.at(candidates.reshape(n, a*self.candidates, 2), goal=self._agent).reshape(n, a, self.candidates)
        goal, stranded = self.choose(distances, candidates, here, self.min_distance)
        torch.where(reset, stranded, self.stranded, out=self.stranded)
        self._fields = cuda.distance_fields(self.grid, goal.contiguous(), mask=reset, out=self._fields)
        return self.goals

    def distances(self):
        """(n_env, n_agent): how far every agent has to walk to its goal now; +inf where no path exists."""
        return self._fields.at(self.core.agents.positions)

    def waypoints(self, lookahead=16):
        """(n_env, n_agent, 2): where every agent should head for now to walk to its own goal
        (:meth:`cuda.DistanceFields.waypoints`); NaN where no path exists."""
        return self._fields.waypoints(self.core.agents.positions, lookahead=lookahead)

    def observation(self):
        """(n_env, n_agent, 3): the goal's offset in the agent's frame, and its length (the straight line, which is what a
        compass knows: the walking distance is the env's to reward, not the agent's to see)."""
        agents = self.core.agents
        offset = self.goals - agents.positions
        return torch.cat([to_local_frame(agents.angles, offset), offset.norm(dim=-1, keepdim=True)], -1)

    def state(self, e=0):
        return arrdict.arrdict(goals=self.goals[e], stranded=self.stranded[e]).clone()


class SampledGoals:

    def __init__(self, core, grid, min_distance, max_distance, seed=0):
        """A goal per agent at a chosen walking distance (no counterpart in the reference): :class:`Goals`' interface - so
        :class:`PathFollower` and the envs take it unchanged - with the goal drawn on the device by :func:`cuda.cell_draws`,
        uniformly among the free cells of the agent's env whose walking distance from where the agent stands lies in
        ``[min_distance, max_distance]`` metres. Such a goal is reachable by construction, there is no table and no candidate
        count, and moving the band from episode to episode is a curriculum. A draw is three launches and nothing waits for
        the host: the masked :func:`cuda.distance_fields` round the agents; one cell drawn in the band of that field; the
        masked field of the goals. An agent whose band holds no cell - a closet smaller than ``min_distance`` - is flagged in
        :attr:`stranded` (exactly ``draws.counts == 0``) and its goal is the spot it stands on. The band is on the cell's own
        value: the agent's distance to the goal, which adds the leg from the agent to a cell next to it, can be up to a cell's
        diagonal outside it."""
        self.core, self.grid = core, grid
        self.min_distance, self.max_distance, self.seed = float(min_distance), float(max_distance), int(seed)
        if not 0 <= self.min_distance <= self.max_distance:
            raise RuntimeError(f'the band must be 0 <= min_distance <= max_distance; got {min_distance}, {max_distance}')
        self.space = spaces.MultiVector(core.n_agents, 3)
        self.stranded = core.agent_full(False)
        self._around = self._fields = self._draws = None

    #: (n_env, n_agent, 2): every agent's goal
    goals = property(lambda self: self._fields.goals)
    #: the :class:`cuda.DistanceFields` of the goals
    fields = property(lambda self: self._fields)
    #: the :class:`cuda.CellDraws` of the last draw (None before the first)
    draws = property(lambda self: self._draws)

    def __call__(self, reset):
        """Agents marked in the (n_env, n_agent) bool ``reset`` get a new goal, in the band from where they stand now."""
        reset = reset.contiguous()
        here = self.core.agents.positions
        self._around = cuda.distance_fields(self.grid, here, mask=reset, out=self._around)
        if self._draws is None:
            self._draws = cuda.cell_draws(self.grid, self._around, self.core.n_agents, 1, lo=self.min_distance, hi=self.max_distance,
                                          seed=self.seed, mask=reset)
        else:
            self._draws.again(mask=reset)
        stranded = self._draws.counts == 0
        goal = torch.where(stranded[..., None], here, self._draws.points[:, :, 0])
        torch.where(reset, stranded, self.stranded, out=self.stranded)
        self._fields = cuda.distance_fields(self.grid, goal.contiguous(), mask=reset, out=self._fields)
        return self.goals

    distances, waypoints, observation, state = Goals.distances, Goals.waypoints, Goals.observation, Goals.state


class Routes:

    def __init__(self, core, grid, goals, cost):
        """Weighted routes to the goals of a :class:`Goals` or a :class:`SampledGoals` (anything with ``.goals`` (n_env, n_agent, 2)):
        the cells round every agent's goal are the seeds (:func:`cuda.point_marks`, agent k store k) of a :func:`cuda.cost_fields`
        over ``cost`` - an :func:`cuda.inflation_costs` layer keeps the routes off the walls, a :func:`cuda.mark_costs` layer prices
        unknown or watched floor - kept by reference, so a layer rewritten in place bends the routes computed after it.
        :meth:`waypoints` and :meth:`distances` have the shape :class:`PathFollower` takes from :class:`Goals`; a route ends on the
        centre of a cell next to the goal, which is as near as an env's ``arrive`` asks. The goals module draws the goals, so call
        it first; the stores are made by the first call, and from then on a call is a fill, two launches and nothing that waits
        for the host: it can sit in a HIP graph."""
        self.core, self.grid, self.goals, self.cost = core, grid, goals, cost
        #: the :class:`cuda.PointMarks` of the goals and the :class:`cuda.CostFields` seeded by them (None before the first call)
        self.seeds = self.fields = None

    def __call__(self, reset=None):
        """Marks the goals as they stand and recomputes the routes of the agents marked in the (n_env, n_agent) bool ``reset``
        (default all) - those whose goal was drawn anew. Call once per step, after the goals module."""
        if self.seeds is None:
            self.seeds = cuda.point_marks(self.grid, self.goals.goals, self.core.n_agents)
            self.fields = cuda.cost_fields(self.grid, self.seeds.marks, self.core.n_agents, self.cost)
        else:
            self.seeds.points = self.goals.goals
            self.seeds.update()
            self.fields.update(None if reset is None else reset.contiguous())
        return self.fields

    def distances(self):
        """(n_env, n_agent): what the route from where every agent stands costs - metres where the cost is 1; +inf without one."""
        return self.fields.at(self.core.agents.positions)

    def waypoints(self, lookahead=16):
        """(n_env, n_agent, 2): where every agent should head for now to follow its route (:meth:`cuda.CostFields.waypoints`); NaN
        where no route exists."""
        return self.fields.waypoints(self.core.agents.positions, lookahead=lookahead)


class SampledSpawns:

    def __init__(self, core, grid, seed=0, within=None, gate=None):
        """Respawns agents on a cell of the nav grid drawn on the device by :func:`cuda.cell_draws` (no counterpart in the
        reference): :class:`RandomSpawns`' interface without its table. A spawn is the centre of a cell drawn uniformly among
        the env's free cells - every one of them a spot the agent fits, by the grid's own clearance - or, with ``within`` (a
        float32 layer, :func:`cuda.cell_layer`'s, one store an env or one per agent: a distance field from a reference point,
        say), among the free cells where it is finite: the cells of the same connected space as the reference. The heading is
        the draw's spare uniform number, ``uniforms*360 - 180``. Every agent draws for itself: two agents of an env may draw
        the same cell, as they may in the reference's table. An agent of an env without a qualifying cell stays where it is.
        ``gate``: a byte layer (:meth:`cuda.Regions.largest_mask`, say: every agent of an env into the env's largest connected
        space); only cells where its byte is set are drawn - a connectivity test as what it is, for no distance field at all."""
        self.core, self.grid, self.seed = core, grid, int(seed)
        self._within, self._gate = within, gate
        self._choices = torch.zeros((core.n_envs, core.n_agents), dtype=torch.long, device=core.device)
        self._draws = None

    #: the :class:`cuda.CellDraws` of the last draw (None before the first)
    draws = property(lambda self: self._draws)

    def draw(self, reset, after=False):
        """The respawn of the agents marked in the (n_env, n_agent) bool mask ``reset`` as a request in
        :meth:`RandomSpawns.draw`'s form: a table of one freshly drawn spawn per agent, ``choices`` all zero."""
        reset = reset.contiguous()
        if self._draws is None:
            gate = {} if self._gate is None else dict(gate=self._gate)
            if self._within is None:
                self._draws = cuda.cell_draws(self.grid, self.grid, self.core.n_agents, 1, seed=self.seed, mask=reset, **gate)
            else:
                self._draws = cuda.cell_draws(self.grid, self._within, self.core.n_agents, 1, lo=-float('inf'), hi=torch.finfo(torch.float32).max,
                                              seed=self.seed, mask=reset, **gate)
        else:
            self._draws.again(mask=reset)
        d = self._draws
        return dict(mask=reset & (d.counts > 0), choices=self._choices, positions=d.points, angles=d.uniforms*360. - 180., after=after)

    def __call__(self, reset):
        """``reset`` is an (n_env, n_agent) bool mask; the marked agents get a new pose and zero velocity."""
        _respawn(self.core.agents, self.draw(reset))


class Coverage:

    def __init__(self, core, grid, max_range=10., shared=False, countable=None):
        """Floor coverage: which cells of the nav grid every agent's depth rays have passed over since it started over, and
        how much floor each new frame adds (:func:`cuda.seen_maps`; no counterpart in the reference, whose Explorer rewards
        wall texels). ``grid`` is the scenery's :func:`cuda.nav_grid`; rays are followed for at most ``max_range`` metres;
        ``countable``: the cells that count (default: the grid's free cells - then no wall is seen through). Every agent has
        a map of its own; ``shared=True`` gives an env's agents ONE map, which any of them starting over clears, and each of
        them the map's whole gain. One launch behind the render's, nothing waits for the host."""
        self.core, self.grid = core, grid
        self.max_range, self.shared = float(max_range), bool(shared)
        self.maps = cuda.seen_maps(grid, 1 if shared else core.n_agents, countable)
        self.space = spaces.MultiVector(core.n_agents, 1)
        self._slot = torch.zeros((core.n_envs, core.n_agents), dtype=torch.int32, device=core.device) if shared else None
        self._gained = torch.zeros((core.n_envs, self.maps.n_maps), dtype=torch.int32, device=core.device)
        self._area = torch.tensor(grid.cell, dtype=torch.float32, device=core.device)**2

    def _per_agent(self, t):
        return t.expand(-1, self.core.n_agents) if self.shared else t

    def __call__(self, frame, reset=None):
        """(n_env, n_agent) float32: the floor each agent saw for the first time in ``frame`` - a render of the agents as they
        stand, with its ``distances`` - in square metres. ``reset`` (n_env, n_agent) bool: the agents that started over this
        step; their maps are cleared before the frame is marked."""
        if reset is not None and self.shared:
            reset = reset.any(-1, keepdim=True)
        gained = self.maps.mark_render(self.core.agents, frame, slot=self._slot, max_range=self.max_range, reset=reset, out=self._gained)
        return self._per_agent(gained.float()*self._area)

    def fraction(self):
        """(n_env, n_agent) float32: the share of the countable floor each agent('s map) has seen."""
        return self._per_agent(self.maps.fraction())

    def observation(self):
        """(n_env, n_agent, 1): :meth:`fraction`."""
        return self.fraction().unsqueeze(-1)

    def state(self, e=0):
        """(S, ny, nx) bool: a copy of env ``e``'s maps, row 0 at the lowest y."""
        return torch.stack([self.maps.image(e, s) for s in range(self.maps.n_maps)]).clone()


class LocalMap:

    #: the channels that have a name
    NAMED = ('floor', 'wall', 'seen')

    def __init__(self, core, coverage, size=32, radius=4., channels=('floor', 'wall'), samples=1):
        """Egocentric maps of what each agent has SEEN, (n_env, n_agent, C, size, size): the agent at the centre of its own
        ``2*radius`` metre square, its heading up (:func:`cuda.agent_views`, :func:`cuda.local_maps`; no counterpart in the
        reference). ``coverage`` is the :class:`Coverage` whose seen maps gate the picture - with ``coverage.shared`` every
        agent of an env reads the env's one map. Unlike :class:`Overhead`, which draws the scenery's walls whether anybody has
        looked at them or not, nothing shows here before a depth ray has passed over it. ``channels`` names them: ``'floor'``
        - 1 on the free cells of the nav grid the map has seen; ``'wall'`` - 1 on the blocked cells it has seen (the cells
        rays ended on stay marked); ``'seen'`` - the map itself; or any :func:`cuda.map_channel`, a frontier or a goal field
        say. 0 where nothing is seen and beyond the grid. ``samples``: sub-samples a side per pixel, for pixels larger than a
        cell. The tensor a call returns is written again by the next call (the module keeps its buffer): clone it to keep it."""
        self.core, self.coverage = core, coverage
        self.size, self.radius, self.samples = int(size), float(radius), int(samples)
        grid, maps = coverage.grid, coverage.maps
        seen = cuda.cell_layer(maps, field=coverage._slot)
        made = {'floor': lambda: cuda.map_channel(grid, where=True, gate=seen), 'wall': lambda: cuda.map_channel(grid, where=False, gate=seen),
                'seen': lambda: cuda.map_channel(seen)}
        self.channels = []
        for ch in channels:
            if isinstance(ch, str):
                if ch not in made:
                    raise RuntimeError(f'a named channel is one of {self.NAMED}; got {ch!r}')
                ch = made[ch]()
            self.channels.append(ch)
        self.space = spaces.MultiImage(core.n_agents, len(self.channels), self.size, self.size)
        self._out = None

    def views(self):
        """(n_env, n_agent, 6): the views of the agents' maps as they stand now."""
        return cuda.agent_views(self.core.agents, self.size, self.radius)

    def __call__(self):
        """The windows of the maps as they stand: call after the frame's marks."""
        self._out = cuda.local_maps(self.coverage.grid, self.views(), self.size, self.channels, samples=self.samples, out=self._out)
        return self._out

    def state(self, e=0):
        return self._out[e].clone()


class Territories:

    def __init__(self, core, grid, refresh=8):
        """Whose agent is nearest, on foot, to every cell of the floor (no counterpart in the reference): the nav grid partitioned
        by nearest agent - a geodesic Voronoi diagram. The agents' cells are the seeds (:func:`cuda.point_marks` of their
        positions, agent k with id k), a :func:`cuda.seeded_fields` of them the walking distance to the nearest agent, and
        :func:`cuda.basins` of that field says which agent it is. ``basins.labels`` holds the agent's number per cell, -1 where no
        agent can walk to; :attr:`masks` is a :class:`cuda.CellLayer` of one byte store per agent - its territory, a
        :func:`cuda.seeded_fields` ``marks``, a gate or a :func:`cuda.map_channel` as it is. An env's territories are recomputed
        every ``refresh`` steps and when one of its agents starts over. Nothing waits for the host: which envs are due is decided on
        the device, so a call can sit in a HIP graph."""
        self.core, self.grid, self.refresh = core, grid, int(refresh)
        if self.refresh < 1:
            raise RuntimeError(f'refresh must be a positive integer; got {refresh}')
        n, a = core.n_envs, core.n_agents
        self._steps = torch.zeros((n,), dtype=torch.long, device=core.device)
        self.seeds = cuda.point_marks(grid, core.agents.positions, 1)
        self.near = cuda.seeded_fields(grid, self.seeds.marks, 1)
        self.basins = cuda.basins(self.near, ids=self.seeds.ids, n_ids=a)
        self._wanted = torch.arange(a, dtype=torch.int32, device=core.device).expand(n, a).contiguous()
        #: a :class:`cuda.CellLayer` of one byte store per agent: 1 on the cells nearest to it
        self.masks = self.basins.masks(labels=self._wanted)
        self._area = torch.tensor(grid.cell, dtype=torch.float32, device=core.device)**2

    def __call__(self, reset=None):
        """Recomputes the territories of the envs that are due: those with an agent marked in the (n_env, n_agent) bool ``reset``
        and those that have taken a multiple of ``refresh`` steps since. Call once per step."""
        if reset is not None:
            self._steps.masked_fill_(reset.any(-1), 0)
        due = (self._steps % self.refresh == 0)[:, None]
        self._steps += 1
        self.due = due                                  # ((n_env, 1) bool: whose territories were due at this call)
        self.seeds.points = self.core.agents.positions
        self.seeds.update()
        self.near.update(due)
        self.basins.update(due)
        self.basins.masks(labels=self._wanted, out=self.masks)
        return self.masks

    def areas(self):
        """(n_env, n_agent) float32: the floor each agent holds, in square metres."""
        return self.basins.sizes[:, 0].float()*self._area


class Frontiers:

    def __init__(self, core, coverage, refresh=8, territories=None, cost=None):
        """How far every agent has to walk to the nearest floor its map has not seen, and which way (no counterpart in the
        reference): the frontier fields of a :class:`Coverage`'s maps (:meth:`cuda.SeenMaps.frontier_fields`), one field per
        map. A field is recomputed every ``refresh`` steps of its agent and when the agent starts over; in between it is a
        few steps stale, which costs a detour at worst - a stale field is still a whole field, and leads to a cell that was
        unseen when it was computed. :meth:`waypoints` has the shape :class:`PathFollower` takes from :class:`Goals`. With
        ``coverage.shared`` an env has one field, which all its agents follow. Nothing waits for the host: which fields are
        due is decided on the device, so a call can sit in a HIP graph.

        ``territories``: a :class:`Territories` of the same core and grid, with a shared coverage: then every agent ALSO has a field
        of its own (:attr:`own`) - the walk to the nearest unseen floor within its own territory,
        ``seeded_fields(grid, territories.masks.values, A, where=True, among=unseen)`` - and follows that, so that an env's agents
        part ways instead of walking to the same unseen cell; an agent whose territory holds no unseen floor follows the env's
        shared field (:meth:`fallback`). The module calls the territories itself, once per call.

        ``cost``: a cost layer as :func:`cuda.cost_fields` takes it, kept by reference; the frontier fields (and the agents' own)
        are then :class:`cuda.CostFields`, and the walk to the nearest unseen floor is the cheapest one, not the shortest."""
        self.core, self.coverage, self.refresh = core, coverage, int(refresh)
        if self.refresh < 1:
            raise RuntimeError(f'refresh must be a positive integer; got {refresh}')
        if territories is not None and not coverage.shared:
            raise RuntimeError('territories go with a shared coverage: with a map of its own each agent has its own frontier already')
        self._steps = torch.zeros((core.n_envs, core.n_agents), dtype=torch.long, device=core.device)
        self._field = coverage._slot                    # (n_env, n_agent) zeros when the map is shared, else None: agent k field k
        self.cost = cost
        self.fields = coverage.maps.frontier_fields(cost=cost)
        self.territories, self.own = territories, None
        if territories is not None:
            maps = coverage.maps
            self._unseen = torch.zeros_like(maps.countable)           # (grid.free's layout: the shared map is one store an env)
            self._refresh_unseen()
            if cost is None:
                self.own = cuda.seeded_fields(coverage.grid, territories.masks.values, core.n_agents, where=True, among=self._unseen)
            else:
                self.own = cuda.cost_fields(coverage.grid, territories.masks.values, core.n_agents, cost, where=True, among=self._unseen)

    def _refresh_unseen(self):
        """unseen = ~seen & countable, in place, by byte ops on the env-layout stores."""
        maps = self.coverage.maps
        n = min(self._unseen.shape[0], maps.values.shape[0])
        torch.bitwise_xor(maps.values[:n], 1, out=self._unseen[:n])
        self._unseen[:n] &= maps.countable[:n]
        self._unseen[:n] &= 1

    def __call__(self, reset=None):
        """Recomputes the fields that are due: those of the agents marked in the (n_env, n_agent) bool ``reset`` - they started
        over, their maps are empty again - and those whose agent has taken a multiple of ``refresh`` steps since. Call once per
        step, after the maps were marked."""
        if reset is not None:
            self._steps.masked_fill_(reset, 0)
        due = self._steps % self.refresh == 0
        self._steps += 1
        self.due = due                                  # ((n_env, n_agent) bool: whose field was due at this call)
        if self.territories is not None:
            self.territories(reset)
            self._refresh_unseen()
            self.own.update(due.any(-1, keepdim=True).expand_as(due).contiguous())      # (an env's agents share the map: all or none)
        if self.coverage.shared:
            due = due.any(-1, keepdim=True)
        self.fields.update(due)
        return self.fields

    @staticmethod
    def fallback(own, shared):
        """The rule, a pure function: ``own`` where it is a number, ``shared`` where it is NaN or +inf - an agent whose own
        territory holds no unseen floor it can walk to follows the env's field instead."""
        return torch.where(torch.isnan(own) | torch.isinf(own), shared, own)

    def distance(self):
        """(n_env, n_agent): how far every agent has to walk to the nearest unseen floor; +inf where there is none it can reach."""
        shared = self.fields.at(self.core.agents.positions, goal=self._field)
        if self.own is None:
            return shared
        return self.fallback(self.own.at(self.core.agents.positions), shared)

    def waypoints(self, lookahead=16):
        """(n_env, n_agent, 2): where every agent should head for now to walk to the nearest unseen floor
        (:meth:`cuda.SeededFields.waypoints`); NaN where :meth:`distance` is +inf."""
        shared = self.fields.waypoints(self.core.agents.positions, goal=self._field, lookahead=lookahead)
        if self.own is None:
            return shared
        return self.fallback(self.own.waypoints(self.core.agents.positions, lookahead=lookahead), shared)


class Assignments:

    def __init__(self, core, coverage, n_zones=64, refresh=8, cost=None):
        """Which frontier cluster each agent of an env should walk to, by walking distance (no counterpart in the reference): the
        standard multi-robot answer to a shared map - not the floor split by where the agents stand (:class:`Territories`), but a
        different cluster of unseen floor for every agent. Per refresh, for the envs that are due: the clusters the unseen floor
        falls into (:meth:`cuda.SeenMaps.frontier_regions`), a distance field round every agent (:func:`cuda.distance_fields` of
        their positions), and ONE :func:`cuda.zones` launch of the two - ``zones.least`` (n_env, n_agent, K) is each agent's walk to
        the nearest cell of each of the first ``n_zones`` clusters; :meth:`choose` then assigns clusters to agents, the chosen
        clusters become byte masks (:meth:`cuda.Regions.masks`) and every agent gets a field of its own to its cluster's cells
        (:attr:`own`: :func:`cuda.seeded_fields` over the masks, among the unseen cells exactly as :attr:`Frontiers.own`; with
        ``cost`` a :func:`cuda.cost_fields`). An agent without a cluster it can walk to follows the env's shared frontier field
        (:meth:`Frontiers.fallback`).

        :class:`Frontiers`' interface: call once per step after the maps were marked, then :meth:`distance` and :meth:`waypoints`;
        :class:`PathFollower` takes it unchanged. For a shared coverage only. An env is refreshed every ``refresh`` steps and when
        one of its agents starts over. Nothing waits for the host: which envs are due is decided on the device, so a call can sit
        in a HIP graph."""
        self.core, self.coverage, self.refresh, self.cost = core, coverage, int(refresh), cost
        if self.refresh < 1:
            raise RuntimeError(f'refresh must be a positive integer; got {refresh}')
        if not coverage.shared:
            raise RuntimeError('assignments go with a shared coverage: with a map of its own each agent has its own frontier already')
        n, a = core.n_envs, core.n_agents
        grid, maps = coverage.grid, coverage.maps
        self._steps = torch.zeros((n,), dtype=torch.long, device=core.device)
        self._field = coverage._slot                    # ((n_env, n_agent) zeros: every agent reads the env's one shared field)
        self.fields = maps.frontier_fields(cost=cost)   # the env's shared frontier field: the fallback
        self.clusters = maps.frontier_regions()
        self.around = cuda.distance_fields(grid, core.agents.positions)
        self.zones = cuda.zones(self.clusters, values=self.around, n_zones=n_zones)
        #: (n_env, n_agent) int64: the zone each agent was assigned at its env's last refresh, -1 without one
        self.choice = torch.full((n, a), -1, dtype=torch.long, device=core.device)
        self._wanted = torch.full((n, a), -1, dtype=torch.int32, device=core.device)
        self._assign(torch.ones((n, 1), dtype=torch.bool, device=core.device))
        #: a :class:`cuda.CellLayer` of one byte store per agent: 1 on the cells of the cluster it was assigned
        self.masks = self.clusters.masks(labels=self._wanted)
        self._unseen = torch.zeros_like(maps.countable)                 # (grid.free's layout: the shared map is one store an env)
        self._refresh_unseen()
        if cost is None:
            self.own = cuda.seeded_fields(grid, self.masks.values, a, where=True, among=self._unseen)
        else:
            self.own = cuda.cost_fields(grid, self.masks.values, a, cost, where=True, among=self._unseen)

    _refresh_unseen = Frontiers._refresh_unseen

    @staticmethod
    def choose(costs):
        """The rule, a pure function: ``costs`` (..., A, K) float - agent a's walk to zone k, +inf (or NaN) where it cannot get
        there. Returns ``(choice, none)``: ``choice`` (..., A) int64, the zone of every agent, -1 without one; ``none`` (..., A)
        bool, ``choice < 0``.

        1. A times over: among the pairs (a, k) with agent a unassigned, zone k untaken and a finite cost, the least cost - ties to
           the least a, then the least k - is assigned.
        2. Every agent still unassigned that has a finite cost takes its own least-cost zone, taken or not; ties to the least k.
        3. Otherwise -1.

        Greedy and deterministic - NOT the optimal assignment (the least total walk), which it can miss by taking the best pair
        first. Ties are broken by ``where(c == c.amin) -> least index``, never by ``argmin``, whose choice among equals is not
        defined. No host synchronisation."""
        a, k = costs.shape[-2:]
        inf = torch.full_like(costs, float('inf'))
        finite = torch.isfinite(costs)
        open_costs = torch.where(finite, costs, inf)
        flat_index = torch.arange(a*k, device=costs.device)
        zone_index = torch.arange(k, device=costs.device)
        choice = torch.full(costs.shape[:-1], -1, dtype=torch.long, device=costs.device)
        taken = torch.zeros(costs.shape[:-2] + (k,), dtype=torch.bool, device=costs.device)
        for _ in range(a):
            c = torch.where((choice < 0)[..., :, None] & ~taken[..., None, :], open_costs, inf).flatten(-2)
            least = c.amin(-1, keepdim=True)
            pair = torch.where(c == least, flat_index, a*k).amin(-1)   # (row-major: the least a, then the least k)
            found = torch.isfinite(least[..., 0])
            agent, zone = pair // k, pair % k
            hit = found[..., None] & (torch.arange(a, device=costs.device) == agent[..., None])
            choice = torch.where(hit, zone[..., None], choice)
            taken = taken | (found[..., None] & (zone_index == zone[..., None]))
        least = open_costs.amin(-1, keepdim=True)
        nearest = torch.where(open_costs == least, zone_index, k).amin(-1)
        choice = torch.where((choice < 0) & torch.isfinite(least[..., 0]), nearest, choice)
        return choice, choice < 0

    def _assign(self, due):
        """The zones, the choice and the wanted labels of the envs marked in ``due`` (n_env, 1) bool; the others keep theirs."""
        a = self.core.n_agents
        self.clusters.update(due)
        self.around.update(self.core.agents.positions, due.expand(-1, a).contiguous())
        self.zones.update(due.expand(-1, a).contiguous())
        choice, none = self.choose(self.zones.least)
        roots = self.zones.roots.gather(-1, choice.clamp(min=0)[..., None])[..., 0]      # ((n_env, n_agent): F = A fields, one an agent)
        self.choice.copy_(torch.where(due, choice, self.choice))
        self._wanted.copy_(torch.where(due, torch.where(none, -1, roots).int(), self._wanted))

    def __call__(self, reset=None):
        """Refreshes the envs that are due: those with an agent marked in the (n_env, n_agent) bool ``reset`` - it started over, the
        env's map is empty again - and those that have taken a multiple of ``refresh`` steps since. Call once per step, after the
        maps were marked."""
        if reset is not None:
            self._steps.masked_fill_(reset.any(-1), 0)
        due = (self._steps % self.refresh == 0)[:, None]
        self._steps += 1
        self.due = due                                  # ((n_env, 1) bool: which envs were due at this call)
        self._assign(due)
        self.clusters.masks(labels=self._wanted, out=self.masks)
        self._refresh_unseen()
        self.own.update(due.expand(-1, self.core.n_agents).contiguous())
        self.fields.update(due)
        return self.own

    def distance(self):
        """(n_env, n_agent): how far every agent has to walk to the nearest unseen floor of its cluster (of the env, without one);
        +inf where there is none it can reach."""
        positions = self.core.agents.positions
        return Frontiers.fallback(self.own.at(positions), self.fields.at(positions, goal=self._field))

    def waypoints(self, lookahead=16):
        """(n_env, n_agent, 2): where every agent should head for now; NaN where :meth:`distance` is +inf."""
        positions = self.core.agents.positions
        return Frontiers.fallback(self.own.waypoints(positions, lookahead=lookahead),
                                  self.fields.waypoints(positions, goal=self._field, lookahead=lookahead))


class Idleness:

    def __init__(self, core, grid, max_range=10., shared=False, threshold=64, countable=None):
        """Floor idleness: how long ago every cell of the nav grid was last under one of an agent's depth rays, and a reward for
        looking again at floor that was left alone (:func:`cuda.age_maps`; no counterpart in the reference) - what patrol,
        surveillance and search tasks are made of, and unlike :class:`Coverage` never used up. ``grid`` is the scenery's
        :func:`cuda.nav_grid`; rays are followed for at most ``max_range`` metres; a countable cell (default: the grid's free
        cells) is stale once it has not been seen for ``threshold`` steps. Every agent has a map of its own; ``shared=True``
        gives an env's agents ONE map, which any of them starting over clears, and each of them the map's whole reward. One
        launch behind the render's, nothing waits for the host; the maps' clocks live on the device."""
        self.core, self.grid = core, grid
        self.max_range, self.shared, self.threshold = float(max_range), bool(shared), int(threshold)
        n, s = core.n_envs, 1 if shared else core.n_agents
        self.ages = cuda.age_maps(grid, s, countable, self.threshold)
        self.space = spaces.MultiVector(core.n_agents, 2)
        self._slot = torch.zeros((n, core.n_agents), dtype=torch.int32, device=core.device) if shared else None
        self._sweep = cuda.Sweep(torch.zeros((n, s), dtype=torch.int32, device=core.device), torch.zeros((n, s), dtype=torch.int32, device=core.device),
                                 torch.zeros((n, s), dtype=torch.int64, device=core.device))
        self._area = torch.tensor(grid.cell, dtype=torch.float32, device=core.device)**2

    def _per_agent(self, t):
        return t.expand(-1, self.core.n_agents) if self.shared else t

    def __call__(self, frame, reset=None):
        """(n_env, n_agent) float32: ``(idle - swept).float()*cell**2/threshold`` over the countable cells ``frame`` - a render of
        the agents as they stand, with its ``distances`` - passes over: ``swept`` how many they are, ``idle`` the steps since each
        was last seen, summed (:class:`cuda.Sweep`). Floor seen again a step later pays nothing; floor left alone for
        ``threshold`` steps pays its area in square metres, less a ``threshold``-th; floor never seen pays by the map's clock.
        ``reset`` (n_env, n_agent) bool: the agents that started over this step; their maps and clocks are cleared first."""
        if reset is not None and self.shared:
            reset = reset.any(-1, keepdim=True)
        sweep = self.ages.mark_render(self.core.agents, frame, slot=self._slot, max_range=self.max_range, reset=reset, out=self._sweep)
        return self._per_agent((sweep.idle - sweep.swept).float()*self._area/self.threshold)

    def mean_age(self):
        """(n_env, n_agent) float32: the mean age, in steps, of the countable floor of each agent('s map)."""
        return self._per_agent(self.ages.mean_age())

    def oldest(self):
        """(n_env, n_agent) int32: the worst age, in steps, of the countable floor of each agent('s map)."""
        return self._per_agent(self.ages.oldest)

    def observation(self):
        """(n_env, n_agent, 2): ``min(mean_age/threshold, 1)`` and ``min(oldest/threshold, 1)``."""
        both = torch.stack([self.mean_age(), self.oldest().float()], -1)
        return (both/self.threshold).clamp(max=1.)

    def state(self, e=0):
        """(S, ny, nx) float32: a copy of the ages in env ``e``'s maps, row 0 at the lowest y."""
        return torch.stack([self.ages.age_image(e, s) for s in range(self.ages.n_maps)]).clone()


class Patrols:

    def __init__(self, core, idleness, refresh=8, cost=None):
        """How far every agent has to walk to the nearest stale floor of its map, and which way (no counterpart in the
        reference): :class:`Frontiers`' interface - so :class:`PathFollower` takes it unchanged - over the stale cells of an
        :class:`Idleness`' maps (:meth:`cuda.AgeMaps.stale_fields`), one field per map. A field is recomputed every ``refresh``
        steps of its agent and when the agent starts over; with ``idleness.shared`` an env has one field, which all its agents
        follow. An agent whose map holds no stale cell gets NaN. ``cost``: a cost layer as :func:`cuda.cost_fields` takes it.
        Nothing waits for the host: which fields are due is decided on the device, so a call can sit in a HIP graph."""
        self.core, self.idleness, self.refresh = core, idleness, int(refresh)
        if self.refresh < 1:
            raise RuntimeError(f'refresh must be a positive integer; got {refresh}')
        self._steps = torch.zeros((core.n_envs, core.n_agents), dtype=torch.long, device=core.device)
        self._field = idleness._slot                    # (n_env, n_agent) zeros when the map is shared, else None: agent k field k
        self.cost = cost
        self.fields = idleness.ages.stale_fields(cost=cost)

    def __call__(self, reset=None):
        """Recomputes the fields that are due: those of the agents marked in the (n_env, n_agent) bool ``reset`` and those whose
        agent has taken a multiple of ``refresh`` steps since. Call once per step, after the maps were marked and surveyed."""
        if reset is not None:
            self._steps.masked_fill_(reset, 0)
        due = self._steps % self.refresh == 0
        self._steps += 1
        self.due = due                                  # ((n_env, n_agent) bool: whose field was due at this call)
        if self.idleness.shared:
            due = due.any(-1, keepdim=True)
        self.fields.update(due)
        return self.fields

    def distance(self):
        """(n_env, n_agent): how far every agent has to walk to the nearest stale floor; +inf where there is none it can reach."""
        return self.fields.at(self.core.agents.positions, goal=self._field)

    def waypoints(self, lookahead=16):
        """(n_env, n_agent, 2): where every agent should head for now to walk to the nearest stale floor; NaN where
        :meth:`distance` is +inf."""
        return self.fields.waypoints(self.core.agents.positions, goal=self._field, lookahead=lookahead)


class BestViews:

    def __init__(self, core, coverage, n_candidates=16, max_range=None, band=(.25, 3.), refresh=8, seed=0):
        """Next-best-view goals over a :class:`Coverage` (no counterpart in the reference): :class:`Frontiers`' interface - so
        :class:`PathFollower` takes it unchanged - with a goal chosen by what standing there would REVEAL instead of the nearest
        unseen cell, be that a sliver behind a pillar or the doorway of an unseen room. It holds a :class:`Frontiers` of the same
        coverage, and for the agents that are due by its device-side rule (every ``refresh`` steps, and when they start over):

        * draws ``n_candidates`` cells within ``band`` metres (walking) of floor the agent's map has not seen -
          :func:`cuda.cell_draws` on the frontier field with ``lo`` and ``hi`` - so every candidate is reachable from unseen floor
          that counts, hence from the agent;
        * measures the walk to each with a masked :func:`cuda.distance_fields` round the agents and its ``at``;
        * scores each by :func:`cuda.view_fields` ``(..., unseen=coverage.maps, slot=..., store=False).gains``: the countable cells
          in sight of it, within ``max_range`` (default the coverage's), that the agent's map lacks;
        * takes a masked :func:`cuda.distance_fields` of the goal :meth:`choose` picks.

        An agent without a candidate worth walking to follows its frontier field, as under :class:`Frontiers`. Nothing waits for
        the host: everything is driven by masks, so a call can sit in a HIP graph once a first call outside it has made the
        tensors."""
        self.core, self.coverage = core, coverage
        self.n_candidates, self.seed = int(n_candidates), int(seed)
        self.max_range = float(coverage.max_range if max_range is None else max_range)
        self.band = (float(band[0]), float(band[1]))
        from .nav import DRAW_MAX_DRAWS
        if not 1 <= self.n_candidates <= DRAW_MAX_DRAWS:
            raise RuntimeError(f'n_candidates must be in 1..{DRAW_MAX_DRAWS}; got {n_candidates}')
        if not 0 <= self.band[0] <= self.band[1]:
            raise RuntimeError(f'the band must be 0 <= lo <= hi; got {band}')
        self.frontiers = Frontiers(core, coverage, refresh)
        n, a, k = core.n_envs, core.n_agents, self.n_candidates
        agent = torch.arange(a, dtype=torch.int32, device=core.device)[None, :, None].expand(n, a, k).reshape(n, -1).contiguous()
        self._agent = agent                             # (n_env, n_agent*K): the agent - its field, its map - of each candidate
        self._slot = torch.zeros_like(agent) if coverage.shared else agent
        self._goal = core.agents.positions.clone()
        #: (n_env, n_agent) bool: the agent found no candidate with a finite walk and a positive gain, and follows the frontier
        self.none = core.agent_full(True)
        self._draws = self._around = self._views = self._fields = None
        self.gains = self.distances = None

    #: (n_env, n_agent, 2): every agent's goal (where :attr:`none`: the spot it stood on when it found none)
    goals = property(lambda self: self._goal)
    #: (n_env, n_agent, K, 2): the candidates of the last draw of every agent (NaN where its band held no cell)
    candidates = property(lambda self: self._draws.points)
    #: the :class:`cuda.DistanceFields` of the goals
    fields = property(lambda self: self._fields)

    @staticmethod
    def choose(gains, distances, d0=1.):
        """The rule, a pure function: ``gains`` (..., K) integers and ``distances`` (..., K) -> ((...) int64: the first candidate
        with the largest ``gains/(distances + d0)`` among those with a finite distance and a positive gain; (...) bool ``none``:
        there is no such candidate - the index is 0 then)."""
        k = gains.shape[-1]
        valid = torch.isfinite(distances) & (gains > 0)
        score = torch.where(valid, gains.float()/(distances + d0), torch.full_like(distances, -1.))
        best = valid & (score == score.amax(-1, keepdim=True))
        order = torch.arange(k, device=gains.device).expand(best.shape)
        first = torch.where(best, order, torch.full_like(order, k)).amin(-1)
        none = ~valid.any(-1)
        return torch.where(none, torch.zeros_like(first), first), none

    def __call__(self, reset=None):
        """Refreshes the frontier fields and, for the agents that are due, the goals. Call once per step, after the maps were
        marked. ``reset`` (n_env, n_agent) bool: the agents that started over."""
        c, grid = self.core, self.coverage.grid
        n, a, k = c.n_envs, c.n_agents, self.n_candidates
        fields = self.frontiers(reset)
        due = self.frontiers.due.contiguous()
        here = c.agents.positions
        if self._draws is None:
            source = cuda.cell_layer(fields, field=self.frontiers._field)
            self._draws = cuda.cell_draws(grid, source, a, k, lo=self.band[0], hi=self.band[1], seed=self.seed, mask=due)
        else:
            self._draws.again(mask=due)
        points = self._draws.points.reshape(n, a*k, 2)
        self._around = cuda.distance_fields(grid, here, mask=due, out=self._around)
        distances = self._around.at(points, goal=self._agent).reshape(n, a, k)
        each = due[:, :, None].expand(n, a, k).reshape(n, a*k).contiguous()
        if self._views is None:
            self._views = cuda.view_fields(grid, c.scenery, points, self.max_range, unseen=self.coverage.maps, slot=self._slot, store=False, mask=each)
        else:
            self._views.update(each)
        gains = self._views.gains.reshape(n, a, k)
        index, none = self.choose(gains, distances)
        goal = self._draws.points.gather(2, index[..., None, None].expand(-1, -1, 1, 2)).squeeze(2)
        goal = torch.where(none[..., None], here, goal)
        self._goal.copy_(torch.where(due[..., None], goal, self._goal))
        self.none.copy_(torch.where(due, none, self.none))
        self.gains, self.distances = gains, distances
        self._fields = cuda.distance_fields(grid, self._goal, mask=due, out=self._fields)
        return self._fields

    def waypoints(self, lookahead=16):
        """(n_env, n_agent, 2): where every agent should head for now: towards its goal (:meth:`cuda.DistanceFields.waypoints`),
        or, where it has :attr:`none`, towards the nearest unseen floor (:meth:`Frontiers.waypoints`)."""
        own = self._fields.waypoints(self.core.agents.positions, lookahead=lookahead)
        return torch.where(self.none[..., None], self.frontiers.waypoints(lookahead), own)


class PathFollower:

    def __init__(self, core, goals, lookahead=16, cone=45., speed=2.):
        """The shortest-path expert over a :class:`Goals` (or a :class:`Frontiers` or a :class:`BestViews`: anything with ``waypoints(lookahead)``): every agent turns towards its waypoint - the furthest of the next
        ``lookahead`` cells of its shortest path that it can see (:meth:`Goals.waypoints`) - and walks once that lies within
        ``cone`` degrees of straight ahead. Something to imitate, to fill a replay buffer with, to score a learned policy
        against (Habitat's ``ShortestPathFollower``; no counterpart in the reference). Other agents are not obstacles to
        it: the paths are the building's. One launch and a few tensor ops; nothing waits for the host.

        The paths keep a POINT clear of the walls, and an agent is a disc as wide as that clearance that physics stops dead
        - velocity and spin - whenever it touches anything. So two things are added to the plain rule (:meth:`choose`):
        under momentum the agent stops accelerating once it is faster than ``speed`` times the waypoint's distance (a
        waypoint is near exactly where a corner hides the rest of the path); and an agent found at a dead stop tries a
        sidestep, the other sidestep, a step back and a step forward in turn until one of them frees it - pressed against a
        wall it can no longer even turn. The module counts the dead stops, so call it once per step."""
        self.core, self.goals = core, goals
        self.lookahead, self.cone, self.speed = int(lookahead), float(cone), speed
        self._blocked = torch.zeros((core.n_envs, core.n_agents), dtype=torch.long, device=core.device)

    #: what an agent at a dead stop tries, in turn: strafe right, strafe left, back, forward
    ESCAPE = (3, 4, 2, 1)
    #: the least speed limit, m/s: one forward action from rest under :class:`MomentumMovement` stays below it
    CREEP = .6

    @staticmethod
    def choose(local, cone=45., velocity=None, blocked=None, speed=2.):
        """The rule, a pure function of its arguments. ``local`` (..., 2): the waypoint's offset in the agent's frame (x to the
        right, y ahead, as :func:`to_local_frame` gives it): forward (1) when ``y > 0`` and ``|x| <= y*tan(cone)``; otherwise
        turn left (5) when ``x < 0``, else turn right (6). ``velocity`` (..., 2), optional: the agent's velocity in its own
        frame, m/s - forward becomes nothing (0) while the speed ahead exceeds ``max(speed*|local|, CREEP)``. ``blocked``
        (...) integers, optional: for how many decisions in a row the agent has been at a dead stop - where positive, the
        action is ``ESCAPE[(blocked - 1) % 4]`` instead. Nothing (0) where the waypoint is NaN. Returns (...) int64, the
        movement modules' actions."""
        x, y = local[..., 0], local[..., 1]
        ahead = (y > 0) & (x.abs() <= y*float(np.tan(np.deg2rad(cone))))
        actions = torch.where(ahead, 1, torch.where(x < 0, 5, 6))
        if velocity is not None and speed is not None:
            limit = (speed*local.norm(dim=-1)).clamp(min=PathFollower.CREEP)
            actions = torch.where(ahead & (velocity[..., 1] > limit), 0, actions)
        if blocked is not None:
            turn = (blocked - 1) % 4                                    # (scalars only: nothing here may copy from the host)
            e0, e1, e2, e3 = PathFollower.ESCAPE
            escape = torch.where(turn == 0, e0, torch.where(turn == 1, e1, torch.where(turn == 2, e2, e3)))
            actions = torch.where(blocked > 0, escape, actions)
        return torch.where(torch.isnan(x) | torch.isnan(y), 0, actions)

    def __call__(self):
        """``arrdict(actions=(n_env, n_agent) int64)``: the decision for the agents as they stand."""
        agents = self.core.agents
        still = (agents.velocity == 0).all(-1) & (agents.angvelocity == 0)
        self._blocked.copy_(torch.where(still, self._blocked + 1, torch.zeros_like(self._blocked)))
        local = to_local_frame(agents.angles, self.goals.waypoints(self.lookahead) - agents.positions)
        velocity = to_local_frame(agents.angles, agents.velocity)
        return arrdict.arrdict(actions=self.choose(local, self.cone, velocity, self._blocked, self.speed))


class LookAhead:

    def __init__(self, core, goals, mover, horizon=8, switch=2, stop_cost=.5, fallback=None, others='rest'):
        """A look-ahead expert with :class:`PathFollower`'s call interface (a local planner in the style of the dynamic-window
        approach; no counterpart in the reference): every agent rolls the plans ``cuda.plans(n_actions, horizon, switch)`` -
        "action i for ``switch`` steps, then action j" - through the physics step itself (``mover.rollouts``, with the env's other
        agents as obstacles at rest when there are any), values the pose each plan ends on by the walking distance from there
        to its goal (``goals.fields.at``: a :class:`Goals`, a :class:`SampledGoals`, a :class:`Routes` - anything with
        ``.fields``), adds ``stop_cost`` metres for every step the plan was stopped dead at, and takes the first action of the
        cheapest plan - the lowest-numbered of several (:meth:`choose`). Where no plan ends on a pose with a finite value, the
        agent does what ``fallback`` does (default: a :class:`PathFollower` on the same goals). Unlike the follower, which plans
        for a point, it knows what physics does to the disc. One rollout launch, one ``at`` and a few tensor ops; the module
        keeps the launch's buffers and nothing waits for the host: a call can sit in a HIP graph. The fallback counts dead
        stops, so call the module once per step.

        ``others='repeat'``: the env's other agents are not at rest - every one of them is taken to repeat, for the whole
        horizon, the action this module returned for it at its previous call (the no-op, 0, before the first), all of them
        moving and meeting together as in the step itself (``mover.rollouts(plans, others=base)``). ``base`` is
        an (n_env, n_agent, H) buffer written in place, so the call still captures."""
        if others not in ('rest', 'repeat'):
            raise RuntimeError(f"others must be 'rest' or 'repeat'; got {others!r}")
        self.core, self.goals, self.mover = core, goals, mover
        self.horizon, self.switch, self.stop_cost = int(horizon), switch, float(stop_cost)
        self.fallback = PathFollower(core, goals) if fallback is None else fallback
        n_actions = mover._table.shape[0]
        #: (K, H) int64: the plans every agent rolls
        self.plans = cuda.plans(n_actions, self.horizon, switch, device=core.device)
        n, a, k = core.n_envs, core.n_agents, self.plans.shape[0]
        self._agent = torch.arange(a, dtype=torch.int32, device=core.device)[None, :, None].expand(n, a, k).reshape(n, -1).contiguous()
        self._others = 'rest' if a > 1 else None
        #: (n_env, n_agent, H) int64 with ``others='repeat'``: what every agent is taken to do when it is one of the others
        self.base = torch.zeros((n, a, self.horizon), dtype=torch.int64, device=core.device) if others == 'repeat' else None
        self._rolled = None
        #: (n_env, n_agent, K): what the last call's plans were worth (None before the first)
        self.values = None

    #: the :class:`cuda.Rollouts` of the last call (None before the first)
    rolled = property(lambda self: self._rolled)

    @staticmethod
    def choose(values, stops, plans, stop_cost):
        """The rule, a pure function: ``values`` (..., K) floats, ``stops`` (..., K) integers, ``plans`` (K, H) or (..., K, H) ->
        ((...) int64: the first action of the lowest-numbered plan of least ``values + stop_cost*stops``, a NaN or +inf value
        scoring +inf; (...) bool ``none``: every plan scores +inf - the action is plan 0's then)."""
        k = values.shape[-1]
        score = values + stop_cost*stops.to(values.dtype)
        score = torch.where(torch.isnan(score), torch.full_like(score, float('inf')), score)
        least = score.amin(-1, keepdim=True)
        order = torch.arange(k, device=values.device).expand(score.shape)
        index = torch.where(score == least, order, torch.full_like(order, k)).amin(-1)
        none = torch.isinf(least[..., 0]) & (least[..., 0] > 0)
        first = plans[..., 0]
        action = first[index] if first.ndim == 1 else first.gather(-1, index[..., None]).squeeze(-1)
        return action, none

    @staticmethod
    def repeat(base, actions):
        """The buffer rule of ``others='repeat'``, in place: ``base`` (..., H) <- ``actions`` (...) at every step. Returns ``base``."""
        return base.copy_(actions[..., None].expand_as(base))

    def __call__(self):
        """``arrdict(actions=(n_env, n_agent) int64)``: the decision for the agents as they stand."""
        n, a, k = self.core.n_envs, self.core.n_agents, self.plans.shape[0]
        self._rolled = self.mover.rollouts(self.plans, others=self._others if self.base is None else self.base, out=self._rolled)
        self.values = self.goals.fields.at(self._rolled.positions.view(n, a*k, 2), goal=self._agent).view(n, a, k)
        action, none = self.choose(self.values, self._rolled.stops, self.plans, self.stop_cost)
        actions = torch.where(none, self.fallback().actions, action)
        if self.base is not None:
            self.repeat(self.base, actions)
        return arrdict.arrdict(actions=actions)


class SPL:

    def __init__(self, core, goals, reach=256):
        """Success weighted by path length (Anderson et al., "On evaluation of embodied navigation agents"; no counterpart in the
        reference) over a :class:`Goals` or a :class:`SampledGoals` - anything with ``.fields`` and ``.goals``: per episode
        ``arrived * shortest / max(walked, shortest)``. ``shortest`` is the length of the pulled path
        (:meth:`cuda.DistanceFields.pulled`, with ``reach``) from where the agent stood when its episode began to its goal - the
        any-angle length, not the grid's 8-direction one, which overstates open floor by up to 8 % and would let a walker
        score above 1; ``walked`` is the sum of the agent's moves since. Pulling is greedy, so ``shortest`` is an upper bound on
        the true shortest walk, and an agent that finds a shorter one scores 1, not more. Call once per step, after the goals
        module; a call is one masked launch and a few tensor ops, nothing waits for the host: it can sit in a HIP graph."""
        self.core, self.goals, self.reach = core, goals, int(reach)
        self.walked = torch.zeros((core.n_envs, core.n_agents), dtype=torch.float32, device=core.device)
        self._last = torch.zeros((core.n_envs, core.n_agents, 2), dtype=torch.float32, device=core.device)
        self._pulled = None

    #: (n_env, n_agent): the pulled length from where each agent's episode began to its goal (+inf: no path; None before the
    #: first call)
    shortest = property(lambda self: None if self._pulled is None else self._pulled.lengths)

    @staticmethod
    def score(shortest, walked, arrived, ended):
        """The rule, a pure function of its arguments, all (...): NaN where no episode ``ended`` or ``shortest`` is not finite;
        0 for an episode that ended without having ``arrived``; otherwise ``shortest / max(walked, shortest)``."""
        ratio = shortest/torch.maximum(walked, shortest)
        value = torch.where(arrived, ratio, torch.zeros_like(ratio))
        return torch.where(ended & torch.isfinite(shortest), value, torch.full_like(ratio, float('nan')))

    def __call__(self, reset, arrived, ended):
        """(n_env, n_agent) float32: the score of the episodes that ``ended`` at this step, NaN for everyone else. ``reset``
        (n_env, n_agent) bool: who began a new episode at this step - their shortest path is pulled from where they stand
        now, to the goal they were just given, and they have walked nothing; ``arrived``: who is at the goal."""
        positions = self.core.agents.positions
        reset = reset.contiguous()
        self._pulled = self.goals.fields.pulled(positions, reach=self.reach, max_points=2, mask=reset, out=self._pulled)
        self.walked.add_((positions - self._last).norm(dim=-1)).masked_fill_(reset, 0.)
        self._last.copy_(positions)
        return self.score(self._pulled.lengths, self.walked, arrived, ended)
