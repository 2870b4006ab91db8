"""Forage: every env holds ``n_items`` items; an agent that comes within reach of one takes it, earns its kind's value, and the
item returns a while later on a free cell drawn on the device. The agents SEE the items: they are drawn into the camera's RGB-D
fan (:func:`megastep_amd.cuda.overlay_items`, a pass of its own over the planes :func:`~megastep_amd.cuda.render` wrote) and the
nearest visible ones are listed as percepts. No counterpart in the reference, whose two envs are an explorer and a deathmatch;
foraging and collection are the most common task family of a simulator of this kind.

The observations come from the full-resolution frame through :class:`~megastep_amd.modules.RGB`'s and
:class:`~megastep_amd.modules.Depth`'s tensor-op path: THE KERNEL-POOLED PATH CANNOT SEE ITEMS - the render kernel pools its own
rays before the items are drawn - so this env does not ask for it.

A step has no host synchronisation and draws no random numbers of its own besides :class:`~megastep_amd.modules.RandomLifespans`',
so it can be captured in a HIP graph (:class:`megastep_amd.graphs.GraphedStep`)."""
import torch

from ... import arrdict, core, cubicasa, cuda, dotdict, modules, scene
from .explorer import _plan_workers


class _Nearest:
    """What the expert's :class:`~megastep_amd.modules.PathFollower` follows: the shortest walk to the nearest item."""

    def __init__(self, env):
        self.env = env
        self.seeds = cuda.point_marks(env.grid, env.items.positions)
        self.fields = cuda.seeded_fields(env.grid, self.seeds.marks, 1)
        self._fresh = True

    def waypoints(self, lookahead=16):
        if not self._fresh:
            self.seeds.update()
            self.fields.update()
        self._fresh = False
        return self.fields.waypoints(self.env.core.agents.positions, lookahead=lookahead)


class Forage:

    def __init__(self, n_envs, n_agents=1, n_items=16, *args, values=(1.,), colors=None, radius=.1, reach=None, delay=32, sight=10., k=4,
                 max_lifespan=512, slide=False, device='cuda', geometries=None, cell=.125, seed=0, **kwargs):
        """``n_items``: items an env, of ``len(values)`` kinds worth ``values[kind]`` each (:class:`~megastep_amd.modules.Items`, which
        also takes ``colors``, ``radius``, ``reach``, ``delay`` and ``seed``); ``sight``, ``k``: how far an agent's percepts reach,
        metres, and how many of the nearest visible items they list; ``max_lifespan``: episodes end after a random number of steps
        up to this (:class:`~megastep_amd.modules.RandomLifespans`), and by nothing else; ``cell``: the nav grid's cell size - spawns
        and items are drawn among its free cells. ``slide``: ``True`` or ``dict(bounce=.05)`` - the agents slide along what they hit
        instead of stopping dead (:func:`~megastep_amd.cuda.physics`)."""
        if geometries is None:
            geometries = cubicasa.sample(n_envs, workers=_plan_workers(), context='subprocess')
        self.core = core.Core(scene.scenery(geometries, n_agents, device=device), *args, res=4*64, fov=130, **kwargs)
        c = self.core
        self.device = c.device
        self.sight = float(sight)

        self._mover = modules.MomentumMovement(c, slide=slide or None)
        self._lifespans = modules.RandomLifespans(c, max_lifespan)
        self._rgb = modules.RGB(c, subsample=4)
        self._depth = modules.Depth(c, subsample=4)
        self.grid = cuda.nav_grid(c.scenery, cell, config=c.config)
        self._respawner = modules.SampledSpawns(c, self.grid, seed=seed)
        #: the :class:`~megastep_amd.modules.Items` of the env
        self.items = modules.Items(c, self.grid, n_items, values=values, colors=colors, radius=radius, reach=reach, delay=delay, seed=seed + 1)
        self._percepts = modules.Percepts(c, points=self.items.positions, max_range=self.sight, fov=c.fov, k=k)
        self.action_space = self._mover.space
        self.obs_space = dotdict.dotdict(rgb=self._rgb.space, d=self._depth.space, percepts=self._percepts.space)

        self._ended = c.agent_full(True)                # whose episode ended at the last step
        self._frame = None                              # the step's cuda.Render, items drawn in
        self._nearest = self._follower = None           # made when the expert is first asked: they cost nothing until then

    #: the :class:`~megastep_amd.cuda.Render` of the last step, the items drawn into it, with ``.items`` (None before the first)
    frame = property(lambda self: self._frame)

    def _world(self, ended):
        c = self.core
        reset = ended.any(-1)
        reward = self.items(reset=reset)
        self._frame = self.items.draw(cuda.render(c.scenery, c.agents, out=self._frame))
        frame = modules._frame(self._frame, None)
        self._ended.copy_(self._lifespans())
        obs = arrdict.arrdict(rgb=self._rgb(frame), d=self._depth(frame), percepts=self._percepts())
        return arrdict.arrdict(obs=obs, reset=reset, reward=reward)

    @torch.no_grad()
    def reset(self):
        everyone = self.core.agent_full(True)
        self._respawner(everyone)
        return self._world(everyone)

    @torch.no_grad()
    def step(self, decision):
        """Moves the agents; those whose episode ended at the last step start over on a fresh cell instead, and the items of
        their env are all drawn anew. ``reset`` (n_env,): an agent of the env began a new episode; ``reward`` (n_env, n_agent):
        the value of the items each agent took at this step."""
        ended = self._ended.clone()
        self._mover(decision, respawn=self._respawner.draw(ended, after=True))
        return self._world(ended)

    @torch.no_grad()
    def expert(self):
        """``arrdict(actions=(n_env, n_agent))``: what a privileged player does in the current state - a
        :class:`~megastep_amd.modules.PathFollower` over ``seeded_fields(grid, point_marks(grid, items.positions).marks, 1)``, the
        walking distance to the nearest item, marked and relaxed again every step. Nothing waits for the host:
        ``env.step(env.expert())`` can sit in one graph, once a first call outside it has made the fields. Ask once per step."""
        if self._nearest is None:
            self._nearest = _Nearest(self)
            self._follower = modules.PathFollower(self.core, self._nearest, cone=15.)
        return self._follower()

    def state(self, e=0):
        return arrdict.arrdict(core=self.core.state(e), rgb=self._rgb.state(e), d=self._depth.state(e), items=self.items.state(e),
                               lifespan=self._lifespans.state(e))
