"""Patrol: the agents of an env are rewarded for looking again at floor that has been left alone - per step, for every cell
their depth rays pass over, the steps since it was last seen, in square metres over ``threshold`` - so the task never runs out of
floor the way :class:`~megastep_amd.demo.envs.floorcoverage.FloorCoverage` does: an episode ends by its lifespan only. No
counterpart in the reference; the maps are those of :func:`megastep_amd.cuda.age_maps`.

A step has no host synchronisation and draws no random numbers of its own besides :class:`~megastep_amd.modules.RandomLifespans`',
so it can be captured in a HIP graph (:class:`megastep_amd.graphs.GraphedStep`)."""
import torch

from ... import arrdict, core, cubicasa, cuda, dotdict, modules, scene, spaces
from .explorer import _plan_workers
from .floorcoverage import reachable


class Patrol:

    def __init__(self, n_envs, n_agents=1, *args, device='cuda', geometries=None, cell=.125, max_range=10., threshold=64, shared=True,
                 local_map=False, max_lifespan=512, n_spawns=100, slide=False, **kwargs):
        """``cell``: the nav grid's cell size; ``max_range``: how far a ray is followed, metres; ``threshold``: the steps after
        which floor not looked at is stale; ``shared``: an env's agents keep ONE map (:class:`~megastep_amd.modules.Idleness`) -
        a patrol is a team's; ``max_lifespan``: episodes end after a random number of steps up to this
        (:class:`~megastep_amd.modules.RandomLifespans`), and by nothing else; ``local_map``: ``True``, or a dict of ``size``,
        ``radius`` and ``samples``, adds ``obs['map']`` and ``obs_space['map']`` (read them by key: ``.map`` is the tree's
        method) - the egocentric window round the agent, its heading up, with the channels floor, wall and age: the age of the
        floor in the agent's map over ``threshold``, clamped to 1.

        The floor that counts is what can be walked to from the env's first spawn point, as in
        :class:`~megastep_amd.demo.envs.floorcoverage.FloorCoverage`. ``slide``: ``True`` or ``dict(bounce=.05)`` - the agents
        slide along what they hit instead of stopping dead (:func:`~megastep_amd.cuda.physics`)."""
        if geometries is None:
            geometries = cubicasa.sample(n_envs, workers=_plan_workers(), context='subprocess')
        self.core = core.Core(scene.scenery(geometries, n_agents, device=device), *args, res=4*64, fov=130, **kwargs)
        c = self.core
        self.device = c.device

        self._mover = modules.MomentumMovement(c, slide=slide or None)
        self._respawner = modules.RandomSpawns(geometries, c, n_spawns=n_spawns)
        self._lifespans = modules.RandomLifespans(c, max_lifespan)
        self._rgb = modules.RGB(c, subsample=4)
        self._depth = modules.Depth(c, subsample=4)
        self.grid = cuda.nav_grid(c.scenery, cell, config=c.config)
        countable = reachable(self.grid, self._respawner._spawns.positions[:, 0, 0])
        self._idleness = modules.Idleness(c, self.grid, max_range=max_range, shared=shared, threshold=threshold, countable=countable)
        self.action_space = self._mover.space
        self.obs_space = dotdict.dotdict(rgb=self._rgb.space, d=self._depth.space, idleness=self._idleness.space)
        self._window = self._map = None
        if local_map:
            w = {'size': 32, 'radius': 4., 'samples': 1, **(local_map if isinstance(local_map, dict) else {})}
            self._window = (int(w['size']), float(w['radius']), int(w['samples']))
            age = cuda.cell_layer(self.ages, field=self._idleness._slot)
            self._channels = [cuda.map_channel(self.grid, where=True), cuda.map_channel(self.grid, where=False),
                              cuda.map_channel(age, scale=1/self._idleness.threshold)]
            self.obs_space['map'] = spaces.MultiImage(c.n_agents, 3, self._window[0], self._window[0])     # (by key: `.map` is the tree's method)

        self._over = c.agent_full(True)                 # who starts over at the next step
        self._episodes = torch.zeros((c.n_envs, c.n_agents), dtype=torch.long, device=c.device)
        self._fresh = c.agent_full(False)               # who started over since the expert was last asked
        self._patrols = self._follower = None           # made when the expert is first asked: they cost nothing until then

    #: the :class:`~megastep_amd.cuda.AgeMaps`
    ages = property(lambda self: self._idleness.ages)

    def _respawn(self, over):
        """The respawn of the agents marked, as a request the physics launch carries out after its step: each agent walks its
        own (randomly ordered) spawn table, one entry per episode."""
        spawns = self._respawner._spawns
        choices = self._episodes % spawns.angles.shape[2]
        request = dict(mask=over.contiguous(), choices=choices.contiguous(), positions=spawns.positions, angles=spawns.angles, after=True)
        self._episodes += over
        return request

    def _local(self):
        size, radius, samples = self._window
        views = cuda.agent_views(self.core.agents, size, radius)
        self._map = cuda.local_maps(self.grid, views, size, self._channels, samples=samples, out=self._map)
        return self._map

    def _world(self, reset):
        frame = modules.render(self.core, observers=(self._rgb, self._depth), fields=('distances',))
        reward = self._idleness(frame, reset)           # (the maps of those who started over are cleared by the same launch)
        self._fresh |= reset
        self._over.copy_(self._lifespans())
        obs = arrdict.arrdict(rgb=self._rgb(frame), d=self._depth(frame), idleness=self._idleness.observation())
        if self._window is not None:
            obs['map'] = self._local()
        return arrdict.arrdict(obs=obs, reset=reset.any(-1), reward=reward)

    @torch.no_grad()
    def reset(self):
        everyone = self.core.agent_full(True)
        modules._respawn(self.core.agents, {**self._respawn(everyone), 'after': False})
        return self._world(everyone)

    @torch.no_grad()
    def step(self, decision):
        """Moves the agents; those whose episode ended at the last step start a new one instead (a new spot; its map, or with
        ``shared`` the env's, empty and at tick 0). ``reset`` (n_env,): an agent of the env started over; ``reward``
        (n_env, n_agent): :class:`~megastep_amd.modules.Idleness`'."""
        over = self._over.clone()
        self._mover(decision, respawn=self._respawn(over))
        return self._world(over)

    @torch.no_grad()
    def expert(self):
        """``arrdict(actions=(n_env, n_agent))``: what the patrol follower does in the current state - every agent towards the
        waypoint of the nearest stale floor of its map (:class:`~megastep_amd.modules.Patrols` under a
        :class:`~megastep_amd.modules.PathFollower`); nothing (0) where no floor is stale. Nothing waits for the host:
        ``env.step(env.expert())`` can sit in one graph, once a first call outside it has made the fields. Ask once per step."""
        if self._patrols is None:
            self._patrols = modules.Patrols(self.core, self._idleness)
            self._follower = modules.PathFollower(self.core, self._patrols, cone=15.)
        self._patrols(self._fresh)
        self._fresh.zero_()
        return self._follower()

    def state(self, e=0):
        state = arrdict.arrdict(core=self.core.state(e), rgb=self._rgb.state(e), d=self._depth.state(e), ages=self._idleness.state(e),
                                idleness=self._idleness.observation()[e].clone(), lifespan=self._lifespans.state(e))
        if self._map is not None:
            state['map'] = self._map[e].clone()
        return state
