"""Floor coverage: every agent is rewarded for the floor its depth rays pass over for the first time since it started over, in
square metres, and its episode ends when it has seen ``complete`` of the floor it can walk to - or by its lifespan. No
counterpart in the reference, whose Explorer rewards wall texels; the maps are those of :func:`megastep_amd.cuda.seen_maps`.

A step has no host synchronisation and draws no random numbers of its own besides :class:`~megastep_amd.modules.RandomLifespans`',
so it can be captured in a HIP graph (:class:`megastep_amd.graphs.GraphedStep`)."""
import torch

from ... import arrdict, core, cubicasa, cuda, dotdict, modules, scene
from .explorer import _plan_workers


def reachable(grid, points):
    """The grid's free cells a walk from ``points`` (n_env, 2) reaches, as a uint8 mask in ``grid.free``'s layout: the cells on
    which the distance field of the point is finite."""
    fields = cuda.distance_fields(grid, points[:, None, :].float().contiguous())
    return (torch.isfinite(fields.values[:len(grid.free)]) & grid.free.bool()).to(torch.uint8)


class FloorCoverage:

    def __init__(self, n_envs, n_agents=1, *args, device='cuda', geometries=None, cell=.125, max_range=10., complete=.9, max_lifespan=512,
                 n_spawns=100, shared=False, local_map=None, slide=False, **kwargs):
        """``cell``: the nav grid's cell size; ``max_range``: how far a ray is followed, metres; ``complete``: the share of the
        floor that ends an episode; ``max_lifespan``: episodes end after a random number of steps up to this
        (:class:`~megastep_amd.modules.RandomLifespans`); ``shared``: see :class:`~megastep_amd.modules.Coverage`; ``local_map``:
        ``True``, or a dict of :class:`~megastep_amd.modules.LocalMap`'s keyword arguments, adds ``obs['map']`` and ``obs_space['map']`` (read them by key: ``.map`` is the tree's method) - the egocentric
        window of what the agent has seen so far, taken after the frame's marks; without it the env makes no such launch.

        The floor that counts is what can be walked to from the env's first spawn point: the free margin the grid keeps round
        the building, and rooms without a door, are never in the denominator. ``slide``: ``True`` or ``dict(bounce=.05)`` - the
        agents slide along what they hit instead of stopping dead (:func:`~megastep_amd.cuda.physics`)."""
        if geometries is None:
            geometries = cubicasa.sample(n_envs, workers=_plan_workers(), context='subprocess')
        self.core = core.Core(scene.scenery(geometries, n_agents, device=device), *args, res=4*64, fov=130, **kwargs)
        c = self.core
        self.device = c.device
        self.complete = float(complete)

        self._mover = modules.MomentumMovement(c, slide=slide or None)
        self._respawner = modules.RandomSpawns(geometries, c, n_spawns=n_spawns)
        self._lifespans = modules.RandomLifespans(c, max_lifespan)
        self._rgb = modules.RGB(c, subsample=4)
        self._depth = modules.Depth(c, subsample=4)
        self.grid = cuda.nav_grid(c.scenery, cell, config=c.config)
        countable = reachable(self.grid, self._respawner._spawns.positions[:, 0, 0])
        self._coverage = modules.Coverage(c, self.grid, max_range=max_range, shared=shared, countable=countable)
        self.action_space = self._mover.space
        self.obs_space = dotdict.dotdict(rgb=self._rgb.space, d=self._depth.space, coverage=self._coverage.space)
        self._local = None
        if local_map:
            self._local = modules.LocalMap(c, self._coverage, **(local_map if isinstance(local_map, dict) else {}))
            self.obs_space['map'] = self._local.space     # (by key: `.map` is the tree's method)

        self._over = c.agent_full(True)                 # who starts over at the next step
        self._episodes = torch.zeros((c.n_envs, c.n_agents), dtype=torch.long, device=c.device)
        self._fresh = c.agent_full(False)               # who started over since the expert was last asked
        self._frontiers = self._follower = None         # made when the expert is first asked: they cost nothing until then
        self._views = self._views_follower = None
        self._split = self._split_follower = self.territories = None
        self._assign = self._assign_follower = None

    #: the :class:`~megastep_amd.cuda.SeenMaps`
    maps = property(lambda self: self._coverage.maps)

    def _respawn(self, over):
        """The respawn of the agents marked, as a request the physics launch carries out after its step: each agent walks its
        own (randomly ordered) spawn table, one entry per episode."""
        spawns = self._respawner._spawns
        choices = self._episodes % spawns.angles.shape[2]
        request = dict(mask=over.contiguous(), choices=choices.contiguous(), positions=spawns.positions, angles=spawns.angles, after=True)
        self._episodes += over
        return request

    def _world(self, reset):
        frame = modules.render(self.core, observers=(self._rgb, self._depth), fields=('distances',))
        reward = self._coverage(frame, reset)           # (the maps of those who started over are cleared by the same launch)
        self._fresh |= reset
        ended = self._coverage.fraction() >= self.complete
        self._over.copy_(self._lifespans(ended))
        obs = arrdict.arrdict(rgb=self._rgb(frame), d=self._depth(frame), coverage=self._coverage.observation())
        if self._local is not None:
            obs['map'] = self._local()
        return arrdict.arrdict(obs=obs, reset=reset.any(-1), reward=reward)

    @torch.no_grad()
    def reset(self):
        everyone = self.core.agent_full(True)
        modules._respawn(self.core.agents, {**self._respawn(everyone), 'after': False})
        return self._world(everyone)

    @torch.no_grad()
    def step(self, decision):
        """Moves the agents; those whose episode ended at the last step start a new one instead (a new spot, an empty map).
        ``reset`` (n_env,): an agent of the env started over; ``reward`` (n_env, n_agent): square metres of floor first seen."""
        over = self._over.clone()
        self._mover(decision, respawn=self._respawn(over))
        return self._world(over)

    @torch.no_grad()
    def expert(self, kind='frontier'):
        """``arrdict(actions=(n_env, n_agent))``: what the frontier follower does in the current state - every agent towards the
        waypoint of the nearest floor its map has not seen (:class:`~megastep_amd.modules.Frontiers` under a
        :class:`~megastep_amd.modules.PathFollower`); nothing (0) where nothing is left to see. Nothing waits for the host:
        ``env.step(env.expert())`` can sit in one graph, once a first call outside it has made the fields. The fields are
        refreshed, and the follower counts the steps an agent has been stuck, on every call: ask once per step.
        ``kind='views'``: the next-best-view follower instead - every agent towards the candidate standpoint that would reveal
        the most unseen floor per metre walked (:class:`~megastep_amd.modules.BestViews`). ``kind='split'``, for ``shared=True``
        with several agents: the frontier follower over ``Frontiers(territories=Territories(...))`` - every agent towards the
        nearest unseen floor of the part of the plan it is the nearest agent to, so that an env's agents part ways.
        ``kind='assign'``, for ``shared=True``: the frontier follower over :class:`~megastep_amd.modules.Assignments` - every agent
        towards a frontier cluster of its own, the clusters dealt to the agents by walking distance. Ask one kind per step."""
        if kind not in ('frontier', 'views', 'split', 'assign'):
            raise RuntimeError(f"kind must be 'frontier', 'views', 'split' or 'assign'; got {kind!r}")
        if kind == 'assign':
            if not self._coverage.shared:
                raise RuntimeError("expert('assign') needs shared=True: agents with a map each have a frontier each already")
            if self._assign is None:
                self._assign = modules.Assignments(self.core, self._coverage)
                self._assign_follower = modules.PathFollower(self.core, self._assign, cone=15.)
            self._assign(self._fresh)
            self._fresh.zero_()
            return self._assign_follower()
        if kind == 'split':
            if not self._coverage.shared:
                raise RuntimeError("expert('split') needs shared=True: agents with a map each have a frontier each already")
            if self._split is None:
                self.territories = modules.Territories(self.core, self.grid)
                self._split = modules.Frontiers(self.core, self._coverage, territories=self.territories)
                self._split_follower = modules.PathFollower(self.core, self._split, cone=15.)
            self._split(self._fresh)
            self._fresh.zero_()
            return self._split_follower()
        if kind == 'views':
            if self._views is None:
                self._views = modules.BestViews(self.core, self._coverage)
                self._views_follower = modules.PathFollower(self.core, self._views, cone=15.)
            self._views(self._fresh)
            self._fresh.zero_()
            return self._views_follower()
        if self._frontiers is None:
            self._frontiers = modules.Frontiers(self.core, self._coverage)
            self._follower = modules.PathFollower(self.core, self._frontiers, cone=15.)
        self._frontiers(self._fresh)
        self._fresh.zero_()
        return self._follower()

    def state(self, e=0):
        state = arrdict.arrdict(core=self.core.state(e), rgb=self._rgb.state(e), d=self._depth.state(e), seen=self._coverage.state(e),
                                fraction=self._coverage.fraction()[e].clone(), lifespan=self._lifespans.state(e))
        if self._local is not None:
            state['map'] = self._local.state(e)
        return state
