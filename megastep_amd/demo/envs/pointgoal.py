"""Point-goal navigation: every agent is given a goal it can walk to and is rewarded for its progress along the shortest
path - last step's walking distance minus this step's - plus a bonus when it arrives within ``arrive`` metres, which also
ends its episode. An agent without a goal it can walk to - none of its candidates was reachable, or it has left the cells
the nav grid can see - is flagged (``Goals.stranded``), earns nothing and starts over at the next step. No counterpart in the reference, whose two envs are an explorer and a deathmatch; this is the third env
every user of such a simulator writes, on the distance fields of :func:`megastep_amd.cuda.distance_fields`.

A step has no host synchronisation and draws no random numbers of its own besides :class:`~megastep_amd.modules.RandomLifespans`',
so it can be captured in a HIP graph (:class:`megastep_amd.graphs.GraphedStep`)."""
import torch

from ... import arrdict, core, cubicasa, cuda, dotdict, modules, scene
from .explorer import _plan_workers


def books(before, now, reset, stranded, arrive, bonus):
    """The arithmetic between two frames, all (n_env, n_agent): ``before`` / ``now`` the walking distances to the goal at the
    last step and at this one, ``reset`` who started over this step, ``stranded`` who has no goal. Returns (reward, ended):
    progress - nothing on a reset step, nothing where either distance is not finite - plus ``bonus`` on arrival; an agent's
    episode ends when it arrives (``now < arrive``) or is stranded."""
    arrived = (now < arrive) & ~stranded
    counts = torch.isfinite(before) & torch.isfinite(now) & ~reset
    reward = torch.where(counts, before - now, torch.zeros_like(now)) + bonus*arrived
    return reward, arrived | stranded


class PointGoal:

    def __init__(self, n_envs, n_agents=1, *args, device='cuda', geometries=None, cell=.125, arrive=.5, bonus=1., max_lifespan=512,
                 candidates=8, n_spawns=100, goal_range=None, sampled_spawns=False, one_region=False, margin=None, spl=False, slide=False, panorama=False,
                 **kwargs):
        """``cell``: the nav grid's cell size; ``arrive``: how near the goal counts as there, metres (walking distance);
        ``bonus``: the reward for arriving; ``max_lifespan``: episodes end after a random number of steps up to this
        (:class:`~megastep_amd.modules.RandomLifespans`); ``candidates``: see :class:`~megastep_amd.modules.Goals`.
        ``goal_range=(lo, hi)``: goals drawn on the device at a walking distance of ``lo`` to ``hi`` metres from where the agent
        starts (:class:`~megastep_amd.modules.SampledGoals`) instead of from the spawn table; ``sampled_spawns=True``: spawns
        drawn on the device among the nav grid's free cells (:class:`~megastep_amd.modules.SampledSpawns`) instead of from a
        table made on the host. ``one_region=True`` (with ``sampled_spawns``): the spawns are drawn in the env's largest connected
        space only (:func:`~megastep_amd.cuda.regions` of the grid, once), so all agents of an env can reach one another and no
        spawn lands in a closet. ``margin``: metres; then the expert does not follow the shortest path, which runs along the walls at
        exactly the body's clearance, but the cheapest route (:class:`~megastep_amd.modules.Routes`) over an inflation layer -
        ``inflation_costs(clearance_fields(grid, scenery, margin), margin)`` - that makes a cell dearer the nearer a wall comes
        within ``margin``: it keeps to the middle where there is room. Reward and observations do not change. ``spl=True``: the
        world also carries ``spl`` (n_env, n_agent) - :class:`~megastep_amd.modules.SPL` over the goals: the score of every
        episode that ended at this step, NaN elsewhere - and ``env.spl`` holds the module. ``slide``: ``True`` or
        ``dict(bounce=.05)`` - the agents slide along what they hit instead of stopping dead (:func:`~megastep_amd.cuda.physics`).
        ``panorama=True``: the observations also hold ``pano_rgb`` and ``pano_d`` - a 360-degree ring camera on every agent
        (:class:`~megastep_amd.modules.Panorama`: 256 rays pooled by 4)."""
        if one_region and not sampled_spawns:
            raise RuntimeError('one_region gates the sampled spawns: it needs sampled_spawns=True')
        if geometries is None:
            geometries = cubicasa.sample(n_envs, workers=_plan_workers(), context='subprocess')
        self.core = core.Core(scene.scenery(geometries, n_agents, device=device), *args, res=4*64, fov=130, **kwargs)
        c = self.core
        self.device = c.device
        self.arrive, self.bonus = float(arrive), float(bonus)

        self._mover = modules.MomentumMovement(c, slide=slide or None)
        self._respawner = None if sampled_spawns else modules.RandomSpawns(geometries, c, n_spawns=n_spawns)
        self._lifespans = modules.RandomLifespans(c, max_lifespan)
        self._rgb = modules.RGB(c, subsample=4)
        self._depth = modules.Depth(c, subsample=4)
        self.grid = cuda.nav_grid(c.scenery, cell, config=c.config)
        self.regions = cuda.regions(self.grid) if one_region else None
        if sampled_spawns:
            self._respawner = modules.SampledSpawns(c, self.grid, gate=self.regions.largest_mask() if one_region else None)
        if goal_range is not None:
            self._goals = modules.SampledGoals(c, self.grid, *goal_range)
        else:
            # goals come from the spawn table; one closer than twice `arrive` would be a bonus for nothing
            self._goals = modules.Goals(geometries, c, self.grid, candidates=candidates, min_distance=2*self.arrive,
                                        table=None if sampled_spawns else self._respawner._spawns.positions, n_spawns=n_spawns)
        self.clearance = self.costs = self._routes = None
        if margin is not None:
            if not (margin > 0 and margin < float('inf')):
                raise RuntimeError(f'margin must be a positive number of metres; got {margin}')
            self.clearance = cuda.clearance_fields(self.grid, c.scenery, max_range=float(margin))
            self.costs = cuda.inflation_costs(self.clearance, float(margin))
            self._routes = modules.Routes(c, self.grid, self._goals, self.costs)
        # (under momentum a narrow cone walks a third less far: DESIGN 3.15)
        self._follower = modules.PathFollower(c, self._goals if self._routes is None else self._routes, cone=15.)
        self._lookahead = None                          # (the 'lookahead' expert: made when first asked for)
        self._anticipate = None                         # (the 'anticipate' expert, likewise)
        self.spl = modules.SPL(c, self._goals) if spl else None
        self._pano = modules.Panorama(c) if panorama else None
        self.action_space = self._mover.space
        self.obs_space = dotdict.dotdict(rgb=self._rgb.space, d=self._depth.space, goal=self._goals.space)
        if panorama:
            self.obs_space.update(pano_rgb=self._pano.space, pano_d=self._pano.depth_space)

        self._over = c.agent_full(True)                 # who starts over at the next step
        self._episodes = torch.zeros((c.n_envs, c.n_agents), dtype=torch.long, device=c.device)
        self._distance = torch.full((c.n_envs, c.n_agents), float('inf'), device=c.device)

    def _respawn(self, over):
        """The respawn of the agents marked, as a request the physics launch carries out after its step: each agent walks its
        own (randomly ordered) spawn table, one entry per episode - or, with ``sampled_spawns``, draws a cell."""
        if isinstance(self._respawner, modules.SampledSpawns):
            return self._respawner.draw(over, after=True)
        spawns = self._respawner._spawns
        choices = self._episodes % spawns.angles.shape[2]
        request = dict(mask=over.contiguous(), choices=choices.contiguous(), positions=spawns.positions, angles=spawns.angles, after=True)
        self._episodes += over
        return request

    def _world(self, reset):
        self._goals(reset)
        if self._routes is not None:
            self._routes(reset)
        now = self._goals.distances()
        # An agent can squeeze into a spot the grid has no free cell near (a gap between a pillar and a wall that is wider than
        # the agent and narrower than the grid can see): from there no distance is defined. It counts as stranded from then on -
        # no reward, and a new episode at the next step.
        self._goals.stranded |= ~torch.isfinite(now)
        reward, ended = books(self._distance, now, reset, self._goals.stranded, self.arrive, self.bonus)
        self._distance.copy_(now)
        self._over.copy_(self._lifespans(ended))
        frame = modules.render(self.core, observers=(self._rgb, self._depth), fields=())
        obs = arrdict.arrdict(rgb=self._rgb(frame), d=self._depth(frame), goal=self._goals.observation())
        if self._pano is not None:
            around = self._pano()
            obs['pano_rgb'], obs['pano_d'] = around.rgb, around.d
        world = arrdict.arrdict(obs=obs, reset=reset.any(-1), reward=reward)
        if self.spl is not None:
            # (an episode ends when its agent arrives, is stranded or outlives its lifespan: only the first scores above 0)
            world['spl'] = self.spl(reset, (now < self.arrive) & ~self._goals.stranded, self._over)
        return world

    @torch.no_grad()
    def reset(self):
        everyone = self.core.agent_full(True)
        modules._respawn(self.core.agents, {**self._respawn(everyone), 'after': False})
        return self._world(everyone)

    @torch.no_grad()
    def step(self, decision):
        """Moves the agents; those whose episode ended at the last step start a new one instead (a new spot, a new goal) and earn
        nothing for this frame. ``reset`` (n_env,): an agent of the env started over; ``reward`` (n_env, n_agent)."""
        over = self._over.clone()
        self._mover(decision, respawn=self._respawn(over))
        return self._world(over)

    @torch.no_grad()
    def expert(self, kind='follow'):
        """``arrdict(actions=(n_env, n_agent))``: what the shortest-path follower (:class:`~megastep_amd.modules.PathFollower`)
        does in the current state - every agent towards the waypoint of its own goal. Nothing waits for the host:
        ``env.step(env.expert())`` can sit in one graph. The follower counts the steps an agent has been stuck, so ask once
        per step. ``kind='lookahead'``: what :class:`~megastep_amd.modules.LookAhead` does instead - it rolls its plans through
        the physics step and takes the one that ends nearest the goal (by the env's routes, with ``margin``) - with a follower
        of its own to fall back on; as capturable, and made by the first call that asks for it (outside a graph).
        ``kind='anticipate'``: a ``LookAhead(others='repeat')`` - the same plans rolled among the env's other agents MOVING, each
        taken to repeat what this expert last chose for it, where ``'lookahead'`` has them stand still; made likewise."""
        if kind == 'follow':
            return self._follower()
        if kind not in ('lookahead', 'anticipate'):
            raise RuntimeError(f"kind must be 'follow', 'lookahead' or 'anticipate'; got {kind!r}")
        source = self._goals if self._routes is None else self._routes
        if kind == 'anticipate':
            if self._anticipate is None:
                self._anticipate = modules.LookAhead(self.core, source, self._mover, fallback=modules.PathFollower(self.core, source, cone=15.),
                                                     others='repeat')
            return self._anticipate()
        if self._lookahead is None:
            self._lookahead = modules.LookAhead(self.core, source, self._mover, fallback=modules.PathFollower(self.core, source, cone=15.))
        return self._lookahead()

    def state(self, e=0):
        return arrdict.arrdict(core=self.core.state(e), rgb=self._rgb.state(e), d=self._depth.state(e), goals=self._goals.state(e),
                               distance=self._distance[e].clone(), lifespan=self._lifespans.state(e))
