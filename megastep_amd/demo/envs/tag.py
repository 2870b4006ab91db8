"""Tag: the first ``n_seekers`` agents of an env seek, the rest hide. A hider is tagged when a seeker SEES it from no further than
``tag_range`` metres: the seeker earns 1 for every hider it tags at a step, the hider -1, and it starts over on a fresh cell at the
next step; a hider that no seeker sees earns ``hide_bonus`` a step. An episode ends by its lifespan only. No counterpart in the
reference, whose multi-agent env reads two centre pixels; who sees whom is one :func:`megastep_amd.cuda.percepts` call a step -
range, the camera's cone and the building's walls; bodies do not occlude - and the agents observe each other through it.

A step has no host synchronisation and draws no random numbers of its own besides :class:`~megastep_amd.modules.RandomLifespans`',
so it can be captured in a HIP graph (:class:`megastep_amd.graphs.GraphedStep`)."""
import torch

from ... import arrdict, core, cubicasa, cuda, dotdict, modules, scene, spaces
from .explorer import _plan_workers


class _Chase:
    """What the expert's :class:`~megastep_amd.modules.PathFollower` follows: the seekers the shortest path to the hider nearest on
    foot, the hiders the way to the nearest floor the seeker nearest to them cannot see."""

    REFRESH = 8                                     # steps between two looks at what the seekers see

    def __init__(self, env):
        self.env = env
        c = env.core
        s, h = env.n_seekers, c.n_agents - env.n_seekers
        self._steps = torch.zeros((c.n_envs, 1), dtype=torch.long, device=c.device)
        self._seekers = c.agents.positions[:, :s].clone()
        self._each = torch.arange(h, dtype=torch.int32, device=c.device).repeat(s)[None].expand(c.n_envs, s*h).contiguous()
        self._to_hiders = self._views = self._cover = None

    def waypoints(self, lookahead=16):
        env, c = self.env, self.env.core
        s, h = env.n_seekers, c.n_agents - env.n_seekers
        positions = c.agents.positions
        seekers, hiders = positions[:, :s].contiguous(), positions[:, s:].contiguous()
        # the seekers: towards the hider that is the shortest walk away
        self._to_hiders = cuda.distance_fields(env.grid, hiders, out=self._to_hiders)
        walks = self._to_hiders.at(seekers.repeat_interleave(h, 1).contiguous(), goal=self._each).reshape(-1, s, h)
        chase = self._to_hiders.waypoints(seekers, goal=walks.argmin(-1), lookahead=lookahead)
        # the hiders: cover from what the seekers saw when last looked at
        due = self._steps % self.REFRESH == 0
        self._steps += 1
        due = due.expand(-1, s).contiguous()
        torch.where(due[..., None], seekers, self._seekers, out=self._seekers)
        if self._views is None:
            self._views = cuda.view_fields(env.grid, c.scenery, self._seekers, max_range=env.sight)
            self._cover = cuda.seeded_fields(env.grid, self._views.values, s, where=False)
        else:
            self._views.update(due)
            self._cover.update(due)
        away = hiders[:, :, None] - seekers[:, None]
        nearest = (away*away).sum(-1).argmin(-1)
        hide = self._cover.waypoints(hiders, goal=nearest, lookahead=lookahead)
        return torch.cat([chase, hide], 1)


class Tag:

    def __init__(self, n_envs, n_seekers=1, n_hiders=1, *args, tag_range=1., sight=10., hide_bonus=.01, max_lifespan=512, slide=False,
                 device='cuda', geometries=None, cell=.125, **kwargs):
        """``n_seekers``, ``n_hiders``: agents ``0 .. n_seekers - 1`` of an env seek, the other ``n_hiders`` hide; ``tag_range``: how
        near a seeker must see a hider to tag it, metres; ``sight``: how far anybody sees, metres; ``hide_bonus``: what a hider earns
        for a step out of every seeker's sight; ``max_lifespan``: episodes end after a random number of steps up to this
        (:class:`~megastep_amd.modules.RandomLifespans`), and by nothing else; ``cell``: the nav grid's cell size - spawns are drawn
        among its free cells (:class:`~megastep_amd.modules.SampledSpawns`). ``slide``: ``True`` or ``dict(bounce=.05)`` - the agents
        slide along what they hit instead of stopping dead (:func:`~megastep_amd.cuda.physics`)."""
        if n_seekers < 1 or n_hiders < 1:
            raise RuntimeError(f'Tag needs at least one seeker and one hider; got {n_seekers} and {n_hiders}')
        n_agents = n_seekers + n_hiders
        if geometries is None:
            geometries = cubicasa.sample(n_envs, workers=_plan_workers(), context='subprocess')
        self.core = core.Core(scene.scenery(geometries, n_agents, device=device), *args, res=4*64, fov=130, **kwargs)
        c = self.core
        self.device = c.device
        self.n_seekers, self.n_hiders = int(n_seekers), int(n_hiders)
        self.tag_range, self.sight, self.hide_bonus = float(tag_range), float(sight), float(hide_bonus)

        self._mover = modules.MomentumMovement(c, slide=slide or None)
        self._lifespans = modules.RandomLifespans(c, max_lifespan)
        self._rgb = modules.RGB(c, subsample=4)
        self._depth = modules.Depth(c, subsample=4)
        self.grid = cuda.nav_grid(c.scenery, cell, config=c.config)
        self._respawner = modules.SampledSpawns(c, self.grid)
        #: (n_agent,) bool: who seeks
        self.roles = torch.arange(n_agents, device=c.device) < self.n_seekers
        self._role = self.roles.float()[None, :, None].expand(c.n_envs, n_agents, 1).contiguous()
        self._seen = None                               # the step's cuda.Percepts
        self.action_space = self._mover.space
        self.obs_space = dotdict.dotdict(rgb=self._rgb.space, d=self._depth.space, percepts=spaces.MultiRows(n_agents, n_agents - 1, 4),
                                         role=spaces.MultiVector(n_agents, 1))

        self._ended = c.agent_full(True)                # whose episode ended at the last step
        self._tagged = c.agent_full(False)              # who was tagged at the last step
        self._chase = self._follower = None             # made when the expert is first asked: they cost nothing until then

    #: the :class:`~megastep_amd.cuda.Percepts` of the last step: who sees whom (None before the first)
    seen = property(lambda self: self._seen)

    @staticmethod
    def books(visible, squares, roles, tag_range, hide_bonus):
        """The game between two frames, pure torch: ``visible`` and ``squares`` (n_env, n_agent, n_agent) - agent e sees agent p, and
        the square of how far away - ``roles`` (n_agent,) bool, who seeks. Returns (reward (n_env, n_agent) float32, tagged
        (n_env, n_agent) bool): hider h is tagged when some seeker s has ``visible[s, h]`` and ``squares[s, h] <= tag_range**2``; a
        seeker earns 1 per hider it tags at this step; a hider earns -1 when tagged, else ``hide_bonus`` when no seeker sees it,
        else 0."""
        pair = roles[:, None] & ~roles[None, :]                          # (a seeker's row, a hider's column)
        sees = (visible != 0) & pair
        tags = sees & (squares <= tag_range**2)
        tagged = tags.any(1)
        nothing = torch.zeros(tagged.shape, dtype=torch.float32, device=tagged.device)
        hiding = torch.where(tagged, nothing - 1., torch.where(sees.any(1), nothing, nothing + hide_bonus))
        return torch.where(roles, tags.sum(2).float(), hiding), tagged

    def _world(self, ended):
        c = self.core
        frame = modules.render(c, observers=(self._rgb, self._depth), fields=())
        self._seen = cuda.percepts(c.scenery, agents=c.agents, fov=c.fov, max_range=self.sight, k=c.n_agents - 1, out=self._seen)
        seen = self._seen
        reward, tagged = self.books(seen.visible, seen.squares, self.roles, self.tag_range, self.hide_bonus)
        self._tagged.copy_(tagged)
        self._ended.copy_(self._lifespans())
        obs = arrdict.arrdict(rgb=self._rgb(frame), d=self._depth(frame), role=self._role,
                              percepts=modules.Percepts.pack(seen.counts, seen.near_offsets, seen.near_distances, c.agents.angles, self.sight))
        return arrdict.arrdict(obs=obs, reset=ended.any(-1), reward=reward)

    @torch.no_grad()
    def reset(self):
        everyone = self.core.agent_full(True)
        self._respawner(everyone)
        return self._world(everyone)

    @torch.no_grad()
    def step(self, decision):
        """Moves the agents; those whose episode ended at the last step, and the hiders tagged at it, start over on a fresh cell
        instead. ``reset`` (n_env,): an agent of the env began a new episode; ``reward`` (n_env, n_agent): :meth:`books`'."""
        ended = self._ended.clone()
        over = ended | self._tagged
        self._mover(decision, respawn=self._respawner.draw(over, after=True))
        return self._world(ended)

    @torch.no_grad()
    def expert(self):
        """``arrdict(actions=(n_env, n_agent))``: what a privileged player does in the current state, through a
        :class:`~megastep_amd.modules.PathFollower`. A seeker follows the shortest path (:func:`~megastep_amd.cuda.distance_fields`) to
        the hider that is the shortest walk away. A hider walks to cover: :func:`~megastep_amd.cuda.view_fields` from the seekers'
        positions, looked at again every 8 steps, then ``seeded_fields(grid, views.values, where=False)`` - the way to the nearest
        floor the seeker nearest to it cannot see. Nothing waits for the host: ``env.step(env.expert())`` can sit in one graph, once
        a first call outside it has made the fields. Ask once per step."""
        if self._chase is None:
            self._chase = _Chase(self)
            self._follower = modules.PathFollower(self.core, self._chase, cone=15.)
        return self._follower()

    def state(self, e=0):
        return arrdict.arrdict(core=self.core.state(e), rgb=self._rgb.state(e), d=self._depth.state(e), roles=self.roles.clone(),
                               tagged=self._tagged[e].clone(), lifespan=self._lifespans.state(e))
