"""Dodge: every agent can throw. A shot is a projectile (:func:`megastep_amd.cuda.fly`): it leaves the agent along its heading,
flies a fraction of a metre a step, is stopped by walls and strikes the first other agent it meets - so it can be SEEN COMING,
dodged, and a moving target has to be led. The reference's Deathmatch fires hit-scan shots, over in the frame they are fired in;
this env is what that cannot be. No counterpart in the reference.

The agents see the projectiles: they are drawn into the camera's RGB-D fan (:func:`megastep_amd.cuda.overlay_items`) and the
nearest visible ones are listed as percepts. The observations come from the full-resolution frame through
:class:`~megastep_amd.modules.RGB`'s and :class:`~megastep_amd.modules.Depth`'s tensor-op path, as Forage's do and for its reason.

A step has no host synchronisation and draws no random numbers of its own besides :class:`~megastep_amd.modules.RandomLifespans`',
so it can be captured in a HIP graph (:class:`megastep_amd.graphs.GraphedStep`)."""
import torch

from ... import arrdict, core, cubicasa, cuda, dotdict, modules, scene, spaces
from .explorer import _plan_workers

FIRE = 7                                                # the action after the movement set's seven


class Dodge:

    def __init__(self, n_envs, n_agents=2, *args, per_agent=4, speed=8., life=64, bounces=0, damage=1., sight=10., k=4, max_lifespan=512,
                 device='cuda', geometries=None, cell=.125, seed=0, **kwargs):
        """``per_agent``, ``speed``, ``life``, ``bounces``, ``damage``: :class:`~megastep_amd.modules.Projectiles`'; ``sight``, ``k``:
        how far an agent's percepts reach, metres, and how many of the nearest visible projectiles they list; ``max_lifespan``:
        episodes end after a random number of steps up to this, and by nothing else; ``cell``: the nav grid's cell size - spawns
        are drawn among its free cells."""
        if geometries is None:
            geometries = cubicasa.sample(n_envs, workers=_plan_workers(), context='subprocess')
        self.core = core.Core(scene.scenery(geometries, n_agents, device=device), *args, res=4*64, fov=130, **kwargs)
        c = self.core
        self.device = c.device
        self._mover = modules.MomentumMovement(c)
        self._lifespans = modules.RandomLifespans(c, max_lifespan)
        self._rgb = modules.RGB(c, subsample=4)
        self._depth = modules.Depth(c, subsample=4)
        self.grid = cuda.nav_grid(c.scenery, cell, config=c.config)
        self._respawner = modules.SampledSpawns(c, self.grid, seed=seed)
        #: the :class:`~megastep_amd.modules.Projectiles` of the env
        self.projectiles = modules.Projectiles(c, per_agent, speed=speed, life=life, bounces=bounces, damage=damage, colors=(1., .2, .1))
        self._percepts = modules.Percepts(c, points=self.projectiles.positions, max_range=float(sight), fov=c.fov, k=k)
        self.action_space = spaces.MultiDiscrete(c.n_agents, FIRE + 1)
        self.obs_space = dotdict.dotdict(rgb=self._rgb.space, d=self._depth.space, percepts=self._percepts.space)
        self._over = c.agent_full(True)                 # who starts over at the next step: episode ended, or struck
        self._ended = c.agent_full(True)                # whose episode ended at the last step
        self._frame = None

    #: the :class:`~megastep_amd.cuda.Render` of the last step, the projectiles drawn into it, with ``.items`` (None before the first)
    frame = property(lambda self: self._frame)

    def _world(self, fire, ended):
        c = self.core
        reset = ended.any(-1)
        flown = self.projectiles(fire, reset=reset)
        self._frame = self.projectiles.draw(cuda.render(c.scenery, c.agents, out=self._frame))
        frame = modules._frame(self._frame, None)
        self._ended.copy_(self._lifespans())
        torch.logical_or(self._ended, flown.hits > 0, out=self._over)
        obs = arrdict.arrdict(rgb=self._rgb(frame), d=self._depth(frame), percepts=self._percepts())
        return arrdict.arrdict(obs=obs, reset=reset, reward=self.projectiles.reward())

    @torch.no_grad()
    def reset(self):
        everyone = self.core.agent_full(True)
        self._respawner(everyone)
        return self._world(self.core.agent_full(False), everyone)

    @torch.no_grad()
    def step(self, decision):
        """``decision.actions`` (n_env, n_agent) in 0..7: the movement set's seven, and 7: fire (the agent's momentum carries it on).
        The agents whose episode ended at the last step, and those a projectile struck, start over on a fresh cell; an env in
        which an episode ended has its projectiles taken out of the air. ``reward`` (n_env, n_agent): ``scored - hits``."""
        ended, over = self._ended.clone(), self._over.clone()
        fire = decision.actions == FIRE
        moves = arrdict.arrdict(actions=torch.where(fire, torch.zeros_like(decision.actions), decision.actions))
        self._mover(moves, respawn=self._respawner.draw(over, after=True))
        return self._world(fire & ~over, ended)

    def state(self, e=0):
        return arrdict.arrdict(core=self.core.state(e), rgb=self._rgb.state(e), d=self._depth.state(e), projectiles=self.projectiles.state(e),
                               lifespan=self._lifespans.state(e))
