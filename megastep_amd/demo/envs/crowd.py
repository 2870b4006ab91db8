"""Crowd: :class:`PointGoal`'s task among OTHERS WHO WALK. Every env holds a crowd of walkers (:func:`megastep_amd.cuda.walk`) that
go from destination to destination along the shortest paths, keep apart from each other and from the agents, and are stopped by
walls, by each other and by the agents - pedestrians, not learners: they have no camera and cast no rays. The agents see them,
drawn into the camera's RGB-D fan (:func:`megastep_amd.cuda.overlay_items`), and are not stopped by them: walking into one costs
``bump``, coming within the walkers' personal distance of one costs ``close``. With ``solid=True`` the crowd is in the agents' way
(:func:`megastep_amd.cuda.physics`, ``bodies``): an agent is stopped at a walker as it is at another agent. No counterpart in the
reference.

The observations come from the full-resolution frame through :class:`~megastep_amd.modules.RGB`'s and
:class:`~megastep_amd.modules.Depth`'s tensor-op path, as Forage's do and for its reason. A step has no host synchronisation and
draws no random numbers of its own besides :class:`~megastep_amd.modules.RandomLifespans`', so it can be captured in a HIP graph
(:class:`megastep_amd.graphs.GraphedStep`)."""
import torch

from ... import arrdict, cuda, modules
from .pointgoal import PointGoal, books


class Crowd(PointGoal):

    def __init__(self, n_envs, n_walkers=16, *args, n_goals=4, speeds=(.6, 1.4), bump=.5, close=.05, seed=0, walk=None, flow=False, solid=False,
                 **kwargs):
        """``n_walkers``, ``n_goals``, ``speeds``, ``seed``, ``walk`` (a dict of :func:`~megastep_amd.cuda.walk`'s ``personal``,
        ``push``, ``keep``, ``agents_push``, ``slide``), ``flow``: :class:`~megastep_amd.modules.Walkers`'; ``bump``, ``close``: what a walker that runs into
        an agent, and one within ``personal`` of it, take off the agent's reward of the step. Everything else is
        :class:`PointGoal`'s, less ``spl`` and ``panorama``. The crowd keeps walking across the agents' episodes. ``solid=True``: the
        walkers stop the agents (not with ``slide``); the observation and the reward keep their keys."""
        if kwargs.get('spl') or kwargs.get('panorama'):
            raise RuntimeError('Crowd takes neither spl nor panorama')
        if solid and kwargs.get('slide'):
            raise RuntimeError('a solid Crowd does not slide: bodies and slide do not go together')
        super().__init__(n_envs, *args, **kwargs)
        #: the :class:`~megastep_amd.modules.Walkers` of the env
        self.walkers = modules.Walkers(self.core, self.grid, n_walkers, n_goals=n_goals, speeds=speeds, seed=seed, colors=(.9, .6, .1), flow=flow,
                                       solid=solid, **(walk or {}))
        if solid:
            self.walkers.stop(self._mover)
        self.bump, self.close = float(bump), float(close)
        self._frame = None

    #: the :class:`~megastep_amd.cuda.Render` of the last step, the walkers drawn into it, with ``.items`` (None before the first)
    frame = property(lambda self: self._frame)

    def _world(self, reset):
        c = self.core
        self._goals(reset)
        if self._routes is not None:
            self._routes(reset)
        now = self._goals.distances()
        self._goals.stranded |= ~torch.isfinite(now)
        reward, ended = books(self._distance, now, reset, self._goals.stranded, self.arrive, self.bonus)
        self._distance.copy_(now)
        self._over.copy_(self._lifespans(ended))
        walked = self.walkers()                         # (behind the agents' step: they are met where they stand)
        self._frame = self.walkers.draw(cuda.render(c.scenery, c.agents, out=self._frame))
        frame = modules._frame(self._frame, None)
        obs = arrdict.arrdict(rgb=self._rgb(frame), d=self._depth(frame), goal=self._goals.observation())
        return arrdict.arrdict(obs=obs, reset=reset.any(-1), reward=reward - self.bump*walked.bumps - self.close*walked.close)

    def _among(self):
        """A solid crowd's 'lookahead' expert rolls its plans among the walkers, each going on as it goes now (:func:`cuda.rollouts`, ``bodies``)."""
        return dict(bodies=dict(store=self.walkers.store, moving=True)) if self.walkers.solid else {}

    def state(self, e=0):
        state = super().state(e)
        state['walkers'] = self.walkers.state(e)
        return state
