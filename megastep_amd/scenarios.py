"""Whole envs forked into scenarios - every agent on a plan of its own - and rolled through the agent step in one launch
(kernel: ``csrc/kernels/scenario.h``): the multi-agent completion of :mod:`~megastep_amd.rollouts`. No counterpart in the
reference; reached as ``megastep_amd.cuda.<name>``."""
import ctypes as C
import torch
from . import _lib
from ._lib import _on, _stream
from ._call import _cfg, _check, _query_device, _result_for
from .rollouts import ROLLOUT_MAX_HORIZON, _fresh

SCENARIO_MAX_SCENARIOS = 256
SCENARIO_MAX_AGENTS = 64


class Scenarios:
    """Result of :func:`scenarios`, one row per (env, scenario, agent): ``positions`` (N, S, A, 2), ``angles`` (N, S, A),
    ``velocity`` (N, S, A, 2) and ``angvelocity`` (N, S, A) after the scenario's last step; ``progress`` (N, S, A) float32, the
    least share of a step the agent could take; ``stops`` (N, S, A) int32, the steps at which it was stopped; ``first_stop``
    (N, S, A) int32, the first of them, ``H`` when there was none; ``trail`` (N, S, A, H, 2), the position after every step, or
    ``None`` when it was not asked for."""

    def __init__(self, positions, angles, velocity, angvelocity, progress, stops, first_stop, trail):
        self._t = (positions, angles, velocity, angvelocity, progress, stops, first_stop, trail)

    positions = property(lambda self: self._t[0])
    angles = property(lambda self: self._t[1])
    velocity = property(lambda self: self._t[2])
    angvelocity = property(lambda self: self._t[3])
    progress = property(lambda self: self._t[4])
    stops = property(lambda self: self._t[5])
    first_stop = property(lambda self: self._t[6])
    trail = property(lambda self: self._t[7])


def _common(scenery, agents, table, keep, h, what):
    """The checks both modes share; returns (n, a, keep)."""
    n, a = len(scenery.lines), scenery.n_agents
    if tuple(agents.angles.shape) != (n, a):
        raise RuntimeError(f'agents do not match the scenery: expected (n_envs, n_agents) = {(n, a)}, got {tuple(agents.angles.shape)}')
    if not 1 <= a <= SCENARIO_MAX_AGENTS:
        raise RuntimeError(f'{what} take 1..{SCENARIO_MAX_AGENTS} agents an env; got {a}')
    if not 1 <= h <= ROLLOUT_MAX_HORIZON:
        raise RuntimeError(f'the horizon H must be in 1..{ROLLOUT_MAX_HORIZON}; got {h}')
    _check(table, 'table', torch.float32, 2)
    if table.shape[1] != 3 or table.shape[0] < 1:
        raise RuntimeError(f'table must be (n_actions, 3) with n_actions >= 1; got {tuple(table.shape)}')
    keep = float(keep)
    if keep != keep:
        raise RuntimeError('keep must be a number')
    return n, a, keep


def _mask(mask, shape, tensors):
    if mask is not None:
        _check(mask, 'mask', torch.bool, len(shape))
        if tuple(mask.shape) != shape:
            raise RuntimeError(f'mask must be {shape}; got {tuple(mask.shape)}')
        tensors.append(mask)
    return mask.data_ptr() if mask is not None else None


def _launch(scenery, agents, query, cfg, dev):
    scenery._check_grid(dev)
    with _on(dev):
        _lib.check(_lib.lib().ms_scenarios(C.byref(scenery._as_struct()), C.byref(agents._plain), C.byref(query), C.byref(cfg), _stream(dev)))


def scenarios(scenery, agents, actions, table, keep=0., trail=False, mask=None, out=None, config=None):
    """Forks every env into ``S`` scenarios, in each of which EVERY agent follows a plan of ``H`` actions of its own, steps them
    all through the step :func:`physics` takes, in one launch, and returns :class:`Scenarios`. Neither the scenery nor the agents
    are modified.

    ``actions``: (N, S, A, H) int64 rows of ``table`` - clamped to it - or (S, A, H), the same scenarios for every env (the
    kernel reads the one copy). ``table`` (n_actions, 3) float32 and ``keep``: a movement module's, as :func:`physics`'
    ``movement``. Every scenario starts from all agents' states as they stand and takes, per step, what one
    ``physics(movement=...)`` call does to a copy of the env: every agent's movement update, then every agent's collision tests
    against all static walls of its env and against every other agent where and as fast as that one moves in this scenario,
    then everybody's integration - bit for bit. ``trail=True`` also gives the position after every step. ``mask`` (N,) bool:
    only the marked envs are rolled; the others keep what ``out`` held, and without ``out`` read as NaN poses, progress 1, no
    stops. ``out``: the :class:`Scenarios` of an earlier call with the same shapes, to write into. ``config``: see
    :func:`physics` (``agent_radius`` and ``fps`` are read).

    ``1 <= S <= 256``, ``1 <= H <= 64``, at most 64 agents an env. Sliding steps, respawns, lifespans and the IMU are not part of
    a scenario. No host synchronisation, nothing allocated with ``out``: the call can be captured in a HIP graph (DESIGN.md
    3.32). :func:`rollouts` with a tensor ``others`` is the focal mode of the same kernel."""
    if not isinstance(actions, torch.Tensor) or actions.ndim not in (3, 4):
        raise RuntimeError('actions must be a (N, S, A, H) or (S, A, H) int64 tensor')
    _check(actions, 'actions', torch.int64, actions.ndim)
    s, a_, h = actions.shape[-3:]
    n, a, keep = _common(scenery, agents, table, keep, h, 'scenarios')
    shared = actions.ndim == 3
    if a_ != a or (not shared and actions.shape[0] != n):
        raise RuntimeError(f'actions must be ({n}, S, {a}, H) or (S, {a}, H); got {tuple(actions.shape)}')
    if not 1 <= s <= SCENARIO_MAX_SCENARIOS:
        raise RuntimeError(f'the scenarios S must be in 1..{SCENARIO_MAX_SCENARIOS}; got {s}')
    tensors = [actions, table]
    mask_ptr = _mask(mask, (n,), tensors)
    dev = _query_device(scenery, agents, *tensors)
    cfg = _cfg(agents, config)
    trail = bool(trail)

    def fresh():
        r = _fresh(n, s, a, h, trail, dev)                              # (the same fills, the middle axes the other way round)
        return Scenarios(*r._t[:8])
    result = _result_for(out, (n, s, a, h, trail, dev), 'a scenarios', fresh)
    ptrs = [t.data_ptr() if t is not None else None for t in result._t]
    query = _lib.MsScenarios(s, h, 0, actions.data_ptr(), int(shared), None, table.data_ptr(), table.shape[0], keep, mask_ptr, *ptrs)
    _launch(scenery, agents, query, cfg, dev)
    return result


def _focal(scenery, agents, plans, base, table, keep, trail, mask, out, config, k, h, shared):
    """:func:`rollouts` with a tensor ``others`` - the focal mode: its checks of ``plans`` are done; returns its ``Rollouts``."""
    n, a, keep = _common(scenery, agents, table, keep, h, 'rollouts among moving others')
    _check(base, 'others', torch.int64, 3)
    if tuple(base.shape) != (n, a, h):
        raise RuntimeError(f'others must be ({n}, {a}, {h}) = (n_envs, n_agents, H); got {tuple(base.shape)}')
    tensors = [plans, base, table]
    mask_ptr = _mask(mask, (n, a), tensors)
    dev = _query_device(scenery, agents, *tensors)
    cfg = _cfg(agents, config)
    trail = bool(trail)
    result = _result_for(out, (n, a, k, h, trail, dev), 'a rollouts', lambda: _fresh(n, a, k, h, trail, dev))
    ptrs = [t.data_ptr() if t is not None else None for t in result._t[:8]]
    query = _lib.MsScenarios(k, h, 1, plans.data_ptr(), int(shared), base.data_ptr(), table.data_ptr(), table.shape[0], keep, mask_ptr, *ptrs)
    _launch(scenery, agents, query, cfg, dev)
    return result
