"""Candidate action plans rolled through the agent step in one launch (kernel: ``csrc/kernels/rollout.h``). No counterpart in the
reference, where the only way to know what a sequence of actions leads to is to step a copy of the world once per plan and
step; reached as ``megastep_amd.cuda.<name>``."""
import ctypes as C
import torch
from . import _lib
from ._lib import _on, _stream
from ._call import _cfg, _check, _query_device, _result_for

ROLLOUT_MAX_CANDIDATES = 256
ROLLOUT_MAX_HORIZON = 64


class Rollouts:
    """Result of :func:`rollouts`, one row per (env, agent, candidate): ``positions`` (N, A, K, 2), ``angles`` (N, A, K),
    ``velocity`` (N, A, K, 2) and ``angvelocity`` (N, A, K) after the plan's last step; ``progress`` (N, A, K) float32, the least
    share of a step the candidate could take; ``stops`` (N, A, K) int32, the steps at which it was stopped; ``first_stop``
    (N, A, K) int32, the first of them, ``H`` when there was none; ``trail`` (N, A, K, H, 2), the position after every step, or
    ``None`` when it was not asked for. Of a call with ``slide``: ``stops`` and ``first_stop`` count the steps that ended in a dead
    stop - the velocity zeroed - and ``slides`` (N, A, K) int32 the steps that slid the whole of their remainder; else ``None``."""

    def __init__(self, positions, angles, velocity, angvelocity, progress, stops, first_stop, trail, slides=None):
        self._t = (positions, angles, velocity, angvelocity, progress, stops, first_stop, trail, slides)

    positions = property(lambda self: self._t[0])
    angles = property(lambda self: self._t[1])
    velocity = property(lambda self: self._t[2])
    angvelocity = property(lambda self: self._t[3])
    progress = property(lambda self: self._t[4])
    stops = property(lambda self: self._t[5])
    first_stop = property(lambda self: self._t[6])
    trail = property(lambda self: self._t[7])
    slides = property(lambda self: self._t[8])


def plans(n_actions, horizon, switch=None, device=None):
    """Plans to roll, as :func:`rollouts`' ``(K, H)`` int64 ``actions``. ``switch=None``: the ``n_actions`` constant plans, plan
    ``i`` action ``i`` at every step. ``switch=s``: the ``n_actions**2`` plans "action ``i`` for the first ``s`` steps, then action
    ``j``", plan ``i*n_actions + j``. Pure torch."""
    if n_actions < 1 or horizon < 1:
        raise RuntimeError(f'n_actions and horizon must be positive; got {n_actions}, {horizon}')
    acts = torch.arange(n_actions, dtype=torch.int64, device=device)
    if switch is None:
        return acts[:, None].expand(n_actions, horizon).contiguous()
    if not 0 <= switch <= horizon:
        raise RuntimeError(f'switch must be in 0..horizon; got {switch}')
    first = acts[:, None, None].expand(n_actions, n_actions, horizon)
    then = acts[None, :, None].expand(n_actions, n_actions, horizon)
    late = torch.arange(horizon, device=device)[None, None, :] >= switch
    return torch.where(late, then, first).reshape(n_actions*n_actions, horizon).contiguous()


def _bounce(slide):
    """``slide`` (None / False, True, or dict(bounce=...)) as the bounce of a sliding call, or None for a plain one."""
    if slide is None or slide is False:
        return None
    if slide is not True and not isinstance(slide, dict):
        raise RuntimeError('slide must be True or a dict(bounce=...)')
    options = {} if slide is True else dict(slide)
    bounce = float(options.pop('bounce', .05))
    if options:
        raise RuntimeError(f'slide takes bounce only, got {sorted(options)}')
    if not 0 <= bounce <= 1:
        raise RuntimeError(f'slide needs 0 <= bounce <= 1, got {bounce}')
    return bounce


def _fresh(n, a, k, h, trail, dev, slide=False):
    """The buffers of a call without ``out``, holding what an agent that is not rolled reads as: NaN poses, progress 1, no stop."""
    nan = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=dev)
    return Rollouts(nan(n, a, k, 2), nan(n, a, k), nan(n, a, k, 2), nan(n, a, k), torch.ones((n, a, k), dtype=torch.float32, device=dev),
                    torch.zeros((n, a, k), dtype=torch.int32, device=dev), torch.full((n, a, k), h, dtype=torch.int32, device=dev),
                    nan(n, a, k, h, 2) if trail else None, torch.zeros((n, a, k), dtype=torch.int32, device=dev) if slide else None)


def rollouts(scenery, agents, actions, table, keep=0., others=None, trail=False, mask=None, out=None, config=None, slide=None):
    """Rolls ``K`` candidate plans of ``H`` actions for every agent through the step :func:`physics` takes, in one launch, and
    returns :class:`Rollouts`. Neither the scenery nor the agents are modified.

    ``actions``: (N, A, K, H) int64 rows of ``table`` - clamped to it, as :func:`physics` clamps its ``movement`` - or (K, H), the
    same plans for every agent (the kernel reads the one copy: nothing is expanded). ``table`` (n_actions, 3) float32 and
    ``keep``: a movement module's, as :func:`physics`' ``movement``. Every candidate starts from its agent's state as it stands
    and takes, per step, the movement update, the collision tests against all static walls of its env - through the wall grid's
    lists where they are exact, against every wall where not: the same bits - and the integration. ``others='rest'``: the env's
    other agents are obstacles too, standing still where the call found them for the whole horizon; ``None``: they are absent;
    a (N, A, H) int64 tensor: they MOVE - while agent ``f`` rolls its plan ``k``, every other agent ``b`` of its env takes the
    actions ``others[n, b, :]``, everybody meeting everybody as in one :func:`physics` step (the focal mode of
    :func:`scenarios`; at most 64 agents an env, not with ``slide``). ``trail=True`` also gives the position after every step. ``mask`` (N, A) bool: only the marked agents are rolled; the others
    keep what ``out`` held, and without ``out`` read as NaN poses, progress 1, no stops. ``out``: the :class:`Rollouts` of an
    earlier call with the same shapes, to write into. ``config``: see :func:`physics` (``agent_radius`` and ``fps`` are read).
    ``slide``: ``True`` or ``dict(bounce=.05)`` - every step is :func:`physics`' sliding step, the others at rest in both its
    phases; the result then has ``slides``, and its ``stops`` count dead stops.

    ``1 <= K <= 256`` and ``1 <= H <= 64``. Respawns, lifespans and the IMU are not part of a rollout.
    No host synchronisation, nothing allocated with ``out``: the call can be captured in a HIP graph."""
    n, a = len(scenery.lines), scenery.n_agents
    if tuple(agents.angles.shape) != (n, a):
        raise RuntimeError(f'agents do not match the scenery: expected (n_envs, n_agents) = {(n, a)}, got {tuple(agents.angles.shape)}')
    if not isinstance(actions, torch.Tensor) or actions.ndim not in (2, 4):
        raise RuntimeError('actions must be a (N, A, K, H) or (K, H) int64 tensor')
    _check(actions, 'actions', torch.int64, actions.ndim)
    _check(table, 'table', torch.float32, 2)
    shared = actions.ndim == 2
    k, h = actions.shape[-2:]
    if not shared and tuple(actions.shape[:2]) != (n, a):
        raise RuntimeError(f'actions must be ({n}, {a}, K, H) or (K, H); got {tuple(actions.shape)}')
    if not 1 <= k <= ROLLOUT_MAX_CANDIDATES:
        raise RuntimeError(f'the candidates K must be in 1..{ROLLOUT_MAX_CANDIDATES}; got {k}')
    if not 1 <= h <= ROLLOUT_MAX_HORIZON:
        raise RuntimeError(f'the horizon H must be in 1..{ROLLOUT_MAX_HORIZON}; got {h}')
    if table.shape[1] != 3 or table.shape[0] < 1:
        raise RuntimeError(f'table must be (n_actions, 3) with n_actions >= 1; got {tuple(table.shape)}')
    if isinstance(others, torch.Tensor):
        if slide is not None and slide is not False:
            raise RuntimeError('slide is not part of a rollout among moving others: sliding steps are stated for others at rest only')
        from .scenarios import _focal
        return _focal(scenery, agents, actions, others, table, keep, trail, mask, out, config, k, h, shared)
    if others not in (None, 'rest'):
        raise RuntimeError(f"others must be None, 'rest' or a (N, A, H) int64 tensor; got {others!r}")
    keep = float(keep)
    if keep != keep:
        raise RuntimeError('keep must be a number')
    tensors = [actions, table]
    if mask is not None:
        _check(mask, 'mask', torch.bool, 2)
        if tuple(mask.shape) != (n, a):
            raise RuntimeError(f'mask must be ({n}, {a}); got {tuple(mask.shape)}')
        tensors.append(mask)
    dev = _query_device(scenery, agents, *tensors)
    cfg = _cfg(agents, config)
    trail = bool(trail)
    bounce = _bounce(slide)
    sliding = bounce is not None
    key = (n, a, k, h, trail, dev) + ((True,) if sliding else ())       # (a plain call's key is what it was)
    result = _result_for(out, key, 'a rollouts', lambda: _fresh(n, a, k, h, trail, dev, sliding))
    ptrs = [t.data_ptr() if t is not None else None for t in result._t]
    query = _lib.MsRollouts(k, h, actions.data_ptr(), int(shared), table.data_ptr(), table.shape[0], keep, int(others == 'rest'),
                            mask.data_ptr() if mask is not None else None, *ptrs[:8], int(sliding), bounce if sliding else 0., ptrs[8])
    scenery._check_grid(dev)
    with _on(dev):
        _lib.check(_lib.lib().ms_rollouts(C.byref(scenery._as_struct()), C.byref(agents._plain), C.byref(query), C.byref(cfg), _stream(dev)))
    return result
