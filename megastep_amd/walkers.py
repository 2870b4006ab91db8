"""Walkers: bodies that steer, keep apart and stop at walls - pedestrians, guards, a crowd - without being agents (kernel:
``csrc/kernels/walker.h``). No counterpart in the reference; reached as ``megastep_amd.cuda.<name>``."""
import ctypes as C
import torch
from . import _lib
from ._lib import _on, _stream
from ._call import _cfg, _check, _query_device, _result_for
from .items import Items
from .percepts import _bytes
from .rollouts import _bounce

#: the most slots an env may hold, and the most agents an env may have for :func:`walk`
WALK_MAX_SLOTS, WALK_MAX_AGENTS = 1024, 64


class Walkers(Items):
    """The store of the walkers, ``P`` slots an env: ``positions`` (N, P, 2) float32 - a slot is present exactly when both coordinates
    are finite, as an :class:`Items`' is, and the store IS one: :func:`overlay_items`, ``modules.Percepts(points=store.positions)``,
    :func:`point_marks` and ``scene.display(items=store)`` take it as it is; ``velocities`` (N, P, 2) float32, m/s; ``speeds`` (N, P)
    float32 - each walker's preferred speed, m/s; ``colors`` (N, P, 3) float32 linear RGB. Read as items, every walker is of kind 0.
    The tensors are the caller's to write: a walker put there by hand walks at the next :func:`walk`."""

    def __init__(self, positions, velocities, speeds, colors):
        n, p = positions.shape[:2]
        zeros = torch.zeros((n, p), dtype=torch.int32, device=positions.device)
        super().__init__(positions, zeros, zeros.clone(), colors, 1)
        self.velocities, self.speeds = velocities, speeds

    n_slots = property(lambda self: self.positions.shape[1])


def walkers(n_envs, n_slots, speed=1., colors=None, device='cuda'):
    """A :class:`Walkers` of ``n_slots`` (1..1024) slots in each of ``n_envs`` envs, all absent and at rest, every preferred speed
    ``speed`` m/s. ``colors``: (3,), (P, 3) or (N, P, 3) linear RGB, default white."""
    if not isinstance(n_envs, int) or n_envs < 1 or not isinstance(n_slots, int) or not 1 <= n_slots <= WALK_MAX_SLOTS:
        raise RuntimeError(f'walkers takes n_envs >= 1 and 1 to {WALK_MAX_SLOTS} slots an env; got {n_envs} and {n_slots}')
    if not isinstance(speed, (int, float)) or not (0 <= speed < float('inf')):
        raise RuntimeError(f'speed must be a number of metres a second >= 0; got {speed}')
    colors = torch.ones(3) if colors is None else torch.as_tensor(colors, dtype=torch.float32)
    if tuple(colors.shape) not in ((3,), (n_slots, 3), (n_envs, n_slots, 3)):
        raise RuntimeError(f'colors must be (3,), (P, 3) or (N, P, 3) with (N, P) = ({n_envs}, {n_slots}); got {tuple(colors.shape)}')
    device = torch.device(device)
    return Walkers(torch.full((n_envs, n_slots, 2), float('nan'), dtype=torch.float32, device=device),
                   torch.zeros((n_envs, n_slots, 2), dtype=torch.float32, device=device),
                   torch.full((n_envs, n_slots), float(speed), dtype=torch.float32, device=device),
                   colors.to(device).expand(n_envs, n_slots, 3).contiguous())


class Walked:
    """Result of :func:`walk`: ``progress`` (N, P) float32 - the fraction of its step each walker took, NaN for an empty slot;
    ``blocked`` (N, P) uint8 - what stopped it: 0 nothing, 1 an agent, 2 a walker, 3 a wall, 4 the slot is empty; ``bumps`` (N, A)
    int32 - the walkers that ran into each agent; ``close`` (N, A) int32 - the walkers within ``personal`` of each agent when the
    tick began. Of a walk with ``slide`` also ``slid`` (N, P) float32 - the share of its step each walker spent sliding, 0 where it
    did not, NaN for an empty slot - and ``stopped`` (N, P) uint8 - 1 where the tick left the walker at rest, 4 for an empty slot;
    both are ``None`` when the walk did not slide."""

    def __init__(self, progress, blocked, bumps, close, slid=None, stopped=None):
        self.progress, self.blocked, self.bumps, self.close, self.slid, self.stopped = progress, blocked, bumps, close, slid, stopped


def walk(scenery, agents, store, towards, personal=.6, push=1., keep=.5, agents_push=True, reset=None, out=None, config=None, slide=False):
    """One tick of the walkers. The envs marked in ``reset`` (N,) are emptied and nothing else happens there. Every present walker
    steers at its preferred speed towards its point of ``towards`` (N, P, 2) - a NaN there means "stand", and it never oversteps
    the point within the tick - is pushed away from the bodies within ``personal`` metres of it (the agents too when
    ``agents_push``) with ``push`` m/s at contact, blends the result into its velocity (``keep`` of the old one, 0 <= keep < 1)
    and is then moved by the agents' own contact rule: stopped dead, at the fraction of the step it can take, by the agents where
    they stand, by the other walkers as they move, and by the static walls. Everything a walker reads of another body is that
    body's state when the call began. Returns :class:`Walked`; ``out`` takes the one of an earlier call with the same shapes to
    rewrite. ``fps`` and ``agent_radius`` are the config's.

    A WALKER'S BODY IS A DISC OF THE CONFIG'S ``agent_radius``; another radius is out of scope. AGENTS ARE NOT STOPPED BY WALKERS:
    :func:`physics` does not know them, an agent can walk through one - ``bumps`` and ``close`` are what an env penalises. The
    call is meant to follow :func:`physics`: the agents are met at rest, where they stand. A velocity that does not come out finite
    (a stored NaN, a NaN speed, an infinite target) makes the walker stand for the tick.

    ``slide=True`` or ``dict(bounce=.05)``: a walker that something blocks is not stopped dead but spends the rest of its tick along
    what blocked it, as an agent does under ``cuda.physics(slide=)`` - its velocity deflected off the contact normal with ``bounce``
    (0..1) of it turned outwards, the second move stopped by the agents, by the other walkers where their first move left them and
    by the walls (``MsWalkers``' slide). ``progress``, ``blocked``, ``bumps`` and ``close`` are the plain walk's; the
    result also carries ``slid`` and ``stopped``. A walk nobody is blocked in is the plain walk, bit for bit.

    One launch - a wavefront an env up to 64 slots, a workgroup an env beyond; exact - the rule is written out in
    include/megastep_hip.h (``MsWalkers``) and DESIGN.md 3.37 and the kernel computes it bit for bit. No host synchronisation, and
    with ``out`` nothing is allocated: the call can be captured in a HIP graph. At most 64 agents and 1024 slots an env."""
    n, a = agents.angles.shape
    if (n, a) != (len(scenery.lines), scenery.n_agents):
        raise RuntimeError('agents do not match the scenery')
    if not isinstance(store, Walkers):
        raise RuntimeError('store must be a cuda.Walkers (cuda.walkers(n_envs, n_slots))')
    p = store.positions.shape[1] if isinstance(store.positions, torch.Tensor) and store.positions.ndim == 3 else 0
    if not 1 <= a <= WALK_MAX_AGENTS or not 1 <= p <= WALK_MAX_SLOTS:
        raise RuntimeError(f'walk takes 1 to {WALK_MAX_AGENTS} agents and 1 to {WALK_MAX_SLOTS} slots an env; got A = {a}, P = {p}')
    for name, t, shape in (('store.positions', store.positions, (n, p, 2)), ('store.velocities', store.velocities, (n, p, 2)),
                           ('store.speeds', store.speeds, (n, p)), ('towards', towards, (n, p, 2))):
        if tuple(_check(t, name, torch.float32, len(shape)).shape) != shape:
            raise RuntimeError(f'{name} must be {shape} for these agents and this store; got {tuple(t.shape)}')
    if not isinstance(personal, (int, float)) or not (0 < personal < float('inf')):
        raise RuntimeError(f'personal must be a positive number of metres; got {personal}')
    if not isinstance(push, (int, float)) or not (0 <= push < float('inf')):
        raise RuntimeError(f'push must be a number >= 0; got {push}')
    if not isinstance(keep, (int, float)) or not (0 <= keep < 1):
        raise RuntimeError(f'keep must lie in [0, 1); got {keep}')
    reset = _bytes(reset, 'reset', ((n,),), '(N,)')
    given = [t for t in (reset,) if t is not None]
    dev = _query_device(scenery, agents, store.positions, store.velocities, store.speeds, towards, *given)
    bounce = _bounce(slide)
    sliding = bounce is not None
    result = _result_for(out, (n, a, p, dev) + ((True,) if sliding else ()), 'a walk', lambda: Walked(
        torch.empty((n, p), dtype=torch.float32, device=dev), torch.empty((n, p), dtype=torch.uint8, device=dev),
        torch.empty((n, a), dtype=torch.int32, device=dev), torch.empty((n, a), dtype=torch.int32, device=dev),
        torch.empty((n, p), dtype=torch.float32, device=dev) if sliding else None,
        torch.empty((n, p), dtype=torch.uint8, device=dev) if sliding else None))
    cfg = _cfg(agents, config)
    spec = _lib.MsWalkers(p, store.positions.data_ptr(), store.velocities.data_ptr(), store.speeds.data_ptr(), towards.data_ptr(),
                          reset.data_ptr() if reset is not None else None, float(personal), float(push), float(keep), int(bool(agents_push)),
                          float(cfg.fps), float(cfg.agent_radius), result.progress.data_ptr(), result.blocked.data_ptr(),
                          result.bumps.data_ptr(), result.close.data_ptr(), int(sliding), bounce if sliding else 0.,
                          result.slid.data_ptr() if sliding else None, result.stopped.data_ptr() if sliding else None)
    with _on(dev):
        _lib.check(_lib.lib().ms_walkers(C.byref(scenery._as_struct()), C.byref(agents._plain), C.byref(spec), _stream(dev)))
    return result
