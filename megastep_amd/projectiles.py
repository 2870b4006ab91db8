"""Projectiles: things that fly, bounce off walls and strike agents (kernel: ``csrc/kernels/projectile.h``). No counterpart in the
reference, whose shots are hit-scan; reached as ``megastep_amd.cuda.<name>``."""
import ctypes as C
import torch
from . import _lib
from ._lib import _on, _stream
from ._call import _cfg, _check, _query_device, _result_for
from .items import Items
from .percepts import _bytes

#: the most slots an env may hold, the most agents an env may have for :func:`fly`, and the most slots an agent may own
PROJ_MAX_SLOTS, PROJ_MAX_AGENTS, PROJ_MAX_PER_AGENT = 1024, 64, 16


class Projectiles(Items):
    """The store of the projectiles, ``P = n_agents*per_agent`` slots an env, agent ``a`` owning slots ``a*S .. a*S + S - 1``:
    ``positions`` (N, P, 2) float32 - a slot is present exactly when both coordinates are finite, as an :class:`Items`' is, and the
    store IS one: :func:`overlay_items`, ``modules.Percepts(points=store.positions)``, :func:`point_marks` and
    ``scene.display(items=store)`` take it as it is; ``velocities`` (N, P, 2) float32, m/s; ``owners``, ``timers`` (ticks left),
    ``bounces`` (bounces left) (N, P) int32; ``colors`` (N, P, 3) float32 linear RGB. Read as items, a projectile's kind is its
    owner. The tensors are the caller's to write: a projectile put there by hand flies at the next :func:`fly`."""

    def __init__(self, positions, velocities, owners, timers, bounces, colors, per_agent):
        super().__init__(positions, timers, owners, colors, max(positions.shape[1]//int(per_agent), 1))
        self.velocities, self.owners, self.bounces, self.per_agent = velocities, owners, bounces, int(per_agent)

    n_slots = property(lambda self: self.positions.shape[1])


def projectiles(n_envs, n_agents, per_agent, colors=None, device='cuda'):
    """A :class:`Projectiles` of ``per_agent`` (1..16) slots for each of ``n_agents`` (1..64) agents in each of ``n_envs`` envs, all
    absent. ``colors``: (3,), (P, 3) or (N, P, 3) linear RGB, default white."""
    ok = all(isinstance(v, int) for v in (n_envs, n_agents, per_agent))
    if not ok or n_envs < 1 or not 1 <= n_agents <= PROJ_MAX_AGENTS or not 1 <= per_agent <= PROJ_MAX_PER_AGENT:
        raise RuntimeError(f'projectiles takes n_envs >= 1, 1 to {PROJ_MAX_AGENTS} agents and 1 to {PROJ_MAX_PER_AGENT} slots an agent; '
                           f'got {n_envs}, {n_agents} and {per_agent}')
    p = n_agents*per_agent
    colors = torch.ones(3) if colors is None else torch.as_tensor(colors, dtype=torch.float32)
    if tuple(colors.shape) not in ((3,), (p, 3), (n_envs, p, 3)):
        raise RuntimeError(f'colors must be (3,), (P, 3) or (N, P, 3) with (N, P) = ({n_envs}, {p}); got {tuple(colors.shape)}')
    device = torch.device(device)
    zeros = lambda *shape, dtype: torch.zeros((n_envs, p) + shape, dtype=dtype, device=device)
    owners = (torch.arange(p, dtype=torch.int32, device=device)//per_agent).expand(n_envs, p).contiguous()
    return Projectiles(torch.full((n_envs, p, 2), float('nan'), dtype=torch.float32, device=device), zeros(2, dtype=torch.float32), owners,
                       zeros(dtype=torch.int32), zeros(dtype=torch.int32), colors.to(device).expand(n_envs, p, 3).contiguous(), per_agent)


class Flown:
    """Result of :func:`fly`: ``struck`` (N, P) int32 - the agent each projectile hit in this tick, else -1; ``ended`` (N, P) uint8 -
    0 still flying, 1 struck an agent, 2 stopped by a wall, 3 ran out of time, 4 the slot was empty; ``hits`` (N, A) int32 - the
    projectiles that struck each agent; ``scored`` (N, A) int32 - the projectiles of each agent that struck someone; ``misfires``
    (N, A) uint8 - the agent fired with all its slots in flight."""

    def __init__(self, struck, ended, hits, scored, misfires):
        self.struck, self.ended, self.hits, self.scored, self.misfires = struck, ended, hits, scored, misfires


def fly(scenery, agents, store, fire=None, speed=8., muzzle=.25, life=64, bounces=0, restitution=1., reset=None, out=None, config=None):
    """One tick of the projectiles. The envs marked in ``reset`` (N,) are emptied and nothing else happens there. Every agent marked
    in ``fire`` (N, A) with a finite pose shoots from the least of its free slots - ``muzzle`` metres in front of it, along its
    heading, at ``speed`` m/s, with ``life`` ticks and ``bounces`` bounces to go - or misfires when it has none. Then every
    projectile in the store, the fresh ones too, flies ``velocity/fps``: through the air, into an agent that is not its owner
    (``struck``; the projectile is gone), into a wall (gone - or, with bounces left, reflected with ``restitution`` of its speed
    into the wall kept, a bounce a leg and at most four legs a tick), until its timer runs out. PROJECTILES DO NOT MEET EACH OTHER;
    bodies are the agents' outlines as :func:`raycast` sees them. Returns :class:`Flown`; ``out`` takes the one of an earlier call with the same
    shapes to rewrite. ``fps`` is the config's.

    One launch, a workgroup an env; exact - the rule is written out in include/megastep_hip.h (``MsProjectiles``) and DESIGN.md
    3.36 and the kernel computes it bit for bit. No host synchronisation, and with ``out`` nothing is allocated: the call can be
    captured in a HIP graph. At most 64 agents, 16 slots an agent and 1024 slots an env."""
    n, a = agents.angles.shape
    if (n, a) != (len(scenery.lines), scenery.n_agents):
        raise RuntimeError('agents do not match the scenery')
    if not isinstance(store, Projectiles):
        raise RuntimeError('store must be a cuda.Projectiles (cuda.projectiles(n_envs, n_agents, per_agent))')
    s, p = store.per_agent, a*store.per_agent
    if not 1 <= a <= PROJ_MAX_AGENTS or not 1 <= s <= PROJ_MAX_PER_AGENT:
        raise RuntimeError(f'fly takes 1 to {PROJ_MAX_AGENTS} agents an env and 1 to {PROJ_MAX_PER_AGENT} slots an agent; got A = {a}, S = {s}')
    for name, dtype, shape in (('positions', torch.float32, (n, p, 2)), ('velocities', torch.float32, (n, p, 2)), ('owners', torch.int32, (n, p)),
                               ('timers', torch.int32, (n, p)), ('bounces', torch.int32, (n, p))):
        if tuple(_check(getattr(store, name), f'store.{name}', dtype, len(shape)).shape) != shape:
            raise RuntimeError(f'store.{name} must be {shape} for these agents; got {tuple(getattr(store, name).shape)}')
    for name, value in (('speed', speed), ('muzzle', muzzle)):
        if not isinstance(value, (int, float)) or not (0 < value < float('inf')):
            raise RuntimeError(f'{name} must be a positive number; got {value}')
    if not isinstance(restitution, (int, float)) or not (0 <= restitution <= 1):
        raise RuntimeError(f'restitution must lie in [0, 1]; got {restitution}')
    if not isinstance(life, int) or not 1 <= life < 2**31 or not isinstance(bounces, int) or not 0 <= bounces < 2**31:
        raise RuntimeError(f'life must be an integer >= 1 and bounces one >= 0; got {life} and {bounces}')
    fire = _bytes(fire, 'fire', ((n, a),), '(N, A)')
    reset = _bytes(reset, 'reset', ((n,),), '(N,)')
    given = [t for t in (fire, reset) if t is not None]
    dev = _query_device(scenery, agents, store.positions, store.velocities, store.owners, store.timers, store.bounces, *given)
    result = _result_for(out, (n, a, p, dev), 'a fly', lambda: Flown(
        torch.empty((n, p), dtype=torch.int32, device=dev), torch.empty((n, p), dtype=torch.uint8, device=dev),
        torch.empty((n, a), dtype=torch.int32, device=dev), torch.empty((n, a), dtype=torch.int32, device=dev),
        torch.empty((n, a), dtype=torch.uint8, device=dev)))
    ptr = lambda t: t.data_ptr() if t is not None else None
    spec = _lib.MsProjectiles(p, s, store.positions.data_ptr(), store.velocities.data_ptr(), store.owners.data_ptr(), store.timers.data_ptr(),
                              store.bounces.data_ptr(), ptr(fire), ptr(reset), float(speed), float(muzzle), life, bounces, float(restitution),
                              float(_cfg(agents, config).fps), result.struck.data_ptr(), result.ended.data_ptr(), result.hits.data_ptr(),
                              result.scored.data_ptr(), result.misfires.data_ptr())
    with _on(dev):
        _lib.check(_lib.lib().ms_projectiles(C.byref(scenery._as_struct()), C.byref(agents._plain), C.byref(spec), _stream(dev)))
    return result
