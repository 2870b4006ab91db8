"""Items: things in the world that agents see, touch and collect (kernels: ``csrc/kernels/items.h``). No counterpart in the
reference; reached as ``megastep_amd.cuda.<name>``."""
import ctypes as C
import torch
from . import _lib
from ._lib import _on, _stream
from ._call import _cfg, _check, _query_device, _require_gpu, _result_for
from .percepts import _bytes

#: the most items an env may hold, the most agents an env may have for :func:`collect_items`, and the most kinds of item
ITEM_MAX_ITEMS, ITEM_MAX_AGENTS, ITEM_MAX_KINDS = 1024, 64, 8


class Items:
    """The store of the items, ``P`` an env: ``positions`` (N, P, 2) float32 - AN ITEM IS PRESENT EXACTLY WHEN BOTH COORDINATES ARE
    FINITE, an absent one holds (NaN, NaN), which ``point_marks`` marks nothing for, :func:`percepts` never sees and no ray of
    :func:`overlay_items` hits: no consumer needs a ``valid`` mask; ``timers`` (N, P) int32 - the :func:`collect_items` calls left
    until an absent item is due to return, negative: never; ``kinds`` (N, P) int32 in ``[0, n_kinds)``; ``colors`` (N, P, 3) float32
    linear RGB. The tensors are the caller's to move, recolour and refill in place."""

    def __init__(self, positions, timers, kinds, colors, n_kinds):
        self.positions, self.timers, self.kinds, self.colors, self.n_kinds = positions, timers, kinds, colors, int(n_kinds)

    n_envs = property(lambda self: self.positions.shape[0])
    n_items = property(lambda self: self.positions.shape[1])

    def present(self):
        """(N, P) bool: the items that are there."""
        return torch.isfinite(self.positions).all(-1)


def items(n_envs, n_items, kinds=None, colors=None, n_kinds=None, device='cuda'):
    """An :class:`Items` of ``n_items`` (1..1024) items in each of ``n_envs`` envs, all of them absent and due (timer 0): the first
    :func:`collect_items` reports them, the first :func:`place_items` puts them down. ``kinds``: (P,) or (N, P) integers in
    ``[0, n_kinds)``, default all 0; ``n_kinds`` (1..8) defaults to the largest kind given plus one. ``colors``: (3,), (P, 3) or
    (N, P, 3) linear RGB, default white."""
    if not isinstance(n_envs, int) or n_envs < 1 or not isinstance(n_items, int) or not 1 <= n_items <= ITEM_MAX_ITEMS:
        raise RuntimeError(f'items takes n_envs >= 1 and 1 to {ITEM_MAX_ITEMS} items an env; got {n_envs} and {n_items}')
    kinds = torch.zeros(n_items, dtype=torch.int32) if kinds is None else torch.as_tensor(kinds)
    if kinds.dtype.is_floating_point or kinds.dtype == torch.bool or tuple(kinds.shape) not in ((n_items,), (n_envs, n_items)):
        raise RuntimeError(f'kinds must be (P,) or (N, P) = ({n_envs}, {n_items}) integers; got {tuple(kinds.shape)} {kinds.dtype}')
    top = int(kinds.max()) + 1
    n_kinds = top if n_kinds is None else n_kinds
    if not isinstance(n_kinds, int) or not 1 <= n_kinds <= ITEM_MAX_KINDS or int(kinds.min()) < 0 or top > n_kinds:
        raise RuntimeError(f'kinds must lie in [0, n_kinds) with 1 <= n_kinds <= {ITEM_MAX_KINDS}; got kinds up to {top - 1} and n_kinds = {n_kinds}')
    colors = torch.ones(3) if colors is None else torch.as_tensor(colors, dtype=torch.float32)
    if tuple(colors.shape) not in ((3,), (n_items, 3), (n_envs, n_items, 3)):
        raise RuntimeError(f'colors must be (3,), (P, 3) or (N, P, 3) with (N, P) = ({n_envs}, {n_items}); got {tuple(colors.shape)}')
    device = torch.device(device)
    return Items(torch.full((n_envs, n_items, 2), float('nan'), dtype=torch.float32, device=device),
                 torch.zeros((n_envs, n_items), dtype=torch.int32, device=device),
                 kinds.to(device=device, dtype=torch.int32).expand(n_envs, n_items).contiguous(),
                 colors.to(device).expand(n_envs, n_items, 3).contiguous(), n_kinds)


def _store(store, n):
    """The checks of a store every call makes: (N, P)."""
    if not isinstance(store, Items):
        raise RuntimeError('items must be a cuda.Items (cuda.items(n_envs, n_items))')
    _check(store.positions, 'items.positions', torch.float32, 3)
    _check(store.timers, 'items.timers', torch.int32, 2)
    _check(store.kinds, 'items.kinds', torch.int32, 2)
    _check(store.colors, 'items.colors', torch.float32, 3)
    p = store.positions.shape[1]
    if tuple(store.positions.shape) != (n, p, 2) or tuple(store.timers.shape) != (n, p) or tuple(store.kinds.shape) != (n, p) or \
            tuple(store.colors.shape) != (n, p, 3) or not 1 <= p <= ITEM_MAX_ITEMS:
        raise RuntimeError(f'the items must be positions (N, P, 2), timers (N, P), kinds (N, P) and colors (N, P, 3) with N = {n} and 1 <= P <= '
                           f'{ITEM_MAX_ITEMS}; got {tuple(store.positions.shape)}, {tuple(store.timers.shape)}, {tuple(store.kinds.shape)}, '
                           f'{tuple(store.colors.shape)}')
    return p


class Collected:
    """Result of :func:`collect_items`: ``taker`` (N, P) int32 - the agent that took each item in this call, -1 for none; ``counts``
    (N, A, K) int32 - the items of each kind each agent took in this call; ``due`` (N, P) bool - the items that are absent now with
    nothing left on their timer: :func:`place_items`' mask."""

    def __init__(self, taker, counts, due):
        self.taker, self.counts, self.due = taker, counts, due


def collect_items(scenery, agents, items, reach, delay=0, takers=None, reset=None, through_walls=False, out=None):
    """One step of the items' life: every present item within ``reach`` metres of an agent that may take it (``takers`` (N, A) bool
    or uint8, default everyone) and - unless ``through_walls`` - with no static wall between the two is TAKEN by the nearest such
    agent (equal distances: the lower index): it becomes absent, (NaN, NaN), with ``delay`` on its timer. An item that was absent
    already has a positive timer lowered by one. ``reset`` (N,) bool or uint8: the marked envs' items all become absent with timer
    0 instead, and nothing is collected there. Returns :class:`Collected`; ``out`` takes the one of an earlier call with the same
    shapes to rewrite. BODIES DO NOT OCCLUDE; the wall test is :func:`percepts`', by its own device function.

    One launch, a wave an env; exact - the rule is written out in include/megastep_hip.h (``MsItemCollect``) and DESIGN.md 3.34 and
    the kernel computes it bit for bit. No host synchronisation, and with ``out`` nothing is allocated: the call can be captured
    in a HIP graph. At most 64 agents and 1024 items an env."""
    n, a = agents.angles.shape
    if (n, a) != (len(scenery.lines), scenery.n_agents):
        raise RuntimeError('agents do not match the scenery')
    if not 1 <= a <= ITEM_MAX_AGENTS:
        raise RuntimeError(f'collect_items takes 1 to {ITEM_MAX_AGENTS} agents an env; got A = {a}')
    p = _store(items, n)
    if not isinstance(reach, (int, float)) or not (0 < reach < float('inf')):
        raise RuntimeError(f'reach must be a positive number; got {reach}')
    if not isinstance(delay, int) or not -2**31 <= delay < 2**31:
        raise RuntimeError(f'delay must be an integer that fits 32 bits; got {delay}')
    takers = _bytes(takers, 'takers', ((n, a),), '(N, A)')
    reset = _bytes(reset, 'reset', ((n,),), '(N,)')
    given = [t for t in (takers, reset) if t is not None]
    dev = _query_device(scenery, agents, items.positions, items.timers, items.kinds, *given)
    k = items.n_kinds
    result = _result_for(out, (n, a, p, k, dev), 'a collect_items', lambda: Collected(
        torch.empty((n, p), dtype=torch.int32, device=dev), torch.empty((n, a, k), dtype=torch.int32, device=dev),
        torch.empty((n, p), dtype=torch.bool, device=dev)))
    ptr = lambda t: t.data_ptr() if t is not None else None
    spec = _lib.MsItemCollect(p, k, items.positions.data_ptr(), items.timers.data_ptr(), items.kinds.data_ptr(), ptr(takers), ptr(reset),
                              float(reach), delay, int(bool(through_walls)), result.taker.data_ptr(), result.counts.data_ptr(),
                              result.due.data_ptr())
    with _on(dev):
        _lib.check(_lib.lib().ms_item_collect(C.byref(scenery._as_struct()), C.byref(agents._plain), C.byref(spec), _stream(dev)))
    return result


def place_items(items, draws, due):
    """The return of the due items: ``draws.again(mask=due)`` on a ``cell_draws(grid, source, n_sets=P, n_draws=1, ...)`` - the
    source and the gate are the caller's: the free cells, a clearance band, what a view field does not see - then each due item
    takes its set's drawn point. An item whose draw found no cell stays (NaN, NaN) with timer 0 and is due again at the next
    :func:`collect_items`. One launch and one select, no host synchronisation, nothing allocated: with the collect before it the
    three steps sit in one HIP graph, and every replay draws afresh. Returns ``items``."""
    n, p = items.positions.shape[:2]
    if tuple(draws.cells.shape) != (n, p, 1):
        raise RuntimeError(f'draws must be a cell_draws of n_sets = P = {p} and n_draws = 1 over {n} envs; got {tuple(draws.cells.shape)}')
    if not isinstance(due, torch.Tensor) or due.dtype != torch.bool or tuple(due.shape) != (n, p):
        raise RuntimeError(f'due must be an (N, P) = ({n}, {p}) bool tensor (Collected.due)')
    _require_gpu(items.positions, draws.points, due)
    draws.again(mask=due)
    torch.where(due[:, :, None], draws.points[:, :, 0], items.positions, out=items.positions)
    return items


def overlay_items(items, frame, agents=None, origins=None, dirs=None, radius=.1, near=None, out_items=None, scenery=None, config=None):
    """Draws the items into a frame of rays, in place: ``frame`` is a :class:`Render` - then ``agents`` are the ones it was rendered
    for: the origins are their positions, the rays :func:`camera_rays` - or a :class:`Raycast` - then ``origins`` and ``dirs`` are
    the (N, R, 2) tensors it was cast with. Seen from a ray's origin an item is a segment of length ``2*radius`` that always faces
    it; it is folded by :func:`raycast`'s own rule (``near`` as there, default the config's ``agent_radius``) and replaces the ray
    where it is strictly nearer than what the frame holds: ``distances``; ``screen`` - the item's colour times ``1 - dot^2``, items
    are emissive; ``indices`` - the env's number of lines plus the item's number, no line of the env (:func:`shade` leaves such a
    ray black); ``locations``; ``dots`` - each where the frame has it. So an agent's body nearer than the item hides it and an item
    nearer than a wall hides the wall. The frame gains ``.items`` (its planes' shape, int32): the item each ray shows, else -1
    (``out_items``: the tensor to write it into).

    ``dirs`` may be given with a :class:`Render` too (the ``camera_rays(agents)`` of the frame, kept from an earlier call - then
    nothing is allocated); ``scenery``: the one the frame was made against, where the frame does not remember it. One launch, a workgroup
    up to 256 rays of one origin; exact - include/megastep_hip.h (``MsItemOverlay``), DESIGN.md 3.34. No host synchronisation; the
    call can be captured in a HIP graph. Returns ``frame``."""
    from . import cuda
    from .rays import Raycast, camera_rays
    if not isinstance(frame, (cuda.Render, Raycast)):
        raise RuntimeError('frame must be a cuda.Render or a cuda.Raycast')
    planes = frame.distances
    if planes is None:
        raise RuntimeError('the frame has no distances: the overlay needs them to know what an item hides')
    n = planes.shape[0]
    p = _store(items, n)
    if isinstance(frame, cuda.Render):
        if agents is None or origins is not None:
            raise RuntimeError('a Render needs agents= (and no origins): its rays start at their positions')
        if tuple(planes.shape[:2]) != tuple(agents.angles.shape):
            raise RuntimeError('agents do not match the frame')
        origins = agents.positions
        if dirs is None:
            dirs = camera_rays(agents, config)
        dirs = dirs.view(n, -1, 2) if isinstance(dirs, torch.Tensor) and dirs.ndim == 4 else dirs
    elif origins is None or dirs is None:
        raise RuntimeError('a Raycast needs origins= and dirs=, the tensors it was cast with')
    _check(origins, 'origins', torch.float32, 3)
    _check(dirs, 'dirs', torch.float32, 3)
    r, q = planes[0].numel(), origins.shape[1]
    if tuple(dirs.shape) != (n, r, 2) or tuple(origins.shape) != (n, q, 2) or q < 1 or r % q:
        raise RuntimeError(f'dirs must be (N, R, 2) = ({n}, {r}, 2) and origins (N, Q, 2) with R % Q == 0; got {tuple(dirs.shape)} and {tuple(origins.shape)}')
    if scenery is None:
        scenery = getattr(frame, '_scenery', None)
    if scenery is None:
        raise RuntimeError('overlay_items needs scenery= (the one the frame was rendered or cast against)')
    if len(scenery.lines) != n:
        raise RuntimeError('the scenery does not match the frame')
    if not isinstance(radius, (int, float)) or not (0 < radius < float('inf')):
        raise RuntimeError(f'radius must be a positive number; got {radius}')
    if near is None:
        near = _cfg(agents, config).agent_radius
    if not near >= 0:
        raise RuntimeError('near must be a non-negative number')
    wanted = [t for t in (frame.indices, frame.locations, frame.dots, getattr(frame, 'screen', None)) if t is not None]
    if any(not t.is_contiguous() for t in (planes, *wanted)):
        raise RuntimeError('the frame\'s planes must be contiguous')
    dev = _query_device(scenery, agents, items.positions, items.colors, origins, dirs, planes, *wanted)
    if out_items is None:
        out_items = torch.empty(planes.shape, dtype=torch.int32, device=dev)
    elif not isinstance(out_items, torch.Tensor) or out_items.dtype != torch.int32 or out_items.shape != planes.shape or \
            not out_items.is_contiguous() or out_items.device != dev:
        raise RuntimeError(f'out_items must be a contiguous int32 tensor of shape {tuple(planes.shape)} on {dev}')
    ptr = lambda t: t.data_ptr() if t is not None else None
    spec = _lib.MsItemOverlay(p, r, q, items.positions.data_ptr(), items.colors.data_ptr(), origins.data_ptr(), dirs.data_ptr(), float(radius),
                              float(near), planes.data_ptr(), ptr(frame.indices), ptr(frame.locations), ptr(frame.dots),
                              ptr(getattr(frame, 'screen', None)), out_items.data_ptr())
    with _on(dev):
        _lib.check(_lib.lib().ms_item_overlay(C.byref(scenery._as_struct()), C.byref(spec), _stream(dev)))
    frame.items = out_items
    return frame
