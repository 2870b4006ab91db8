"""Navigation grids, shortest-path distance fields (to a goal, or to the nearest of a set of cells), waypoints and paths on the
floorplans, the seen maps of the depth rays, windows of all of them as images round the agents, and random draws of cells by what
they hold (kernels: ``csrc/kernels/navfield.h``, ``csrc/kernels/navpath.h``, ``csrc/kernels/navpull.h`` - paths pulled straight
and their lengths -, ``csrc/kernels/navseen.h``, ``csrc/kernels/navage.h``
- when each cell was last seen -, ``csrc/kernels/navwindow.h``,
``csrc/kernels/navdraw.h``), the connected regions of any per-cell mask (``csrc/kernels/navregion.h``), the cells in sight of a
point (``csrc/kernels/navview.h``), the seed each cell of a seeded field leads to (``csrc/kernels/navbasin.h``), per-zone counts, least values and nearest cells of any labels (``csrc/kernels/navzone.h``), and
the distance to the nearest wall, per cell and per point (``csrc/kernels/navclear.h``).
No counterpart in the reference;
reached as ``megastep_amd.cuda.<name>``."""
import ctypes as C
import torch
from . import _lib
from ._lib import _on, _stream
from ._call import _cfg, _check, _hw, _query_device, _require_gpu, _result_for


# ---------------------------------------------------------------------------------------------------------------------
# the argument rules and the launch the calls below share, each stated once
# ---------------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return t.data_ptr() if t is not None else None


def _some(*tensors):
    """Those of ``tensors`` that were given."""
    return [t for t in tensors if t is not None]


def _new(dev):
    return lambda shape, dtype, fill: torch.full(shape, fill, dtype=dtype, device=dev)


def _same(a, b):
    """Are ``a`` and ``b`` the same memory, or both None: what an ``out`` was made with against what this call was given."""
    return (a is None) == (b is None) and (a is None or a.data_ptr() == b.data_ptr())


def _fits(out, shape, dtype):
    return isinstance(out, torch.Tensor) and out.shape == shape and out.dtype == dtype and out.is_contiguous()


def _mask(mask, n, g, letters, name='mask'):
    """``mask`` as the kernels read it: an (N, G) bool tensor, made contiguous; None stays None."""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.shape != (n, g):
        raise RuntimeError(f'{name} must be an (N, {letters}) = ({n}, {g}) bool tensor')
    return mask.contiguous()


def _index(t, name, n=None, p=None):
    """``t`` as the (N, P) int32 tensor a kernel reads an index per item from - a store, a map, a label, an id: any integer dtype,
    but not bool (that is a mask mistaken for an index), converted only when it is not int32 or not contiguous, so that a tensor
    a result keeps by reference stays the caller's own. ``n``, ``p``: what N and P must be, where the call knows them."""
    if not isinstance(t, torch.Tensor) or t.dtype.is_floating_point or t.dtype == torch.bool or t.ndim != 2 or \
            (n is not None and (t.shape[0] != n or t.shape[1] < 1)) or (p is not None and t.shape[1] != p):
        raise RuntimeError(f'{name} must be an (N, P){"" if p is None else f" = ({n}, {p})"} integer tensor'
                           f'{"" if n is None or p is not None else f" with N = {n}"}')
    return t if t.dtype == torch.int32 and t.is_contiguous() else t.to(torch.int32).contiguous()


def _points(grid, points, name='points'):
    """The rule of the points a call asks at: (N, P, 2) float32 with N the grid's envs and P >= 1; returns (N, P)."""
    _check(points, name, torch.float32, 3)
    n, p = points.shape[:2]
    if n != grid.n_envs or points.shape[2] != 2 or p < 1:
        raise RuntimeError(f'{name} must be (N, P, 2) with N = {grid.n_envs}; got {tuple(points.shape)}')
    return n, p


def _default_store(count, p, message):
    """Without an index item k of ``p`` reads the one store its env has, or store k: ``count`` stores must be 1 or ``p``."""
    if count not in (1, p):
        raise RuntimeError(message)


def _field_rule(field, n, p, g, what):
    """The argument rule of a per-point ``field``: int32 (N, P) or None - then one store an env, or one per point."""
    if field is None:
        return _default_store(g, p, f'without {what}, there must be one field per env or one per point ({p}); there are {g}')
    return _index(field, what, n, p)


def _store_view(grid, store, n_stores, e, k):
    """(ny, nx) view of store ``k`` of env ``e`` in a flat ``store`` of ``n_stores`` an env, row 0 at the lowest y."""
    s, ny, nx = grid.cells(e)
    at = n_stores*s + k*ny*nx
    return store[at:at + ny*nx].reshape(ny, nx)


def _launch(dev, entry, grid, spec, *before):
    """The tail of every call: ``ms_nav_<entry>(*before, grid, spec, stream)`` on ``dev``, its status checked."""
    args = [*before, grid._struct] + ([] if spec is None else [spec])
    with _on(dev):
        _lib.check(getattr(_lib.lib(), 'ms_nav_' + entry)(*(C.byref(a) for a in args), _stream(dev)))


def _static_boxes(scenery):
    """((N, 2) lo, (N, 2) hi) float32: the bounding box of every env's static lines (+inf / -inf for an env without any)."""
    lines = scenery.lines
    vals, starts, inverse = lines.vals, lines.starts.long(), lines.inverse.long()
    n = len(lines.widths)
    af = scenery.n_agents*scenery.model.shape[0]
    static = (torch.arange(vals.shape[0], device=vals.device) - starts[inverse]) >= af
    pts = vals.reshape(-1, 4)
    inf = torch.full((n, 2), float('inf'), dtype=torch.float32, device=vals.device)
    lo_pts = torch.where(static[:, None], torch.minimum(pts[:, :2], pts[:, 2:]), torch.full_like(pts[:, :2], float('inf')))
    hi_pts = torch.where(static[:, None], torch.maximum(pts[:, :2], pts[:, 2:]), torch.full_like(pts[:, :2], -float('inf')))
    index = inverse[:, None].expand(-1, 2)
    return inf.scatter_reduce(0, index, lo_pts, 'amin'), (-inf).scatter_reduce(0, index, hi_pts, 'amax')


def nav_geometry(scenery, cell):
    """The nav grids' placement, on the host: ((N, 4) int32 numpy ``jx0, iy0, nx, ny``, (N + 1,) int64 numpy cell starts). Env n's
    grid covers the bounding box of its static walls and one cell of margin round it: columns ``floor(xmin/c) - 1`` to
    ``floor(xmax/c) + 1``, rows likewise; an env without finite static walls gets no cells."""
    import numpy as np
    lo, hi = (t.double().cpu().numpy() for t in _static_boxes(scenery))
    ok = np.isfinite(lo).all(1) & np.isfinite(hi).all(1)
    c = float(np.float32(cell))
    first = np.floor(np.where(ok[:, None], lo, 0.)/c).astype(np.int64) - 1
    last = np.floor(np.where(ok[:, None], hi, 0.)/c).astype(np.int64) + 1
    size = np.where(ok[:, None], last - first + 1, 0)
    if (np.abs(first) > 2**24).any() or (size > 2**15).any():
        raise RuntimeError(f'a nav grid of {cell} m cells over these walls would be larger than 32768 cells a side')
    geom = np.concatenate([first, size], 1).astype(np.int32)
    starts = np.concatenate([[0], np.cumsum(size[:, 0]*size[:, 1])]).astype(np.int64)
    return geom, starts


class NavGrid:
    """Result of :func:`nav_grid`: which cells of a grid over every env's floorplan keep ``clearance`` metres clear of every
    static wall. ``geom`` (N, 4) int32 ``jx0, iy0, nx, ny``: cell (row i, column j) of env n has its centre at
    ``((jx0 + j) + .5)*cell, ((iy0 + i) + .5)*cell``; ``starts`` (N + 1,) int64: env n's ``nx*ny`` cells are
    ``free[starts[n]:starts[n + 1]]``, row-major (ragged, not padded); ``free`` uint8, 1 free / 0 blocked."""

    def __init__(self, geom, starts, free, cell, clearance, host_geom, host_starts):
        self.geom, self.starts, self.free = geom, starts, free
        self.cell, self.clearance = float(cell), float(clearance)
        self._host_geom, self._host_starts = host_geom, host_starts
        framed = (host_geom[:, 2].astype('int64') + 2)*(host_geom[:, 3].astype('int64') + 2)
        framed = framed[(host_geom[:, 2] > 0) & (host_geom[:, 3] > 0)]
        self._max_framed = int(framed.max()) if len(framed) else 0
        self._max_cells = int(host_geom[:, 2:].astype('int64').prod(1).max(initial=0))        # the largest env's
        self._struct = _lib.MsNavGrid(len(host_geom), self.cell, self.clearance, geom.data_ptr(), starts.data_ptr(), self._max_framed,
                                      free.data_ptr())

    n_envs = property(lambda self: len(self._host_geom))
    #: cells of all envs together
    n_cells = property(lambda self: int(self._host_starts[-1]))

    def cells(self, e):
        """(first cell, ny, nx) of env ``e`` (host numbers: no synchronisation)."""
        return int(self._host_starts[e]), int(self._host_geom[e, 3]), int(self._host_geom[e, 2])

    def image(self, e):
        """(ny, nx) bool: env ``e``'s free cells, row 0 at the lowest y (row i holds the cells centred at ``y = ((iy0 + i) + .5)*cell``):
        the convention of :meth:`SeenMaps.image` and :meth:`DistanceFields.image`."""
        s, ny, nx = self.cells(e)
        return self.free[s:s + ny*nx].reshape(ny, nx).bool()

    def centres(self, e):
        """((nx,) x, (ny,) y) float32 of env ``e``'s cell centres, as the kernels form them."""
        jx0, iy0, nx, ny = (int(v) for v in self._host_geom[e])
        dev = self.free.device
        x = (torch.arange(jx0, jx0 + nx, device=dev).float() + .5)*torch.tensor(self.cell, dtype=torch.float32, device=dev)
        y = (torch.arange(iy0, iy0 + ny, device=dev).float() + .5)*torch.tensor(self.cell, dtype=torch.float32, device=dev)
        return x, y


def nav_grid(scenery, cell=.125, clearance=None, config=None):
    """The navigation grid of every env: square cells of ``cell`` metres over the env's static walls, a cell *free* when no
    static wall comes within ``clearance`` metres of its centre (default: the configured ``agent_radius``) - the very rule
    :func:`overhead` draws lines of that half width by. One launch; needs neither :func:`bake` nor the wall grid. The agents'
    own lines are not looked at: the grid is the building, not who is in it.

    ``cell`` must be at most ``1.4*clearance``: then no edge between two free cells (and no leg from a point that is itself
    ``clearance`` clear of the walls to a free cell next to it) can cross a wall, however thin or oblique - see
    include/megastep_hip.h (``MsNavGrid``) and DESIGN.md 3.14. Envs are gridded one by one, whether or not they share a
    floorplan."""
    import numpy as np
    if clearance is None:
        clearance = _cfg(explicit=config).agent_radius
    if not (cell > 0 and clearance > 0 and cell < float('inf') and clearance < float('inf')):
        raise RuntimeError('cell and clearance must be positive numbers')
    if np.float32(cell) > np.float32(1.4)*np.float32(clearance):
        raise RuntimeError(f'cell ({cell}) must be at most 1.4 x clearance ({clearance}): a coarser grid could step through a wall')
    dev = scenery._device()
    host_geom, host_starts = nav_geometry(scenery, cell)
    geom = torch.as_tensor(host_geom, device=dev).contiguous()
    starts = torch.as_tensor(host_starts, device=dev).contiguous()
    free = torch.zeros(max(int(host_starts[-1]), 1), dtype=torch.uint8, device=dev)
    grid = NavGrid(geom, starts, free, cell, clearance, host_geom, host_starts)
    _launch(dev, 'free', grid, None, scenery._as_struct())
    return grid


#: the framed cells - ``(nx + 2)*(ny + 2)`` - an env may have for :func:`distance_fields` and :func:`seeded_fields` to relax it in
#: LDS, for each of the kernel's three instantiations (40, 80 and 160 KiB); the launch is the least that holds the grid's largest
#: env, and a larger env is relaxed in global memory, to the same bits
FIELD_CAPACITY = (8176, 16368, 32752)


class _Fields:
    """What :class:`DistanceFields` and :class:`SeededFields` share: the flat store of ``n_goals`` fields per env, its views, the
    query and the argument rules of the calls that follow the fields. A subclass names its own tensors (``_own``) and makes the
    two launches that differ (``_waypoints_call``, ``_paths_call``: the entry's name, the grid and the filled-in spec)."""

    def image(self, e, g=0):
        """(ny, nx) float32 view of field ``g`` of env ``e``, row 0 at the lowest y."""
        return _store_view(self.grid, self.values, self.n_goals, e, g)

    def at(self, points, goal=None, out=None):
        """(N, P) float32: the distance from each of ``points`` (N, P, 2) to a goal of its env - ``goal`` (N, P) integers name
        the field each point asks, default point k against field k (then P must be G). The distance is the least, over the
        (at most four) free cells round the point, of the cell's value plus the straight leg to its centre: continuous
        enough that an agent's progress per step is not quantised to cells. +inf where no path exists. Meant for points
        that are themselves ``clearance`` clear of the walls (an agent's centre, a spawn point): the leg of any other point
        may cross a wall. One launch, no host synchronisation."""
        n, p, goal, dev = self._queries(points, goal)
        out = _answer(out, (n, p), dev)
        _launch(dev, 'query', self.grid, _lib.MsNavQuery(p, points.data_ptr(), _ptr(goal), self.values.data_ptr(), self.n_goals, out.data_ptr()))
        return out

    def _queries(self, points, goal):
        """The argument rules of :meth:`at` and of the calls that follow the fields: (n, p, goal as int32 or None, device)."""
        n, p = _points(self.grid, points)
        if goal is not None:
            goal = _index(goal, 'goal', n, p)
        elif p != self.n_goals:
            raise RuntimeError(f'without goal, points must be one per field ({self.n_goals}); got {p}')
        return n, p, goal, _require_gpu(points, self.values, *self._own(), self.grid.free, *_some(goal))

    def waypoints(self, points, goal=None, lookahead=16, hops=False, out=None):
        """(N, P, 2) float32: where to head for from each of ``points`` (N, P, 2) to walk to its goal (``goal``: as :meth:`at`) -
        the furthest of the next ``lookahead`` (1..64) cells down the field that the point can see in a straight line clear of
        the walls, the goal itself once that is in sight; NaN where no path exists (exactly where :meth:`at` gives +inf).
        Heading for the waypoint, step after step, walks round the walls to the goal, and less far than :meth:`at` says: the
        look-ahead cuts the grid's 8-direction staircase short. ``hops=True`` also returns (N, P) int32: how many cells
        ahead the waypoint is (-1: no path). ``out``: the (N, P, 2) tensor to write. One launch, a wavefront a point, no host
        synchronisation. The rule: include/megastep_hip.h (``MsNavWaypoints``), DESIGN.md 3.15."""
        if not isinstance(lookahead, int) or not 1 <= lookahead <= 64:
            raise RuntimeError(f'lookahead must be an integer in 1..64; got {lookahead}')
        n, p, goal, dev = self._queries(points, goal)
        out = _answer(out, (n, p, 2), dev)
        chosen = torch.empty((n, p), dtype=torch.int32, device=dev) if hops else None
        _launch(dev, *self._waypoints_call(p, points.data_ptr(), _ptr(goal), lookahead, out.data_ptr(), _ptr(chosen)))
        return (out, chosen) if hops else out

    def paths(self, points, goal=None, max_points=256):
        """The whole path from each of ``points`` (N, P, 2) to its goal (``goal``: as :meth:`at`), as a :class:`Paths`: the point,
        the centres of the cells down the field, the goal; the first ``max_points`` of them written. One launch, a lane a
        path, no host synchronisation; for drawing and for scoring, not for every step - that is :meth:`waypoints`."""
        if not isinstance(max_points, int) or not 2 <= max_points <= 2**20:
            raise RuntimeError(f'max_points must be an integer in 2..2^20; got {max_points}')
        n, p, goal, dev = self._queries(points, goal)
        pts = torch.empty((n, p, max_points, 2), dtype=torch.float32, device=dev)
        counts = torch.empty((n, p), dtype=torch.int32, device=dev)
        _launch(dev, *self._paths_call(p, points.data_ptr(), _ptr(goal), max_points, pts.data_ptr(), counts.data_ptr()))
        return Paths(pts, counts)

    def pulled(self, points, goal=None, reach=256, max_points=64, indices=False, mask=None, out=None):
        """The path from each of ``points`` (N, P, 2) to its goal (``goal``: as :meth:`at`) pulled straight, as a
        :class:`PulledPaths`: of :meth:`paths`' points - the point, the centres of the cells down the field, the goal - the
        corners that are left when, from the point on, each vertex is followed by the furthest of the next ``reach`` (1..1024)
        points it can see in a straight line clear of the walls (:meth:`waypoints`' sight), or by the chain's own next point when
        it sees none. A handful of vertices where the chain has hundreds of points, the first ``max_points`` (2..2^20) of them
        written; and ``lengths``, the length of the walk along ALL of them: some 5 % below :meth:`at`, whose 8-direction metric
        overstates open floor - the any-angle length a score such as SPL divides by. This is greedy string pulling: an upper
        bound on the true shortest walk, not that walk. ``reach=1`` keeps every point: the chain itself.

        ``indices=True`` also records each vertex's index in the chain; ``mask`` (N, P) bool: pull only the marked points, the
        others keep what ``out`` held; ``out``: a :class:`PulledPaths` of an earlier call with the same shapes to rewrite in
        place. One launch, a wavefront a path, no host synchronisation: the call can be captured in a HIP graph. The rule:
        include/megastep_hip.h (``MsNavPulls``), DESIGN.md 3.26."""
        if not isinstance(reach, int) or not 1 <= reach <= 1024:
            raise RuntimeError(f'reach must be an integer in 1..1024; got {reach}')
        if not isinstance(max_points, int) or not 2 <= max_points <= 2**20:
            raise RuntimeError(f'max_points must be an integer in 2..2^20; got {max_points}')
        n, p = _points(self.grid, points)
        mask = _mask(mask, n, p, 'P')
        if out is not None and (not isinstance(out, PulledPaths) or out.points.shape != (n, p, max_points, 2) or
                                (out.indices is None) == bool(indices)):
            raise RuntimeError(f'`out` must be the PulledPaths of a call with the same shapes: ({n}, {p}) paths of {max_points} vertices, '
                               f'{"with" if indices else "without"} indices')
        n, p, goal, dev = self._queries(points, goal)
        if out is None:
            new = _new(dev)
            out = PulledPaths(new((n, p, max_points, 2), torch.float32, float('nan')), new((n, p), torch.int32, 0),
                              new((n, p), torch.float32, float('inf')), new((n, p), torch.int32, 0),
                              new((n, p, max_points), torch.int32, -1) if indices else None)
        _require_gpu(points, *out._own(), *_some(mask))
        _launch(dev, *self._pulls_call((p, points.data_ptr(), _ptr(goal)),
                                       (reach, max_points, _ptr(mask), out.points.data_ptr(), _ptr(out.indices), out.counts.data_ptr(),
                                        out.cells.data_ptr(), out.lengths.data_ptr())))
        return out


class DistanceFields(_Fields):
    """Result of :func:`distance_fields`: for each env ``G`` fields, field (n, g) holding for every cell of env n's grid the
    length of the shortest 8-connected path from the cell's centre to ``goals[n, g]`` (+inf on blocked cells and on cells no
    path reaches). ``values`` is the flat float32 store: field (n, g) starts at ``G*grid.starts[n] + g*nx*ny``."""

    def __init__(self, grid, goals, values, passes=None):
        self.grid, self.goals, self.values, self.passes = grid, goals, values, passes

    n_goals = property(lambda self: self.goals.shape[1])

    def _own(self):
        return (self.goals,)

    def _waypoints_call(self, p, points, goal, lookahead, out, hops):
        return 'waypoints', self.grid, _lib.MsNavWaypoints(p, points, goal, self.values.data_ptr(), self.goals.data_ptr(), self.n_goals, lookahead, out, hops)

    def _paths_call(self, p, points, goal, max_points, out, counts):
        return 'paths', self.grid, _lib.MsNavPaths(p, points, goal, self.values.data_ptr(), self.goals.data_ptr(), self.n_goals, max_points, out, counts)

    def _pulls_call(self, query, rest):
        return 'pulls', self.grid, _lib.MsNavPulls(*query, self.values.data_ptr(), self.goals.data_ptr(), self.n_goals, None, 0, *rest)

    def update(self, goals=None, mask=None):
        """Recomputes the fields marked in the (N, G) bool ``mask`` (default all) in place - for ``goals`` (N, G, 2), which are
        copied into :attr:`goals` where marked, or for the goals as they stand. One launch, no host synchronisation."""
        if goals is not None:
            _check(goals, 'goals', torch.float32, 3)
            if goals.shape != self.goals.shape:
                raise RuntimeError(f'goals must be {tuple(self.goals.shape)}; got {tuple(goals.shape)}')
            if goals is not self.goals:
                if mask is None:
                    self.goals.copy_(goals)
                else:
                    torch.where(mask[..., None], goals, self.goals, out=self.goals)
        _nav_fields_call(self, mask)
        return self


def _answer(out, shape, dev):
    """The tensor a query writes its (N, P[, 2]) answer to: ``out`` if it fits, a fresh one without."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if not _fits(out, shape, torch.float32) or out.device != dev:
        raise RuntimeError(f"`out` must be a contiguous (N, P{', 2'*(len(shape) - 2)}) float32 tensor on the fields' device")
    return out


class Paths:
    """Result of :meth:`DistanceFields.paths`. ``points`` (N, P, M, 2) float32: path (e, k)'s points - where it starts, cell
    centre after cell centre, the goal - NaN in the slots not written; ``counts`` (N, P) int32: the points of the whole path,
    which may be more than the M written; 0 where no path exists; negative (the points got, negated) where the field did not
    lead to its goal - a stale field, or one of another grid."""

    def __init__(self, points, counts):
        self.points, self.counts = points, counts

    def path(self, e, k):
        """(n, 2): the written points of path ``k`` of env ``e`` (synchronises: n comes from the device)."""
        n = min(abs(int(self.counts[e, k])), self.points.shape[2])
        return self.points[e, k, :n]


class PulledPaths(Paths):
    """Result of :meth:`DistanceFields.pulled`: a :class:`Paths` of the pulled paths' vertices - ``points`` (N, P, M, 2), NaN in the
    slots not written; ``counts`` (N, P) int32: the vertices of the whole pulled path, 0 where no path exists, negated where the
    field did not lead to its goal - and ``lengths`` (N, P) float32: the length of the walk along all the vertices, +inf where no
    path exists; ``cells`` (N, P) int32: the points of the chain that was pulled, :meth:`DistanceFields.paths`' count; ``indices``
    (N, P, M) int32 or None: each written vertex's index in that chain, -1 in the slots not written."""

    def __init__(self, points, counts, lengths, cells, indices=None):
        super().__init__(points, counts)
        self.lengths, self.cells, self.indices = lengths, cells, indices

    def _own(self):
        return _some(self.points, self.counts, self.lengths, self.cells, self.indices)


def _nav_fields_call(fields, mask):
    grid = fields.grid
    n, g = fields.goals.shape[:2]
    mask = _mask(mask, n, g, 'G')
    dev = _require_gpu(fields.goals, fields.values, grid.free, *_some(mask))
    _launch(dev, 'fields', grid, _lib.MsNavFields(g, fields.goals.data_ptr(), _ptr(mask), fields.values.data_ptr(), _ptr(fields.passes)))


def distance_fields(grid, goals, mask=None, out=None, passes=False):
    """Shortest-path distance fields on the :func:`nav_grid`: for every env and each of its ``G`` goals (``goals``: (N, G, 2)
    float32 world points) the distance from every free cell to the goal along the grid's 8-connected graph - straight steps
    of ``cell``, diagonal steps of ``cell*1.41421356`` that cut no corner - joined to the goal by the straight legs from the
    free cells round it. The 8-connected metric is up to 8 % longer than the true (any-angle) shortest path in open space;
    an agent that heads for :meth:`DistanceFields.waypoints` cuts the staircase short and walks less than the field says, and
    :meth:`DistanceFields.pulled` gives the length of the path pulled straight.
    One launch, one workgroup per field, the field relaxed in LDS until nothing changes; the result does not depend on the
    order of relaxation and equals Dijkstra's with binary32 additions bit for bit (include/megastep_hip.h, ``MsNavGrid``).

    ``mask`` (N, G) bool: compute only the marked fields (the others keep what ``out`` held); ``out``: the
    :class:`DistanceFields` of an earlier call with the same grid and G to write into (its goals are updated where marked);
    ``passes=True`` also records the relaxation passes each field took (``.passes``, (N, G) int32). No host synchronisation:
    the call can be captured in a HIP graph."""
    _check(goals, 'goals', torch.float32, 3)
    n, g = goals.shape[:2]
    if n != grid.n_envs or g < 1 or goals.shape[2] != 2:
        raise RuntimeError(f'goals must be (N, G, 2) with N = {grid.n_envs} and G >= 1; got {tuple(goals.shape)}')
    if out is not None:
        if out.grid is not grid or out.goals.shape != goals.shape:
            raise RuntimeError('`out` must come from a distance_fields call with the same grid and number of goals')
        return out.update(goals, mask)
    dev = goals.device
    values = torch.empty(max(g*grid.n_cells, 1), dtype=torch.float32, device=dev)
    if mask is not None:
        values.fill_(float('inf'))                                      # (a field never computed is a field nothing reaches)
    fields = DistanceFields(grid, goals.clone(), values, torch.zeros((n, g), dtype=torch.int32, device=dev) if passes else None)
    _nav_fields_call(fields, mask)
    return fields


def geodesic(grid, a, b):
    """(N, P) float32: the walking distance from ``a[n, k]`` to ``b[n, k]`` (both (N, P, 2)) - the fields of ``b``, asked at
    ``a``. A convenience for a handful of pairs; keep the :func:`distance_fields` when the goals stay."""
    return distance_fields(grid, b).at(a)


class SeededFields(_Fields):
    """Result of :func:`seeded_fields`: for each env ``G`` fields, field (n, g) holding for every cell of env n's grid the length
    of the shortest 8-connected path from the cell's centre to the NEAREST seed of that field (0 on the seeds, +inf on blocked
    cells, on cells no seed reaches and everywhere when the field has no seed). ``values`` is the flat float32 store, in
    :class:`DistanceFields`' layout; ``marks`` the byte per cell and field the seeds are read from - kept by reference, so
    :meth:`update` sees them as they stand; ``n_seeds`` (N, G) int32: the seeds each field had when it was last computed;
    ``passes`` (N, G) int32 or None. :meth:`at`, :meth:`waypoints` and :meth:`paths` are :class:`DistanceFields`', with one
    change: there is no goal point - a chain ends on the first seed's centre, and a start that stands by a seed is sent to it
    (``hops`` 0). The rule: include/megastep_hip.h (``MsNavSeedFields``), DESIGN.md 3.17."""

    def __init__(self, grid, marks, n_fields, where, among, values, n_seeds, passes=None):
        self.grid, self.marks, self.where, self.among = grid, marks, bool(where), among
        self.values, self.n_seeds, self.passes = values, n_seeds, passes
        self._n_fields = int(n_fields)

    n_goals = property(lambda self: self._n_fields)
    n_fields = n_goals

    def _own(self):
        return ()

    def _waypoints_call(self, p, points, goal, lookahead, out, hops):
        return 'seed_waypoints', self.grid, _lib.MsNavSeedWaypoints(p, points, goal, self.values.data_ptr(), self.n_goals, lookahead, out, hops)

    def _paths_call(self, p, points, goal, max_points, out, counts):
        return 'seed_paths', self.grid, _lib.MsNavSeedPaths(p, points, goal, self.values.data_ptr(), self.n_goals, max_points, out, counts)

    def _pulls_call(self, query, rest):
        return 'pulls', self.grid, _lib.MsNavPulls(*query, self.values.data_ptr(), None, self.n_goals, None, 0, *rest)

    def basins(self, ids=None, n_ids=0, mask=None, out=None, passes=False):
        """:func:`basins` of these fields: which seed each cell leads to."""
        return basins(self, ids=ids, n_ids=n_ids, mask=mask, out=out, passes=passes)

    def update(self, mask=None):
        """Recomputes the fields marked in the (N, G) bool ``mask`` (default all) in place, from :attr:`marks` as they stand now.
        One launch, no host synchronisation."""
        grid, g = self.grid, self.n_goals
        mask = _mask(mask, grid.n_envs, g, 'G')
        dev = _require_gpu(self.marks, self.values, self.n_seeds, grid.free, *_some(self.among, mask, self.passes))
        _launch(dev, 'seed_fields', grid, _lib.MsNavSeedFields(g, self.marks.data_ptr(), int(self.where), _ptr(self.among), _ptr(mask),
                                                               self.values.data_ptr(), _ptr(self.passes), self.n_seeds.data_ptr()))
        return self


def _cell_bytes(t, name, length, what):
    """``t`` as the uint8 tensor a kernel reads a byte per cell from, sharing its memory: a contiguous 1-D uint8 or bool tensor
    of ``length`` entries."""
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.bool) or t.ndim != 1 or not t.is_contiguous():
        raise RuntimeError(f'{name} must be a contiguous 1-dimensional uint8 or bool tensor')
    if t.shape[0] != length:
        raise RuntimeError(f'{name} must have {length} entries, {what}; got {t.shape[0]}')
    return t.view(torch.uint8)


def seeded_fields(grid, marks, n_fields, where=True, among=None, mask=None, out=None, passes=False):
    """Shortest-path distance fields on the :func:`nav_grid` whose sources are a SET of cells: for every env ``n_fields`` fields,
    each the walking distance from every free cell to the nearest seed of that field along :func:`distance_fields`' graph.
    ``marks``: a uint8 or bool tensor of ``n_fields*grid.n_cells`` entries, a byte per cell and field in the layout of
    :attr:`SeenMaps.values` (field (n, g) at ``G*grid.starts[n] + g*nx*ny``) - kept by reference, not copied, so a live seen map
    can be the source. A cell is a seed of its field when it is free, its mark's bit 0 equals ``where``, and - with ``among``,
    a uint8 or bool tensor of one entry per cell of the grid (``grid.free``'s layout) shared by an env's fields - its ``among``
    bit is set. Distance to the nearest door cell, to any of K pickups, to the nearest floor not yet seen
    (:meth:`SeenMaps.frontier_fields`).

    One launch, one workgroup per field: :func:`distance_fields`' relaxation from many sources at 0 instead of a goal's anchors;
    the result does not depend on the order of relaxation and equals a multi-source Dijkstra's with binary32 additions bit for
    bit (include/megastep_hip.h, ``MsNavSeedFields``).

    ``mask`` (N, G) bool: compute only the marked fields (the others keep what ``out`` held; +inf without ``out``); ``out``: the
    :class:`SeededFields` of an earlier call with the same grid, marks and arguments to write into; ``passes=True`` also records
    the relaxation passes each field took. No host synchronisation: the call can be captured in a HIP graph."""
    if not isinstance(n_fields, int) or n_fields < 1:
        raise RuntimeError(f'n_fields must be a positive integer; got {n_fields}')
    marks = _cell_bytes(marks, 'marks', max(n_fields*grid.n_cells, 1), f'a byte per cell and field (n_fields*n_cells = {n_fields}*{grid.n_cells})')
    if among is not None:
        among = _cell_bytes(among, 'among', grid.free.shape[0], 'one per cell of the grid')
    where = bool(where)
    if out is not None:
        if not isinstance(out, SeededFields) or out.grid is not grid or out.n_goals != n_fields or out.where != where or \
                not _same(out.marks, marks) or not _same(out.among, among):
            raise RuntimeError('`out` must come from a seeded_fields call with the same grid, marks, n_fields, where and among')
        return out.update(mask)
    dev = _require_gpu(marks, grid.free, *_some(among))
    values = torch.empty(max(n_fields*grid.n_cells, 1), dtype=torch.float32, device=dev)
    if mask is not None:
        values.fill_(float('inf'))                                      # (a field never computed is a field nothing reaches)
    shape = (grid.n_envs, n_fields)
    fields = SeededFields(grid, marks, n_fields, where, among, values, torch.zeros(shape, dtype=torch.int32, device=dev),
                          torch.zeros(shape, dtype=torch.int32, device=dev) if passes else None)
    return fields.update(mask)


#: the framed cells an env may have for :func:`cost_fields` to relax it in LDS when the launch keeps the cells' multipliers there too
#: (a float, a float and a byte a cell in 40, 80 and 160 KiB); the library's own launch reads them from global memory instead and
#: has :data:`FIELD_CAPACITY`. A larger env is relaxed in global memory, to the same bits
COST_CAPACITY = (4544, 9092, 18196)
#: the dearest a cell can be: a cost above it - +inf, a NaN - counts as this; a cost below 1 counts as 1
COST_MAX = 256.


_WEIGHTED_BASINS = 'basins follow the unweighted hop: they cannot be taken of cost fields (weighted basins are not built)'


class CostFields(SeededFields):
    """Result of :func:`cost_fields`: a :class:`SeededFields` whose steps are weighted by ``cost`` - the flat float32 store of
    ``n_costs`` (1 or G) stores per env, kept by reference as ``marks`` are, so :meth:`update` sees both as they stand. Field
    (n, g) holds the cost of the cheapest 8-connected path from each cell to a seed: a step out of cell v costs its length times
    ``clamp(cost[v], 1, COST_MAX)``. :meth:`at` is the seeded query on the weighted values (the leg from the point to its cell,
    under a cell long, is charged at 1); :meth:`waypoints` and :meth:`paths` descend the weighted field with the weights of the
    cell each hop leaves. The rule: include/megastep_hip.h (``MsNavCostFields``), DESIGN.md 3.24."""

    def __init__(self, grid, marks, n_fields, where, among, cost, n_costs, values, n_seeds, passes=None):
        super().__init__(grid, marks, n_fields, where, among, values, n_seeds, passes)
        self.cost, self.n_costs = cost, int(n_costs)

    def _own(self):
        return (self.cost,)

    def _waypoints_call(self, p, points, goal, lookahead, out, hops):
        return 'cost_waypoints', self.grid, _lib.MsNavCostWaypoints(p, points, goal, self.values.data_ptr(), self.n_goals, lookahead, out, hops,
                                                                    self.cost.data_ptr(), self.n_costs)

    def _paths_call(self, p, points, goal, max_points, out, counts):
        return 'cost_paths', self.grid, _lib.MsNavCostPaths(p, points, goal, self.values.data_ptr(), self.n_goals, max_points, out, counts,
                                                            self.cost.data_ptr(), self.n_costs)

    def _pulls_call(self, query, rest):
        return 'pulls', self.grid, _lib.MsNavPulls(*query, self.values.data_ptr(), None, self.n_goals, self.cost.data_ptr(), self.n_costs, *rest)

    def basins(self, ids=None, n_ids=0, mask=None, out=None, passes=False):
        """Not served: :func:`basins` follow the unweighted hop, which does not descend a weighted field."""
        raise RuntimeError(_WEIGHTED_BASINS)

    def update(self, mask=None):
        """Recomputes the fields marked in the (N, G) bool ``mask`` (default all) in place, from :attr:`marks` and :attr:`cost` as
        they stand now. One launch, no host synchronisation."""
        grid, g = self.grid, self.n_goals
        mask = _mask(mask, grid.n_envs, g, 'G')
        dev = _require_gpu(self.marks, self.cost, self.values, self.n_seeds, grid.free, *_some(self.among, mask, self.passes))
        _launch(dev, 'cost_fields', grid, _lib.MsNavCostFields(g, self.marks.data_ptr(), int(self.where), _ptr(self.among), _ptr(mask),
                                                               self.values.data_ptr(), _ptr(self.passes), self.n_seeds.data_ptr(),
                                                               self.cost.data_ptr(), self.n_costs))
        return self


def _cost_store(grid, cost, n_fields):
    """``cost`` as the flat float32 store the kernels read, sharing its memory, and its stores an env (1 or ``n_fields``)."""
    if isinstance(cost, torch.Tensor):
        values, n_costs = cost, None
    else:
        layer = _layer(cost)
        if layer.field is not None:
            raise RuntimeError("cost must be a layer without a `field`: a cell's cost is its env's or its field's")
        values, n_costs = layer.values, layer.n_fields
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.ndim != 1 or not values.is_contiguous():
        raise RuntimeError('cost must be a contiguous 1-dimensional float32 tensor, or a layer of one')
    lengths = {max(k*grid.n_cells, 1): k for k in (n_fields, 1)}        # (n_fields == 1: one store either way)
    if n_costs is None:
        n_costs = lengths.get(values.shape[0])
    if n_costs not in (1, n_fields) or values.shape[0] < max(n_costs*grid.n_cells, 1):
        raise RuntimeError(f'cost must hold a float per cell ({grid.n_cells} entries: one store an env) or per cell and field '
                           f'({n_fields}*{grid.n_cells}); got {values.shape[0]} entries' + ('' if n_costs is None else f' in {n_costs} stores an env'))
    return values, n_costs


def cost_fields(grid, marks, n_fields, cost, where=True, among=None, mask=None, out=None, passes=False):
    """:func:`seeded_fields` over a per-cell cost layer: weighted shortest paths to the nearest seed. ``cost``: a float32 tensor of
    one entry per cell of the grid (``grid.free``'s layout, shared by an env's fields) or of ``n_fields*grid.n_cells`` entries (the
    fields' layout, a store a field), or any float layer - a :class:`ClearanceFields`, fields, a :func:`cell_layer`; kept by
    reference, as ``marks`` are. A step out of cell v costs its length times ``k_v``, the cell's cost clamped to
    [1, :data:`COST_MAX`] (a NaN counts as the dearest): costs bend paths, they never close a cell - connectivity, the corner rule
    and a waypoint's sight are :func:`seeded_fields`'. A cost of 1 everywhere gives :func:`seeded_fields`' bits.
    :func:`inflation_costs` and :func:`mark_costs` build the usual layers.

    One launch, one workgroup per field, the seeded relaxation with per-cell weights; the result does not depend on the order of
    relaxation and equals a multi-source Dijkstra's with binary32 additions bit for bit (include/megastep_hip.h,
    ``MsNavCostFields``). ``where``, ``among``, ``mask``, ``out`` (a :class:`CostFields` of the same grid, marks,
    cost and arguments), ``passes``: as :func:`seeded_fields`. No host synchronisation: the call can be captured in a HIP graph."""
    if not isinstance(n_fields, int) or n_fields < 1:
        raise RuntimeError(f'n_fields must be a positive integer; got {n_fields}')
    marks = _cell_bytes(marks, 'marks', max(n_fields*grid.n_cells, 1), f'a byte per cell and field (n_fields*n_cells = {n_fields}*{grid.n_cells})')
    if among is not None:
        among = _cell_bytes(among, 'among', grid.free.shape[0], 'one per cell of the grid')
    cost, n_costs = _cost_store(grid, cost, n_fields)
    where = bool(where)
    if out is not None:
        if not isinstance(out, CostFields) or out.grid is not grid or out.n_goals != n_fields or out.where != where or \
                not _same(out.marks, marks) or not _same(out.among, among) or not _same(out.cost, cost) or out.n_costs != n_costs:
            raise RuntimeError('`out` must come from a cost_fields call with the same grid, marks, n_fields, cost, where and among')
        return out.update(mask)
    dev = _require_gpu(marks, cost, grid.free, *_some(among))
    values = torch.empty(max(n_fields*grid.n_cells, 1), dtype=torch.float32, device=dev)
    if mask is not None:
        values.fill_(float('inf'))                                      # (a field never computed is a field nothing reaches)
    shape = (grid.n_envs, n_fields)
    fields = CostFields(grid, marks, n_fields, where, among, cost, n_costs, values, torch.zeros(shape, dtype=torch.int32, device=dev),
                        torch.zeros(shape, dtype=torch.int32, device=dev) if passes else None)
    return fields.update(mask)


def _cost_out(like, out):
    """The float32 tensor a cost builder writes: ``out`` if it fits the layer ``like``, a fresh one without."""
    if out is None:
        return torch.empty(like.shape, dtype=torch.float32, device=like.device)
    if not _fits(out, like.shape, torch.float32) or out.device != like.device:
        raise RuntimeError('`out` must be a contiguous float32 tensor of the layer\'s length, on its device')
    return out


def inflation_costs(clear, radius, weight=4., out=None):
    """An inflation layer for :func:`cost_fields`: ``1 + weight*clamp(1 - d/radius, 0, 1)`` per cell, from ``clear`` - a
    :class:`ClearanceFields` or its flat float32 ``values``, d metres to the nearest wall: 1 from ``radius`` metres out (and where
    the clearance is +inf, beyond its range), rising linearly to ``1 + weight`` at the wall, so that paths keep to the middle
    where there is room. Plain element-wise torch: capturable; ``out``: the tensor of an earlier call to rewrite in place - every
    step is then written into it (it may not be the clearance itself)."""
    d = clear.values if isinstance(clear, ClearanceFields) else clear
    if not isinstance(d, torch.Tensor) or d.dtype != torch.float32:
        raise RuntimeError('clear must be a ClearanceFields or a float32 tensor of distances to the nearest wall')
    if not (radius > 0 and radius < float('inf')) or not (weight >= 0 and weight < float('inf')):
        raise RuntimeError(f'radius must be a positive number and weight a number >= 0; got {radius}, {weight}')
    if out is not None and out.data_ptr() == d.data_ptr():
        raise RuntimeError('`out` must not be the clearance itself')
    out = _cost_out(d, out)
    # every step written into `out`: nothing is allocated but two 0-dimensional tensors - the radius as a tensor makes a true
    # division (by a host scalar torch multiplies by the reciprocal on the device, which is not the formula's bits); so is the 1
    torch.div(d, torch.full((), float(radius), dtype=torch.float32, device=d.device), out=out)
    torch.sub(torch.ones((), dtype=torch.float32, device=d.device), out, out=out)      # (1 - q as written: a NaN keeps its bits)
    return out.clamp_(0, 1).mul_(weight).add_(1)


def mark_costs(layer, on=1., off=256., where=True, gate=None, out=None):
    """A cost layer for :func:`cost_fields` from any byte layer - a :class:`SeenMaps`, a :class:`ViewFields`, a territory mask, a
    :func:`cell_layer`: ``on`` where ``(byte != 0) == where``, ``off`` elsewhere, in the layer's own layout (so a layer of G stores
    an env prices field g by store g). The defaults are known-space planning over a seen map: a seen cell costs 1, an unseen one
    256, and a route crosses unknown floor only when there is no other. ``gate``: a byte layer of the same layout; where its byte
    is 0 the layer says nothing and the cell costs 1. Plain element-wise torch: capturable; ``out``: the tensor of an earlier call to
    write the result into (the mask and the chosen values on the way are torch's temporaries)."""
    layer = _layer(layer, byte=True)
    if layer.is_float:
        raise RuntimeError('mark_costs reads a byte layer (uint8 or bool), not float32')
    if gate is not None:
        gate = _layer(gate, byte=True)
        if gate.is_float or gate.values.shape != layer.values.shape:
            raise RuntimeError("a gate must be a byte layer (uint8 or bool) of the layer's own layout")
    out = _cost_out(layer.values, out)
    # (an exact choice of two values: the mask and the chosen values are torch's temporaries, the result lands in `out`)
    value = torch.where((layer.values != 0) == bool(where), float(on), float(off))
    if gate is not None:
        value = torch.where(gate.values != 0, value, 1.)
    return out.copy_(value)


def _viewers(grid, S, origins, dirs, distances, slot, max_range, reset):
    """The argument rule of the calls that mark what rays pass over in ``S`` maps an env (:meth:`SeenMaps.mark`,
    :meth:`AgeMaps.mark`); returns (N, P, R, slot, reset) as the kernels read them."""
    _check(origins, 'origins', torch.float32, 3)
    _check(dirs, 'dirs', torch.float32, 4)
    _check(distances, 'distances', torch.float32, 3)
    n, p = origins.shape[:2]
    r = dirs.shape[2]
    if n != grid.n_envs or origins.shape[2] != 2 or p < 1 or r < 1 or dirs.shape != (n, p, r, 2) or distances.shape != (n, p, r):
        raise RuntimeError(f'origins, dirs and distances must be (N, P, 2), (N, P, R, 2) and (N, P, R) with N = {grid.n_envs}; got '
                           f'{tuple(origins.shape)}, {tuple(dirs.shape)} and {tuple(distances.shape)}')
    if slot is not None:
        slot = _index(slot, 'slot', n, p)
    elif p != S:
        raise RuntimeError(f'without slot, the viewers must be one per map ({S}); got {p}')
    reset = _mask(reset, n, S, 'S', 'reset')
    if not (0 < max_range < float('inf')):
        raise RuntimeError(f'max_range must be a positive number; got {max_range}')
    return n, p, r, slot, reset


def _render_rays(agents, frame, config):
    """(origins, dirs, distances) of the agents' own camera rays and the ``distances`` of ``frame``, a render of them."""
    from .rays import camera_rays
    dirs = camera_rays(agents, config=config)
    n, a, r = dirs.shape[:3]
    distances = getattr(frame, 'distances', None) if not isinstance(frame, dict) else frame.get('distances')
    if distances is None:
        raise RuntimeError('the frame has no distances: render with fields that include them')
    return agents.positions, dirs, distances.reshape(n, a, r)


#: the most cells an env may have for :func:`seen_maps`: the kernel keeps a call's marks as one bit per cell in LDS (128 KiB)
SEEN_MAX_CELLS = 2**20


class SeenMaps:
    """Result of :func:`seen_maps`: for each env ``S`` maps, map (n, s) holding one byte per cell of env n's grid - 1 where a
    depth ray of a viewer of that map has passed over the cell since the map was last cleared. ``values`` is the flat uint8
    store: map (n, s) starts at ``S*grid.starts[n] + s*nx*ny`` (the layout of :class:`DistanceFields`); ``countable`` the
    uint8 mask (one byte per cell of the grid, shared by an env's maps) of the cells that count; ``totals`` (N, S) int32: the
    countable cells seen; ``n_countable`` (N,) int32: the countable cells there are."""

    def __init__(self, grid, n_maps, values, countable, totals, n_countable):
        self.grid, self.n_maps, self.values, self.countable, self.totals, self.n_countable = grid, int(n_maps), values, countable, totals, n_countable

    def image(self, e, s=0):
        """(ny, nx) bool view of map ``s`` of env ``e``, row 0 at the lowest y - the convention of :meth:`NavGrid.image`, so the
        two can be laid over each other as they are."""
        return _store_view(self.grid, self.values.view(torch.bool), self.n_maps, e, s)

    def fraction(self):
        """(N, S) float32: the share of its env's countable cells each map has seen; 0 where nothing is countable."""
        return self.totals.float()/self.n_countable.clamp(min=1)[:, None].float()

    def mark(self, origins, dirs, distances, slot=None, max_range=10., reset=None, out=None):
        """Marks the cells the rays pass over and returns ``gained`` (N, S) int32: the countable cells each map saw for the first
        time. ``origins`` (N, P, 2): where the P viewers of each env stand; ``dirs`` (N, P, R, 2): their R rays' directions (any
        length; :func:`camera_rays`); ``distances`` (N, P, R): how far each ray got, metres (+inf: it met nothing), as
        :func:`render` and :func:`raycast` return them. A ray is followed up to ``min(distance, max_range)`` and sampled at most
        half a cell apart, both ends included; the cell under every sample is marked. ``slot`` (N, P) integers: the map each
        viewer marks (outside 0..S-1: the viewer is skipped); default viewer k marks map k (then P must be S). ``reset`` (N, S)
        bool: maps cleared (and their totals zeroed) before the marks - an agent that starts over. ``out``: the (N, S) int32
        tensor to write ``gained`` to. :attr:`totals` moves on by what was gained.

        With the grid's free cells as the countable mask no wall is seen through: the cell a hit point falls in, and any cell
        a wall runs through, has its centre within the clearance of that wall, so it is blocked and never counts. One launch, a
        workgroup a map, no host synchronisation. The rule: include/megastep_hip.h (``MsNavSeen``), DESIGN.md 3.16."""
        grid, S = self.grid, self.n_maps
        n, p, r, slot, reset = _viewers(grid, S, origins, dirs, distances, slot, max_range, reset)
        if grid._max_cells > SEEN_MAX_CELLS:
            raise RuntimeError(f'an env of this grid has {grid._max_cells} cells; seen maps take at most {SEEN_MAX_CELLS} an env')
        dev = _require_gpu(origins, dirs, distances, self.values, self.countable, self.totals, grid.free, *_some(slot, reset))
        if out is None:
            out = torch.empty((n, S), dtype=torch.int32, device=dev)
        elif not _fits(out, (n, S), torch.int32) or out.device != dev:
            raise RuntimeError("`out` must be a contiguous (N, S) int32 tensor on the maps' device")
        _launch(dev, 'seen', grid, _lib.MsNavSeen(S, p, r, origins.data_ptr(), dirs.data_ptr(), distances.data_ptr(), _ptr(slot), float(max_range),
                                                  _ptr(reset), self.countable.data_ptr(), self.values.data_ptr(), out.data_ptr(),
                                                  self.totals.data_ptr(), grid._max_cells))
        return out

    def mark_render(self, agents, frame, slot=None, max_range=10., reset=None, out=None, config=None):
        """:meth:`mark` for the agents' own camera rays: ``frame`` is what :func:`render` (or ``modules.render``) returned for
        ``agents``, with its ``distances``; the directions are :func:`camera_rays`' and the origins the agents' positions. The
        viewers are the agents: by default agent k marks map k."""
        return self.mark(*_render_rays(agents, frame, config), slot=slot, max_range=max_range, reset=reset, out=out)


    def frontier_fields(self, mask=None, out=None, passes=False, cost=None):
        """The walking distance from every cell to the nearest countable cell each map has NOT seen, as a :class:`SeededFields`
        of one field per map: ``seeded_fields(grid, self.values, self.n_maps, where=False, among=self.countable)``. The fields
        read the maps by reference: :meth:`SeededFields.update` follows the marks. With a countable mask of cells that can be
        walked to (:class:`~megastep_amd.demo.envs.floorcoverage.FloorCoverage`'s) every seed can be reached; a field without
        a seed - nothing is left to see - is +inf throughout. ``mask``, ``out``, ``passes``: as :func:`seeded_fields`. ``cost``:
        a cost layer as :func:`cost_fields` takes it; the frontier fields are then :class:`CostFields`."""
        if cost is not None:
            return cost_fields(self.grid, self.values, self.n_maps, cost, where=False, among=self.countable, mask=mask, out=out, passes=passes)
        return seeded_fields(self.grid, self.values, self.n_maps, where=False, among=self.countable, mask=mask, out=out, passes=passes)

    def frontier_regions(self, mask=None, out=None, passes=False):
        """The clusters the countable cells each map has NOT seen fall into, as a :class:`Regions` of one field per map:
        ``regions(grid, self.values, self.n_maps, where=False, among=self.countable)`` - :meth:`frontier_fields`' arguments, so a
        frontier field's seeds are exactly the open cells here, and ``areas`` says how much unseen floor hangs together at each
        of them: a sliver behind a pillar or a room. The regions read the maps by reference: :meth:`Regions.update` follows the
        marks. ``mask``, ``out``, ``passes``: as :func:`regions`."""
        return regions(self.grid, self.values, self.n_maps, where=False, among=self.countable, mask=mask, out=out, passes=passes)


def seen_maps(grid, n_maps, countable=None):
    """``n_maps`` seen maps per env on the :func:`nav_grid`, all unseen: which cells of the floor the depth rays of an agent have
    passed over (:meth:`SeenMaps.mark`) - coverage rewards on floor area, a mask to hand a policy or to draw. ``countable``: a
    uint8 or bool tensor of one entry per cell of the grid (``grid.free``'s layout) naming the cells that count towards
    ``gained``, ``totals`` and :meth:`SeenMaps.fraction`; default the grid's free cells. Marks are kept for every cell, counted
    or not."""
    if not isinstance(n_maps, int) or n_maps < 1:
        raise RuntimeError(f'n_maps must be a positive integer; got {n_maps}')
    dev = grid.free.device
    countable, n_countable = _countable(grid, countable, 'seen maps')
    n = grid.n_envs
    values = torch.zeros(max(n_maps*grid.n_cells, 1), dtype=torch.uint8, device=dev)
    return SeenMaps(grid, n_maps, values, countable, torch.zeros((n, n_maps), dtype=torch.int32, device=dev), n_countable)


def _countable(grid, countable, what):
    """The countable mask of a set of maps (``what``) as the kernels read it, and (N,) int32: how many cells of each env count."""
    dev = grid.free.device
    if countable is None:
        countable = grid.free
    else:
        if not isinstance(countable, torch.Tensor) or countable.dtype not in (torch.uint8, torch.bool) or countable.shape != grid.free.shape:
            raise RuntimeError(f'countable must be a uint8 or bool tensor of {tuple(grid.free.shape)}, one entry per cell of the grid')
        countable = countable.to(device=dev, dtype=torch.uint8).contiguous()
    if grid._max_cells > SEEN_MAX_CELLS:
        raise RuntimeError(f'{what} take at most {SEEN_MAX_CELLS} cells an env')
    starts = torch.as_tensor(grid._host_starts, device=dev)
    sums = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), (countable[:grid.n_cells] & 1).long().cumsum(0)])
    return countable, (sums[starts[1:]] - sums[starts[:-1]]).int()


#: the last tick an :class:`AgeMaps`' clock reaches: binary32 holds every tick up to here exactly
AGE_MAX_TICK = 2**24


class Sweep:
    """Result of :meth:`AgeMaps.mark`, each (N, S): ``swept`` int32, the countable cells the call's rays passed over; ``gained``
    int32, those of them never seen since the map was cleared; ``idle`` int64, the sum over them of the ticks since each was last
    seen (its whole clock for one never seen)."""

    def __init__(self, swept, gained, idle):
        self.swept, self.gained, self.idle = swept, gained, idle


class AgeMaps:
    """Result of :func:`age_maps`: for each env ``S`` maps, map (n, s) holding one float32 per cell of env n's grid - the tick of
    the map's clock at which a depth ray of one of its viewers last passed over the cell, 0 where none has since the map was
    cleared. ``last`` is the flat float32 store in :class:`SeenMaps`' layout; ``clock`` (N, S) int32 the tick of each map's last
    :meth:`mark`, on the device; ``countable`` the uint8 mask of the cells that count, ``n_countable`` (N,) int32 how many there
    are; ``threshold`` the age from which a cell is stale. The survey's outputs, rewritten in place by every surveying call:
    ``oldest`` (N, S) int32 and ``total_age`` (N, S) int64 - the largest and the summed age of the countable cells, ``n_stale``
    (N, S) int32 - how many of them are stale, ``stale`` - a byte store in the maps' layout, 1 on the stale countable cells, and
    ``ages`` - a float32 store of every cell's age (None when made with ``ages=False``). As a layer (:func:`cell_layer`,
    :func:`map_channel`, :func:`cell_draws`) the maps present ``ages``, and as a gate or a byte layer (:func:`mark_costs`)
    ``stale``."""

    def __init__(self, grid, n_maps, threshold, last, clock, countable, n_countable, oldest, total_age, n_stale, stale, ages):
        self.grid, self.n_maps, self.threshold = grid, int(n_maps), int(threshold)
        self.last, self.clock, self.countable, self.n_countable = last, clock, countable, n_countable
        self.oldest, self.total_age, self.n_stale, self.stale, self.ages = oldest, total_age, n_stale, stale, ages

    def image(self, e, s=0):
        """(ny, nx) float32 view of the ticks of map ``s`` of env ``e``, row 0 at the lowest y (:meth:`NavGrid.image`'s convention)."""
        return _store_view(self.grid, self.last, self.n_maps, e, s)

    def age_image(self, e, s=0):
        """(ny, nx) float32 view of the ages the last survey found in map ``s`` of env ``e``."""
        if self.ages is None:
            raise RuntimeError('these maps were made with ages=False: there is no store of ages')
        return _store_view(self.grid, self.ages, self.n_maps, e, s)

    def stale_image(self, e, s=0):
        """(ny, nx) bool view of the stale cells the last survey found in map ``s`` of env ``e``."""
        return _store_view(self.grid, self.stale.view(torch.bool), self.n_maps, e, s)

    def mean_age(self):
        """(N, S) float32: the mean age of its env's countable cells at each map's last survey; 0 where nothing is countable."""
        return self.total_age.float()/self.n_countable.clamp(min=1)[:, None].float()

    def _call(self, dev, advance, survey, p, r, origins, dirs, distances, slot, max_range, reset, sweep):
        some = lambda t: _ptr(t) if survey else None
        _launch(dev, 'ages', self.grid, _lib.MsNavAges(
            self.n_maps, p, r, _ptr(origins), _ptr(dirs), _ptr(distances), _ptr(slot), float(max_range), _ptr(reset), self.countable.data_ptr(),
            int(advance), self.threshold, self.last.data_ptr(), self.clock.data_ptr(), _ptr(sweep and sweep.swept), _ptr(sweep and sweep.gained),
            _ptr(sweep and sweep.idle), some(self.oldest), some(self.total_age), some(self.n_stale), some(self.stale), some(self.ages),
            self.grid._max_cells))

    def _tensors(self):
        return [self.last, self.clock, self.countable, self.oldest, self.total_age, self.n_stale, self.stale, self.grid.free, *_some(self.ages)]

    def mark(self, origins, dirs, distances, slot=None, max_range=10., reset=None, survey=True, out=None):
        """Moves every map's clock on by one tick, stamps the cells the rays pass over with it and returns a :class:`Sweep`.
        ``origins``, ``dirs``, ``distances``, ``slot``, ``max_range``: as :meth:`SeenMaps.mark`'s, and the cells marked are the
        ones it would mark. ``reset`` (N, S) bool: maps cleared, and their clocks set to 0, before the tick. ``survey``: the
        survey behind the marks, in the same launch - :attr:`oldest`, :attr:`total_age`, :attr:`n_stale`, :attr:`stale` and
        :attr:`ages` are rewritten, a cell just marked with age 0; without it they keep what the last survey left. ``out``: the
        :class:`Sweep` of an earlier call to write into; then nothing is allocated. One launch, a workgroup a map, no host
        synchronisation; the clock lives on the device, so in a HIP graph every replay is a later tick. A clock stops at
        ``AGE_MAX_TICK``. The rule: include/megastep_hip.h (``MsNavAges``), DESIGN.md 3.25."""
        grid, S = self.grid, self.n_maps
        n, p, r, slot, reset = _viewers(grid, S, origins, dirs, distances, slot, max_range, reset)
        dev = _require_gpu(origins, dirs, distances, *self._tensors(), *_some(slot, reset))
        if out is None:
            out = Sweep(torch.empty((n, S), dtype=torch.int32, device=dev), torch.empty((n, S), dtype=torch.int32, device=dev),
                        torch.empty((n, S), dtype=torch.int64, device=dev))
        elif not isinstance(out, Sweep) or not _fits(out.swept, (n, S), torch.int32) or not _fits(out.gained, (n, S), torch.int32) or \
                not _fits(out.idle, (n, S), torch.int64) or {out.swept.device, out.gained.device, out.idle.device} != {dev}:
            raise RuntimeError("`out` must be a Sweep of contiguous (N, S) int32, int32 and int64 tensors on the maps' device")
        self._call(dev, True, survey, p, r, origins, dirs, distances, slot, max_range, reset, out)
        return out

    def mark_render(self, agents, frame, slot=None, max_range=10., reset=None, survey=True, out=None, config=None):
        """:meth:`mark` for the agents' own camera rays, as :meth:`SeenMaps.mark_render`: ``frame`` is what :func:`render` (or
        ``modules.render``) returned for ``agents``, with its ``distances``. By default agent k marks map k."""
        return self.mark(*_render_rays(agents, frame, config), slot=slot, max_range=max_range, reset=reset, survey=survey, out=out)

    def survey(self):
        """The survey alone: nothing is marked and the clocks stand; :attr:`oldest`, :attr:`total_age`, :attr:`n_stale`,
        :attr:`stale` and :attr:`ages` are rewritten from the maps as they are. One launch; returns the maps."""
        dev = _require_gpu(*self._tensors())
        self._call(dev, False, True, 0, 0, None, None, None, None, 1., None, None)
        return self

    def stale_fields(self, cost=None, mask=None, out=None, passes=False):
        """The walking distance from every cell to the nearest stale cell of each map, as a :class:`SeededFields` of one field per
        map: ``seeded_fields(grid, self.stale, self.n_maps)`` - or, with ``cost`` (a cost layer as :func:`cost_fields` takes it),
        a :class:`CostFields`. The fields read :attr:`stale` by reference: :meth:`SeededFields.update` follows the surveys. A
        field without a seed - nothing is stale - is +inf throughout. ``mask``, ``out``, ``passes``: as :func:`seeded_fields`."""
        if cost is not None:
            return cost_fields(self.grid, self.stale, self.n_maps, cost, mask=mask, out=out, passes=passes)
        return seeded_fields(self.grid, self.stale, self.n_maps, mask=mask, out=out, passes=passes)

    def stale_regions(self, mask=None, out=None, passes=False):
        """The clusters the stale cells of each map fall into, as a :class:`Regions` of one field per map:
        ``regions(grid, self.stale, self.n_maps)``, read by reference. ``mask``, ``out``, ``passes``: as :func:`regions`."""
        return regions(self.grid, self.stale, self.n_maps, mask=mask, out=out, passes=passes)


def age_maps(grid, n_maps, countable=None, threshold=64, ages=True):
    """``n_maps`` age maps per env on the :func:`nav_grid`, all never seen and their clocks at 0: WHEN each cell of the floor was
    last passed over by a depth ray of an agent (:meth:`AgeMaps.mark`) - idleness, for patrol, surveillance and search tasks, which
    do not end when the floor runs out as those on :func:`seen_maps` do. ``countable``: as :func:`seen_maps`'; ``threshold``: the
    age, in ticks, from which a countable cell is stale (an integer, at least 1); ``ages=False``: no store of every cell's age
    (the survey then writes four bytes a cell less)."""
    if not isinstance(n_maps, int) or n_maps < 1:
        raise RuntimeError(f'n_maps must be a positive integer; got {n_maps}')
    if not isinstance(threshold, int) or isinstance(threshold, bool) or threshold < 1:
        raise RuntimeError(f'threshold must be an integer of at least 1; got {threshold}')
    countable, n_countable = _countable(grid, countable, 'age maps')
    new = _new(grid.free.device)
    n, size = grid.n_envs, max(n_maps*grid.n_cells, 1)
    return AgeMaps(grid, n_maps, threshold, new((size,), torch.float32, 0.), new((n, n_maps), torch.int32, 0), countable, n_countable,
                   new((n, n_maps), torch.int32, 0), new((n, n_maps), torch.int64, 0), new((n, n_maps), torch.int32, 0),
                   new((size,), torch.uint8, 0), new((size,), torch.float32, 0.) if ages else None)


#: the most channels, samples a side and pixels a side of :func:`local_maps`
WINDOW_MAX_CHANNELS, WINDOW_MAX_SAMPLES, WINDOW_MAX_SIDE = 8, 4, 1024


class CellLayer:
    """Result of :func:`cell_layer`: a per-cell store :func:`local_maps` reads. ``values``: the flat uint8 or float32 store of
    ``n_fields`` stores per env; ``field``: the (N, P) int32 tensor naming the store each view reads, or None."""

    def __init__(self, values, n_fields, field):
        self.values, self.n_fields, self.field = values, int(n_fields), field

    is_float = property(lambda self: self.values.dtype == torch.float32)

    def _tensors(self):
        return (self.values,) if self.field is None else (self.values, self.field)


def cell_layer(values, n_fields=1, field=None):
    """A per-cell store as a layer for :func:`map_channel`: ``values`` is a contiguous 1-dimensional uint8, bool or float32 tensor
    of (at least) ``n_fields*grid.n_cells`` entries in the layout the fields and maps use - ``n_fields`` stores per env, store (n, f) at
    ``n_fields*grid.starts[n] + f*nx*ny``, row-major with row 0 at the lowest y - kept by reference, so a live seen map or field
    can be the source. ``field``: an (N, P) integer tensor naming the store each view reads; without it store 0 is read when
    ``n_fields`` is 1 and view p reads store p when ``n_fields`` is the number of views. A :class:`NavGrid` (its ``free``), a
    :class:`SeenMaps`, a :class:`DistanceFields` and a :class:`SeededFields` are layers as they are, with their own number of
    stores, an :class:`AgeMaps` too (its ``ages``, in ticks; as a gate its ``stale``), and so are a :class:`Regions` (its ``areas``, square metres), a :class:`ViewFields` (its ``values``, a store a
    viewpoint) and a :class:`ClearanceFields` (its ``values``, metres to the nearest wall: one float store);
    ``cell_layer(maps, field=slot)`` gives one of them a ``field``. An int32 tensor makes a layer of labels, which only
    :func:`zones` takes."""
    if isinstance(values, CellLayer):
        values, n_fields = values.values, values.n_fields
    elif isinstance(values, NavGrid):
        values, n_fields = values.free, 1
    elif isinstance(values, SeenMaps):
        values, n_fields = values.values, values.n_maps
    elif isinstance(values, AgeMaps):
        if values.ages is None:
            raise RuntimeError('these age maps were made with ages=False: as a float layer they have nothing to present')
        values, n_fields = values.ages, values.n_maps
    elif isinstance(values, _Fields):
        values, n_fields = values.values, values.n_goals
    elif isinstance(values, Regions):
        values, n_fields = values.areas, values.n_fields
    elif isinstance(values, ViewFields):
        values, n_fields = values.values, values.n_points
    elif isinstance(values, ClearanceFields):
        values, n_fields = values.values, 1
    if not isinstance(n_fields, int) or n_fields < 1:
        raise RuntimeError(f'n_fields must be a positive integer; got {n_fields}')
    if not isinstance(values, torch.Tensor) or values.dtype not in (torch.uint8, torch.bool, torch.float32, torch.int32) or values.ndim != 1 or \
            not values.is_contiguous():
        raise RuntimeError('a layer must be a contiguous 1-dimensional uint8, bool or float32 tensor (or int32: labels, for zones)')
    if values.dtype == torch.bool:
        values = values.view(torch.uint8)
    return CellLayer(values, n_fields, None if field is None else _index(field, 'field'))


def _layer(x, byte=False):
    """``x`` as a :class:`CellLayer`. ``byte``: the place asks for a byte layer - a gate, marks to price - and an :class:`AgeMaps`,
    which as a float layer presents its ages, presents its stale cells there."""
    if byte and isinstance(x, AgeMaps):
        return cell_layer(x.stale, x.n_maps)
    layer = x if isinstance(x, CellLayer) else cell_layer(x)
    if layer.values.dtype == torch.int32:
        raise RuntimeError('an int32 layer holds labels: only zones takes it')
    return layer


class MapChannel:
    """Result of :func:`map_channel`: one channel of :func:`local_maps`."""

    def __init__(self, source, where, scale, gate, outside, hidden):
        self.source, self.where, self.scale, self.gate, self.outside, self.hidden = source, where, scale, gate, outside, hidden


def map_channel(source, where=True, scale=None, gate=None, outside=0., hidden=0.):
    """One channel of :func:`local_maps`. ``source``: a layer (:func:`cell_layer`, or a :class:`NavGrid`, :class:`SeenMaps`,
    :class:`DistanceFields`, :class:`SeededFields`, :class:`Regions`, :class:`ViewFields` or :class:`ClearanceFields` as it is). A byte source gives 1 where ``(byte != 0) == where`` and 0
    elsewhere; a float source holding D gives ``D*scale`` clamped to [0, 1] (a NaN and +inf: 1), and ``scale`` is required.
    ``gate``: a byte layer with a ``field`` of its own; where its byte is 0 the channel shows ``hidden`` - ``grid.free`` gated by
    an agent's seen map is the floor that agent knows. ``outside``: what a sample beyond the env's grid shows."""
    source = _layer(source)
    gate = None if gate is None else _layer(gate, byte=True)
    if gate is not None and gate.is_float:
        raise RuntimeError('a gate must be a byte layer (uint8 or bool), not float32')
    if source.is_float:
        if scale is None:
            raise RuntimeError('a float32 source needs a scale: the channel shows D*scale clamped to [0, 1]')
        scale = float(scale)
    return MapChannel(source, bool(where), 0. if scale is None else float(scale), gate, float(outside), float(hidden))


def _window_layer(layer, name, grid, n, p, spec):
    """Checks ``layer`` against the grid and the views and fills in the MsNavLayer ``spec``; returns its tensors."""
    want = layer.n_fields*grid.n_cells
    if layer.values.shape[0] < want:
        raise RuntimeError(f"{name} must have at least {want} entries, a value per cell and store (n_fields*n_cells = {layer.n_fields}*{grid.n_cells}); "
                           f'got {layer.values.shape[0]}')
    if layer.field is None:
        _default_store(layer.n_fields, p, f'without field, {name} must hold one store per env or one per view ({p}); it holds {layer.n_fields}')
    elif layer.field.shape != (n, p):
        raise RuntimeError(f"{name}'s field must be (N, P) = ({n}, {p}); got {tuple(layer.field.shape)}")
    spec.values, spec.is_float, spec.n_fields = layer.values.data_ptr(), int(layer.is_float), layer.n_fields
    spec.field = _ptr(layer.field)
    return layer._tensors()


def local_maps(grid, views, size, channels, samples=1, out=None):
    """Per-cell stores of the :func:`nav_grid` cropped, turned and resampled into images: (N, P, C, H, W) float32, planar
    (``spaces.MultiImage``'s layout), image (n, p) showing env n through ``views[n, p]`` - the six-number affine maps of
    :func:`overhead`, so :func:`agent_views` gives every agent the egocentric window round it, its heading up, and
    :func:`plan_views` the whole plan. ``size``: an int or (H, W), at most 1024 a side. ``channels``: 1 to 8
    :func:`map_channel`; a bare layer stands for ``map_channel(layer)``. ``samples`` (1..4): a pixel is the mean of
    ``samples**2`` sub-samples, each the value of the cell under it - for pixels larger than a cell. ``out``: the tensor of an
    earlier call with the same shapes to write into.

    One launch for every image and channel, a lane a pixel, the cell under a sample found once for all channels; no host
    synchronisation, nothing allocated besides ``out``: the call can be captured in a HIP graph. The rule is written out in
    include/megastep_hip.h (``MsNavWindows``) and DESIGN.md 3.18; the kernel computes it bit for bit."""
    _check(views, 'views', torch.float32, 3)
    h, w = _hw(size)
    n, p = views.shape[:2]
    if n != grid.n_envs or p < 1 or views.shape[2] != 6:
        raise RuntimeError(f'views must be (N, P, 6) with N = {grid.n_envs} and P >= 1; got {tuple(views.shape)}')
    if h > WINDOW_MAX_SIDE or w > WINDOW_MAX_SIDE:
        raise RuntimeError(f'size must be at most {WINDOW_MAX_SIDE} a side; got {size}')
    if not isinstance(samples, int) or not 1 <= samples <= WINDOW_MAX_SAMPLES:
        raise RuntimeError(f'samples must be an integer in 1..{WINDOW_MAX_SAMPLES}; got {samples}')
    channels = [ch if isinstance(ch, MapChannel) else map_channel(ch) for ch in channels]
    c = len(channels)
    if not 1 <= c <= WINDOW_MAX_CHANNELS:
        raise RuntimeError(f'channels must be 1 to {WINDOW_MAX_CHANNELS} map_channel; got {c}')
    specs = (_lib.MsNavChannel*c)()
    tensors = [views, grid.free]
    for k, (ch, spec) in enumerate(zip(channels, specs)):
        if ch.gate is not None and ch.gate.is_float:                    # (a MapChannel made by hand has not been through map_channel)
            raise RuntimeError('a gate must be a byte layer (uint8 or bool), not float32')
        if ch.source.is_float and ch.scale is None:
            raise RuntimeError('a float32 source needs a scale')
        tensors += _window_layer(ch.source, f"channel {k}'s source", grid, n, p, spec.source)
        if ch.gate is not None:
            tensors += _window_layer(ch.gate, f"channel {k}'s gate", grid, n, p, spec.gate)
        spec.where, spec.scale, spec.outside, spec.hidden = int(bool(ch.where)), float(ch.scale or 0.), float(ch.outside), float(ch.hidden)
    shape = (n, p, c, h, w)
    if out is not None:
        if not _fits(out, shape, torch.float32):
            raise RuntimeError(f'`out` must be a contiguous (N, P, C, H, W) = {shape} float32 tensor')
        tensors.append(out)
    dev = _require_gpu(*tensors)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    _launch(dev, 'windows', grid, _lib.MsNavWindows(p, h, w, samples, views.data_ptr(), c, specs, out.data_ptr()))
    return out


#: the most draws a set of :func:`cell_draws` makes: the kernel gives a lane of its workgroup to each
DRAW_MAX_DRAWS = 256


class CellDraws:
    """Result of :func:`cell_draws`: ``n_sets`` draw sets per env of ``n_draws`` draws each. ``cells`` (N, P, K) int32: the index of
    each drawn cell within its env's grid, row-major with row 0 at the lowest y, -1 where no cell of the env qualified; ``points``
    (N, P, K, 2) float32: the cells' centres (NaN where none qualified); ``uniforms`` (N, P, K) float32: a spare uniform number in
    [0, 1) per draw; ``values`` (N, P, K) float32, None for a byte source: what the source holds at the cell; ``counts`` (N, P)
    int32: how many cells qualified; ``counter`` (N, P) int32: how many times each set has been drawn - the kernel reads it and
    moves it on, so the next draw of a set is another one. ``source`` and ``gate`` are kept by reference: :meth:`again` reads
    them as they stand."""

    def __init__(self, grid, n_sets, n_draws, cells, points, uniforms, values, counts, counter):
        self.grid, self.n_sets, self.n_draws = grid, int(n_sets), int(n_draws)
        self.cells, self.points, self.uniforms, self.values, self.counts, self.counter = cells, points, uniforms, values, counts, counter

    def _set(self, source, gate, where, lo, hi, seed):
        """Takes the arguments of a call: checks the layers against the grid and the sets and fills in the MsNavDraws."""
        grid, n, p = self.grid, self.grid.n_envs, self.n_sets
        spec = _lib.MsNavDraws()
        tensors = [grid.free, self.cells, self.points, self.uniforms, self.counts, self.counter]
        tensors += _window_layer(source, 'source', grid, n, p, spec.source)
        if gate is not None:
            tensors += _window_layer(gate, 'gate', grid, n, p, spec.gate)
        spec.where, spec.lo, spec.hi = int(bool(where)), float(lo or 0.), float(hi or 0.)
        spec.n_sets, spec.n_draws, spec.seed, spec.max_cells = p, self.n_draws, seed, grid._max_cells
        spec.counter, spec.cells, spec.points = self.counter.data_ptr(), self.cells.data_ptr(), self.points.data_ptr()
        spec.uniforms, spec.counts = self.uniforms.data_ptr(), self.counts.data_ptr()
        if self.values is not None:
            spec.values = self.values.data_ptr()
            tensors.append(self.values)
        self.source, self.gate, self.where, self.lo, self.hi, self.seed = source, gate, bool(where), lo, hi, seed
        self._spec, self._tensors = spec, tensors

    def again(self, mask=None):
        """Draws again in place, from the layers as they stand now; the counter moves on, so the draws are new ones. ``mask``
        (N, P) bool: only the marked sets are drawn - the others keep their draws, their counts and their counter. One launch, no
        host synchronisation, nothing allocated: the call can be captured in a HIP graph, and every replay draws afresh."""
        mask = _mask(mask, self.grid.n_envs, self.n_sets, 'P')
        dev = _require_gpu(*self._tensors, *_some(mask))
        self._spec.mask = _ptr(mask)
        _launch(dev, 'draws', self.grid, self._spec)
        return self


def cell_draws(grid, source, n_sets, n_draws, lo=None, hi=None, where=True, gate=None, seed=0, mask=None, out=None):
    """Cells of the :func:`nav_grid` drawn uniformly at random: for every env ``n_sets`` draw sets of ``n_draws`` (1..256) draws each,
    with replacement, among the env's free cells that satisfy a predicate on ``source`` - a layer (:func:`cell_layer`, or a
    :class:`NavGrid`, :class:`SeenMaps`, :class:`DistanceFields`, :class:`SeededFields`, :class:`Regions`, :class:`ViewFields` or :class:`ClearanceFields` as it is), read per set the way
    :func:`local_maps` reads a layer per view: one store an env, one per set, or the one the layer's ``field`` (N, P) names. A byte
    source qualifies a cell where ``(byte != 0) == where``; a float32 source holding D where ``lo <= D <= hi`` (both required
    then, both ends in; a NaN never qualifies) - a band of a distance field is a goal at a chosen walking distance, reachable by
    construction; ``grid`` itself any spot an agent fits; a seen map with ``where=False`` a cell not yet seen. ``gate``: a byte
    layer; only cells where its byte is non-zero qualify.

    The numbers come from a hash of ``seed``, the set, the draw and the set's own counter, which the kernel moves on by one in
    every call that computes the set: nothing is drawn on the host, and a captured :meth:`CellDraws.again` draws afresh at every
    replay. ``mask`` (N, P) bool: only the marked sets are computed; ``out``: the :class:`CellDraws` of an earlier call with the same
    grid, ``n_sets``, ``n_draws`` and kind of source to write into - its counter goes on counting. One launch, a workgroup a set, no
    host synchronisation. The rule is written out in include/megastep_hip.h (``MsNavDraws``) and DESIGN.md 3.19; the kernel
    computes it exactly."""
    if not isinstance(n_sets, int) or n_sets < 1:
        raise RuntimeError(f'n_sets must be a positive integer; got {n_sets}')
    if not isinstance(n_draws, int) or not 1 <= n_draws <= DRAW_MAX_DRAWS:
        raise RuntimeError(f'n_draws must be an integer in 1..{DRAW_MAX_DRAWS}; got {n_draws}')
    if not isinstance(seed, int) or not 0 <= seed < 2**64:
        raise RuntimeError(f'seed must be an integer in 0..2^64 - 1; got {seed}')
    source = _layer(source)
    gate = None if gate is None else _layer(gate, byte=True)
    if gate is not None and gate.is_float:
        raise RuntimeError('a gate must be a byte layer (uint8 or bool), not float32')
    if source.is_float:
        if lo is None or hi is None or lo != lo or hi != hi:
            raise RuntimeError('a float32 source needs the bounds lo and hi of its band (numbers, not NaN)')
        lo, hi = float(lo), float(hi)
    elif lo is not None or hi is not None:
        raise RuntimeError('a byte source takes no bounds: lo and hi go with a float32 source')
    n, shape = grid.n_envs, (grid.n_envs, n_sets, n_draws)
    if out is not None:
        if not isinstance(out, CellDraws) or out.grid is not grid or tuple(out.cells.shape) != shape or (out.values is not None) != source.is_float:
            raise RuntimeError(f'`out` must come from a cell_draws call with the same grid, (N, P, K) = {shape} and kind of source')
        draws = out
    else:
        if grid._max_cells > SEEN_MAX_CELLS:
            raise RuntimeError(f'cell draws take at most {SEEN_MAX_CELLS} cells an env')
        new = _new(grid.free.device)
        draws = CellDraws(grid, n_sets, n_draws, new(shape, torch.int32, -1), new(shape + (2,), torch.float32, float('nan')),
                          new(shape, torch.float32, 0.), new(shape, torch.float32, float('nan')) if source.is_float else None,
                          new((n, n_sets), torch.int32, 0), new((n, n_sets), torch.int32, 0))
    draws._set(source, gate, where, lo, hi, seed)
    return draws.again(mask)


#: the framed cells - ``(nx + 2)*(ny + 2)`` - an env may have for :func:`regions` to label it in LDS, for each of the kernel's three
#: instantiations (40, 80 and 160 KiB); the launch is the least that holds the grid's largest env, and a larger env is labelled
#: in global memory, to the same result
REGION_CAPACITY = (10224, 20464, 40944)


def _masks(grid, store, n_fields, points, labels, field, out):
    """:meth:`Regions.masks` and :meth:`Basins.masks`: the requests' rules and the one launch, on the labels ``store``."""
    if points is not None:
        n, p = _points(grid, points)
    else:
        labels = _index(labels, 'labels', grid.n_envs)
        n, p = labels.shape
    field = _field_rule(field, n, p, n_fields, 'field')
    dev = _require_gpu(points if points is not None else labels, store, grid.free, *_some(field))
    size = max(p*grid.n_cells, 1)
    if out is None:
        out = CellLayer(torch.zeros(size, dtype=torch.uint8, device=dev), p, None)
    elif not isinstance(out, CellLayer) or out.is_float or out.n_fields != p or out.values.shape[0] != size or out.values.device != dev:
        raise RuntimeError(f'`out` must be the layer of a masks call with the same grid and P = {p}')
    _launch(dev, 'region_masks', grid, _lib.MsNavRegionMasks(p, _ptr(points), _ptr(labels), _ptr(field), store.data_ptr(), n_fields,
                                                              out.values.data_ptr()))
    return out


class Regions:
    """Result of :func:`regions`: for each env ``G`` regions fields, field (n, g) labelling the connected components of its open
    cells. ``labels``: the flat int32 store, field (n, g) at ``G*grid.starts[n] + g*nx*ny`` (the layout of
    :class:`DistanceFields`) - the least row-major index, within the env, of an open cell of the cell's component, -1 on a closed
    cell; ``areas``: the flat float32 store in the same layout - the component's area in square metres, 0 on a closed cell (a
    layer: :func:`cell_layer` of a :class:`Regions` is this store); ``counts``, ``open_cells``, ``largest``, ``largest_cells``
    (N, G) int32: the regions, the open cells, the label of the region with the most cells (the least on a tie, -1 without an
    open cell) and its cells; ``passes`` (N, G) int32 or None. ``marks`` and ``among`` are kept by reference: :meth:`update`
    sees them as they stand. The rule: include/megastep_hip.h (``MsNavRegions``), DESIGN.md 3.20."""

    def __init__(self, grid, marks, n_fields, where, among, labels, areas, counts, open_cells, largest, largest_cells, passes=None):
        self.grid, self.marks, self.where, self.among = grid, marks, bool(where), among
        self.labels, self.areas, self.counts, self.open_cells = labels, areas, counts, open_cells
        self.largest, self.largest_cells, self.passes = largest, largest_cells, passes
        self._n_fields = int(n_fields)

    n_fields = property(lambda self: self._n_fields)

    def image(self, e, g=0):
        """(ny, nx) int32 view of the labels of field ``g`` of env ``e``, row 0 at the lowest y."""
        return _store_view(self.grid, self.labels, self.n_fields, e, g)

    def area_image(self, e, g=0):
        """(ny, nx) float32 view of the areas of field ``g`` of env ``e``, row 0 at the lowest y."""
        return _store_view(self.grid, self.areas, self.n_fields, e, g)

    def update(self, mask=None):
        """Labels the fields marked in the (N, G) bool ``mask`` (default all) again in place, from :attr:`marks` and
        :attr:`among` as they stand now; the others keep labels, areas and summary. One launch, no host synchronisation, nothing
        allocated: the call can be captured in a HIP graph."""
        grid, g = self.grid, self.n_fields
        mask = _mask(mask, grid.n_envs, g, 'G')
        dev = _require_gpu(self.labels, self.areas, self.counts, self.open_cells, self.largest, self.largest_cells, grid.free,
                           *_some(self.marks, self.among, mask, self.passes))
        _launch(dev, 'regions', grid, _lib.MsNavRegions(g, _ptr(self.marks), int(self.where), _ptr(self.among), _ptr(mask), self.labels.data_ptr(),
                                                        self.areas.data_ptr(), self.counts.data_ptr(), self.open_cells.data_ptr(),
                                                        self.largest.data_ptr(), self.largest_cells.data_ptr(), _ptr(self.passes)))
        return self

    def labels_at(self, points, field=None):
        """(N, P, 4) int32: the label under each of the four cells round each of ``points`` (N, P, 2) - the anchors of
        :meth:`DistanceFields.at`, in its order - and -1 where that cell is outside the grid or closed. ``field`` (N, P) integers
        name the regions field each point asks; default the one field, or point k field k (then P must be G). All -1 for a NaN
        point, a point far from the grid, an env without cells and a field index out of range. One launch, no host
        synchronisation."""
        n, p = _points(self.grid, points)
        field = _field_rule(field, n, p, self.n_fields, 'field')
        dev = _require_gpu(points, self.labels, self.grid.free, *_some(field))
        out = torch.empty((n, p, 4), dtype=torch.int32, device=dev)
        _launch(dev, 'region_query', self.grid, _lib.MsNavRegionQuery(p, points.data_ptr(), _ptr(field), self.labels.data_ptr(), self.n_fields,
                                                                      out.data_ptr()))
        return out

    def at(self, points, field=None):
        """(N, P) int32: the region each of ``points`` stands in - the least non-negative label of :meth:`labels_at`, -1 without
        one."""
        found = self.labels_at(points, field)
        top = torch.iinfo(torch.int32).max
        least = torch.where(found < 0, torch.full_like(found, top), found).amin(-1)
        return torch.where(least == top, torch.full_like(least, -1), least)

    def together(self, a, b, field=None):
        """(N, P) bool: can one walk from ``a[n, k]`` to ``b[n, k]`` (both (N, P, 2)) - does some anchor of the one share a label
        with some anchor of the other. On the regions of the grid itself this is exactly where :func:`geodesic` is finite, for
        two launches of a lane a point instead of a distance field a pair."""
        la, lb = self.labels_at(a, field), self.labels_at(b, field)
        return ((la[..., :, None] == lb[..., None, :]) & (la[..., :, None] >= 0)).any(-1).any(-1)

    def masks(self, points=None, labels=None, field=None, out=None):
        """Byte masks of chosen regions, as a :class:`CellLayer` of ``P`` stores per env (store (n, p) at
        ``P*grid.starts[n] + p*nx*ny``): a byte is 1 on the cells of the regions request (n, p) wants. Exactly one of ``points``
        (N, P, 2) float32 - the regions under the point's four anchors: where one can walk to from there - and ``labels`` (N, P)
        integers - that one region; -1 wants none - is given. ``field``: as :meth:`labels_at`. ``out``: the layer of an earlier call
        with the same P to write into; every byte is written, so it needs no clearing. With P = 1 the layer has ``grid.free``'s
        layout: :func:`seeded_fields`' ``among`` and :func:`seen_maps`' ``countable`` take its ``values``, and
        :func:`cell_draws` and :func:`map_channel` take it as a ``gate`` or a source, as it is. One launch, no host
        synchronisation."""
        if (points is None) == (labels is None):
            raise RuntimeError('exactly one of points and labels must be given')
        return _masks(self.grid, self.labels, self.n_fields, points, labels, field, out)

    def zones(self, values=None, marks=None, n_zones=16, where=True, within_marks=False, mask=None, out=None):
        """:func:`zones` of these regions: per region the cells, the marked cells, the least value and the cell attaining it."""
        return zones(self, values=values, marks=marks, n_zones=n_zones, where=where, within_marks=within_marks, mask=mask, out=out)

    def largest_mask(self, out=None):
        """The byte mask of every env's largest region, ``grid.free``'s layout: ``masks(labels=self.largest[:, :1])``. One regions
        field per env only."""
        if self.n_fields != 1:
            raise RuntimeError(f'largest_mask is for one regions field per env; there are {self.n_fields}: use masks(labels=..., field=...)')
        return self.masks(labels=self.largest[:, :1], out=out)


def regions(grid, marks=None, n_fields=1, where=True, among=None, mask=None, out=None, passes=False):
    """The connected regions of the :func:`nav_grid`: which cells belong together. Without ``marks`` the open cells are the grid's
    free cells, and two cells share a label exactly when one can walk from one to the other - where a :func:`distance_fields`
    field of the one is finite on the other (the diagonal steps of the fields' graph join nothing its straight steps do not:
    DESIGN.md 3.20). With ``marks``, ``n_fields``, ``where`` and ``among`` - :func:`seeded_fields`' arguments, by its rules - the open
    cells of field (n, g) are the cells that would be its seeds: the unseen floor of a seen map falls into clusters
    (:meth:`SeenMaps.frontier_regions`). Open cells are joined to their open 4-neighbours; a cell's label is the least row-major
    index within its env of an open cell of its component, its area the component's cells times ``cell**2``; see
    :class:`Regions`.

    One launch, one workgroup per field: min-label propagation with pointer jumping in LDS, until nothing changes; the labels are
    canonical, so the result does not depend on the schedule (include/megastep_hip.h, ``MsNavRegions``).

    ``mask`` (N, G) bool: label only the marked fields (the others keep what ``out`` held; no open cell without ``out``);
    ``out``: the :class:`Regions` of an earlier call with the same grid, marks and arguments to write into; ``passes=True`` also
    records the passes each field took. No host synchronisation: the call can be captured in a HIP graph."""
    if not isinstance(n_fields, int) or n_fields < 1:
        raise RuntimeError(f'n_fields must be a positive integer; got {n_fields}')
    if marks is not None:
        marks = _cell_bytes(marks, 'marks', max(n_fields*grid.n_cells, 1), f'a byte per cell and field (n_fields*n_cells = {n_fields}*{grid.n_cells})')
    if among is not None:
        if marks is None:
            raise RuntimeError('among goes with marks: without marks the open cells are the free cells')
        among = _cell_bytes(among, 'among', grid.free.shape[0], 'one per cell of the grid')
    where = bool(where)
    if out is not None:
        if not isinstance(out, Regions) or out.grid is not grid or out.n_fields != n_fields or out.where != where or \
                not _same(out.marks, marks) or not _same(out.among, among):
            raise RuntimeError('`out` must come from a regions call with the same grid, marks, n_fields, where and among')
        return out.update(mask)
    new = _new(_require_gpu(grid.free, *_some(marks, among)))
    size, shape = max(n_fields*grid.n_cells, 1), (grid.n_envs, n_fields)
    result = Regions(grid, marks, n_fields, where, among, new((size,), torch.int32, -1), new((size,), torch.float32, 0.),
                     new(shape, torch.int32, 0), new(shape, torch.int32, 0), new(shape, torch.int32, -1), new(shape, torch.int32, 0),
                     new(shape, torch.int32, 0) if passes else None)
    return result.update(mask)


#: the static walls :func:`view_fields`' kernel stages in LDS for one viewpoint - those whose bounding box meets the box of everything
#: in range; a viewpoint that keeps more reads its env's walls from global memory instead, to the same result
VIEW_WALL_CAPACITY = 512


class ViewFields:
    """Result of :func:`view_fields`: for each env ``P`` viewpoints, and for viewpoint (n, p) the cells of env n's grid whose centre
    is in sight of it. ``values``: the flat uint8 store, a byte a cell - 1 in sight, 0 not - store (n, p) at
    ``P*grid.starts[n] + p*nx*ny`` (the layout of :class:`SeenMaps`: a layer, :func:`seeded_fields`' and :func:`regions`' ``marks``),
    None with ``store=False``; ``counts`` (N, P) int32: the visible cells that count; ``gains`` (N, P) int32, None without
    ``unseen``: those of them the viewpoint's seen map has not seen. ``points``, ``headings``, ``countable``, ``slot`` and the maps are
    kept by reference: :meth:`update` reads them as they stand. The rule: include/megastep_hip.h (``MsNavViews``), DESIGN.md 3.21."""

    def __init__(self, grid, scenery, points, max_range, headings, cos_half, countable, unseen, slot, values, counts, gains):
        self.grid, self.scenery, self.points, self.max_range, self.headings, self.cos_half = grid, scenery, points, float(max_range), headings, cos_half
        self.countable, self.unseen, self.slot, self.values, self.counts, self.gains = countable, unseen, slot, values, counts, gains

    n_points = property(lambda self: self.points.shape[1])

    def image(self, e, p=0):
        """(ny, nx) bool view of the store of viewpoint ``p`` of env ``e``, row 0 at the lowest y."""
        if self.values is None:
            raise RuntimeError('these view fields keep no byte store (store=False)')
        return _store_view(self.grid, self.values.view(torch.bool), self.n_points, e, p)

    def update(self, mask=None):
        """Computes the viewpoints marked in the (N, P) bool ``mask`` (default all) again in place, from :attr:`points` and
        :attr:`headings` as they stand now - move them in place - and from the maps as they stand; the others keep their bytes,
        count and gain. One launch, no host synchronisation, nothing allocated: the call can be captured in a HIP graph."""
        grid, p = self.grid, self.n_points
        mask = _mask(mask, grid.n_envs, p, 'P')
        maps = self.unseen.values if self.unseen is not None else None
        dev = _require_gpu(self.points, self.countable, self.counts, grid.free, *_some(self.headings, maps, self.slot, mask, self.values, self.gains))
        if self.scenery._device() != dev:
            raise RuntimeError(f'all tensors must live on one device; got {self.scenery._device()} and {dev}')
        spec = _lib.MsNavViews(p, self.points.data_ptr(), _ptr(self.headings), self.max_range, self.cos_half if self.headings is not None else 0.,
                               self.countable.data_ptr(), _ptr(maps), self.unseen.n_maps if self.unseen is not None else 0, _ptr(self.slot),
                               _ptr(mask), _ptr(self.values), self.counts.data_ptr(), _ptr(self.gains))
        _launch(dev, 'views', grid, spec, self.scenery._as_struct())
        return self


def view_fields(grid, scenery, points, max_range=10., headings=None, fov=None, countable=None, unseen=None, slot=None, store=True, mask=None,
                out=None):
    """What can be seen from a place: for every env and each of its ``P`` viewpoints (``points``: (N, P, 2) float32 world points) the
    cells of the :func:`nav_grid` whose CENTRE is in sight - no further than ``max_range`` metres, within ``fov`` degrees round
    ``headings`` (N, P, 2; any length) when both are given, and with no static wall of ``scenery`` across the straight line between
    the two. The agents' own lines are not looked at: the grid is the building. A byte a cell for every cell, free or not - a blocked
    cell on the viewer's side of a wall is a known obstacle - so an opponent's view is a layer: ``cell_draws(grid, views, ...,
    where=False)`` draws a hiding spot, ``seeded_fields(grid, views.values, P, where=False)`` is the walking distance to cover,
    :func:`regions` labels the pockets, :func:`local_maps` shows it to a policy.

    ``counts`` is the number of visible cells that count: ``countable``, a uint8 or bool tensor of one entry per cell of the grid,
    default ``unseen.countable`` with ``unseen``, else the grid's free cells. ``unseen``: a :class:`SeenMaps`; then ``gains`` is the
    number of visible countable cells the viewpoint's map has NOT seen - what standing there would reveal; ``slot`` (N, P) integers
    names the map of each viewpoint (outside 0..S-1: gain 0), default viewpoint k map k (then P must be S) or the env's one map.
    ``store=False`` keeps no bytes at all, only the counts: scoring candidate standpoints costs 4 bytes a viewpoint.

    One launch, one workgroup per viewpoint: the walls near enough to matter staged in LDS, a lane a cell of the window round the
    viewpoint; exact - the rule is written out in include/megastep_hip.h (``MsNavViews``) and DESIGN.md 3.21, every operation binary32
    in a fixed order, and the kernel computes it bit for bit. Unlike a ring of :func:`raycast` rays through :meth:`SeenMaps.mark`
    it misses no cell at range and marks no cell whose centre is hidden.

    ``mask`` (N, P) bool: compute only the marked viewpoints (the others keep what ``out`` held; nothing in sight without ``out``);
    ``out``: the :class:`ViewFields` of an earlier call with the same grid, P and kind of outputs to write into - it takes this call's
    arguments. ``points`` and ``headings`` are kept by reference, not copied: :meth:`ViewFields.update` follows them. No host
    synchronisation: the call can be captured in a HIP graph."""
    import math
    n, p = _points(grid, points)
    if not isinstance(max_range, (int, float)) or not (0 < max_range < float('inf')):
        raise RuntimeError(f'max_range must be a positive number; got {max_range}')
    if (headings is None) != (fov is None):
        raise RuntimeError('headings and fov go together: a cone needs both')
    cos_half = 0.
    if headings is not None:
        _check(headings, 'headings', torch.float32, 3)
        if headings.shape != points.shape:
            raise RuntimeError(f'headings must be (N, P, 2) = {tuple(points.shape)}; got {tuple(headings.shape)}')
        if not isinstance(fov, (int, float)) or not (0 <= fov <= 360):
            raise RuntimeError(f'fov must be a number of degrees in 0..360; got {fov}')
        cos_half = max(-1., min(1., math.cos(math.radians(float(fov))/2.)))
    if unseen is not None and not isinstance(unseen, SeenMaps):
        raise RuntimeError('unseen must be a SeenMaps')
    if unseen is not None and unseen.grid is not grid:
        raise RuntimeError("unseen must be seen maps of the same grid")
    if countable is None:
        countable = unseen.countable if unseen is not None else grid.free
    else:
        countable = _cell_bytes(countable, 'countable', grid.free.shape[0], 'one per cell of the grid')
    if slot is not None:
        if unseen is None:
            raise RuntimeError('slot goes with unseen: it names the seen map of each viewpoint')
        slot = _index(slot, 'slot', n, p)
    elif unseen is not None:
        _default_store(unseen.n_maps, p, f'without slot, unseen must hold one map per env or one per viewpoint ({p}); it holds {unseen.n_maps}')
    if not hasattr(scenery, 'lines') or len(scenery.lines) != n:
        raise RuntimeError(f'scenery must be the Scenery the grid was laid over: {n} envs')
    store = bool(store)
    size = max(p*grid.n_cells, 1)
    if out is not None:
        if not isinstance(out, ViewFields) or out.grid is not grid or out.n_points != p or (out.values is not None) != store or \
                (out.gains is not None) != (unseen is not None):
            raise RuntimeError('`out` must come from a view_fields call with the same grid, P, store and use of unseen')
        views = out
        views.scenery, views.points, views.max_range, views.headings, views.cos_half = scenery, points, float(max_range), headings, cos_half
        views.countable, views.unseen, views.slot = countable, unseen, slot
    else:
        dev = _require_gpu(points, grid.free, countable)
        views = ViewFields(grid, scenery, points, max_range, headings, cos_half, countable, unseen, slot,
                           torch.zeros(size, dtype=torch.uint8, device=dev) if store else None,
                           torch.zeros((n, p), dtype=torch.int32, device=dev),
                           torch.zeros((n, p), dtype=torch.int32, device=dev) if unseen is not None else None)
    return views.update(mask)


#: the cells - ``nx*ny`` - an env may have for :func:`basins` to keep its successors in LDS, for each of the kernel's three
#: instantiations (40, 80 and 160 KiB, less the 256 size counters); the launch is the least whose capacity holds the framed cells
#: ``(nx + 2)*(ny + 2)`` of the grid's largest env, and a larger env is jumped in global memory, to the same result
BASIN_CAPACITY = (9968, 20208, 40688)
#: the most ids :func:`basins` counts the sizes of
BASIN_MAX_IDS = 256
_INT_MAX = 2**31 - 1


class PointMarks:
    """Result of :func:`point_marks`: the cells round each of ``points`` as the seeds of ``n_fields`` seeded fields per env.
    ``marks``: the flat uint8 store, a byte a cell and field in the fields' layout (:func:`seeded_fields`' ``marks``) - 1 on every
    free cell among a point's four anchors; ``ids``: the flat int32 store in the same layout - the least id of the points that
    marked the cell, ``2**31 - 1`` where none did (:func:`basins`' ``ids``). ``points``, ``point_ids`` and ``field`` are kept by
    reference: :meth:`update` reads them as they stand."""

    def __init__(self, grid, points, n_fields, point_ids, field, marks, ids):
        self.grid, self.points, self.point_ids, self.field, self.marks, self.ids = grid, points, point_ids, field, marks, ids
        self._n_fields = int(n_fields)

    n_fields = property(lambda self: self._n_fields)
    n_points = property(lambda self: self.points.shape[1])

    def image(self, e, g=0):
        """(ny, nx) int32 view of the ids of store ``g`` of env ``e``, row 0 at the lowest y."""
        return _store_view(self.grid, self.ids, self.n_fields, e, g)

    def update(self):
        """Clears both stores and marks again in place, from :attr:`points` as they stand now - move them in place. Two fills and
        one launch of a lane a point, no host synchronisation, nothing allocated: the call can be captured in a HIP graph."""
        grid = self.grid
        dev = _require_gpu(self.points, self.marks, self.ids, grid.free, *_some(self.point_ids, self.field))
        self.marks.zero_()
        self.ids.fill_(_INT_MAX)
        _launch(dev, 'point_marks', grid, _lib.MsNavPointMarks(self.n_points, self.points.data_ptr(), _ptr(self.field), _ptr(self.point_ids),
                                                               self.n_fields, self.marks.data_ptr(), self.ids.data_ptr()))
        return self


def point_marks(grid, points, n_fields=1, ids=None, field=None):
    """The cells round points as seeds: for every env ``n_fields`` mark stores, and for point (n, k) of ``points`` (N, P, 2) float32 -
    kept by reference - mark byte 1 and id ``min(what the cell holds, id_k)`` on every FREE cell among the point's four anchors
    (:meth:`DistanceFields.at`'s). ``ids`` (N, P) integers: the points' ids, default ``k``. ``field`` (N, P) integers: the store
    each point marks; default the one store, or point k store k (then ``n_fields`` must be P). Two points that share an anchor leave
    the lower id; a point without an anchor (NaN, far from the grid, a field index out of range) marks nothing.

    ``seeded_fields(grid, seeds.marks, n_fields)`` is then the walking distance to the nearest point, and
    ``basins(fields, ids=seeds.ids, n_ids=P)`` says WHICH point that is: with the agents' positions, the floor partitioned by
    nearest agent. See :class:`PointMarks`; the rule: include/megastep_hip.h (``MsNavPointMarks``), DESIGN.md 3.22."""
    if not isinstance(n_fields, int) or n_fields < 1:
        raise RuntimeError(f'n_fields must be a positive integer; got {n_fields}')
    n, p = _points(grid, points)
    field = _field_rule(field, n, p, n_fields, 'field')
    if ids is not None:
        ids = _index(ids, 'ids', n, p)
    dev = _require_gpu(points, grid.free, *_some(ids, field))
    size = max(n_fields*grid.n_cells, 1)
    seeds = PointMarks(grid, points, n_fields, ids, field, torch.zeros(size, dtype=torch.uint8, device=dev),
                       torch.full((size,), _INT_MAX, dtype=torch.int32, device=dev))
    return seeds.update()


class Basins:
    """Result of :func:`basins`: for each field of a :class:`SeededFields` the seed every cell's path ends on. ``labels``: the flat
    int32 store in the fields' layout (field (n, g) at ``G*grid.starts[n] + g*nx*ny``) - the row-major index within the env of the
    seed the cell's chain of :meth:`SeededFields.paths` hops ends on, or, with ``ids``, what ``ids`` holds at that seed; -1 on a
    blocked cell, on a cell no seed reaches and on a cell whose chain breaks (a stale field). ``sizes`` (N, G, K) int32, None without
    ``n_ids``: the cells of each label 0..K-1; ``reached`` (N, G) int32: the cells with a label >= 0; ``passes`` (N, G) int32 or
    None. ``fields`` and ``ids`` are kept by reference: :meth:`update` reads them as they stand. The rule: include/megastep_hip.h
    (``MsNavBasins``), DESIGN.md 3.22."""

    def __init__(self, fields, ids, n_ids, labels, sizes, reached, passes=None):
        self.fields, self.grid, self.ids, self.n_ids = fields, fields.grid, ids, int(n_ids)
        self.labels, self.sizes, self.reached, self.passes = labels, sizes, reached, passes

    n_fields = property(lambda self: self.fields.n_goals)

    def image(self, e, g=0):
        """(ny, nx) int32 view of the labels of field ``g`` of env ``e``, row 0 at the lowest y."""
        return _store_view(self.grid, self.labels, self.n_fields, e, g)

    def update(self, mask=None):
        """Labels the fields marked in the (N, G) bool ``mask`` (default all) again in place, from the fields' values and
        :attr:`ids` as they stand now; the others keep labels, sizes, reached and passes. One launch, no host synchronisation,
        nothing allocated: the call can be captured in a HIP graph."""
        grid, g = self.grid, self.n_fields
        mask = _mask(mask, grid.n_envs, g, 'G')
        dev = _require_gpu(self.fields.values, self.labels, self.reached, grid.free, *_some(self.ids, mask, self.sizes, self.passes))
        _launch(dev, 'basins', grid, _lib.MsNavBasins(g, self.fields.values.data_ptr(), _ptr(self.ids), self.n_ids, _ptr(mask), self.labels.data_ptr(),
                                                      _ptr(self.sizes), self.reached.data_ptr(), _ptr(self.passes)))
        return self

    def at(self, points, goal=None):
        """(N, P) int32: the label each of ``points`` (N, P, 2) leads to - that of the cell :meth:`SeededFields.paths` starts from,
        the anchor :meth:`SeededFields.at`'s minimum is attained at; -1 exactly where that distance is +inf. ``goal`` (N, P)
        integers name the field each point asks; default the one field, or point k field k (then P must be G). One launch, a lane
        a point, no host synchronisation."""
        grid = self.grid
        n, p = _points(grid, points)
        goal = _field_rule(goal, n, p, self.n_fields, 'goal')
        dev = _require_gpu(points, self.fields.values, self.labels, grid.free, *_some(goal))
        out = torch.empty((n, p), dtype=torch.int32, device=dev)
        _launch(dev, 'basin_query', grid, _lib.MsNavBasinQuery(p, points.data_ptr(), _ptr(goal), self.fields.values.data_ptr(), self.labels.data_ptr(),
                                                               self.n_fields, out.data_ptr()))
        return out

    def masks(self, labels, field=None, out=None):
        """Byte masks of chosen basins, as a :class:`CellLayer` of ``P`` stores per env (store (n, p) at
        ``P*grid.starts[n] + p*nx*ny``): a byte is 1 on the cells whose label is ``labels[n, p]`` ((N, P) integers; a negative one
        wants none). ``field`` (N, P) integers: the field each request reads; default the one field, or request p field p.
        ``out``: the layer of an earlier call with the same P to write into; every byte is written. With ids 0..A-1 and
        ``labels=torch.arange(A).expand(N, A)`` the stores are the agents' territories: :func:`seeded_fields`' ``marks``, a
        ``gate``, a :func:`map_channel` as they are. :meth:`Regions.masks`' launch (``ms_nav_region_masks``), no host
        synchronisation."""
        return _masks(self.grid, self.labels, self.n_fields, None, labels, field, out)

    def zones(self, values=None, marks=None, n_zones=16, where=True, within_marks=False, mask=None, out=None):
        """:func:`zones` of these basins: ranked by seed without ``ids``, the id itself the zone with them."""
        return zones(self, values=values, marks=marks, n_zones=n_zones, where=where, within_marks=within_marks, mask=mask, out=out)


def basins(fields, ids=None, n_ids=0, mask=None, out=None, passes=False):
    """Which seed each cell of a :class:`SeededFields` leads to: for every field and every cell of its env the seed that the chain
    of hops :meth:`SeededFields.paths` and :meth:`SeededFields.waypoints` follow from the cell ends on - as the seed's row-major cell
    index within the env, or, with ``ids`` (a contiguous int32 tensor of one entry per cell and field in the fields' layout: a
    :class:`PointMarks`' ``ids``, a :class:`Regions`' ``labels``), as what ``ids`` holds at that seed. With the agents' cells as seeds
    this is the floor partitioned by nearest agent - a geodesic Voronoi diagram; with the unseen floor as seeds and
    ``ids=maps.frontier_regions().labels``, the frontier cluster nearest to every cell. ``n_ids`` (0..256): also count, per field, the
    cells of each label 0..n_ids-1 (``sizes``). See :class:`Basins`.

    One launch, one workgroup per field: a cell's successor once, through the very hop the paths follow, then pointer jumping in LDS
    until nothing changes; every output is an integer with one definition (include/megastep_hip.h, ``MsNavBasins``).
    The fields' values are read as they stand: on a stale field a cell whose chain breaks gets -1, and the call still ends.

    ``mask`` (N, G) bool: label only the marked fields (the others keep what ``out`` held; -1 and 0 without ``out``); ``out``: the
    :class:`Basins` of an earlier call with the same fields, ids and n_ids to write into; ``passes=True`` also records the passes
    each field took. A :class:`DistanceFields` is refused: a single goal's chains end on the goal's four anchors, not on a seed; so is
    a :class:`CostFields`: the basins' hop is unweighted and does not descend a weighted field. No
    host synchronisation: the call can be captured in a HIP graph."""
    if isinstance(fields, DistanceFields):
        raise RuntimeError("basins are of seeded fields: a DistanceFields has one goal, and its chains end on the goal's four anchors - "
                           'nothing to tell apart')
    if isinstance(fields, CostFields):
        raise RuntimeError(_WEIGHTED_BASINS)
    if not isinstance(fields, SeededFields):
        raise RuntimeError('fields must be a SeededFields')
    grid, g = fields.grid, fields.n_goals
    if not isinstance(n_ids, int) or isinstance(n_ids, bool) or not 0 <= n_ids <= BASIN_MAX_IDS:
        raise RuntimeError(f'n_ids must be an integer in 0..{BASIN_MAX_IDS}; got {n_ids}')
    size = max(g*grid.n_cells, 1)
    if ids is not None:
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.ndim != 1 or not ids.is_contiguous():
            raise RuntimeError('ids must be a contiguous 1-dimensional int32 tensor')
        if ids.shape[0] != size:
            raise RuntimeError(f'ids must have {size} entries, an int per cell and field (n_fields*n_cells = {g}*{grid.n_cells}); got {ids.shape[0]}')
    if out is not None:
        if not isinstance(out, Basins) or out.fields is not fields or out.n_ids != n_ids or not _same(out.ids, ids):
            raise RuntimeError('`out` must come from a basins call with the same fields, ids and n_ids')
        return out.update(mask)
    new = _new(_require_gpu(fields.values, grid.free, *_some(ids)))
    shape = (grid.n_envs, g)
    result = Basins(fields, ids, n_ids, new((size,), torch.int32, -1), new(shape + (n_ids,), torch.int32, 0) if n_ids else None,
                    new(shape, torch.int32, 0), new(shape, torch.int32, 0) if passes else None)
    return result.update(mask)


#: the most zones one :func:`zones` call tells apart
ZONE_MAX = 256


class Zones:
    """Result of :func:`zones`: for each env ``F`` fields and ``K`` zones a field. ``cells`` (N, F, K) int32: the cells of zone k;
    ``marked`` (N, F, K) int32: those of them that are marked (``cells`` without marks); ``least`` (N, F, K) float32: the least value
    over the zone's cells that take part - non-negative and below +inf, and marked under ``within_marks`` - +inf when none does;
    ``nearest`` (N, F, K) int32: the least cell index attaining it, -1 without one; ``points`` (N, F, K, 2) float32: that cell's
    centre, NaN without one; ``roots`` (N, F, K) int32: the label zone k stands for (ranked: the k-th root, -1 beyond the last;
    direct: k where the zone has cells, else -1); ``n_zones`` (N, F) int32: the roots there are - which may exceed K: zones from K
    on are counted there and nowhere else - or, direct, the zones that have cells. ``K``: the zones a field. The labels, values and
    marks are kept by reference: :meth:`update` reads them as they stand. The rule: include/megastep_hip.h (``MsNavZones``),
    DESIGN.md 3.28."""

    def __init__(self, grid, source, labels, n_labels, values, n_values, marks, n_marks, where, within_marks, ranked, n_fields, K, new):
        self.grid, self.source, self.labels, self.values, self.marks = grid, source, labels, values, marks
        self.n_labels, self.n_values, self.n_marks = int(n_labels), int(n_values), int(n_marks)
        self.where, self.within_marks, self.ranked = bool(where), bool(within_marks), bool(ranked)
        self._n_fields, self.K = int(n_fields), int(K)
        shape = (grid.n_envs, self._n_fields, self.K)
        self.cells, self.marked = new(shape, torch.int32, 0), new(shape, torch.int32, 0)
        self.least, self.nearest = new(shape, torch.float32, float('inf')), new(shape, torch.int32, -1)
        self.points, self.roots = new(shape + (2,), torch.float32, float('nan')), new(shape, torch.int32, -1)
        self.n_zones = new(shape[:2], torch.int32, 0)
        self._area = new((), torch.float32, grid.cell)**2

    n_fields = property(lambda self: self._n_fields)

    def update(self, mask=None):
        """Takes the fields marked in the (N, F) bool ``mask`` (default all) again in place, from the labels, values and marks as
        they stand now; the others keep every output. One launch, no host synchronisation, nothing allocated: the call can be
        captured in a HIP graph."""
        grid, f = self.grid, self.n_fields
        mask = _mask(mask, grid.n_envs, f, 'F')
        dev = _require_gpu(self.labels, self.cells, self.marked, self.least, self.nearest, self.points, self.roots, self.n_zones, grid.free,
                           *_some(self.values, self.marks, mask))
        _launch(dev, 'zones', grid, _lib.MsNavZones(f, self.labels.data_ptr(), self.n_labels, _ptr(self.values), self.n_values, _ptr(self.marks),
                                                    self.n_marks, int(self.where), int(self.within_marks), int(self.ranked), self.K, _ptr(mask),
                                                    self.cells.data_ptr(), self.marked.data_ptr(), self.least.data_ptr(), self.nearest.data_ptr(),
                                                    self.points.data_ptr(), self.roots.data_ptr(), self.n_zones.data_ptr()))
        return self

    def areas(self):
        """(N, F, K) float32: the zones' areas in square metres, ``cells*cell**2``."""
        return self.cells.float()*self._area


def _zone_store(grid, layer, what, dtype):
    """A zones layer's flat store and its stores per env: no ``field`` (store f serves field f), the dtype the place asks, and an
    entry per store and cell of the grid."""
    name = lambda d: str(d).replace('torch.', '')
    if layer.field is not None:
        raise RuntimeError(f'{what} must be a layer without a `field`: store f serves field f, one store every field')
    if layer.values.dtype != dtype:
        raise RuntimeError(f'{what} must be a layer of {name(dtype)}, not {name(layer.values.dtype)}')
    if layer.values.shape[0] < max(layer.n_fields*grid.n_cells, 1):
        raise RuntimeError(f'{what} must have {layer.n_fields}*{grid.n_cells} entries, one per store and cell; got {layer.values.shape[0]}')
    return layer.values, layer.n_fields


def zones(labels, values=None, marks=None, n_zones=16, where=True, within_marks=False, mask=None, out=None, ranked=None, grid=None):
    """A label and a number together: per zone of a labels layer the cells, the marked cells, the least value and where it is - how
    far each agent is from the nearest cell of each frontier cluster and which cell that is
    (``zones(maps.frontier_regions(), values=distance_fields(grid, positions))``), how much of each room has been seen
    (``zones(regions(grid), marks=maps)``), the oldest cell of each territory.

    ``labels``: a :class:`Regions` (ranked: zone k is the k-th region in the order of their labels), a :class:`Basins` (ranked without
    ``ids``; with them the id is the zone), or a :func:`cell_layer` of int32 with ``ranked=`` and ``grid=`` given explicitly.
    ``values``: any float layer :func:`map_channel` and :func:`cell_draws` take; ``marks``: any byte layer, with ``where``.
    Each of the three has 1 or F stores per env - F the largest of the three counts - and one store serves every field.
    ``n_zones`` (1..256): K, the zones a field. ``within_marks``: only marked cells take part in ``least``. See :class:`Zones`.

    One launch, one workgroup per field, whatever the env's size: counts by integer atomics in LDS, least and nearest by one 64-bit
    atomic min on ``(value bits, cell)``; every output is an integer or a copied float (include/megastep_hip.h, ``MsNavZones``;
    DESIGN.md 3.28).

    ``mask`` (N, F) bool: take only the marked fields (the others keep what ``out`` held; zeros, +inf, -1 and NaN without ``out``);
    ``out``: the :class:`Zones` of an earlier call with the same labels, values, marks and arguments to write into. No host
    synchronisation: the call can be captured in a HIP graph."""
    if isinstance(labels, Regions):
        own_grid, layer, is_ranked = labels.grid, CellLayer(labels.labels, labels.n_fields, None), True
    elif isinstance(labels, Basins):
        own_grid, layer, is_ranked = labels.grid, CellLayer(labels.labels, labels.n_fields, None), labels.ids is None
    elif isinstance(labels, CellLayer):
        if ranked is None or grid is None:
            raise RuntimeError('a cell_layer of labels needs ranked= (are the labels canonical cell indices?) and grid= given explicitly')
        own_grid, layer, is_ranked = grid, labels, bool(ranked)
    else:
        raise RuntimeError('labels must be a Regions, a Basins or a cell_layer of int32')
    if ranked is not None and bool(ranked) != is_ranked:
        raise RuntimeError(f'these labels are {"ranked" if is_ranked else "direct"}: ranked={ranked} contradicts them')
    if grid is not None and grid is not own_grid:
        raise RuntimeError('grid must be the grid of the labels')
    grid = own_grid
    store, n_labels = _zone_store(grid, layer, 'labels', torch.int32)
    v_store, n_values = (None, 1) if values is None else _zone_store(grid, _layer(values), 'values', torch.float32)
    m_store, n_marks = (None, 1) if marks is None else _zone_store(grid, _layer(marks, byte=True), 'marks', torch.uint8)
    f = max(n_labels, n_values, n_marks)
    for name, count in (('labels', n_labels), ('values', n_values), ('marks', n_marks)):
        if count not in (1, f):
            raise RuntimeError(f'{name} has {count} stores per env: each of labels, values and marks must have 1 or F = {f}')
    if not isinstance(n_zones, int) or isinstance(n_zones, bool) or not 1 <= n_zones <= ZONE_MAX:
        raise RuntimeError(f'n_zones must be an integer in 1..{ZONE_MAX}; got {n_zones}')
    where, within_marks = bool(where), bool(within_marks)
    if out is not None:
        if not isinstance(out, Zones) or out.grid is not grid or out.K != n_zones or out.n_fields != f or out.ranked != is_ranked or \
                out.where != where or out.within_marks != within_marks or not _same(out.labels, store) or not _same(out.values, v_store) or \
                not _same(out.marks, m_store) or (out.n_labels, out.n_values, out.n_marks) != (n_labels, n_values, n_marks):
            raise RuntimeError('`out` must come from a zones call with the same labels, values, marks, n_zones, where and within_marks')
        return out.update(mask)
    new = _new(_require_gpu(store, grid.free, *_some(v_store, m_store)))
    return Zones(grid, labels, store, n_labels, v_store, n_values, m_store, n_marks, where, within_marks, is_ranked, f, n_zones, new).update(mask)


#: the most body sizes one :func:`clearance_fields` call grids for
CLEARANCE_MAX_RADII = 8
_CLEAR_TILE = 16


def _range(max_range):
    if not isinstance(max_range, (int, float)) or isinstance(max_range, bool) or not (0 < max_range < float('inf')):
        raise RuntimeError(f'max_range must be a positive number; got {max_range}')
    return float(max_range)


class ClearanceFields:
    """Result of :func:`clearance_fields`: how much room there is at every cell of the grid. ``values``: flat float32, a value a cell in
    ``grid.free``'s layout - the distance from the cell's centre to the nearest static wall within ``max_range`` metres, +inf where
    there is none: a float layer of one store as it is (:func:`cell_draws`' band, :func:`map_channel`'s source). ``nearest``: flat
    int32 or None, that wall's env-local line index (:func:`overhead`'s ``indices``), -1 without one. ``fits``: flat uint8 or None,
    ``K = len(radii)`` stores an env in the fields' layout - store (n, k) at ``K*grid.starts[n] + k*nx*ny`` - byte k 1 where a body
    of radius ``radii[k]`` fits, exactly the ``free`` byte of ``nav_grid(scenery, cell, clearance=radii[k])``: ``marks`` for
    :func:`regions` and :func:`seeded_fields` (``n_fields=K``), ``cell_layer(clear.fits, n_fields=K)``. The scenery is kept by
    reference: :meth:`update` reads its walls as they stand. The rule: include/megastep_hip.h (``MsNavClearance``), DESIGN.md 3.23."""

    def __init__(self, grid, scenery, max_range, radii, values, nearest, fits):
        self.grid, self.scenery, self.max_range, self.radii = grid, scenery, float(max_range), tuple(float(r) for r in radii)
        self.values, self.nearest, self.fits = values, nearest, fits
        geom = grid._host_geom.astype('int64')
        self._max_tiles = max(int((((geom[:, 2] + _CLEAR_TILE - 1)//_CLEAR_TILE)*((geom[:, 3] + _CLEAR_TILE - 1)//_CLEAR_TILE)).max(initial=0)), 1)

    def image(self, e):
        """(ny, nx) float32 view of env ``e``'s distances, row 0 at the lowest y."""
        return _store_view(self.grid, self.values, 1, e, 0)

    def nearest_image(self, e):
        """(ny, nx) int32 view of env ``e``'s nearest walls, row 0 at the lowest y."""
        if self.nearest is None:
            raise RuntimeError('these clearance fields keep no nearest wall (nearest=False)')
        return _store_view(self.grid, self.nearest, 1, e, 0)

    def fits_image(self, e, k=0):
        """(ny, nx) bool view of where a body of ``radii[k]`` fits in env ``e``, row 0 at the lowest y."""
        if self.fits is None:
            raise RuntimeError('these clearance fields keep no fits (radii=None)')
        if not 0 <= k < len(self.radii):
            raise RuntimeError(f'k must be in 0..{len(self.radii) - 1}; got {k}')
        return _store_view(self.grid, self.fits.view(torch.bool), len(self.radii), e, k)

    def update(self, mask=None):
        """Computes the envs marked in the (N,) bool ``mask`` (default all) again in place, from the scenery's walls as they stand;
        the others keep their stores. One launch, no host synchronisation, nothing allocated: the call can be captured in a HIP
        graph."""
        grid = self.grid
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.shape != (grid.n_envs,):
                raise RuntimeError(f'mask must be an (N,) = ({grid.n_envs},) bool tensor')
            mask = mask.contiguous()
        dev = _require_gpu(self.values, grid.free, *_some(self.nearest, self.fits, mask))
        if self.scenery._device() != dev:
            raise RuntimeError(f'all tensors must live on one device; got {self.scenery._device()} and {dev}')
        radii = (C.c_float*8)(*self.radii)
        spec = _lib.MsNavClearance(self.max_range, len(self.radii), radii, self._max_tiles, _ptr(mask), self.values.data_ptr(), _ptr(self.nearest),
                                   _ptr(self.fits))
        _launch(dev, 'clearance', grid, spec, self.scenery._as_struct())
        return self

    def nav_grid(self, k=0):
        """The :class:`NavGrid` of body size ``radii[k]``: this grid's geometry, ``free`` a compact copy of store ``k`` of ``fits`` and
        ``clearance = radii[k]`` - what ``nav_grid(scenery, cell, clearance=radii[k])`` gives, byte for byte, without another pass
        over the walls. Raises unless ``cell <= 1.4*radii[k]`` (:func:`nav_grid`'s own condition)."""
        import numpy as np
        if self.fits is None:
            raise RuntimeError('these clearance fields keep no fits (radii=None)')
        if not isinstance(k, int) or not 0 <= k < len(self.radii):
            raise RuntimeError(f'k must be an integer in 0..{len(self.radii) - 1}; got {k}')
        grid, r, n_radii = self.grid, self.radii[k], len(self.radii)
        if np.float32(grid.cell) > np.float32(1.4)*np.float32(r):
            raise RuntimeError(f'cell ({grid.cell}) must be at most 1.4 x clearance ({r}): a coarser grid could step through a wall')
        dev = self.fits.device
        starts = grid._host_starts
        counts = torch.as_tensor(starts[1:] - starts[:-1], device=dev)
        first = torch.as_tensor(starts[:-1], device=dev)
        env = torch.repeat_interleave(torch.arange(grid.n_envs, device=dev), counts, output_size=grid.n_cells)
        at = torch.arange(grid.n_cells, device=dev) + (n_radii - 1)*first[env] + k*counts[env]
        free = torch.zeros_like(grid.free)
        free[:grid.n_cells] = self.fits[at]
        return NavGrid(grid.geom, grid.starts, free, grid.cell, r, grid._host_geom, grid._host_starts)


def clearance_fields(grid, scenery, max_range=2., nearest=False, radii=None, mask=None, out=None):
    """How much room there is: for every cell of the :func:`nav_grid` the distance from its centre to the nearest STATIC wall of
    ``scenery`` within ``max_range`` metres (+inf beyond) - the point-to-segment rule :func:`nav_grid` and :func:`overhead` test
    against a threshold, its minimum kept. The agents' own lines are not looked at: the grid is the building. See
    :class:`ClearanceFields`: ``values`` is a float layer - ``cell_draws(grid, clear, 1, 64, lo=.5, hi=inf)`` draws spawns half a
    metre from any wall, ``map_channel(clear, scale=1/max_range)`` shows the policy a distance-to-obstacle channel.
    ``nearest=True`` also keeps which wall it is. ``radii``: up to 8 body sizes (metres, each at most ``max_range``); then ``fits``
    holds, per size, the free byte :func:`nav_grid` would compute at that clearance - a scenery gridded for several bodies from one
    pass over the walls (:meth:`ClearanceFields.nav_grid`).

    One launch, a workgroup per 16 x 16 tile of cells: the env's walls culled against the tile into LDS, culled again against what
    each wave has found so far; exact - every operation is binary32 in a fixed order (include/megastep_hip.h, ``MsNavClearance``;
    DESIGN.md 3.23) and the kernel computes the rule bit for bit.

    ``mask`` (N,) bool: compute only the marked envs (the others keep what ``out`` held; +inf, -1 and 1 without ``out``); ``out``:
    the :class:`ClearanceFields` of an earlier call with the same grid, kinds of outputs and number of radii to write into - it
    takes this call's arguments. No host synchronisation: the call can be captured in a HIP graph."""
    import numpy as np
    max_range = _range(max_range)
    radii = () if radii is None else tuple(float(r) for r in radii)
    if len(radii) > CLEARANCE_MAX_RADII:
        raise RuntimeError(f'at most {CLEARANCE_MAX_RADII} radii; got {len(radii)}')
    for r in radii:
        if not (r > 0 and np.float32(r) <= np.float32(max_range)):
            raise RuntimeError(f'every radius must be positive and at most max_range ({max_range}); got {r}')
    if not hasattr(scenery, 'lines') or len(scenery.lines) != grid.n_envs:
        raise RuntimeError(f'scenery must be the Scenery the grid was laid over: {grid.n_envs} envs')
    if out is not None:
        if not isinstance(out, ClearanceFields) or out.grid is not grid or (out.nearest is not None) != bool(nearest) or len(out.radii) != len(radii):
            raise RuntimeError('`out` must come from a clearance_fields call with the same grid, use of nearest and number of radii')
        out.scenery, out.max_range, out.radii = scenery, max_range, radii
        return out.update(mask)
    new = _new(_require_gpu(grid.free))
    size = max(grid.n_cells, 1)
    result = ClearanceFields(grid, scenery, max_range, radii, new((size,), torch.float32, float('inf')),
                             new((size,), torch.int32, -1) if nearest else None, new((len(radii)*size,), torch.uint8, 1) if radii else None)
    return result.update(mask)


class Clearance:
    """Result of :func:`clearance`: ``distances`` (N, P) float32 - from each point to the nearest line within ``max_range``, +inf
    without one; ``nearest`` (N, P) int32 - that line's env-local index (below ``n_agents*n_model``: an agent's), -1 without one;
    ``towards`` (N, P, 2) float32 - the unit vector from the point to the nearest point of that line, (0, 0) on the line and
    without one."""

    def __init__(self, distances, nearest, towards):
        self.distances, self.nearest, self.towards = distances, nearest, towards


def clearance(scenery, points, max_range=2., agents=None, skip=None, mask=None, out=None):
    """A proximity reading at arbitrary points: for ``points`` (N, P, 2) float32 world points - no grid is needed - how near the
    nearest static wall of the point's env within ``max_range`` metres is, which line it is and in which direction it lies
    (:class:`Clearance`). With ``agents`` the agents' bodies count too, at their current poses; ``skip`` (N, P) integers names the
    agent whose own body each point passes over (-1, or anything else outside 0..A-1: none) - with the agents' positions as points
    and ``skip`` the agent's own number, every agent reads how near the nearest thing that is not itself is.

    One launch, one wave a point, exact: the rule of :func:`clearance_fields` (include/megastep_hip.h, ``MsNavClearQuery``;
    DESIGN.md 3.23) - at a cell's centre, without agents, the field's ``values`` and ``nearest`` bit for bit.

    ``mask`` (N, P) bool: compute only the marked points (the others keep what ``out`` held; +inf, -1 and 0 without ``out``);
    ``out``: the :class:`Clearance` of an earlier call with the same shapes. No host synchronisation: the call can be captured in
    a HIP graph."""
    _check(points, 'points', torch.float32, 3)
    n, p = points.shape[:2]
    if not hasattr(scenery, 'lines') or n != len(scenery.lines) or points.shape[2] != 2 or p < 1:
        raise RuntimeError(f'points must be (N, P, 2) with N = {len(scenery.lines)} and P >= 1; got {tuple(points.shape)}')
    max_range = _range(max_range)
    if agents is not None and tuple(agents.angles.shape) != (n, scenery.n_agents):
        raise RuntimeError('agents do not match the scenery')
    if skip is not None:
        if agents is None:
            raise RuntimeError('skip goes with agents: it names the agent whose own body each point passes over')
        skip = _index(skip, 'skip', n, p)
    mask = _mask(mask, n, p, 'P')
    dev = _query_device(scenery, agents, points, *_some(skip, mask))
    new = _new(dev)
    result = _result_for(out, (n, p, dev), 'a clearance', lambda: Clearance(new((n, p), torch.float32, float('inf')), new((n, p), torch.int32, -1),
                                                                             new((n, p, 2), torch.float32, 0.)))
    spec = _lib.MsNavClearQuery(n, p, points.data_ptr(), _ptr(skip), max_range, _ptr(mask), result.distances.data_ptr(), result.nearest.data_ptr(),
                                result.towards.data_ptr())
    with _on(dev):
        _lib.check(_lib.lib().ms_nav_clear_query(C.byref(scenery._as_struct()), C.byref(agents._plain) if agents is not None else None,
                                                 C.byref(spec), _stream(dev)))
    return result
