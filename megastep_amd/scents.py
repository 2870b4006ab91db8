"""Scent fields: a quantity that is deposited on the nav grid, diffuses through the open cells and decays (kernels:
``csrc/kernels/navscent.h``). No counterpart in the reference; reached as ``megastep_amd.cuda.<name>``."""
import torch
from . import _lib
from ._call import _check, _require_gpu, _result_for
from .nav import NavGrid, _field_rule, _launch, _mask, _points, _ptr, _some, _store_view, cell_layer

#: the framed cells - ``(nx + 2)*(ny + 2)`` - an env may have for :meth:`ScentFields.step` to tick it in LDS, for each of the kernel's
#: three instantiations (40, 80 and 160 KiB); the launch is the least that holds the grid's largest env, and a larger env is swept in
#: global memory through a workspace, to the same result
SCENT_CAPACITY = (10224, 20464, 40944)
#: the most sources an env may deposit in one tick, and the most sub-steps a tick may have
SCENT_MAX_SOURCES, SCENT_MAX_SUBSTEPS = 1024, 64


class Sniff:
    """Result of :meth:`ScentFields.sniff`: ``values`` (N, P) float32 - the scent in the cell under each point, 0 outside the
    grid, on a closed cell and for a field index out of range; ``gradients`` (N, P, 2) float32 - its central differences per
    metre in the world frame, a closed or missing side standing in as the cell itself, (0, 0) where the value is forced to 0."""

    def __init__(self, values, gradients):
        self.values, self.gradients = values, gradients


class ScentFields:
    """Result of :func:`scent_fields`: ``G`` stores per env of a quantity that evolves. ``values``: the flat float32 store, store
    (n, g) at ``G*grid.starts[n] + g*nx*ny`` (the layout of :class:`DistanceFields`; a layer as it is); ``peaks`` (N, G) float32 -
    the largest value of each store after its last tick; ``scented`` (N, G) int32 - its cells with a value above 0. The rule:
    include/megastep_hip.h (``MsNavScent``), DESIGN.md 3.35."""

    def __init__(self, grid, n_fields, rate, keep, substeps, floor, values, workspace, peaks, scented):
        self.grid, self.rate, self.keep, self.substeps, self.floor = grid, float(rate), float(keep), int(substeps), float(floor)
        self.values, self.peaks, self.scented = values, peaks, scented
        self._n_fields, self._workspace, self._ones = int(n_fields), workspace, None

    n_fields = property(lambda self: self._n_fields)

    def image(self, e, g=0):
        """(ny, nx) float32 view of store ``g`` of env ``e``, row 0 at the lowest y."""
        return _store_view(self.grid, self.values, self.n_fields, e, g)

    def layer(self, field=None):
        """The stores as a :class:`CellLayer`; ``field`` (N, P) integers name the store each view reads."""
        return cell_layer(self, field=field)

    def step(self, points=None, amounts=None, field=None, reset=None, mask=None):
        """One tick, in place, of the stores marked in the (N, G) bool ``mask`` (default all): the stores marked in the (N, G) bool
        ``reset`` are cleared; then every source deposits - ``points`` (N, P, 2) float32 with ``P`` up to 1024, ``amounts`` (N, P)
        float32 (default 1 each), ``field`` (N, P) integers naming the store each source feeds (default the one store, or source k
        store k) - in ascending source index, so that two sources on one cell add in a fixed order; a source outside the grid, on
        a closed cell, with a field index out of range or with an amount that is not above 0 deposits nothing; then ``substeps``
        sweeps of diffusion to the four open neighbours, decay and the floor; then :attr:`peaks` and :attr:`scented` are
        rewritten. One launch, one workgroup per store; exact - the kernel computes the rule bit for bit. No host
        synchronisation, nothing allocated (but a tensor of ones at the first call without ``amounts``): the call can be
        captured in a HIP graph. Returns ``self``."""
        grid, g = self.grid, self.n_fields
        n, p = grid.n_envs, 0
        if points is None:
            if amounts is not None or field is not None:
                raise RuntimeError('amounts and field go with points')
        else:
            n, p = _points(grid, points)
            if p > SCENT_MAX_SOURCES:
                raise RuntimeError(f'a tick takes at most {SCENT_MAX_SOURCES} sources an env; got {p}')
            if amounts is None:
                if self._ones is None or self._ones.shape != (n, p):
                    self._ones = torch.ones((n, p), dtype=torch.float32, device=points.device)
                amounts = self._ones
            _check(amounts, 'amounts', torch.float32, 2)
            if tuple(amounts.shape) != (n, p):
                raise RuntimeError(f'amounts must be (N, P) = ({n}, {p}); got {tuple(amounts.shape)}')
            field = _field_rule(field, n, p, g, 'field')
        reset, mask = _mask(reset, n, g, 'G', 'reset'), _mask(mask, n, g, 'G')
        dev = _require_gpu(self.values, self.peaks, self.scented, grid.free, *_some(points, amounts, field, reset, mask, self._workspace))
        _launch(dev, 'scent', grid, _lib.MsNavScent(g, p, _ptr(points), _ptr(amounts), _ptr(field), _ptr(reset), _ptr(mask), self.rate, self.keep,
                                                    self.floor, self.substeps, self.values.data_ptr(), _ptr(self._workspace),
                                                    self.peaks.data_ptr(), self.scented.data_ptr()))
        return self

    def sniff(self, points, field=None, out=None):
        """The scent under each of ``points`` (N, P, 2) float32 and which way it rises: a :class:`Sniff`. ``field`` (N, P) integers
        name the store each point asks; default the one store, or point k store k (then P must be G). ``out``: the result of an
        earlier call with the same shapes to rewrite - then nothing is allocated. One launch, a lane a point, no host
        synchronisation: the call can be captured in a HIP graph."""
        n, p = _points(self.grid, points)
        field = _field_rule(field, n, p, self.n_fields, 'field')
        dev = _require_gpu(points, self.values, self.grid.free, *_some(field))
        result = _result_for(out, (n, p, dev), 'a sniff', lambda: Sniff(torch.empty((n, p), dtype=torch.float32, device=dev),
                                                                         torch.empty((n, p, 2), dtype=torch.float32, device=dev)))
        _launch(dev, 'scent_query', self.grid, _lib.MsNavScentQuery(p, points.data_ptr(), _ptr(field), self.values.data_ptr(), self.n_fields,
                                                                    result.values.data_ptr(), result.gradients.data_ptr()))
        return result


def scent_fields(grid, n_fields=1, rate=.2, keep=.98, substeps=4, floor=1e-6):
    """``n_fields`` scent stores per env of the :func:`nav_grid`, all empty: a :class:`ScentFields`. A tick
    (:meth:`ScentFields.step`) deposits, then runs ``substeps`` (1..64) sweeps in each of which an open cell gains ``rate``
    (0..0.25) times the sum of its open 4-neighbours' differences to it - nothing flows into or out of a closed cell, so the
    scent goes through doorways and round corners, never through walls - and keeps ``keep`` (0..1) of the result; a value below
    ``floor`` (>= 0) becomes 0, so that a trail ends. With ``keep=1, floor=0`` the sum of a store is conserved up to rounding.
    The workspace of a grid too large for the kernel's LDS (:data:`SCENT_CAPACITY`) is allocated here, once."""
    if not isinstance(grid, NavGrid):
        raise RuntimeError('grid must be a cuda.NavGrid (cuda.nav_grid(scenery))')
    if not isinstance(n_fields, int) or n_fields < 1:
        raise RuntimeError(f'n_fields must be a positive integer; got {n_fields}')
    if not isinstance(substeps, int) or not 1 <= substeps <= SCENT_MAX_SUBSTEPS:
        raise RuntimeError(f'substeps must be an integer in 1..{SCENT_MAX_SUBSTEPS}; got {substeps}')
    f32 = lambda x: torch.tensor(x, dtype=torch.float32).item()           # (what the kernel is given)
    if not 0 <= f32(rate) <= .25 or not 0 <= f32(keep) <= 1 or not 0 <= f32(floor) < float('inf'):
        raise RuntimeError(f'rate must lie in [0, 0.25], keep in [0, 1] and floor in [0, inf); got {rate}, {keep}, {floor}')
    dev = grid.free.device
    size, shape = max(n_fields*grid.n_cells, 1), (grid.n_envs, n_fields)
    workspace = torch.zeros(size, dtype=torch.float32, device=dev) if grid._max_framed > SCENT_CAPACITY[-1] else None
    return ScentFields(grid, n_fields, rate, keep, substeps, floor, torch.zeros(size, dtype=torch.float32, device=dev), workspace,
                       torch.zeros(shape, dtype=torch.float32, device=dev), torch.zeros(shape, dtype=torch.int32, device=dev))
