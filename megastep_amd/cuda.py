"""The ``megastep.cuda`` operator surface on MI355X.

Mirrors the reference's pybind module ``megastepcuda`` (reference: megastep/src/wrappers.cpp:30-173) name for name -
``initialize, bake, physics, render, Ragged1D/2D/3D, Agents, Scenery, Render, Physics`` - but every compute entry
point is a hand-written gfx950 kernel reached through the C-ABI in ``include/megastep_hip.h``. Tensors stay torch-owned
(PyTorch-ROCm is the allocator/stream plumbing); the kernels run on ``torch.cuda.current_stream()``.

There is no CPU implementation here, exactly as in the reference ("If you haven't got CUDA, megastep will not work",
reference: docs/faq.rst:23-26): calling bake/physics/render on non-GPU tensors raises.
"""
import ctypes as C
import math
import numbers
import os
import torch
from . import _lib, grids
from ._lib import _on, _stream

# ---------------------------------------------------------------------------------------------------------------------
# initialize                                                                   reference: kernels.cu:18-27
# ---------------------------------------------------------------------------------------------------------------------
_config = None


_switched = __import__('threading').local()


def _ab_switches():
    """A/B switches of the library that tools set through the environment (the library itself reads none on its hot path).
    The library's pins are per THREAD (megastep_hip.hip: thread_local), so they are applied once on every thread that launches -
    physics() and render() call this - not only on the one that called initialize() (an A/B run that stepped from a
    worker thread compared two identical builds)."""
    if getattr(_switched, 'done', False):
        return
    _switched.done = True
    g = os.environ.get('MEGASTEP_RAY_GROUPS')
    if g:
        _lib.lib().ms_debug_ray_groups(int(g))           # 64-ray groups per render wave: 1, 2, 4 (default: by resolution)
    k = os.environ.get('MEGASTEP_PHYSICS_PACK')
    if k:
        _lib.lib().ms_debug_physics_pack(int(k))         # envs a physics wave takes side by side (default: by the world's size)
    o = os.environ.get('MEGASTEP_RENDER_ORDER')
    if o:
        _lib.lib().ms_debug_render_order(int(o))         # the fan schedule: 0 = render waves in fan order, 1 = slowest of last frame first
    t, e = os.environ.get('MEGASTEP_RAY_GROUP_TAIL'), os.environ.get('MEGASTEP_RAY_GROUP_TAIL_ENVS')
    if t or e:                                           # the one-group waves at the end of a launch of wide ones: in rounds / in envs
        _lib.lib().ms_debug_ray_group_tail(float(t) if t else -1., int(e) if e else -1)


def config(agent_radius, res, fov, fps):
    """The four constants of :func:`initialize` as a value (the C-ABI's ``MsConfig``, passed by value with every launch):
    what a :class:`~megastep_amd.core.Core` keeps for itself and hangs on its ``Agents``, so that several Cores of
    different resolutions, fields of view or frame rates live side by side in one process - on one device or several."""
    if not (0 < fov < 180):
        raise RuntimeError('fov must be in (0, 180) degrees')
    if res <= 0 or fps <= 0 or agent_radius <= 0:
        raise RuntimeError('agent_radius, res and fps must be positive')
    return _lib.MsConfig(float(agent_radius), int(res), float(fov), float(fps))


def initialize(agent_radius, res, fov, fps):
    """Sets the constants used by :func:`physics` and :func:`render` for callers that hand them bare tensors' holders
    (reference: wrappers.cpp:53) - the drop-in path. As in the reference this is process-global; unlike it, nothing
    device-side is mutated (the values travel by value with every launch), and it is only the FALLBACK: a call that is
    given ``config=``, or whose ``agents`` carry one (every ``Core``'s do), never looks at it."""
    global _config
    _config = config(agent_radius, res, fov, fps)
    _ab_switches()


def _cfg(agents=None, explicit=None):
    """The constants of one call: the ``config=`` argument, else the ones the agents' Core hung on them, else initialize()'s."""
    if explicit is not None:
        if not isinstance(explicit, _lib.MsConfig):
            raise RuntimeError('config must come from megastep_amd.cuda.config(agent_radius, res, fov, fps)')
        return explicit
    own = getattr(agents, '_config', None)
    if own is not None:
        return own
    if _config is None:
        raise RuntimeError('megastep_amd.cuda.initialize(agent_radius, res, fov, fps) has not been called')
    return _config


# ---------------------------------------------------------------------------------------------------------------------
# checks                                                                       reference: common.h:12-14,33-37
# ---------------------------------------------------------------------------------------------------------------------
def _check(t, name, dtype, ndim):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f'{name} must be a tensor')
    if not t.is_contiguous():
        raise RuntimeError(f'{name} must be contiguous')
    if t.dtype != dtype:
        raise RuntimeError(f'{name} must have dtype {dtype}, not {t.dtype}')
    if t.ndim != ndim:
        raise RuntimeError(f'{name} must be {ndim}-dimensional, not {t.ndim}')
    return t


def _require_gpu(*tensors):
    dev = tensors[0].device
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError('megastep_amd kernels need GPU (HIP) tensors; got a tensor on ' + str(t.device))
        if t.device != dev:
            raise RuntimeError(f'all tensors must live on one device; got {t.device} and {dev}')
    return dev


# ---------------------------------------------------------------------------------------------------------------------
# Ragged                                                                       reference: common.h:91-155
# ---------------------------------------------------------------------------------------------------------------------
class _Ragged:
    """Arrays-of-arrays over one contiguous backing tensor (reference: common.h:102-155, wrappers.cpp:14-28).

    ``starts/ends/inverse`` are int32 like ``widths``. Zero-width rows are legal here (the reference's scatter-based
    ``inverses`` mis-handles them, common.h:91-98): ``inverse`` simply never mentions them."""
    _ndim = None

    def __init__(self, vals, widths):
        _check(vals, 'vals', torch.float32, self._ndim)
        _check(widths, 'widths', torch.int32, 1)
        if vals.device != widths.device:
            raise RuntimeError('vals and widths must be on the same device')
        ends = widths.cumsum(0).to(torch.int32)
        total = int(ends[-1]) if len(widths) else 0
        if total != vals.shape[0]:
            raise RuntimeError(f'widths sum to {total} but vals has {vals.shape[0]} rows')
        self._vals, self._widths = vals, widths
        self._starts, self._ends = ends - widths, ends
        self._inverse = torch.repeat_interleave(
            torch.arange(len(widths), dtype=torch.int32, device=widths.device), widths.long())

    vals = property(lambda self: self._vals)
    widths = property(lambda self: self._widths)
    starts = property(lambda self: self._starts)
    ends = property(lambda self: self._ends)
    inverse = property(lambda self: self._inverse)

    def __len__(self):
        return len(self._widths)

    def __getitem__(self, x):
        if isinstance(x, numbers.Integral):
            return self._vals[int(self._starts[x]):int(self._ends[x])]
        if isinstance(x, slice):
            start, stop, step = x.indices(len(self._widths))
            if step != 1:
                raise IndexError('Ragged slices must have step 1')
            if stop <= start:
                return type(self)(self._vals[:0], self._widths[:0])
            return type(self)(self._vals[int(self._starts[start]):int(self._ends[stop - 1])], self._widths[start:stop])
        raise TypeError(f"Can't index a Ragged with a {type(x).__name__}")

    def size(self, i):
        return self._vals.shape[i]

    def clone(self):
        return type(self)(self._vals.clone(), self._widths.clone())

    def numpyify(self):
        from .ragged import RaggedNumpy
        return RaggedNumpy(self._vals.detach().cpu().numpy().copy(), self._widths.detach().cpu().numpy().copy())

    def to(self, device):
        return type(self)(self._vals.to(device), self._widths.to(device))

    def __repr__(self):
        return f'{type(self).__name__}(vals={tuple(self._vals.shape)}, widths=({len(self._widths)},))'


class Ragged1D(_Ragged):
    _ndim = 1


class Ragged2D(_Ragged):
    _ndim = 2


class Ragged3D(_Ragged):
    _ndim = 3


# ---------------------------------------------------------------------------------------------------------------------
# Agents / Scenery / Render / Physics                                          reference: common.h:157-226
# ---------------------------------------------------------------------------------------------------------------------
class Agents:
    """Holds the (N, A[, 2]) state tensors of the agents (reference: common.h:157-177, wrappers.cpp:103-120).
    :func:`physics` updates them in place."""

    #: ``False`` sends ms_render through its own heading kernel instead of the cache ms_physics leaves (tests, A/B runs)
    HEADING_CACHE = True
    #: ``False`` leaves ``MsAgents.schedule`` NULL: the render deals its waves in fan order (tests, A/B runs)
    SCHEDULE = True

    def __init__(self, angles, positions, angvelocity, velocity, config=None):
        #: the constants :func:`physics` / :func:`render` use for these agents (:func:`config`); None: initialize()'s
        self._config = config
        self._angles = _check(angles, 'angles', torch.float32, 2)
        self._positions = _check(positions, 'positions', torch.float32, 3)
        self._angvelocity = _check(angvelocity, 'angvelocity', torch.float32, 2)
        self._velocity = _check(velocity, 'velocity', torch.float32, 3)
        n, a = angles.shape
        if positions.shape != (n, a, 2) or velocity.shape != (n, a, 2) or angvelocity.shape != (n, a):
            raise RuntimeError('agent tensors must be (N, A), (N, A, 2), (N, A), (N, A, 2)')
        # The heading cache (include/megastep_hip.h, MsAgents.headings): physics leaves each agent's sin/cos there for
        # the next render. `_struct` carries it; `_plain` does not, for renders before any physics call has filled it.
        self._headings = torch.full((n, a, 4), float('nan'), dtype=torch.float32, device=angles.device)
        # The fan schedule (MsAgents.schedule): the render leaves every (env, agent)'s cost in its first half, the next physics
        # step sorts them into its second half - the order the render behind it starts its waves in. The identity to begin
        # with, so that a render before any physics is served; SCHEDULE = False goes without (today's mapping).
        self._schedule = torch.stack([torch.zeros(n*a, dtype=torch.int32, device=angles.device),
                                      torch.arange(n*a, dtype=torch.int32, device=angles.device)]) if self.SCHEDULE else None
        ptrs = (angles.data_ptr(), positions.data_ptr(), angvelocity.data_ptr(), velocity.data_ptr())
        schedule = self._schedule.data_ptr() if self.SCHEDULE and angles.device.type == 'cuda' else None
        self._struct = _lib.MsAgents(*ptrs, self._headings.data_ptr(), schedule)
        self._plain = _lib.MsAgents(*ptrs, None, schedule)
        self._cached = False
        self._epoch = 0             # moved on by every physics call and every respawn (modules.IMU's stale-reading check)
        # (measured at 16 k to 262 k agents: one launch and one kernel boundary fewer per step, 1-3 % of the step)
        self._use_cache = bool(self.HEADING_CACHE)
        devices = {t.device for t in (angles, positions, angvelocity, velocity)}
        self._dev = devices.pop() if len(devices) == 1 else None         # None: tensors on mixed devices

    angles = property(lambda self: self._angles)
    positions = property(lambda self: self._positions)
    angvelocity = property(lambda self: self._angvelocity)
    velocity = property(lambda self: self._velocity)

    def state(self, e):
        from . import arrdict
        return arrdict.arrdict(angles=self._angles[e], positions=self._positions[e],
                               angvelocity=self._angvelocity[e], velocity=self._velocity[e])


class Scenery:
    """Holds the geometry, lights and textures of every env (reference: common.h:179-214, wrappers.cpp:122-145).

    ``lines`` is ragged per env with the ``n_agents*len(model)`` agent lines first; ``textures`` and ``baked`` are
    ragged per *line*. ``baked`` starts as ones and is filled in by :func:`bake`."""

    def __init__(self, n_agents, lights, lines, textures, model, geom=None):
        if not isinstance(lights, Ragged2D) or not isinstance(lines, Ragged3D) or not isinstance(textures, Ragged2D):
            raise RuntimeError('lights, lines, textures must be Ragged2D, Ragged3D, Ragged2D')
        _check(model, 'model', torch.float32, 3)
        if lights.vals.shape[1:] != (3,) or lines.vals.shape[1:] != (2, 2) or textures.vals.shape[1:] != (3,) \
                or model.shape[1:] != (2, 2):
            raise RuntimeError('lights/lines/textures/model rows must be (3,), (2, 2), (3,), (2, 2)')
        if len(lights) != len(lines):
            raise RuntimeError('lights and lines must have one row per env')
        if len(textures) != lines.vals.shape[0]:
            raise RuntimeError('textures must have one row per line')
        self._n_agents = int(n_agents)
        self._lights, self._lines, self._textures, self._model = lights, lines, textures, model
        self._baked = Ragged1D(torch.ones_like(textures.vals[:, 0]).contiguous(), textures.widths)
        # how far the agent's outline reaches from its origin (MsScenery.model_radius): inside the near plane, as the
        # reference's is, an agent's rays cannot hit its own outline and the renderer does not try
        radius = float(model.reshape(-1, 2).norm(dim=1).max()) if model.numel() else 0.
        self._model_radius = radius if radius == radius and radius < float('inf') else 0.
        # Beyond the reference: `geom` (n_envs,) int32 names, for every env, the first env with bit-identical walls
        # and light positions (see MsScenery.env_geom). bake() then does the expensive part once per distinct
        # floorplan, and such envs share one light grid. None: every env stands alone.
        if geom is not None:
            _check(geom, 'geom', torch.int32, 1)
            if len(geom) != len(lines) or geom.device != lines.vals.device:
                raise RuntimeError('geom must have one entry per env, on the same device as the lines')
        self._geom = geom
        self._struct = None
        self._lg = None             # the grids.LightGrid, or None; decided by _as_struct unless sharding carried one over
        self._lg_decided = False
        self._wg_sum = None         # checksum of the static walls the wall grid was built from
        self._wg_weights = None
        self._wg = None             # the grids.WallGrid, or None; made by bake()
        self._wg_report = self._lg_report = None      # what was built, at which cell size, in how many bytes (grid_report())
        self._dev = None

    n_agents = property(lambda self: self._n_agents)
    lights = property(lambda self: self._lights)
    lines = property(lambda self: self._lines)
    textures = property(lambda self: self._textures)
    model = property(lambda self: self._model)
    baked = property(lambda self: self._baked)
    geom = property(lambda self: self._geom)

    def state(self, e):
        from . import dotdict
        s, t = int(self._lines.starts[e]), int(self._lines.ends[e])
        return dotdict.dotdict(n_agents=self._n_agents, lights=self._lights[e], lines=self._lines[e],
                               textures=self._textures[s:t], model=self._model, baked=self._baked[s:t])

    LIGHT_GRID = True           # False: no light grid (ms_render's two-kernel path; tests)
    #: cell size of the light grid, metres. (0.25 -> 0.125 in round 4: half as many rays that land on an agent still have a
    #: light the grid cannot call - the rays whose waves a launch ends up waiting for; four times the cells.)
    LIGHT_GRID_CELL = float(os.environ.get('MEGASTEP_LIGHT_GRID_CELL', .125))     # (the environment switch is for A/B runs)
    LIGHT_GRID_POOL = 12        # pool words per cell (4 bytes each) for the candidate lists
    #: what the light grid may take, bytes. A cell costs 16 B of verdicts + 8 B of list header + LIGHT_GRID_POOL x (4 B candidate
    #: + 16 B of its wall's row) = 264 B: at 0.125 m cells 17 KB per square metre, 3-4 MB per benchmark floorplan, 14 MB per large
    #: one - 1024 plans (the headline world) 3.4 GB, 4096 large ones 54 GB. Over budget the grid first goes without the
    #: candidates' rows (72 B a cell: ms_render then fetches a candidate's wall one trip later, the round-3 behaviour), then
    #: doubles its cells (a quarter of them, and more lights left UNKNOWN per cell: slower for the rays that land on an agent,
    #: the same bits) until it fits. `Scenery.grid_report()` says what was built.
    #: None: an eighth of the device's memory (36 GB of an MI355X's 288; 8 GiB for tensors that are not on a GPU).
    LIGHT_GRID_BYTES = int(float(os.environ['MEGASTEP_LIGHT_GRID_BYTES'])) if os.environ.get('MEGASTEP_LIGHT_GRID_BYTES') else None

    #: the wall grid (include/megastep_hip.h, MsScenery.wg_*): cell size in metres; the step lengths its collision lists
    #: cover (0.7 m: the momentum module at its defaults never reaches farther; 1.3 m: nor does the simple one at 10 fps);
    #: the near plane its visibility lists allow for; how much memory it may take - beyond that the cells are doubled in
    #: size, twice at most, then it is left out
    WALL_GRID = os.environ.get('MEGASTEP_WALL_GRID', '1') != '0'       # (the environment switch is for A/B runs)
    WALL_GRID_CELL = float(os.environ.get('MEGASTEP_WALL_GRID_CELL', .25))        # (the environment switch is for A/B runs)
    WALL_GRID_REACH = (.7, 1.3)
    WALL_GRID_NEAR = .12
    #: (bytes; None: a quarter of the device's memory - 72 GB of an MI355X's 288: the headline world's 1024 plans take 1.7 GB,
    #: C2's 4096 plans 6.9 GB, 4096 large plans - C5's share on the reference's floorplan diversity - 35 GB at 0.25 m cells;
    #: with rounds 3-4's flat 8 GiB that world fell back to 1 m cells and a step a third slower)
    WALL_GRID_BYTES = int(float(os.environ['MEGASTEP_WALL_GRID_BYTES'])) if os.environ.get('MEGASTEP_WALL_GRID_BYTES') else None
    WALL_GRID_MAX_CELLS = 1 << 18       # per floorplan
    WALL_GRID_SCRATCH = 1 << 30         # bytes of bitmaps in flight while it is built
    WALL_GRID_COARSE = 4                # the parent level's cells, in cells (None: one level, every wall a candidate)

    def grid_report(self):
        """What bake() built around the floorplans, for logs and bench lines: {'wall_grid': {bytes, cell, floorplans, ...} or
        None, 'light_grid': {bytes, cell, cells, candidate_rows, ...} or None, 'bake_seconds': {lighting, wall_grid} of the last
        cuda.bake()} - the sizes actually allocated and the cell sizes actually used (either grid coarsens itself to stay inside
        its byte budget)."""
        marks = getattr(self, '_bake_marks', None)
        if getattr(self, '_bake_s', None) is None and marks is not None and marks[0] is not None:
            ev, wall_grid = marks
            ev[2].synchronize()
            self._bake_s = dict(lighting=ev[0].elapsed_time(ev[1])*1e-3, wall_grid=ev[1].elapsed_time(ev[2])*1e-3 if wall_grid else 0.)
        return dict(wall_grid=self._wg_report, light_grid=self._lg_report, bake_seconds=getattr(self, '_bake_s', None))

    _light_grid = grids.light_grid      # (builds a fresh light grid each call; _as_struct decides once per scenery)

    def _as_struct(self):
        if self._struct is None:
            li, ln, tx = self._lights, self._lines, self._textures
            if not self._lg_decided:
                # (one agent per env: no ray ever lands on an agent line, so nothing would consult the grid)
                self._lg = self._light_grid() if self._n_agents > 1 and self.LIGHT_GRID else None
                self._lg_decided = True
            self._struct = _lib.MsScenery(
                n_envs=len(ln), n_agents=self._n_agents, n_model=self._model.shape[0],
                lights_vals=li.vals.data_ptr(), lights_widths=li.widths.data_ptr(), lights_starts=li.starts.data_ptr(),
                lines_vals=ln.vals.data_ptr(), lines_widths=ln.widths.data_ptr(), lines_starts=ln.starts.data_ptr(), lines_inverse=ln.inverse.data_ptr(),
                textures_vals=tx.vals.data_ptr(), textures_widths=tx.widths.data_ptr(), textures_starts=tx.starts.data_ptr(),
                textures_inverse=tx.inverse.data_ptr(), model=self._model.data_ptr(), baked_vals=self._baked.vals.data_ptr(),
                n_lines_total=ln.vals.shape[0], n_lights_total=li.vals.shape[0], n_texels_total=tx.vals.shape[0],
                env_geom=self._geom.data_ptr() if self._geom is not None else None, model_radius=self._model_radius,
                **grids.struct_fields(self._lg, self._wg))
        return self._struct

    def check_wall_grid(self):
        """Raises if the static walls are no longer the ones the wall grid was built from (see :func:`bake`): rays and
        collisions that walk a stale grid silently miss the walls that moved. One reduction over the lines and a sync -
        switched on for every :func:`render` / :func:`physics` call by ``MEGASTEP_CHECK_GRID=1`` (as the test suite runs)."""
        if self._wg is not None and self._wg_sum != grids.wall_checksum(self):
            raise RuntimeError('static walls have been changed since cuda.bake() built the wall grid from them: bake again '
                               '(or bake(wall_grid=False) to go without a grid)')

    def _build_wall_grid(self):
        """(Re)builds the wall grid from the static walls as they are now (called by :func:`bake`; see grids.wall_grid)."""
        self._wg = self._wg_sum = self._wg_report = self._struct = None      # (the scans read a struct without a wall grid)
        self._wg = grids.wall_grid(self) if self.WALL_GRID else None
        self._wg_sum, self._struct = (grids.wall_checksum(self) if self._wg is not None else None), None

    def _bake_plan(self):
        """Scratch for the two-phase bake (MsScenery.bake_vis): for each representative env, lights x ceil(texels/64)
        words. Returns (vis, starts) - torch tensors that must outlive the launch."""
        li, ln, tx = self._lights, self._lines, self._textures
        first, last = ln.starts.long(), (ln.ends - 1).long().clamp(min=0)
        texels = torch.where(ln.widths > 0, tx.ends.long()[last] - tx.starts.long()[first], torch.zeros_like(first))
        lay = grids.representatives(li.widths.long()*((texels + 63)//64), self._geom)
        # (zeroed: a row that visibility_kernel's bounds check skipped reads as 'nothing blocks', never as garbage)
        return torch.zeros(max(lay.total, 1), dtype=torch.int64, device=ln.vals.device), lay.starts.contiguous()

    def _device(self):
        """The GPU all of this scenery's tensors live on (checked once; the tensors cannot be swapped out)."""
        if self._dev is None:
            self._dev = _require_gpu(*self._tensors())
        return self._dev

    def _tensors(self):
        li, ln, tx = self._lights, self._lines, self._textures
        return (ln.vals, ln.widths, li.vals, li.widths, tx.vals, tx.widths, self._model, self._baked.vals)


class Render:
    """Result of :func:`render` (reference: common.h:216-222, wrappers.cpp:147-164). Fields that were not asked for
    are ``None``; ``obs_rgb``/``obs_depth`` are the pooled observations when the call asked for them."""

    def __init__(self, indices, locations, dots, distances, screen, obs_rgb=None, obs_depth=None, obs_subsample=None,
                 obs_centre=None):
        self._t = (indices, locations, dots, distances, screen)
        self._obs = (obs_rgb, obs_depth, obs_subsample, obs_centre)

    indices = property(lambda self: self._t[0])
    locations = property(lambda self: self._t[1])
    dots = property(lambda self: self._t[2])
    distances = property(lambda self: self._t[3])
    screen = property(lambda self: self._t[4])
    obs_rgb = property(lambda self: self._obs[0])
    obs_depth = property(lambda self: self._obs[1])
    obs_subsample = property(lambda self: self._obs[2])
    obs_centre = property(lambda self: self._obs[3])


class Physics:
    """Result of :func:`physics` (reference: common.h:224-226, wrappers.cpp:166-172)."""

    def __init__(self, progress):
        self._progress = progress

    progress = property(lambda self: self._progress)


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
def _agents_on(agents, dev):
    if agents._dev != dev:
        if agents._dev is None or not agents._dev.type == 'cuda':
            raise RuntimeError('megastep_amd kernels need GPU (HIP) tensors; the agents are on ' + str(agents._dev or 'several devices'))
        raise RuntimeError(f'all tensors must live on one device; got {agents._dev} and {dev}')


def _ms_agents(agents, step, telemetry=False):
    """The MsAgents a launch gets: with the heading cache where the launch fills it (a physics step, while the agents use the
    cache) or reads it (a render after a physics call filled it - not with ``telemetry``, whose counters the self-contained path
    keeps), else without."""
    cached = agents._use_cache if step else agents._cached and not telemetry
    return agents._struct if cached else agents._plain


def bake(scenery, scratch=True, wall_grid=True):
    """Pre-computes the static lighting of every texel into ``scenery.baked`` (reference: wrappers.cpp:61,
    kernels.cu:270-293). ``scratch=False`` selects the library's self-contained one-pass kernel (no temporary
    allocation, no sharing between envs; same result). Baking also (re)builds the scenery's wall grid - the per-cell
    lists of walls that :func:`render` and :func:`physics` walk instead of every line of the env (include/megastep_hip.h,
    ``MsScenery.wg_*``) - from the walls as they are now: like the baked light it goes stale if static walls are moved
    afterwards (bake again, or pass ``wall_grid=False`` to go without). ``Scenery.check_wall_grid()`` tells (it raises if
    the walls are not the ones the grid was built from), and ``MEGASTEP_CHECK_GRID=1`` has every :func:`render` and
    :func:`physics` call ask it first. HIP graphs captured before a re-bake hold pointers into the old grid: capture again."""
    dev = scenery._device()
    # bake uses none of the initialize() constants (kernels.cu:238-293), and scene.scenery() calls it before any Core
    # exists, so the config is optional here
    cfg = C.byref(_config) if _config is not None else None
    struct = scenery._as_struct()
    if scratch:
        vis, starts = scenery._bake_plan()
        struct = _lib.MsScenery.from_buffer_copy(struct)
        struct.bake_vis, struct.bake_vis_starts, struct.bake_vis_words = vis.data_ptr(), starts.data_ptr(), vis.shape[0]
    # What it cost goes into grid_report() - from events on the CURRENT stream, read when the report is asked for: no device-wide
    # synchronize here (round 5 had three: every other stream of the device stalled for a number nobody may want, and a bake
    # inside a stream capture raised).
    with _on(dev):
        timed = not torch.cuda.is_current_stream_capturing()
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timed else None
        if timed:
            marks[0].record()
        _lib.check(_lib.lib().ms_bake(C.byref(struct), cfg, _stream(dev)))
        if timed:
            marks[1].record()
        if wall_grid:
            scenery._build_wall_grid()
        if timed:
            marks[2].record()
    scenery._bake_marks, scenery._bake_s = (marks, wall_grid), None


def _step_options(agents, shape, movement, respawn, lifespans, imu):
    """``physics``' optional arguments (see there) as the C-ABI's MsMovement / MsStepExtras, by reference (or None)."""
    mv = None
    if movement is not None:
        actions, table, keep = movement
        _check(table, 'movement table', torch.float32, 2)
        if actions.dtype != torch.int64 or not actions.is_contiguous() or actions.shape != agents.angles.shape \
                or table.shape[1:] != (3,) or table.shape[0] < 1:
            raise RuntimeError('movement must be ((N, A) contiguous int64 actions, (K, 3) float32 table, keep)')
        _require_gpu(actions, table)
        mv = C.byref(_lib.MsMovement(actions.data_ptr(), table.data_ptr(), table.shape[0], float(keep)))
    ex = None
    if respawn is not None or lifespans is not None or imu is not None:
        x = _lib.MsStepExtras(imu_ang_scale=1., imu_speed_scale=1.)
        used = []
        if respawn is not None:
            mask, choices = respawn['mask'], respawn['choices']
            positions, angles = respawn['positions'], respawn['angles']
            if mask.dtype != torch.bool or mask.shape != shape or choices.dtype != torch.int64 or choices.shape != shape \
                    or positions.dtype != torch.float32 or positions.ndim != 4 or positions.shape[:2] != shape \
                    or positions.shape[3] != 2 or angles.dtype != torch.float32 or angles.shape != positions.shape[:3] \
                    or not all(t.is_contiguous() for t in (mask, choices, positions, angles)):
                raise RuntimeError('respawn needs a (N, A) bool mask, (N, A) int64 choices, (N, A, S, 2) float32 positions '
                                   'and (N, A, S) float32 angles, all contiguous')
            x.respawn_mask, x.respawn_choice = mask.data_ptr(), choices.data_ptr()
            x.spawn_positions, x.spawn_angles, x.n_spawns = positions.data_ptr(), angles.data_ptr(), positions.shape[2]
            x.respawn_after = int(bool(respawn.get('after', False)))
            used += [mask, choices, positions, angles]
        if lifespans is not None:
            if respawn is None:
                raise RuntimeError('lifespans need a respawn mask to report into')
            ages, maxima, fresh = lifespans['lifespans'], lifespans['max_lifespans'], lifespans['fresh']
            if any(t.dtype != torch.int32 or t.shape != shape or not t.is_contiguous() for t in (ages, maxima, fresh)):
                raise RuntimeError('lifespans, max_lifespans and fresh must be contiguous (N, A) int32 tensors')
            x.lifespans, x.max_lifespans, x.fresh_max = ages.data_ptr(), maxima.data_ptr(), fresh.data_ptr()
            used += [ages, maxima, fresh]
        if imu is not None:
            obs, ang_scale, speed_scale = imu
            if obs.dtype != torch.float32 or obs.shape != shape + (3,) or not obs.is_contiguous():
                raise RuntimeError('the imu output must be a contiguous (N, A, 3) float32 tensor')
            x.imu, x.imu_ang_scale, x.imu_speed_scale = obs.data_ptr(), float(ang_scale), float(speed_scale)
            used.append(obs)
        _require_gpu(*used)
        ex = C.byref(x)
    return mv, ex


def physics(scenery, agents, movement=None, out=None, respawn=None, lifespans=None, imu=None, config=None):
    """Advances the agents by one step, stopping them at walls and at each other; updates ``agents`` in place and
    returns :class:`Physics` with the (N, A) ``progress`` (reference: wrappers.cpp:69, kernels.cu:179-230).

    Beyond the reference, the tensor ops its callers run around the step can ride in the same launch
    (include/megastep_hip.h, MsMovement / MsStepExtras):

    * ``movement=(actions, table, keep)``: the movement modules' velocity update first: ``actions`` (N, A) int64 rows of
      ``table`` (K, 3) = agent-frame [dx, dy, d angvelocity]; velocities become ``keep*old + delta`` (``keep = 0`` assigns);
    * ``respawn=dict(mask, choices, positions, angles, after=False)``: agents marked in the (N, A) bool ``mask`` get
      pose ``positions[n, a, choices[n, a]]`` / ``angles[...]`` and zero velocities - before the step (and before the
      movement), or after it with ``after=True``;
    * ``lifespans=dict(lifespans, max_lifespans, fresh)``: (N, A) int32 ages tick first; agents at their maximum are
      added to ``respawn['mask']`` (required with it), start over and take ``fresh`` as their new maximum;
    * ``imu=(out, ang_scale, speed_scale)``: the (N, A, 3) IMU observation of the state the step leaves behind.

    ``out``: the :class:`Physics` of an earlier call, to write ``progress`` into instead of allocating.
    ``config``: the constants of this call (:func:`config`); default: the ones ``agents`` carry (a Core's do), else initialize()'s."""
    dev = scenery._device()
    _agents_on(agents, dev)
    shape = (len(scenery.lines), scenery.n_agents)
    if agents.angles.shape != shape:
        raise RuntimeError('agents do not match the scenery: expected (n_envs, n_agents) = '
                           f'{shape}, got {tuple(agents.angles.shape)}')
    mv, ex = _step_options(agents, shape, movement, respawn, lifespans, imu)
    progress = torch.empty_like(agents.angles) if out is None else out.progress      # `out`: an earlier call's Physics
    _ab_switches()
    _check_grid(scenery, dev)
    with _on(dev):
        _lib.check(_lib.lib().ms_step_physics(C.byref(scenery._as_struct()), C.byref(_ms_agents(agents, step=True)),
                                              mv, ex, C.c_void_p(progress.data_ptr()), C.byref(_cfg(agents, config)), _stream(dev)))
    agents._cached = agents._use_cache
    agents._epoch += 1
    return Physics(progress) if out is None else out


def deathmatch_shoot(centre, positions, upper, health, damage, dead, clearance=1., hit_damage=.05, tick_damage=.001,
                     out=None, matchings=False):
    """The Deathmatch env's game logic between one frame and the next as ONE launch (include/megastep_hip.h, MsDeathmatch;
    reference: demo/envs/deathmatch.py:46-88 - ``_reset`` + ``_shoot`` + the ``health`` observation, some twenty tensor ops).

    ``centre`` (N, A, 2) int32: :func:`render`'s ``obs_centre`` of this frame; ``positions`` (N, A, 2); ``upper`` (N, 2): the
    floorplans' extents + clearance; ``health``, ``damage`` (N, A) float32 and ``dead`` (N, A) bool, all updated IN PLACE:
    agents marked in ``dead`` (the mask this step's physics launch respawned by) start from health 1 / damage 0, then
    everyone takes this frame's hits, wounds and strays, and ``dead`` becomes ``health <= 0`` - the next step's mask.
    Returns ``(reset, reward, health_obs[, matchings])``: the incoming ``dead``, the hits dealt, a copy of the new health -
    fresh tensors, or the ones of an earlier call passed as ``out``."""
    n, a = health.shape
    _check(centre, 'centre', torch.int32, 3); _check(positions, 'positions', torch.float32, 3); _check(upper, 'upper', torch.float32, 2)
    _check(health, 'health', torch.float32, 2); _check(damage, 'damage', torch.float32, 2); _check(dead, 'dead', torch.bool, 2)
    if centre.shape != (n, a, 2) or positions.shape != (n, a, 2) or upper.shape != (n, 2) or damage.shape != (n, a) or dead.shape != (n, a):
        raise RuntimeError('deathmatch_shoot: centre (N, A, 2), positions (N, A, 2), upper (N, 2), health / damage / dead (N, A)')
    dev = _require_gpu(centre, positions, upper, health, damage, dead)
    if out is None:
        out = (torch.empty_like(dead), torch.empty_like(health), torch.empty_like(health)) + \
              ((torch.empty((n, a, a), dtype=torch.bool, device=dev),) if matchings else ())
    dm = _lib.MsDeathmatch(centre.data_ptr(), positions.data_ptr(), upper.data_ptr(), float(clearance), float(hit_damage), float(tick_damage),
                           health.data_ptr(), damage.data_ptr(), dead.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                           out[3].data_ptr() if len(out) > 3 else None)
    with _on(dev):
        _lib.check(_lib.lib().ms_deathmatch_shoot(n, a, C.byref(dm), _stream(dev)))
    return out


def explorer_books(tally, before, lengths, epoch, over, slack, pixels, display=False):
    """The Explorer env's bookkeeping between one frame and the next as ONE launch (include/megastep_hip.h, MsExplorer;
    reference: demo/envs/explorer.py:45-90 - the reward, the counters of ``_reset`` and the episode rule of ``step``, a dozen
    tensor ops). ``tally`` is the first-sight count :func:`render` keeps (``seen=``), ``epoch`` its epochs; ``before``,
    ``lengths`` (N,) int32 and ``over`` (N,) bool are the env's own - all updated IN PLACE: ``over`` comes in as the envs this
    step respawned (they get no reward) and leaves as the envs the next step is to respawn, which have already forgotten what
    they saw. Returns ``(reset, reward)`` - the incoming ``over`` and this frame's reward - plus, with ``display``, the
    potential and the lengths as this step leaves them."""
    n = tally.shape[0]
    for name, t in (('tally', tally), ('before', before), ('lengths', lengths), ('epoch', epoch)):
        _check(t, name, torch.int32, 1)
        if t.shape != (n,):
            raise RuntimeError('explorer_books: tally, before, lengths, epoch and over must all be (N,)')
    _check(over, 'over', torch.bool, 1)
    if over.shape != (n,):
        raise RuntimeError('explorer_books: tally, before, lengths, epoch and over must all be (N,)')
    dev = _require_gpu(tally, before, lengths, epoch, over)
    ptrs = (tally.data_ptr(), before.data_ptr(), lengths.data_ptr(), epoch.data_ptr(), over.data_ptr())
    reset = torch.empty_like(over)
    rest = torch.empty((3 if display else 1, n), dtype=torch.float32, device=dev)         # (one allocation: reward | potential | lengths)
    out = (reset, rest[0]) + ((rest[1], rest[2].view(torch.int32)) if display else ())
    ex = _lib.MsExplorer(*ptrs, int(slack), int(pixels),
                         reset.data_ptr(), rest.data_ptr(), rest.data_ptr() + 4*n if display else None, rest.data_ptr() + 8*n if display else None)
    with _on(dev):
        _lib.check(_lib.lib().ms_explorer_books(n, C.byref(ex), _stream(dev)))
    return out


FIELDS = ('indices', 'locations', 'dots', 'distances', 'screen')
#: MEGASTEP_CHECK_GRID=1: every render / physics call first makes sure the static walls are still the ones the wall grid
#: was built from (a reduction over the lines and a host sync per call - for debugging and the test suite, off by default)
CHECK_GRID = os.environ.get('MEGASTEP_CHECK_GRID', '0') not in ('', '0')


def _check_grid(scenery, dev):
    if CHECK_GRID and scenery._wg is not None:
        with _on(dev):                                                    # (the stream that matters is `dev`'s current one)
            capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            scenery.check_wall_grid()


def step_render(scenery, agents, fields=None, pooled=None, out=None, seen=None, config=None, movement=None, respawn=None,
                lifespans=None, imu=None):
    """One step of the hot path - :func:`physics` then :func:`render`, what every ``env.step()`` of the reference runs
    (wrappers.cpp:69 + :82) - as one call, and where the shapes allow it as ONE LAUNCH (include/megastep_hip.h,
    ``ms_step_render``): with one agent per env and at most 64 rays (BASELINE config 2, the Explorer shape) an agent is a single
    wavefront, which runs its env's physics step and renders from the pose it ends on. Any other shape is the two launches,
    as if the two calls had been made. Same bits either way (tests/test_gpu_step_render.py).

    Arguments as :func:`render`'s, and :func:`physics`' ``movement`` / ``respawn`` / ``lifespans`` / ``imu`` (a whole env.step() of a
    single-agent env of up to 64 rays - the reference's tutorial env - is then one launch); ``out``: the ``(Physics, Render)`` of an
    earlier call, to write into. Returns ``(Physics, Render)``."""
    physics_out, render_out = out if out is not None else (None, None)
    dev, cfg, result = _render_call(scenery, agents, fields, pooled, render_out, seen, config)
    mv, ex = _step_options(agents, tuple(agents.angles.shape), movement, respawn, lifespans, imu)
    progress = torch.empty_like(agents.angles) if physics_out is None else physics_out.progress
    with _on(dev):
        _lib.check(_lib.lib().ms_move_step_render(C.byref(scenery._as_struct()), C.byref(_ms_agents(agents, step=True)), mv, ex,
                                                  C.c_void_p(progress.data_ptr()), C.byref(result._struct), C.byref(cfg), _stream(dev)))
    agents._cached = agents._use_cache
    agents._epoch += 1
    return (Physics(progress) if physics_out is None else physics_out), result


def render(scenery, agents, fields=None, pooled=None, telemetry=False, out=None, seen=None, config=None):
    """Casts ``res`` rays per agent and shades them; also rewrites the agents' model lines in ``scenery.lines``
    (reference: wrappers.cpp:82, kernels.cu:452-475). Returns :class:`Render`.

    Extensions over the reference, all off by default: ``fields`` names the per-ray outputs that are wanted
    (the others are neither written nor allocated; a call that wants no colour - no ``screen``, no pooled RGB - runs an
    instantiation of the kernel without the shading pass: ``fields=('distances',)`` is what ``modules.Depth`` reads,
    reference modules.py:170-184), and ``pooled=dict(subsample=s, max_depth=d, rgb=True, depth=True)``
    has the kernel write the mean-pooled observations of ``modules.RGB`` / ``modules.Depth`` itself
    (``Render.obs_rgb`` (n, a, 3, res/s), ``Render.obs_depth`` (n, a, res/s)). ``out`` takes the :class:`Render` of an
    earlier call with the same arguments and writes into its tensors instead of allocating (the reference allocates
    five tensors per call, kernels.cu:461-469; a caller that consumes a frame before asking for the next need not).
    ``pooled['centre']=True`` adds ``Render.obs_centre`` (n, a, 2) int32: the agent each of the two central observation
    pixels shows, or -1 (all that Deathmatch reads from ``indices``). ``seen=(stamp, epoch, count)`` - int32 tensors
    with one entry per texel, per env and per env - has the kernel do Explorer's first-sight bookkeeping: texels under
    this frame's rays get their env's epoch as stamp, those that did not carry it yet are added to ``count``.
    ``telemetry=True`` (tests) takes the self-contained path whose scratch counters end up in ``Render._telemetry``.

    The contract the wall grid adds: hit indices come from the per-cell lists :func:`bake` made of the
    static walls, so walls must not be moved in place afterwards without baking again - ``Scenery.check_wall_grid()`` /
    ``MEGASTEP_CHECK_GRID=1`` detect it (the reference reads ``lines`` afresh every call and has no such rule)."""
    dev, cfg, result = _render_call(scenery, agents, fields, pooled, out, seen, config)
    with _on(dev):
        if telemetry:
            _lib.lib().ms_debug_pair_telemetry(1)               # the kernels' pair counters too (tools/pair_stats.py)
        try:
            _lib.check(_lib.lib().ms_render(C.byref(scenery._as_struct()), C.byref(_ms_agents(agents, step=False, telemetry=telemetry)),
                                            C.byref(result._struct), C.byref(cfg), _stream(dev)))
        finally:
            if telemetry:
                _lib.lib().ms_debug_pair_telemetry(0)
    return result


def _render_call(scenery, agents, fields, pooled, out, seen, config):
    """What :func:`render` and :func:`step_render` check and prepare alike: the device, the shapes, the config, the first-sight
    books and the :class:`Render` to write into (``out``, or fresh buffers). Returns ``(device, config, Render)``."""
    dev = scenery._device()
    _agents_on(agents, dev)
    n, a = agents.angles.shape
    if (n, a) != (len(scenery.lines), scenery.n_agents):
        raise RuntimeError('agents do not match the scenery')
    cfg = _cfg(agents, config)            # (``config=``: see physics)
    seen_ptrs = None
    if seen is not None:
        stamp, epoch, count = seen
        if any(t.dtype != torch.int32 or not t.is_contiguous() for t in seen) or stamp.shape != (scenery.textures.vals.shape[0],) \
                or epoch.shape != (n,) or count.shape != (n,):
            raise RuntimeError('seen must be contiguous int32 tensors (stamp per texel, epoch per env, count per env)')
        _require_gpu(*seen)
        if a > 1 and scenery._as_struct().lg_vals is None:
            raise RuntimeError('first-sight bookkeeping (seen=) rides in the one-kernel renderer, which needs the light grid that this '
                               'multi-agent scenery was built without (Scenery.LIGHT_GRID = False)')
        seen_ptrs = tuple(t.data_ptr() for t in seen)
    # (what an `out` must have been made for: put together only when one is handed over, or asked of a result later)
    spec = (n, a, cfg.res, fields, pooled, dev, seen_ptrs)
    if out is not None:
        made_for = getattr(out, '_key', None)
        if made_for is None:
            made_for = out._key = _render_key(getattr(out, '_spec', None))   # (once per result)
        if made_for != _render_key(spec):
            raise RuntimeError('`out` must come from a render call with the same shapes, fields and pooling')
        result = out
    else:
        result = _render_buffers(scenery, n, a, cfg.res, fields, pooled, dev)
        result._spec = spec
        if seen is not None:
            result._struct.seen_stamp, result._struct.seen_epoch, result._struct.seen_count = seen_ptrs
    _ab_switches()
    _check_grid(scenery, dev)
    return dev, cfg, result


_layouts = {}
def _render_key(spec):
    """A render call's shapes, fields, pooling and books as a comparable value (see ``out=``)."""
    if spec is None:
        return None
    n, a, res, fields, pooled, dev, seen_ptrs = spec
    return (n, a, res, None if fields is None else tuple(fields), None if pooled is None else tuple(sorted(pooled.items())), dev, seen_ptrs)


def _render_buffers(scenery, n, a, r, fields, pooled, dev):
    """One allocation for the wanted outputs (reference: five at::empty calls, kernels.cu:461-469), the pooled
    observations and the kernels' scratch (MS_RENDER_WORKSPACE_INTS), and the MsRender that points into it."""
    scenery._as_struct()
    lit = a == 1 or scenery._lg is not None
    key = (n, a, r, None if fields is None else tuple(fields), None if pooled is None else tuple(sorted(pooled.items())), lit)
    layout = _layouts.get(key)
    if layout is None:
        layout = _layouts[key] = _render_layout(n, a, r, fields, pooled, lit)
        if len(_layouts) > 64:
            _layouts.pop(next(iter(_layouts)))
    total, offs, sizes, shapes, sub, max_depth, has_pool = layout
    buf = torch.empty(total, dtype=torch.float32, device=dev)
    base = buf.data_ptr()
    pieces = [buf[offs[i]:offs[i] + shapes[i][1]].view(shapes[i][0]) if sizes[i] else None for i in range(8)]
    if pieces[0] is not None:
        pieces[0] = pieces[0].view(torch.int32)
    if pieces[7] is not None:
        pieces[7] = pieces[7].view(torch.int32)
    result = Render(*pieces[:5], pieces[5], pieces[6], sub if has_pool else None, pieces[7])
    ptrs = [base + 4*offs[i] if sizes[i] else None for i in range(8)]
    result._struct = _lib.MsRender(*ptrs[:5], base + 4*offs[-1], ptrs[5], ptrs[6], sub, max_depth, ptrs[7])
    result._telemetry = buf[offs[-1]:offs[-1] + 16].view(torch.int32)     # see render_prep_kernel (which zeroes it); read by the tests
    return result


def _render_layout(n, a, r, fields, pooled, lit):
    """Where everything sits in a render call's one allocation - worked out once per (shapes, fields, pooling) and kept: it is
    a fifth of the host's share of a render call."""
    want = FIELDS if fields is None else tuple(fields)
    if any(f not in FIELDS for f in want):
        raise RuntimeError(f'fields must be among {FIELDS}')
    colour = 'screen' in want or (pooled is not None and pooled.get('rgb', True))
    if not lit and colour:
        # no light grid (Scenery.LIGHT_GRID switched off): agent hits are lit by a second launch that reads all five
        # planes back and patches `screen` - after any pooling. All planes then, and the caller pools.  (Without colour
        # there is nothing to light: the depth-only kernel serves such sceneries like any other.)
        want, pooled = FIELDS, None
    sub, max_depth, w = 1, 1., r
    n_rgb = n_depth = n_centre = 0
    if pooled is not None:
        sub, max_depth = int(pooled.get('subsample', 1)), float(pooled.get('max_depth', 10.))
        if sub < 1 or sub & (sub - 1) or 64 % sub or r % sub:
            raise RuntimeError('pooled subsample must be a power of two dividing 64 and the resolution')
        w = r//sub
        n_rgb = 3*n*a*w if pooled.get('rgb', True) else 0
        n_depth = n*a*w if pooled.get('depth', True) else 0
        n_centre = 2*n*a if pooled.get('centre', False) else 0
    plane = n*a*r
    sizes = [plane*(3 if f == 'screen' else 1) if f in want else 0 for f in FIELDS] + [n_rgb, n_depth, n_centre]
    sizes = [(x + 3) & ~3 for x in sizes]                                # keep every piece 16-byte aligned
    offs = [0]
    for x in sizes:
        offs.append(offs[-1] + x)
    total = offs[-1] + 18 + n*a*((r + 63)//64) + 2*n*a
    shapes = [((n, a, r, 3) if f == 'screen' else (n, a, r)) for f in FIELDS] + [(n, a, 3, w), (n, a, w), (n, a, 2)]
    shapes = [(sh, int(torch.Size(sh).numel())) for sh in shapes]
    return total, offs, sizes, shapes, sub, max_depth, pooled is not None


# ---------------------------------------------------------------------------------------------------------------------
# ray queries                                                  no counterpart in the reference (its rays: kernels.cu:326-382)
# ---------------------------------------------------------------------------------------------------------------------
RAYCAST_FIELDS = ('indices', 'locations', 'dots', 'distances', 'agents')


class Raycast:
    """Result of :func:`raycast`: (N, R) planes - ``indices`` (int32, env-local line, -1 on a miss), ``locations``,
    ``dots`` (NaN on a miss), ``distances`` (+inf on a miss) and ``agents`` (int32, the agent whose body the ray hit, else
    -1). Fields that were not asked for are ``None``."""

    def __init__(self, indices, locations, dots, distances, agents):
        self._t = (indices, locations, dots, distances, agents)

    indices = property(lambda self: self._t[0])
    locations = property(lambda self: self._t[1])
    dots = property(lambda self: self._t[2])
    distances = property(lambda self: self._t[3])
    agents = property(lambda self: self._t[4])


def raycast(scenery, origins, directions, agents=None, near=None, fields=None, out=None, config=None, grid_rays=None):
    """Casts R rays per env from ``origins`` along ``directions`` (both (N, R, 2) float32; a direction need not have unit
    length) by the render's per-ray rule (reference: kernels.cu:349-382) and returns :class:`Raycast`. With ``agents`` the
    rays meet the static walls and every agent's body at its current pose (drawn in registers: ``scenery.lines`` is not
    written); without, the static walls alone. ``near``: hits nearer than ``near`` (along the ray, in metres) are ignored -
    default the config's ``agent_radius``, which is what keeps an agent's own rays off its body. ``fields`` names the wanted
    outputs (default all of ``RAYCAST_FIELDS``); ``out`` takes the :class:`Raycast` of an earlier call with the same shapes and
    fields to write into. ``config``: see :func:`physics` (only needed for the default ``near``). ``grid_rays``: an optional
    one-element int32 tensor the kernel adds the number of rays that took the wall grid to (tests).

    No host synchronisation: the call can be captured in a HIP graph and sits safely between :func:`physics` and
    :func:`render`. The wall grid serves where it is exact and every line where not; the bits are the same."""
    _check(origins, 'origins', torch.float32, 3)
    _check(directions, 'directions', torch.float32, 3)
    n, r = origins.shape[:2]
    if origins.shape[2] != 2 or directions.shape != origins.shape:
        raise RuntimeError(f'origins and directions must both be (N, R, 2); got {tuple(origins.shape)} and {tuple(directions.shape)}')
    if n != len(scenery.lines) or r < 1:
        raise RuntimeError(f'origins must be (n_envs, R, 2) with n_envs = {len(scenery.lines)} and R >= 1; got {tuple(origins.shape)}')
    if agents is not None and tuple(agents.angles.shape) != (n, scenery.n_agents):
        raise RuntimeError('agents do not match the scenery')
    want = RAYCAST_FIELDS if fields is None else tuple(fields)
    if any(f not in RAYCAST_FIELDS for f in want):
        raise RuntimeError(f'fields must be among {RAYCAST_FIELDS}')
    dev = _require_gpu(origins, directions)
    if scenery._device() != dev:
        raise RuntimeError(f'all tensors must live on one device; got {scenery._device()} and {dev}')
    if agents is not None:
        _agents_on(agents, dev)
    if near is None:
        near = _cfg(agents, config).agent_radius
    if not near >= 0:
        raise RuntimeError('near must be a non-negative number')
    if grid_rays is not None:
        _check(grid_rays, 'grid_rays', torch.int32, 1)
        _require_gpu(grid_rays)
    key = (n, r, want, dev)
    if out is not None:
        if getattr(out, '_key', None) != key:
            raise RuntimeError('`out` must come from a raycast call with the same shapes and fields')
        result = out
    else:
        planes = [torch.empty((n, r), dtype=torch.int32 if f in ('indices', 'agents') else torch.float32, device=dev)
                  if f in want else None for f in RAYCAST_FIELDS]
        result = Raycast(*planes)
        result._key = key
    ptrs = [t.data_ptr() if t is not None else None for t in result._t]
    query = _lib.MsRaycast(r, origins.data_ptr(), directions.data_ptr(), float(near), *ptrs,
                           grid_rays.data_ptr() if grid_rays is not None else None)
    _check_grid(scenery, dev)
    with _on(dev):
        _lib.check(_lib.lib().ms_raycast(C.byref(scenery._as_struct()), C.byref(agents._plain) if agents is not None else None,
                                         C.byref(query), None, _stream(dev)))
    return result


def camera_rays(agents, config=None):
    """The direction vector of every ray :func:`render` casts, (N, A, res, 2) float32 - by the render's own device code (ray_y,
    reference kernels.cu:234-236,334-337). ``raycast(scenery, positions broadcast over the rays, camera_rays(agents),
    agents=agents)`` then gives the render's ``indices``, ``locations``, ``dots`` and ``distances`` bit for bit.
    ``config``: see :func:`physics` (``res`` and ``fov`` are read)."""
    dev = agents._dev
    if dev is None or dev.type != 'cuda':
        raise RuntimeError('megastep_amd kernels need GPU (HIP) tensors; the agents are on ' + str(dev or 'several devices'))
    cfg = _cfg(agents, config)
    n, a = agents.angles.shape
    dirs = torch.empty((n, a, cfg.res, 2), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.check(_lib.lib().ms_camera_rays(C.byref(agents._plain), n, a, C.byref(cfg), C.c_void_p(dirs.data_ptr()), _stream(dev)))
    return dirs


def line_of_sight(scenery, agents, a, b, near=None, config=None):
    """(N,) bool: in every env, whether agent ``a`` sees agent ``b`` - the ray from ``a``'s position towards ``b``'s either
    first hits ``b``'s body or meets nothing nearer than ``b``'s position. One :func:`raycast` of one ray per env (with the
    agents' bodies; ``near`` as there). ``a`` and ``b`` are agent numbers, or (N,) int64 tensors of them."""
    n = agents.angles.shape[0]
    rows = torch.arange(n, device=agents.positions.device)
    pa, pb = agents.positions[rows, a], agents.positions[rows, b]
    hit = raycast(scenery, pa[:, None].contiguous(), (pb - pa)[:, None].contiguous(), agents=agents, near=near,
                  fields=('distances', 'agents'), config=config)
    d = pb - pa
    span = torch.sqrt(d[:, 0]*d[:, 0] + d[:, 1]*d[:, 1])             # |b - a|: the ray's direction vector's length, as the kernel has it
    target = b if isinstance(b, int) else b.to(torch.int32)
    return (hit.agents[:, 0] == target) | (hit.distances[:, 0] >= span)


# ---------------------------------------------------------------------------------------------------------------------
# top-down pictures                                     reference: plotting.py (matplotlib, one env at a time on the host)
# ---------------------------------------------------------------------------------------------------------------------
OVERHEAD_FIELDS = ('rgb', 'indices')
#: the reference's background (plotting.adjust_view: '#c6c1b3'), decoded to linear RGB
OVERHEAD_BACKGROUND = tuple(float((c/255)**2.2) for c in (0xc6, 0xc1, 0xb3))


class Overhead:
    """Result of :func:`overhead`: ``rgb`` (K, V, 3, H, W) float32 linear RGB, planar (``spaces.MultiImage``'s layout), and
    ``indices`` (K, V, H, W) int32, the env-local line each pixel shows or -1 (an agent's lines are the first ``A*M``:
    ``index // M`` is the agent). Fields that were not asked for are ``None``."""

    def __init__(self, rgb, indices):
        self._t = (rgb, indices)

    rgb = property(lambda self: self._t[0])
    indices = property(lambda self: self._t[1])


def _hw(size):
    h, w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if h < 1 or w < 1:
        raise RuntimeError(f'size must be positive; got {size}')
    return h, w


def overhead(scenery, views, size, agents=None, envs=None, half_width=.05, lit=True, background=OVERHEAD_BACKGROUND,
             fields=None, out=None):
    """Draws the envs from above into tensors, every image in one launch. Image k shows env ``envs[k]`` (default: env k,
    one image per env) through each of its views: ``views`` is (K, V, 6) float32, an affine map per view from pixel
    coordinates (column + .5, row + .5; row 0 at the top) to world metres, ``x = g0 u + g1 w + g2``, ``y = g3 u + g4 w + g5``
    (:func:`plan_views`, :func:`agent_views`). ``size``: an int or (H, W). A pixel shows the nearest line within
    ``half_width`` metres of its centre - its texel, times its baked light for a wall when ``lit`` - or ``background``
    (linear RGB). With ``agents`` the agents are drawn at their current poses (in registers: ``scenery.lines`` is not
    written); without, their lines are taken as the scenery holds them - where the last :func:`render` drew them, which is
    what the reference's ``scene.display`` shows. An env id out of range gives an image of ``background`` and -1.

    ``fields``: the wanted outputs among ``OVERHEAD_FIELDS`` (default both); ``out``: the :class:`Overhead` of an earlier call
    with the same shapes and fields to write into. No host synchronisation: the call can be captured in a HIP graph. The
    per-pixel rule is written out in include/megastep_hip.h (``MsOverhead``) and DESIGN.md 3.13."""
    _check(views, 'views', torch.float32, 3)
    h, w = _hw(size)
    k, v = views.shape[:2]
    if views.shape[2] != 6 or k < 1 or v < 1:
        raise RuntimeError(f'views must be (K, V, 6) with K, V >= 1; got {tuple(views.shape)}')
    if envs is None:
        if k != len(scenery.lines):
            raise RuntimeError(f'without envs, views must have one row per env ({len(scenery.lines)}); got {tuple(views.shape)}')
    else:
        if not isinstance(envs, torch.Tensor) or envs.dtype.is_floating_point or envs.dtype == torch.bool:
            raise RuntimeError('envs must be an integer tensor')
        if envs.shape != (k,):
            raise RuntimeError(f'envs must be (K,) = ({k},); got {tuple(envs.shape)}')
    if agents is not None and tuple(agents.angles.shape) != (len(scenery.lines), scenery.n_agents):
        raise RuntimeError('agents do not match the scenery')
    want = OVERHEAD_FIELDS if fields is None else tuple(fields)
    if not want or any(f not in OVERHEAD_FIELDS for f in want):
        raise RuntimeError(f'fields must be a non-empty selection of {OVERHEAD_FIELDS}')
    if not 0 <= half_width < float('inf'):
        raise RuntimeError('half_width must be a non-negative number')
    if len(background) != 3:
        raise RuntimeError('background must be three linear RGB values')
    dev = _require_gpu(views, *([envs] if envs is not None else []))
    if scenery._device() != dev:
        raise RuntimeError(f'all tensors must live on one device; got {scenery._device()} and {dev}')
    if agents is not None:
        _agents_on(agents, dev)
    if envs is not None and envs.dtype != torch.int32:
        envs = envs.to(torch.int32)
    envs = envs.contiguous() if envs is not None else None
    key = (k, v, h, w, want, dev)
    if out is not None:
        if getattr(out, '_key', None) != key:
            raise RuntimeError('`out` must come from an overhead call with the same shapes and fields')
        result = out
    else:
        result = Overhead(torch.empty((k, v, 3, h, w), dtype=torch.float32, device=dev) if 'rgb' in want else None,
                          torch.empty((k, v, h, w), dtype=torch.int32, device=dev) if 'indices' in want else None)
        result._key = key
    rgb, idx = result._t
    spec = _lib.MsOverhead(k, v, h, w, envs.data_ptr() if envs is not None else None, views.data_ptr(), float(half_width),
                           1 if lit else 0, (C.c_float*3)(*map(float, background)), rgb.data_ptr() if rgb is not None else None,
                           idx.data_ptr() if idx is not None else None)
    with _on(dev):
        _lib.check(_lib.lib().ms_overhead(C.byref(scenery._as_struct()), C.byref(agents._plain) if agents is not None else None,
                                          C.byref(spec), _stream(dev)))
    return result


def _view_rows(cx, cy, ex, ey, sx, sy, h, w):
    """(..., 6) views: pixel (u, w) -> centre + (u - W/2) * ex*s + (w - H/2) * ey*s, for unit axes ex (right) and ey (down)
    in world coordinates, s = (sx, sy) the metres per pixel."""
    return torch.stack([ex[0]*sx, ey[0]*sy, cx - ex[0]*sx*(w/2) - ey[0]*sy*(h/2),
                        ex[1]*sx, ey[1]*sy, cy - ex[1]*sx*(w/2) - ey[1]*sy*(h/2)], -1)


def plan_views(scenery, size, envs=None, margin=1.):
    """(K, 1, 6) views for :func:`overhead` of whole floorplans, north up: the square the reference's
    ``plotting.extent(zoom=False)`` frames - the env's static lines' bounding box grown by ``margin`` metres on every side,
    squared about its centre - fitted into an image of ``size`` (an int or (H, W)). ``envs``: which envs (default all).
    Worked out with tensor ops on the lines' device, without a host synchronisation."""
    h, w = _hw(size)
    lines = scenery.lines
    vals, widths, starts, inverse = lines.vals, lines.widths.long(), lines.starts.long(), lines.inverse.long()
    n = len(widths)
    af = scenery.n_agents*scenery.model.shape[0]
    static = (torch.arange(vals.shape[0], device=vals.device) - starts[inverse]) >= af
    pts = vals.reshape(-1, 4)
    inf = torch.full((n, 2), float('inf'), dtype=torch.float32, device=vals.device)
    lo_pts = torch.where(static[:, None], torch.minimum(pts[:, :2], pts[:, 2:]), torch.full_like(pts[:, :2], float('inf')))
    hi_pts = torch.where(static[:, None], torch.maximum(pts[:, :2], pts[:, 2:]), torch.full_like(pts[:, :2], -float('inf')))
    index = inverse[:, None].expand(-1, 2)
    lo = inf.scatter_reduce(0, index, lo_pts, 'amin')
    hi = (-inf).scatter_reduce(0, index, hi_pts, 'amax')
    empty = ~torch.isfinite(lo).all(1)                                   # (an env without walls: a 2 margin square about 0)
    lo = torch.where(empty[:, None], torch.zeros_like(lo), lo) - margin
    hi = torch.where(empty[:, None], torch.zeros_like(hi), hi) + margin
    if envs is not None:
        envs = torch.as_tensor(envs, device=vals.device).long()
        lo, hi = lo[envs], hi[envs]
    centre = (lo + hi)/2
    half = torch.maximum(hi[:, 0] - lo[:, 0], hi[:, 1] - lo[:, 1])/2
    s = 2*half/min(h, w)
    one, zero = torch.ones_like(s), torch.zeros_like(s)
    rows = _view_rows(centre[:, 0], centre[:, 1], (one, zero), (zero, -one), s, s, h, w)
    return rows[:, None].float().contiguous()


def agent_views(agents, size, radius):
    """(N, A, 6) views for :func:`overhead` around every agent: the agent at the image's centre, its heading pointing up,
    the image ``2*radius`` metres across (along its shorter side; ``size`` an int or (H, W)). The egocentric local map."""
    h, w = _hw(size)
    a = agents.angles*(math.pi/180)
    fx, fy = torch.cos(a), torch.sin(a)                                  # forward: up the image
    s = torch.full_like(fx, 2*float(radius)/min(h, w))
    p = agents.positions
    rows = _view_rows(p[..., 0], p[..., 1], (fy, -fx), (-fx, -fy), s, s, h, w)    # right of the heading, and down = backward
    return rows.float().contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# shortest-path distance fields                                                no counterpart in the reference
# ---------------------------------------------------------------------------------------------------------------------
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
        self._struct = _lib.MsNavGrid(len(host_geom), self.cell, self.clearance, geom.data_ptr(), starts.data_ptr(), self._max_framed,
                                      free.data_ptr())

    n_envs = property(lambda self: len(self._host_geom))
    #: cells of all envs together
    n_cells = property(lambda self: int(self._host_starts[-1]))

    def cells(self, e):
        """(first cell, ny, nx) of env ``e`` (host numbers: no synchronisation)."""
        return int(self._host_starts[e]), int(self._host_geom[e, 3]), int(self._host_geom[e, 2])

    def image(self, e):
        """(ny, nx) bool: env ``e``'s free cells, row 0 at the lowest y."""
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
    with _on(dev):
        _lib.check(_lib.lib().ms_nav_free(C.byref(scenery._as_struct()), C.byref(grid._struct), _stream(dev)))
    return grid


class DistanceFields:
    """Result of :func:`distance_fields`: for each env ``G`` fields, field (n, g) holding for every cell of env n's grid the
    length of the shortest 8-connected path from the cell's centre to ``goals[n, g]`` (+inf on blocked cells and on cells no
    path reaches). ``values`` is the flat float32 store: field (n, g) starts at ``G*grid.starts[n] + g*nx*ny``."""

    def __init__(self, grid, goals, values, passes=None):
        self.grid, self.goals, self.values, self.passes = grid, goals, values, passes

    n_goals = property(lambda self: self.goals.shape[1])

    def image(self, e, g=0):
        """(ny, nx) float32 view of field ``g`` of env ``e``, row 0 at the lowest y."""
        s, ny, nx = self.grid.cells(e)
        at = self.n_goals*s + g*ny*nx
        return self.values[at:at + ny*nx].reshape(ny, nx)

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

    def at(self, points, goal=None, out=None):
        """(N, P) float32: the distance from each of ``points`` (N, P, 2) to a goal of its env - ``goal`` (N, P) integers name
        the field each point asks, default point k against field k (then P must be G). The distance is the least, over the
        (at most four) free cells round the point, of the cell's value plus the straight leg to its centre: continuous
        enough that an agent's progress per step is not quantised to cells. +inf where no path exists. Meant for points
        that are themselves ``clearance`` clear of the walls (an agent's centre, a spawn point): the leg of any other point
        may cross a wall. One launch, no host synchronisation."""
        grid = self.grid
        _check(points, 'points', torch.float32, 3)
        n, p = points.shape[:2]
        if n != grid.n_envs or points.shape[2] != 2 or p < 1:
            raise RuntimeError(f'points must be (N, P, 2) with N = {grid.n_envs}; got {tuple(points.shape)}')
        if goal is None:
            if p != self.n_goals:
                raise RuntimeError(f'without goal, points must be one per field ({self.n_goals}); got {p}')
        else:
            if not isinstance(goal, torch.Tensor) or goal.dtype.is_floating_point or goal.shape != (n, p):
                raise RuntimeError(f'goal must be an (N, P) = ({n}, {p}) integer tensor')
            goal = goal.to(torch.int32).contiguous()
        dev = _require_gpu(points, self.values, *([goal] if goal is not None else []))
        if out is None:
            out = torch.empty((n, p), dtype=torch.float32, device=dev)
        elif out.shape != (n, p) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
            raise RuntimeError('`out` must be a contiguous (N, P) float32 tensor on the fields\' device')
        spec = _lib.MsNavQuery(p, points.data_ptr(), goal.data_ptr() if goal is not None else None, self.values.data_ptr(),
                               self.n_goals, out.data_ptr())
        with _on(dev):
            _lib.check(_lib.lib().ms_nav_query(C.byref(grid._struct), C.byref(spec), _stream(dev)))
        return out

    def _queries(self, points, goal):
        """:meth:`at`'s argument rules, for the calls that follow the fields: (n, p, goal as int32 or None, device)."""
        grid = self.grid
        _check(points, 'points', torch.float32, 3)
        n, p = points.shape[:2]
        if n != grid.n_envs or points.shape[2] != 2 or p < 1:
            raise RuntimeError(f'points must be (N, P, 2) with N = {grid.n_envs}; got {tuple(points.shape)}')
        if goal is None:
            if p != self.n_goals:
                raise RuntimeError(f'without goal, points must be one per field ({self.n_goals}); got {p}')
        else:
            if not isinstance(goal, torch.Tensor) or goal.dtype.is_floating_point or goal.shape != (n, p):
                raise RuntimeError(f'goal must be an (N, P) = ({n}, {p}) integer tensor')
            goal = goal.to(torch.int32).contiguous()
        dev = _require_gpu(points, self.values, self.goals, grid.free, *([goal] if goal is not None else []))
        return n, p, goal, dev

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
        if out is None:
            out = torch.empty((n, p, 2), dtype=torch.float32, device=dev)
        elif not isinstance(out, torch.Tensor) or out.shape != (n, p, 2) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
            raise RuntimeError('`out` must be a contiguous (N, P, 2) float32 tensor on the fields\' device')
        chosen = torch.empty((n, p), dtype=torch.int32, device=dev) if hops else None
        spec = _lib.MsNavWaypoints(p, points.data_ptr(), goal.data_ptr() if goal is not None else None, self.values.data_ptr(),
                                   self.goals.data_ptr(), self.n_goals, lookahead, out.data_ptr(), chosen.data_ptr() if hops else None)
        with _on(dev):
            _lib.check(_lib.lib().ms_nav_waypoints(C.byref(self.grid._struct), C.byref(spec), _stream(dev)))
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
        spec = _lib.MsNavPaths(p, points.data_ptr(), goal.data_ptr() if goal is not None else None, self.values.data_ptr(),
                               self.goals.data_ptr(), self.n_goals, max_points, pts.data_ptr(), counts.data_ptr())
        with _on(dev):
            _lib.check(_lib.lib().ms_nav_paths(C.byref(self.grid._struct), C.byref(spec), _stream(dev)))
        return Paths(pts, counts)


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


def _nav_fields_call(fields, mask):
    grid = fields.grid
    n, g = fields.goals.shape[:2]
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.shape != (n, g):
            raise RuntimeError(f'mask must be an (N, G) = ({n}, {g}) bool tensor')
        mask = mask.contiguous()
    dev = _require_gpu(fields.goals, fields.values, grid.free, *([mask] if mask is not None else []))
    spec = _lib.MsNavFields(g, fields.goals.data_ptr(), mask.data_ptr() if mask is not None else None, fields.values.data_ptr(),
                            fields.passes.data_ptr() if fields.passes is not None else None)
    with _on(dev):
        _lib.check(_lib.lib().ms_nav_fields(C.byref(grid._struct), C.byref(spec), _stream(dev)))


def distance_fields(grid, goals, mask=None, out=None, passes=False):
    """Shortest-path distance fields on the :func:`nav_grid`: for every env and each of its ``G`` goals (``goals``: (N, G, 2)
    float32 world points) the distance from every free cell to the goal along the grid's 8-connected graph - straight steps
    of ``cell``, diagonal steps of ``cell*1.41421356`` that cut no corner - joined to the goal by the straight legs from the
    free cells round it. The 8-connected metric is up to 8 % longer than the true (any-angle) shortest path in open space;
    an agent that heads for :meth:`DistanceFields.waypoints` cuts the staircase short and walks less than the field says.
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
