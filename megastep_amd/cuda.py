"""The ``megastep.cuda`` operator surface on MI355X.

Mirrors the reference's pybind module ``megastepcuda`` (reference: megastep/src/wrappers.cpp:30-173) name for name -
``initialize, bake, physics, render, Ragged1D/2D/3D, Agents, Scenery, Render, Physics`` - but every compute entry
point is a hand-written gfx950 kernel reached through the C-ABI in ``include/megastep_hip.h``. Tensors stay torch-owned
(PyTorch-ROCm is the allocator/stream plumbing); the kernels run on ``torch.cuda.current_stream()``.

The calls without a counterpart in the reference live in modules named after the kernel files they drive - ``rays``,
``rollouts``, ``scenarios``, ``overhead``, ``nav`` and ``envlogic`` - and are imported at the end of this one, so each is still ``cuda.<name>``.

There is no CPU implementation here, exactly as in the reference ("If you haven't got CUDA, megastep will not work",
reference: docs/faq.rst:23-26): calling bake/physics/render on non-GPU tensors raises.
"""
import ctypes as C
import numbers
import os
import torch
from . import _call, _lib, grids
from ._lib import _on, _stream
from ._call import _agents_on, _cfg, _check, _require_gpu, config

# ---------------------------------------------------------------------------------------------------------------------
# initialize                                                                   reference: kernels.cu:18-27
# ---------------------------------------------------------------------------------------------------------------------
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


def initialize(agent_radius, res, fov, fps):
    """Sets the constants used by :func:`physics` and :func:`render` for callers that hand them bare tensors' holders
    (reference: wrappers.cpp:53) - the drop-in path. As in the reference this is process-global; unlike it, nothing
    device-side is mutated (the values travel by value with every launch), and it is only the FALLBACK: a call that is
    given ``config=``, or whose ``agents`` carry one (every ``Core``'s do), never looks at it."""
    _call._config = config(agent_radius, res, fov, fps)
    _ab_switches()


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
        self._bake_marks = self._bake_s = None        # the last bake()'s events, and the seconds read off them (grid_report())
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
        marks = self._bake_marks
        if self._bake_s is None and marks is not None and marks[0] is not None:
            ev, wall_grid = marks
            ev[2].synchronize()
            self._bake_s = dict(lighting=ev[0].elapsed_time(ev[1])*1e-3, wall_grid=ev[1].elapsed_time(ev[2])*1e-3 if wall_grid else 0.)
        return dict(wall_grid=self._wg_report, light_grid=self._lg_report, bake_seconds=self._bake_s)

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

    def _check_grid(self, dev):
        """What every call that walks the wall grid asks first while ``CHECK_GRID`` is on (not inside a stream capture)."""
        if CHECK_GRID and self._wg is not None:
            with _on(dev):                                                    # (the stream that matters is `dev`'s current one)
                capturing = torch.cuda.is_current_stream_capturing()
            if not capturing:
                self.check_wall_grid()

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

    def __init__(self, progress, slid=None, stopped=None):
        self._progress = progress
        self._slid, self._stopped = slid, stopped

    progress = property(lambda self: self._progress)
    #: of a sliding step (``slide=``), else None: (N, A) float32, the share of the step each agent spent sliding along what blocked it
    slid = property(lambda self: self._slid)
    #: of a sliding step, else None: (N, A) uint8, 1 where the step's collisions zeroed the agent's velocity - a dead stop
    stopped = property(lambda self: self._stopped)


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
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
    cfg = C.byref(_call._config) if _call._config is not None else None
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


def _slide_options(slide, agents, out):
    """``physics``' ``slide`` argument (see there) as ``(MsSlide by reference, slid, stopped)``, or ``(None, None, None)``. The two
    outputs are the ones of ``out``, an earlier sliding call's Physics, else fresh."""
    bounce = _bounce(slide)
    if bounce is None:
        return None, None, None
    if out is not None and (out.slid is None or out.stopped is None):
        raise RuntimeError('out must be the Physics of an earlier sliding step')
    slid = torch.empty_like(agents.angles) if out is None else out.slid
    stopped = torch.empty(agents.angles.shape, dtype=torch.uint8, device=agents.angles.device) if out is None else out.stopped
    return C.byref(_lib.MsSlide(bounce, slid.data_ptr(), stopped.data_ptr())), slid, stopped


def _step_launch(scenery, agents, mv, ex, sl, progress, cfg, dev):
    """The physics launch of :func:`physics` and of a two-launch :func:`step_render`: the sliding step where ``sl`` is given."""
    args = (C.byref(scenery._as_struct()), C.byref(_ms_agents(agents, step=True)), mv, ex)
    if sl is None:
        _lib.check(_lib.lib().ms_step_physics(*args, C.c_void_p(progress.data_ptr()), C.byref(cfg), _stream(dev)))
    else:
        _lib.check(_lib.lib().ms_slide_physics(*args, sl, C.c_void_p(progress.data_ptr()), C.byref(cfg), _stream(dev)))


def physics(scenery, agents, movement=None, out=None, respawn=None, lifespans=None, imu=None, config=None, slide=None):
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
    * ``imu=(out, ang_scale, speed_scale)``: the (N, A, 3) IMU observation of the state the step leaves behind;
    * ``slide=True`` or ``dict(bounce=.05)``: sliding contacts (include/megastep_hip.h, MsSlide). The reference's
      step stops an agent dead, velocity and spin, at whatever it touches; with ``slide`` a blocked agent spends the rest of the
      step along what blocked it, its velocity deflected off the contact normal with ``bounce`` of it turned outwards, in the
      same launch. ``progress`` stays the plain step's, bit for bit, and the result also has ``slid`` and ``stopped``
      (:class:`Physics`). At most 64 agents an env.

    ``out``: the :class:`Physics` of an earlier call, to write ``progress`` (and ``slid``, ``stopped``) into instead of allocating.
    ``config``: the constants of this call (:func:`config`); default: the ones ``agents`` carry (a Core's do), else initialize()'s."""
    dev = scenery._device()
    _agents_on(agents, dev)
    shape = (len(scenery.lines), scenery.n_agents)
    if agents.angles.shape != shape:
        raise RuntimeError('agents do not match the scenery: expected (n_envs, n_agents) = '
                           f'{shape}, got {tuple(agents.angles.shape)}')
    mv, ex = _step_options(agents, shape, movement, respawn, lifespans, imu)
    sl, slid, stopped = _slide_options(slide, agents, out)
    progress = _progress(agents, out)
    _ab_switches()
    scenery._check_grid(dev)
    with _on(dev):
        _step_launch(scenery, agents, mv, ex, sl, progress, _cfg(agents, config), dev)
    return _stepped(agents, progress, out, slid, stopped)


def _progress(agents, out):
    """The (N, A) tensor a step writes its progress to: the one of ``out``, an earlier call's Physics, else a fresh one."""
    return torch.empty_like(agents.angles) if out is None else out.progress


def _stepped(agents, progress, out, slid=None, stopped=None):
    """What a step leaves behind: the agents' heading cache filled (where they use it) and their epoch moved on; ``progress``
    (and a sliding step's ``slid`` and ``stopped``) as a :class:`Physics` - ``out`` if the step wrote into one."""
    agents._cached = agents._use_cache
    agents._epoch += 1
    return Physics(progress, slid, stopped) if out is None else out


FIELDS = ('indices', 'locations', 'dots', 'distances', 'screen')
#: MEGASTEP_CHECK_GRID=1: every render / physics call first makes sure the static walls are still the ones the wall grid
#: was built from (a reduction over the lines and a host sync per call - for debugging and the test suite, off by default)
CHECK_GRID = os.environ.get('MEGASTEP_CHECK_GRID', '0') not in ('', '0')


def step_render(scenery, agents, fields=None, pooled=None, out=None, seen=None, config=None, movement=None, respawn=None,
                lifespans=None, imu=None, slide=None):
    """One step of the hot path - :func:`physics` then :func:`render`, what every ``env.step()`` of the reference runs
    (wrappers.cpp:69 + :82) - as one call, and where the shapes allow it as ONE LAUNCH (include/megastep_hip.h,
    ``ms_step_render``): with one agent per env and at most 64 rays (BASELINE config 2, the Explorer shape) an agent is a single
    wavefront, which runs its env's physics step and renders from the pose it ends on. Any other shape is the two launches,
    as if the two calls had been made. Same bits either way (tests/test_gpu_step_render.py).

    Arguments as :func:`render`'s, and :func:`physics`' ``movement`` / ``respawn`` / ``lifespans`` / ``imu`` (a whole env.step() of a
    single-agent env of up to 64 rays - the reference's tutorial env - is then one launch); ``out``: the ``(Physics, Render)`` of an
    earlier call, to write into. Returns ``(Physics, Render)``.

    ``slide``: :func:`physics`' sliding contacts. A sliding step is always the two launches - the sliding physics launch, then the
    render - whatever the shape."""
    physics_out, render_out = out if out is not None else (None, None)
    dev, cfg, result = _render_call(scenery, agents, fields, pooled, render_out, seen, config)
    mv, ex = _step_options(agents, tuple(agents.angles.shape), movement, respawn, lifespans, imu)
    sl, slid, stopped = _slide_options(slide, agents, physics_out)
    progress = _progress(agents, physics_out)
    with _on(dev):
        if sl is None:
            _lib.check(_lib.lib().ms_move_step_render(C.byref(scenery._as_struct()), C.byref(_ms_agents(agents, step=True)), mv, ex,
                                                      C.c_void_p(progress.data_ptr()), C.byref(result._struct), C.byref(cfg), _stream(dev)))
        else:
            _step_launch(scenery, agents, mv, ex, sl, progress, cfg, dev)
            agents._cached = agents._use_cache                  # (the sliding launch has filled the heading cache the render reads)
            _lib.check(_lib.lib().ms_render(C.byref(scenery._as_struct()), C.byref(_ms_agents(agents, step=False)),
                                            C.byref(result._struct), C.byref(cfg), _stream(dev)))
    return _stepped(agents, progress, physics_out, slid, stopped), result


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
    result._scenery = scenery                                           # (overlay_items reads the envs' numbers of lines)
    _ab_switches()
    scenery._check_grid(dev)
    return dev, cfg, result


_layouts = {}
def _selection(fields, pooled):
    """A call's ``fields`` and ``pooled`` arguments as two hashable, comparable values."""
    return None if fields is None else tuple(fields), None if pooled is None else tuple(sorted(pooled.items()))


def _render_key(spec):
    """A render call's shapes, fields, pooling and books as a comparable value (see ``out=``)."""
    if spec is None:
        return None
    n, a, res, fields, pooled, dev, seen_ptrs = spec
    return (n, a, res, *_selection(fields, pooled), dev, seen_ptrs)


def _render_buffers(scenery, n, a, r, fields, pooled, dev):
    """One allocation for the wanted outputs (reference: five at::empty calls, kernels.cu:461-469), the pooled
    observations and the kernels' scratch (MS_RENDER_WORKSPACE_INTS), and the MsRender that points into it."""
    scenery._as_struct()
    lit = a == 1 or scenery._lg is not None
    key = (n, a, r, *_selection(fields, pooled), lit)
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
# the calls without a counterpart in the reference, from the modules that hold them
# ---------------------------------------------------------------------------------------------------------------------
from .envlogic import deathmatch_shoot, explorer_books
from .rays import RAYCAST_FIELDS, Raycast, raycast, camera_rays, line_of_sight
from .percepts import PERCEPT_FIELDS, PERCEPT_MAX_EYES, PERCEPT_MAX_POINTS, PERCEPT_MAX_NEAREST, Percepts, percepts
from .items import ITEM_MAX_ITEMS, ITEM_MAX_AGENTS, ITEM_MAX_KINDS, Items, Collected, items, collect_items, place_items, overlay_items
from .cameras import PROJECTIONS, LOOK_FIELDS, Cameras, Look, shade, cameras, mounted, look
from .rollouts import ROLLOUT_MAX_CANDIDATES, ROLLOUT_MAX_HORIZON, Rollouts, rollouts, plans, _bounce
from .scenarios import SCENARIO_MAX_SCENARIOS, SCENARIO_MAX_AGENTS, Scenarios, scenarios
from .overhead import OVERHEAD_FIELDS, OVERHEAD_BACKGROUND, Overhead, overhead, plan_views, agent_views
from .nav import nav_geometry, NavGrid, nav_grid, FIELD_CAPACITY, DistanceFields, Paths, PulledPaths, distance_fields, geodesic, SeenMaps, seen_maps, AGE_MAX_TICK, Sweep, AgeMaps, age_maps, SeededFields, seeded_fields, \
    COST_CAPACITY, COST_MAX, CostFields, cost_fields, inflation_costs, mark_costs, \
    CellLayer, cell_layer, MapChannel, map_channel, local_maps, CellDraws, cell_draws, REGION_CAPACITY, Regions, regions, \
    VIEW_WALL_CAPACITY, ViewFields, view_fields, BASIN_CAPACITY, BASIN_MAX_IDS, PointMarks, point_marks, Basins, basins, ZONE_MAX, Zones, zones, \
    CLEARANCE_MAX_RADII, ClearanceFields, clearance_fields, Clearance, clearance
