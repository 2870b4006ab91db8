"""Cameras that look from anywhere (kernels: ``csrc/kernels/shade.h``). :func:`~megastep_amd.cuda.render` draws colour from one
place only - an agent's own pose, through one plane-projected fan narrower than half a turn; here the two halves of a render
are calls of their own: :func:`~megastep_amd.cuda.raycast` casts rays from anywhere, :func:`shade` colours what they hit by the
render's own rule, and :func:`cameras` / :func:`mounted` / :func:`look` put them together - a rear view, a
360-degree panorama, two cameras on one agent, a fixed camera watching a doorway. No counterpart in the reference, whose
shader runs on its own render's rays alone (kernels.cu:407-450); reached as ``megastep_amd.cuda.<name>``."""
import ctypes as C
import math
import torch
from . import _lib, rays
from ._lib import _on, _stream
from ._call import _check, _query_device, _require_gpu, _result_for

PROJECTIONS = {'plane': 0, 'ring': 1}        # MS_CAMERA_PLANE, MS_CAMERA_RING
LOOK_FIELDS = ('screen',) + rays.RAYCAST_FIELDS


def _without_light_grid(scenery):
    """The scenery's struct with the light grid withheld (tests and A/B runs: the plain light path)."""
    plain = _lib.MsScenery.from_buffer_copy(scenery._as_struct())
    plain.lg_vals = plain.lg_list = plain.lg_pool = plain.lg_pool_rows = None
    return plain


def shade(scenery, hits, agents=None, out=None, light_grid=True):
    """The colour of rays that :func:`~megastep_amd.cuda.raycast` has cast: (N, R, 3) float32, by the render's shading rule -
    the 2-tap texel filter, baked light on walls, the lights themselves at the hit point on an agent's body. ``hits`` is a
    :class:`~megastep_amd.cuda.Raycast` holding ``indices``, ``locations`` and ``dots``. With ``agents`` the rays that landed on
    a body are lit at the pose the body has now (drawn in registers: ``scenery.lines`` is not written); without, they are
    black - as are misses. ``out``: the tensor an earlier call with the same shapes returned, to write into.
    ``light_grid=False`` withholds the scenery's light grid from the call (the same bits, by the plain path).

    On the rays of :func:`~megastep_amd.cuda.camera_rays` cast from the agents' positions the result is
    :func:`~megastep_amd.cuda.render`'s ``screen`` bit for bit. No host synchronisation; captures in a HIP graph."""
    planes = (getattr(hits, 'indices', None), getattr(hits, 'locations', None), getattr(hits, 'dots', None))
    if any(p is None for p in planes):
        raise RuntimeError('hits must hold indices, locations and dots (raycast(..., fields=) with all three)')
    idx = _check(planes[0], 'indices', torch.int32, 2)
    loc = _check(planes[1], 'locations', torch.float32, 2)
    dots = _check(planes[2], 'dots', torch.float32, 2)
    n, r = idx.shape
    if loc.shape != idx.shape or dots.shape != idx.shape:
        raise RuntimeError('indices, locations and dots must share one (N, R) shape')
    if n != len(scenery.lines) or r < 1:
        raise RuntimeError(f'hits must be (n_envs, R) with n_envs = {len(scenery.lines)} and R >= 1; got {tuple(idx.shape)}')
    if agents is not None and tuple(agents.angles.shape) != (n, scenery.n_agents):
        raise RuntimeError('agents do not match the scenery')
    dev = _query_device(scenery, agents, idx, loc, dots)
    if out is not None:
        _check(out, 'out', torch.float32, 3)
        if tuple(out.shape) != (n, r, 3) or _require_gpu(out) != dev:
            raise RuntimeError(f'`out` must be the ({n}, {r}, 3) tensor of an earlier shade call')
    screen = out if out is not None else torch.empty((n, r, 3), dtype=torch.float32, device=dev)
    query = _lib.MsShade(r, idx.data_ptr(), loc.data_ptr(), dots.data_ptr(), screen.data_ptr())
    struct = scenery._as_struct() if light_grid else _without_light_grid(scenery)
    with _on(dev):
        _lib.check(_lib.lib().ms_shade(C.byref(struct), C.byref(agents._plain) if agents is not None else None, C.byref(query), None,
                                       _stream(dev)))
    return screen


class Cameras:
    """C cameras per env: ``poses`` (N, C, 3) - x, y, heading in degrees, kept by reference - and the rays they cast,
    ``origins`` and ``directions`` (N, C*res, 2), camera after camera, ray 0 of each leftmost. :meth:`update` forms the rays
    again, in place, from what ``poses`` holds now (cameras made by :func:`mounted` first take their poses from the agents)."""

    def __init__(self, poses, res, fov, projection):
        self.poses, self.res, self.fov, self.projection = poses, int(res), float(fov), projection
        n, c = poses.shape[:2]
        self.origins = torch.empty((n, c*self.res, 2), dtype=torch.float32, device=poses.device)
        self.directions = torch.empty_like(self.origins)
        self._query = _lib.MsCameraPoses(n, c, self.res, poses.data_ptr(), self.fov, PROJECTIONS[projection], self.origins.data_ptr(),
                                         self.directions.data_ptr())
        self._mount = None

    n_cameras = property(lambda self: self.poses.shape[1])

    def update(self):
        if self._mount is not None:
            self._mount()
        dev = self.poses.device
        with _on(dev):
            _lib.check(_lib.lib().ms_camera_pose_rays(C.byref(self._query), _stream(dev)))
        return self


def cameras(poses, res, fov, projection='plane'):
    """Cameras at ``poses`` (N, C, 3) float32 - x, y, heading in degrees - of ``res`` rays each: a :class:`Cameras` with its rays
    formed. ``projection='plane'``: the render's - columns of a screen plane, ``0 < fov < 180``, the rays
    :func:`~megastep_amd.cuda.camera_rays` gives for an agent of that heading, bit for bit. ``projection='ring'``: rays evenly
    spaced in angle, ``0 < fov <= 360`` - ray ``r`` points along ``heading + fov*(res - 2r - 1)/(2*res)`` degrees, unit vectors;
    360 is a panorama."""
    _check(poses, 'poses', torch.float32, 3)
    _require_gpu(poses)
    if poses.shape[2] != 3 or poses.shape[0] < 1 or poses.shape[1] < 1:
        raise RuntimeError(f'poses must be (N, C, 3) - x, y, heading in degrees; got {tuple(poses.shape)}')
    if projection not in PROJECTIONS:
        raise RuntimeError(f'projection must be one of {tuple(PROJECTIONS)}; got {projection!r}')
    if int(res) < 1:
        raise RuntimeError('res must be positive')
    if not (0 < fov < 180 if projection == 'plane' else 0 < fov <= 360):
        raise RuntimeError('fov must be in (0, 180) degrees for a plane and in (0, 360] for a ring')
    return Cameras(poses, res, fov, projection).update()


def mounted(agents, mounts, res, fov, projection='plane'):
    """Cameras on every agent: ``mounts`` (C, 3) gives each camera's place in the agent's frame - x and y offset in metres (x
    along the heading) - and its turn against the heading in degrees (positive: to the left). A :class:`Cameras` of ``A*C``
    cameras per env, agent after agent; :meth:`Cameras.update` takes the agents' poses as they are then. A mount of zeros
    leaves the agent's pose exactly: a plane camera there at the render's ``res`` and ``fov`` casts the render's rays."""
    mounts = torch.as_tensor(mounts, dtype=torch.float32, device=agents.angles.device)
    if mounts.ndim != 2 or mounts.shape[1] != 3 or mounts.shape[0] < 1:
        raise RuntimeError(f'mounts must be (C, 3) - x, y in the agent\'s frame, turn in degrees; got {tuple(mounts.shape)}')
    n, a = agents.angles.shape
    c = mounts.shape[0]
    poses = torch.zeros((n, a*c, 3), dtype=torch.float32, device=agents.angles.device)
    view = poses.view(n, a, c, 3)
    ox, oy, turn = (mounts[:, k].contiguous() for k in range(3))
    rad, sn, cs = (torch.empty((n, a, 1), dtype=torch.float32, device=poses.device) for _ in range(3))

    def mount():
        # (in place, so that a captured update replays on the same memory; x + (cos*0 - sin*0) and angle + 0 are x and angle)
        torch.mul(agents.angles.unsqueeze(-1), math.pi/180, out=rad)
        torch.sin(rad, out=sn)
        torch.cos(rad, out=cs)
        px, py, ph = view[..., 0], view[..., 1], view[..., 2]
        torch.mul(cs, ox, out=px)
        px.addcmul_(sn, oy, value=-1).add_(agents.positions[:, :, None, 0])
        torch.mul(sn, ox, out=py)
        py.addcmul_(cs, oy).add_(agents.positions[:, :, None, 1])
        torch.add(agents.angles.unsqueeze(-1), turn, out=ph)

    mount()
    cams = cameras(poses, res, fov, projection)
    cams._mount = mount
    return cams


class Look:
    """Result of :func:`look`: planes (N, C, res) - ``screen`` (N, C, res, 3) - named as :func:`~megastep_amd.cuda.render`'s and
    :func:`~megastep_amd.cuda.raycast`'s. Fields that were not asked for are ``None``."""

    def __init__(self, hits, screen, want, shape):
        self._hits, self._screen, self._want, self._shape = hits, screen, want, shape
        n, c, res = shape
        for f in LOOK_FIELDS:
            plane = None
            if f in want:
                plane = screen.view(n, c, res, 3) if f == 'screen' else getattr(hits, f).view(n, c, res)
            setattr(self, f, plane)


def look(scenery, cams, agents=None, fields=('screen', 'distances'), near=None, out=None, config=None, light_grid=True):
    """What the cameras see: one :func:`~megastep_amd.cuda.raycast` launch of all their rays and - only when ``screen`` is asked
    for - one :func:`shade` launch behind it. Returns a :class:`Look`. ``fields``: among ``LOOK_FIELDS``; ``agents``, ``near``
    and ``config`` as :func:`~megastep_amd.cuda.raycast`'s (``near`` defaults to the config's ``agent_radius``, which keeps a
    camera at an agent's own position off that agent's body); ``out``: the :class:`Look` of an earlier call with the same shapes
    and fields to write into - nothing is allocated then, and nothing ever waits for the host."""
    if not isinstance(cams, Cameras):
        raise RuntimeError('cams must come from cameras() or mounted()')
    want = tuple(fields)
    if not want or any(f not in LOOK_FIELDS for f in want):
        raise RuntimeError(f'fields must be among {LOOK_FIELDS}')
    n, c, res = cams.poses.shape[0], cams.n_cameras, cams.res
    cast = tuple(f for f in rays.RAYCAST_FIELDS if f in want or ('screen' in want and f in ('indices', 'locations', 'dots')))
    key = (n, c, res, want, cams.origins.device)
    if out is not None and getattr(out, '_key', None) != key:
        raise RuntimeError('`out` must come from a look call with the same shapes and fields')
    hits = rays.raycast(scenery, cams.origins, cams.directions, agents=agents, near=near, fields=cast, config=config,
                        out=out._hits if out is not None else None)
    screen = None
    if 'screen' in want:
        screen = shade(scenery, hits, agents=agents, out=out._screen if out is not None else None, light_grid=light_grid)
    return _result_for(out, key, 'a look', lambda: Look(hits, screen, want, (n, c, res)))
