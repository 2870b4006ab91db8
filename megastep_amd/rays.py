"""Batched ray queries against the scenery (kernels: ``csrc/kernels/raycast.h``). No counterpart in the reference, whose rays
are the render's alone (kernels.cu:326-382); reached as ``megastep_amd.cuda.<name>``."""
import ctypes as C
import torch
from . import _lib
from ._lib import _on, _stream
from ._call import _cfg, _check, _query_device, _require_gpu, _result_for

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
    dev = _query_device(scenery, agents, origins, directions)
    if near is None:
        near = _cfg(agents, config).agent_radius
    if not near >= 0:
        raise RuntimeError('near must be a non-negative number')
    if grid_rays is not None:
        _check(grid_rays, 'grid_rays', torch.int32, 1)
        _require_gpu(grid_rays)
    result = _result_for(out, (n, r, want, dev), 'a raycast', lambda: Raycast(*(
        torch.empty((n, r), dtype=torch.int32 if f in ('indices', 'agents') else torch.float32, device=dev) if f in want else None
        for f in RAYCAST_FIELDS)))
    result._scenery = scenery                                           # (overlay_items reads the envs' numbers of lines)
    ptrs = [t.data_ptr() if t is not None else None for t in result._t]
    query = _lib.MsRaycast(r, origins.data_ptr(), directions.data_ptr(), float(near), *ptrs,
                           grid_rays.data_ptr() if grid_rays is not None else None)
    scenery._check_grid(dev)
    with _on(dev):
        _lib.check(_lib.lib().ms_raycast(C.byref(scenery._as_struct()), C.byref(agents._plain) if agents is not None else None,
                                         C.byref(query), None, _stream(dev)))
    return result


def camera_rays(agents, config=None, out=None):
    """The direction vector of every ray :func:`render` casts, (N, A, res, 2) float32 - by the render's own device code (ray_y,
    reference kernels.cu:234-236,334-337). ``raycast(scenery, positions broadcast over the rays, camera_rays(agents),
    agents=agents)`` then gives the render's ``indices``, ``locations``, ``dots`` and ``distances`` bit for bit.
    ``config``: see :func:`physics` (``res`` and ``fov`` are read). ``out``: the tensor of an earlier call to write into."""
    dev = agents._dev
    if dev is None or dev.type != 'cuda':
        raise RuntimeError('megastep_amd kernels need GPU (HIP) tensors; the agents are on ' + str(dev or 'several devices'))
    cfg = _cfg(agents, config)
    n, a = agents.angles.shape
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (n, a, cfg.res, 2)
                            or not out.is_contiguous() or out.device != dev):
        raise RuntimeError(f'`out` must be a contiguous float32 tensor of shape {(n, a, cfg.res, 2)} on {dev}')
    dirs = torch.empty((n, a, cfg.res, 2), dtype=torch.float32, device=dev) if out is None else out
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

