"""The envs drawn from above into tensors (kernels: ``csrc/kernels/overhead.h``). The reference draws them with matplotlib, one
env at a time on the host (plotting.py); reached as ``megastep_amd.cuda.<name>``."""
import ctypes as C
import math
import torch
from . import _lib
from ._lib import _on, _stream
from ._call import _check, _hw, _query_device, _result_for
from .nav import _static_boxes

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
    dev = _query_device(scenery, agents, views, *([envs] if envs is not None else []))
    if envs is not None and envs.dtype != torch.int32:
        envs = envs.to(torch.int32)
    envs = envs.contiguous() if envs is not None else None
    result = _result_for(out, (k, v, h, w, want, dev), 'an overhead', lambda: Overhead(
        torch.empty((k, v, 3, h, w), dtype=torch.float32, device=dev) if 'rgb' in want else None,
        torch.empty((k, v, h, w), dtype=torch.int32, device=dev) if 'indices' in want else None))
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
    lo, hi = _static_boxes(scenery)
    empty = ~torch.isfinite(lo).all(1)                                   # (an env without walls: a 2 margin square about 0)
    lo = torch.where(empty[:, None], torch.zeros_like(lo), lo) - margin
    hi = torch.where(empty[:, None], torch.zeros_like(hi), hi) + margin
    if envs is not None:
        envs = torch.as_tensor(envs, device=lo.device).long()
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

