"""Percepts: the points each eye sees, nearest first (kernel: ``csrc/kernels/percept.h``). No counterpart in the reference;
reached as ``megastep_amd.cuda.<name>``."""
import ctypes as C
import math
import torch
from . import _lib
from ._lib import _on, _stream
from ._call import _check, _query_device, _result_for

PERCEPT_FIELDS = ('visible', 'squares', 'offsets', 'counts', 'nearest', 'near_offsets', 'near_distances')
#: the most eyes and points an env may have in one :func:`percepts` call, and the most nearest points it lists per eye
PERCEPT_MAX_EYES, PERCEPT_MAX_POINTS, PERCEPT_MAX_NEAREST = 64, 1024, 16


class Percepts:
    """Result of :func:`percepts`, for E eyes, P points and the nearest K: ``visible`` (N, E, P) uint8; ``squares`` (N, E, P) - the
    squared distance where visible, +inf elsewhere; ``offsets`` (N, E, P, 2) - the point less the eye, in the world frame, NaN where
    not visible; ``counts`` (N, E) int32; ``nearest`` (N, E, K) int32 - the visible points nearest first, equal distances to the
    lower index, -1 beyond ``counts``; ``near_offsets`` (N, E, K, 2) and ``near_distances`` (N, E, K) of those, NaN and +inf beyond
    ``counts``. Fields that were not asked for are ``None``. ``eyes``, ``points`` and ``headings`` are what the call read (in agents
    form: the agents' positions, and the headings it made of their angles)."""

    def __init__(self, *tensors):
        self._t = tuple(tensors)
        self.eyes = self.points = self.headings = None

    visible = property(lambda self: self._t[0])
    squares = property(lambda self: self._t[1])
    offsets = property(lambda self: self._t[2])
    counts = property(lambda self: self._t[3])
    nearest = property(lambda self: self._t[4])
    near_offsets = property(lambda self: self._t[5])
    near_distances = property(lambda self: self._t[6])


def _bytes(t, name, shapes, letters):
    """``t`` as the uint8 tensor the kernel reads a byte an entry from, sharing its memory: a contiguous uint8 or bool tensor of one of
    ``shapes``; None stays None."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.bool) or tuple(t.shape) not in shapes or not t.is_contiguous():
        raise RuntimeError(f'{name} must be a contiguous {letters} = {" or ".join(map(str, shapes))} uint8 or bool tensor')
    return t.view(torch.uint8)


def _cos_half(fov):
    if not isinstance(fov, (int, float)) or not (0 < fov <= 360):
        raise RuntimeError(f'fov must be a number of degrees with 0 < fov <= 360; got {fov}')
    return max(-1., min(1., math.cos(math.radians(float(fov))/2.)))


def percepts(scenery, points=None, eyes=None, headings=None, max_range=10., fov=None, k=4, valid=None, pairs=None, mask=None, fields=None,
             out=None, agents=None):
    """Which of a set of points each eye can see, how far away and which way each is, and which are nearest: for every env ``E``
    eyes (``eyes`` (N, E, 2) float32 world points) and ``P`` points (``points`` (N, P, 2)), point p is visible to eye e when it is no
    further than ``max_range`` metres, within ``fov`` degrees round ``headings`` (N, E, 2; any length) when both are given, and no
    static wall of ``scenery`` lies across the straight line between the two - :func:`view_fields`' rule, by :func:`view_fields`'
    own device functions: a point is seen exactly when a cell whose centre it is would be. The agents' own lines are not read:
    BODIES DO NOT OCCLUDE. Returns :class:`Percepts`.

    ``valid`` (N, P) bool or uint8: the points that exist; ``pairs`` (E, P) - shared by all envs - or (N, E, P) bool or uint8: the
    points each eye takes an interest in; ``mask`` (N, E) bool or uint8: compute only the marked eyes (the rows of the others keep
    what ``out`` held; uninitialised without ``out``). ``k``: how many nearest visible points to list, 0 to 16. ``fields`` names the
    wanted outputs (default all of ``PERCEPT_FIELDS``); the others are neither allocated nor written. ``out`` takes the
    :class:`Percepts` of an earlier call with the same shapes and fields and rewrites it in place.

    ``agents=`` instead of ``eyes`` and ``headings``: the eyes are the agents' positions, and with ``fov`` the headings are (cos, sin)
    of their angles, made by torch inside the call into a buffer the result keeps. Without ``points`` the agents look at each
    other: the points are their positions too, and ``pairs`` defaults to everyone but itself.

    One launch, one workgroup per env; exact - the rule is written out in include/megastep_hip.h (``MsPercepts``) and DESIGN.md
    3.31, every operation binary32 in a fixed order, and the kernel computes it bit for bit. The kernel has no trigonometry: a
    frame of the eye's own is the caller's (``modules.Percepts``). No host synchronisation, and with ``out`` nothing is allocated:
    the call can be captured in a HIP graph. At most 64 eyes and 1024 points an env."""
    own = agents is not None and points is None         # (the agents look at each other)
    if agents is not None:
        if eyes is not None or headings is not None:
            raise RuntimeError('agents= stands for eyes and headings: give one or the other')
        eyes = agents.positions
        points = eyes if points is None else points
    elif points is None or eyes is None:
        raise RuntimeError('percepts needs points and eyes, or agents=')
    _check(points, 'points', torch.float32, 3)
    _check(eyes, 'eyes', torch.float32, 3)
    n, p = points.shape[:2]
    e = eyes.shape[1]
    if points.shape[2] != 2 or eyes.shape[2] != 2 or eyes.shape[0] != n or n != len(scenery.lines):
        raise RuntimeError(f'points must be (N, P, 2) and eyes (N, E, 2) with N = {len(scenery.lines)}; got {tuple(points.shape)} and {tuple(eyes.shape)}')
    if not 1 <= p <= PERCEPT_MAX_POINTS or not 1 <= e <= PERCEPT_MAX_EYES:
        raise RuntimeError(f'percepts takes 1 to {PERCEPT_MAX_POINTS} points and 1 to {PERCEPT_MAX_EYES} eyes an env; got P = {p}, E = {e}')
    if not isinstance(k, int) or not 0 <= k <= PERCEPT_MAX_NEAREST:
        raise RuntimeError(f'k must be an integer in 0..{PERCEPT_MAX_NEAREST}; got {k}')
    if not isinstance(max_range, (int, float)) or not (0 < max_range < float('inf')):
        raise RuntimeError(f'max_range must be a positive number; got {max_range}')
    if agents is not None:
        if tuple(agents.angles.shape) != (n, e):
            raise RuntimeError('agents do not match the scenery')
        cos_half = _cos_half(fov) if fov is not None else 0.
    else:
        if (headings is None) != (fov is None):
            raise RuntimeError('headings and fov go together: a cone needs both')
        cos_half = 0.
        if headings is not None:
            _check(headings, 'headings', torch.float32, 3)
            if headings.shape != eyes.shape:
                raise RuntimeError(f'headings must be (N, E, 2) = {tuple(eyes.shape)}; got {tuple(headings.shape)}')
            cos_half = _cos_half(fov)
    valid = _bytes(valid, 'valid', ((n, p),), '(N, P)')
    pairs = _bytes(pairs, 'pairs', ((e, p), (n, e, p)), '(E, P) or (N, E, P)')
    mask = _bytes(mask, 'mask', ((n, e),), '(N, E)')
    want = PERCEPT_FIELDS if fields is None else tuple(fields)
    if not want or any(f not in PERCEPT_FIELDS for f in want):
        raise RuntimeError(f'fields must be some of {PERCEPT_FIELDS}')
    given = [t for t in (headings, valid, pairs, mask) if t is not None]
    dev = _query_device(scenery, agents, points, eyes, *given)
    cone = fov is not None

    def make():
        shapes = dict(visible=((n, e, p), torch.uint8), squares=((n, e, p), torch.float32), offsets=((n, e, p, 2), torch.float32),
                      counts=((n, e), torch.int32), nearest=((n, e, k), torch.int32), near_offsets=((n, e, k, 2), torch.float32),
                      near_distances=((n, e, k), torch.float32))
        result = Percepts(*(torch.empty(shapes[f][0], dtype=shapes[f][1], device=dev) if f in want else None for f in PERCEPT_FIELDS))
        if agents is not None:
            # (what the agents form makes for itself: everyone but itself, and room for the headings)
            result._others = (1 - torch.eye(e, dtype=torch.uint8, device=dev)).contiguous() if own else None
            result._turn = torch.empty((3, n, e), dtype=torch.float32, device=dev) if cone else None
            result._headings = torch.empty((n, e, 2), dtype=torch.float32, device=dev) if cone else None
        return result

    result = _result_for(out, (n, e, p, k, want, dev, agents is not None, own, cone), 'a percepts', make)
    if agents is not None:
        if pairs is None and own:
            pairs = result._others
        if cone:
            radians, c, s = result._turn
            torch.mul(agents.angles, math.pi/180, out=radians)
            torch.cos(radians, out=c)
            torch.sin(radians, out=s)
            headings = torch.stack([c, s], -1, out=result._headings)
    result.eyes, result.points, result.headings = eyes, points, headings
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    spec = _lib.MsPercepts(e, p, k, eyes.data_ptr(), ptr(headings), points.data_ptr(), ptr(valid), ptr(pairs),
                           0 if pairs is None else 1 if pairs.ndim == 2 else 2, ptr(mask), float(max_range), cos_half, *(ptr(t) for t in result._t))
    with _on(dev):
        _lib.check(_lib.lib().ms_percepts(C.byref(scenery._as_struct()), C.byref(spec), _stream(dev)))
    return result
