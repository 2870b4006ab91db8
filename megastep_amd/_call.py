"""What every call of :mod:`megastep_amd.cuda` and of the modules beside it (``rays``, ``rollouts``, ``overhead``, ``nav``, ``envlogic``) does
before its launch: the tensor checks, the device its tensors share, and the constants of :func:`~megastep_amd.cuda.initialize`."""
import torch
from . import _lib

# ---------------------------------------------------------------------------------------------------------------------
# the constants                                                                reference: kernels.cu:18-27
# ---------------------------------------------------------------------------------------------------------------------
_config = None                  # what cuda.initialize() set: the fallback of _cfg


def config(agent_radius, res, fov, fps):
    """The four constants of :func:`initialize` as a value (the C-ABI's ``MsConfig``, passed by value with every launch):
    what a :class:`~megastep_amd.core.Core` keeps for itself and hangs on its ``Agents``, so that several Cores of
    different resolutions, fields of view or frame rates live side by side in one process - on one device or several."""
    if not (0 < fov < 180):
        raise RuntimeError('fov must be in (0, 180) degrees')
    if res <= 0 or fps <= 0 or agent_radius <= 0:
        raise RuntimeError('agent_radius, res and fps must be positive')
    return _lib.MsConfig(float(agent_radius), int(res), float(fov), float(fps))


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


def _agents_on(agents, dev):
    if agents._dev != dev:
        if agents._dev is None or not agents._dev.type == 'cuda':
            raise RuntimeError('megastep_amd kernels need GPU (HIP) tensors; the agents are on ' + str(agents._dev or 'several devices'))
        raise RuntimeError(f'all tensors must live on one device; got {agents._dev} and {dev}')


def _query_device(scenery, agents, *tensors):
    """The GPU a query against the scenery runs on: the one its own ``tensors`` share, which must be the scenery's and, if
    it takes ``agents``, theirs - asked in that order."""
    dev = _require_gpu(*tensors)
    if scenery._device() != dev:
        raise RuntimeError(f'all tensors must live on one device; got {scenery._device()} and {dev}')
    if agents is not None:
        _agents_on(agents, dev)
    return dev


def _hw(size):
    h, w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if h < 1 or w < 1:
        raise RuntimeError(f'size must be positive; got {size}')
    return h, w


def _result_for(out, key, call, make):
    """The result a query writes into: ``out`` - which an earlier ``call`` must have made for the same ``key`` - else what
    ``make()`` gives, marked with the key."""
    if out is not None:
        if getattr(out, '_key', None) != key:
            raise RuntimeError(f'`out` must come from {call} call with the same shapes and fields')
        return out
    result = make()
    result._key = key
    return result
