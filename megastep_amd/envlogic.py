"""The demo envs' game logic between one frame and the next, a launch each (kernels: ``csrc/kernels/envlogic.h``). No counterpart
in the reference's extension, whose envs do this with tensor ops; reached as ``megastep_amd.cuda.<name>``."""
import ctypes as C
import torch
from . import _lib
from ._lib import _on, _stream
from ._call import _check, _require_gpu


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
    for name, t in (('tally', tally), ('before', before), ('lengths', lengths), ('epoch', epoch), ('over', over)):
        _check(t, name, torch.bool if name == 'over' else torch.int32, 1)
        if t.shape != (n,):
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
