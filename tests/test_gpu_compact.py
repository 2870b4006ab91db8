"""The workgroup's ordered compaction (csrc/kernels/math.h: block_compact) alone on the device, through its probe
(include/megastep_hip_test.h: ms_test_block_compact; kernels/culltest.h): one workgroup walks `count` flags in rounds of 256 and
writes each flag's slot. Held to numpy.cumsum EXACTLY - slot[i] == cumsum(keep)[i] - 1 where kept, -1 elsewhere, total == keep.sum() -
at the shapes where a rank can go wrong: a wave with no survivor between two that have some, a partial last round, survivors only
at a ballot's end bits. The six kernels that stage rows in LDS through it are held to their own rules in their own modules."""
import ctypes as C

import numpy as np
import pytest
import torch

COUNTS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1061)


def patterns(count):
    """{name: (count,) uint8}: the masks of the issue, any non-zero byte a kept flag."""
    i = np.arange(count)
    masks = {'none': i < 0, 'all': i >= 0, 'alternate': i % 2 == 0, 'lane 0 of each wave': i % 64 == 0, 'lane 63 of each wave': i % 64 == 63,
             'the last element': i == count - 1}
    for seed, density in ((1, 1/16), (2, 1/2), (3, 15/16)):
        masks[f'random {density}'] = np.random.RandomState(seed).rand(count) < density
    masks = {name: m.astype(np.uint8) for name, m in masks.items()}
    masks['random 0.5'] = masks['random 0.5']*np.random.RandomState(4).choice(np.array([1, 2, 255], np.uint8), count)    # (non-zero is kept)
    return masks


def _probe(keep):
    from megastep_amd import _lib
    dev = torch.device('cuda')
    flags = torch.as_tensor(keep, device=dev)
    slot = torch.full((len(keep),), -7, dtype=torch.int32, device=dev)
    total = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().ms_test_block_compact(ptr(flags), ptr(slot), ptr(total), len(keep), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return slot.cpu().numpy(), int(total.item())


@pytest.mark.gpu
@pytest.mark.parametrize('count', COUNTS)
def test_the_slots_are_numpys_cumsum(count):
    for name, keep in patterns(count).items():
        kept = keep != 0
        want = np.where(kept, np.cumsum(kept) - 1, -1).astype(np.int32)
        slot, total = _probe(keep)
        assert np.array_equal(slot, want), (name, np.flatnonzero(slot != want)[:8])
        assert total == int(kept.sum()), name


def test_the_patterns_hold_the_shapes_they_are_there_for():
    """No GPU: an empty wave between two that keep something, a partial last round, survivors only at a ballot's first or last bit."""
    assert any(count % 256 for count in COUNTS) and any(count % 64 == 1 for count in COUNTS) and max(COUNTS) > 4*256
    for count in COUNTS:
        masks = patterns(count)
        assert len(masks) == 9 and not masks['none'].any() and masks['all'].all() and masks['the last element'].sum() == 1
        assert all(m.dtype == np.uint8 and m.shape == (count,) for m in masks.values())
    per_wave = (patterns(1061)['random 0.0625'][:1024].reshape(-1, 64) != 0).sum(1)
    assert any(per_wave[w] == 0 and per_wave[:w].any() and per_wave[w + 1:].any() for w in range(len(per_wave)))
    assert (patterns(1061)['the last element'][:1024].reshape(-1, 64) != 0).sum() == 0          # (fifteen empty waves, then one flag)


def test_the_probe_refuses_what_cannot_be_launched():
    """A NULL pointer and a negative count are MS_EINVAL; no element is no launch. (Host memory stands in for the device's: nothing
    here gets as far as a kernel.)"""
    from megastep_amd import _lib
    h = _lib.lib()
    buf = np.zeros(16, np.int32)
    p = C.c_void_p(buf.ctypes.data)
    assert h.ms_test_block_compact(p, p, p, 0, None) == 0
    assert h.ms_test_block_compact(p, p, p, -1, None) == -1 and h.ms_test_block_compact(p, p, p, 2**31, None) == -1
    for k in range(3):
        assert h.ms_test_block_compact(*[None if j == k else p for j in range(3)], 0, None) == -1, k
