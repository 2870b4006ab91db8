"""The fan schedule (MsAgents.schedule) on the CPU: ms_host_order_fans - the host mirror of the sort that ms_step_physics' extra
waves do - writes, whatever the costs hold, a permutation of every XCD's run of fans with the slowest classes first; and the
table-less block -> fan mapping it permutes is still render_block's."""
import ctypes as C
import numpy as np
import pytest

from megastep_amd import _lib

CLASSES = 64          # physics.h: FAN_CLASSES
SORT_MAX = 512        # physics.h: FAN_SORT_MAX


def runs(n_fans):
    """XCD x's run of slots (and of fans) in a launch of n_fans one-fan blocks: render_block's ng == 1, restated."""
    q, r = divmod(n_fans, 8)
    return [(x*q + min(x, r), q + (1 if x < r else 0)) for x in range(8)]


def klass(costs):
    return np.minimum(costs.astype(np.int32).view(np.uint32), CLASSES - 1).astype(np.int64)


def order_fans(costs):
    costs = np.ascontiguousarray(costs, dtype=np.int32)
    order = np.full(len(costs), -12345, dtype=np.int32)
    blocks = _lib.lib().ms_host_order_fans(len(costs), costs.ctypes.data_as(_lib._i32p), order.ctypes.data_as(_lib._i32p))
    return order, blocks


def check(costs):
    order, blocks = order_fans(costs)
    n = len(costs)
    longest = max(length for _, length in runs(n))
    per_run = max(-(-longest//SORT_MAX), 1) if longest else 0
    assert blocks == 8*per_run
    cls = klass(np.asarray(costs))
    for first, length in runs(n):
        got = order[first:first + length]
        assert sorted(got.tolist()) == list(range(first, first + length)), 'a permutation of the run'
        # K sort waves deal their sorted K-ths of the run round-robin: every K-th slot from k on is one wave's, classes descending
        for k in range(per_run):
            dealt = cls[got[k::per_run]]
            assert (np.diff(dealt) <= 0).all(), 'slowest classes first'
        if per_run == 1 and length:
            assert cls[got[0]] == cls[first:first + length].max()
    return order


@pytest.mark.parametrize('n_envs, n_agents', [(4096, 4), (4096, 1), (8, 1), (1, 1), (3, 2), (13, 3), (1001, 4), (4099, 5), (9000, 4), (40000, 1)])
def test_random_costs_give_a_permutation_of_every_run_slowest_first(n_envs, n_agents):
    rng = np.random.RandomState(n_envs + n_agents)
    check(rng.randint(0, 80, n_envs*n_agents))
    check(rng.randint(0, 12, n_envs*n_agents))


@pytest.mark.parametrize('n_fans', [1, 7, 8, 9, 4096, 16384, 513*8 + 3])
@pytest.mark.parametrize('value', [0, 5, 63, 64, -1, 2**31 - 1, -2**31])
def test_constant_costs_keep_the_fans_in_fan_order(n_fans, value):
    order = check(np.full(n_fans, value, dtype=np.int64).astype(np.int32))
    longest = max(length for _, length in runs(n_fans))
    if longest <= SORT_MAX:                 # (one sort wave a run: the mirror ranks equal classes in fan order - the identity)
        assert (order == np.arange(n_fans)).all()


def test_every_bit_pattern_is_a_class():
    rng = np.random.RandomState(3)
    bits = rng.randint(0, 2**32, 16384 + 5, dtype=np.uint64).astype(np.uint32)
    bits[:64] = [1 << (i % 32) for i in range(64)]
    bits[64:70] = [0xffffffff, 0x80000000, 0x7fffffff, 0x7fc00000, 0xff800000, 0]
    check(bits.view(np.int32))
    assert klass(np.array([-1, -2**31, 2**31 - 1, 63, 64, 62, 0], dtype=np.int32)).tolist() == [63, 63, 63, 63, 63, 62, 0]


@pytest.mark.parametrize('n_envs', [1, 2, 5, 7, 9, 4095, 4097, 4100])
def test_env_counts_that_do_not_divide_by_eight(n_envs):
    rng = np.random.RandomState(n_envs)
    for n_agents in (1, 3, 4):
        check(rng.randint(-5, 70, n_envs*n_agents))


def test_bad_arguments_are_refused():
    h = _lib.lib()
    one = (C.c_int*1)(0)
    assert h.ms_host_order_fans(0, one, one) == -1 and h.ms_host_order_fans(1, None, one) == -1 and h.ms_host_order_fans(1, one, None) == -1


def test_the_table_less_mapping_is_still_render_blocks():
    """Slot s of XCD x's run is block x + 8 (s - run's first): with the identity for a table, the fans a launch of one-fan blocks
    hands its XCDs are the runs the sort permutes."""
    h = _lib.lib()
    for n_envs, n_agents in ((13, 3), (64, 4), (9, 1)):
        n_fans = n_envs*n_agents
        out4 = (C.c_int*4)()
        for x, (first, length) in enumerate(runs(n_fans)):
            for i in range(length):
                assert h.ms_host_render_block(n_envs, n_agents, 64, 6144, 0, -1., -1, x + 8*i, out4) == 1
                assert out4[0]*n_agents + out4[1] == first + i and out4[2] == 0 and out4[3] == 64


def test_agents_carry_an_identity_schedule():
    import torch
    from megastep_amd import core, cuda
    agents = core._init_agents(5, 3, 'cpu')
    assert agents._schedule.shape == (2, 15) and agents._schedule.dtype == torch.int32
    assert (agents._schedule[0] == 0).all() and (agents._schedule[1] == torch.arange(15)).all()
    assert C.sizeof(_lib.MsAgents) == 6*C.sizeof(C.c_void_p)
