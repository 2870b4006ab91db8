"""The fan schedule (MsAgents.schedule) on the CPU: ms_host_order_fans - the host mirror of the sort that ms_step_physics' extra
waves do - writes, whatever the costs hold, a permutation of every XCD's run of fans with the slowest classes first; and the
table-less block -> fan mapping it permutes is still render_block's.

`order_rule` states which fan goes to which slot, in numpy, from DESIGN.md's words (3.2 "which fan", 3.6): the mirror is held to it
element for element here, the device's sort waves in tests/test_gpu_fan_schedule.py."""
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


def shares(n_fans):
    """The sort's shares: K = max(ceil(longest run / SORT_MAX), 1) sort waves a run; share k of XCD x's run [first, first + len)
    takes len//K + (k < len % K) consecutive fans from first + k*(len//K) + min(k, len % K) on, and its rank j goes to slot
    first + k + K*j. A list of (first_fan, count, first_slot), run after run, and K."""
    K = max(-(-max(length for _, length in runs(n_fans))//SORT_MAX), 1)
    out = []
    for first, length in runs(n_fans):
        lo, rem = divmod(length, K)
        out += [(first + k*lo + min(k, rem), lo + (1 if k < rem else 0), first + k) for k in range(K)]
    return out, K


def order_rule(costs):
    """The fan schedule's order row for a costs row, and K: every share sorted by class, slowest first, fans of one class in fan
    order (numpy's stable sort), dealt to every K-th slot of its run."""
    cls = klass(np.asarray(costs))
    parts, K = shares(len(cls))
    order = np.full(len(cls), -1, dtype=np.int32)
    for first_fan, count, first_slot in parts:
        fans = np.arange(first_fan, first_fan + count)
        order[first_slot + K*np.arange(count)] = fans[np.argsort(-cls[fans], kind='stable')]
    return order, K


def assert_order_follows_the_rule(costs, order, exact=False, what=''):
    """What a sort by LDS atomics owes the rule: every slot written with a fan of the launch; every share's slots a permutation of
    the share's own contiguous fans; slot by slot the class of the fan there is the class of the rule's fan - the classes' sequence
    and each class's set of fans are fixed, the fans' order inside a class is not. `exact`: no two fans of a share tie, so the order
    is the rule's, element for element. Returns the rule's order."""
    costs, order = np.asarray(costs), np.asarray(order)
    n = len(costs)
    assert order.shape == (n,), what
    want, K = order_rule(costs)
    assert ((order >= 0) & (order < n)).all(), f'{what}: slots {np.nonzero((order < 0) | (order >= n))[0][:8].tolist()} hold no fan of the launch: {order[(order < 0) | (order >= n)][:8].tolist()}'
    cls = klass(costs)
    for first_fan, count, first_slot in shares(n)[0]:
        got = order[first_slot + K*np.arange(count)]
        assert sorted(got.tolist()) == list(range(first_fan, first_fan + count)), f'{what}: the share of fans {first_fan}..{first_fan + count - 1} is not what its slots hold'
    differ = np.nonzero(cls[order] != cls[want])[0]
    assert not len(differ), f'{what}: {len(differ)} slots hold a fan of another class than the rule\'s; first: slot {differ[0]}, fan {order[differ[0]]} of class {cls[order[differ[0]]]}, the rule\'s fan {want[differ[0]]} of class {cls[want[differ[0]]]}'
    if exact:
        assert (order == want).all(), f'{what}: no ties, yet slot {int(np.argmax(order != want))} holds another fan than the rule\'s'
    return want


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


def cost_sets(n_fans, seed):
    """The cost rows the rule and the mirror are compared on (int32)."""
    rng = np.random.RandomState(seed)
    bits = rng.randint(0, 2**32, n_fans, dtype=np.uint64).astype(np.uint32).view(np.int32)
    return {'random 0..79': rng.randint(0, 80, n_fans).astype(np.int32), 'random 0..11': rng.randint(0, 12, n_fans).astype(np.int32),
            'constant': np.full(n_fans, 5, np.int32), 'bit patterns': bits, 'arange % 64': (np.arange(n_fans) % 64).astype(np.int32),
            'arange reversed': np.arange(n_fans, dtype=np.int32)[::-1].copy(),
            'arange reversed % 64': (np.arange(n_fans)[::-1] % 64).astype(np.int32)}


@pytest.mark.parametrize('n_fans', [1, 3, 7, 8, 9, 39, 64, 4096, 4097, 4100, 8193, 8196, 12289])
def test_the_mirror_is_the_rule_element_for_element(n_fans):
    for name, costs in cost_sets(n_fans, seed=n_fans).items():
        want, K = order_rule(costs)
        got, blocks = order_fans(costs)
        assert blocks == 8*K, name
        assert (got == want).all(), f'{name}: first slot that differs {int(np.argmax(got != want))}'
        check(costs)
    # the shares the issue's shapes stand for, written out: a change of SORT_MAX fails here
    lengths = lambda n: sorted({count for _, count, _ in shares(n)[0]}, reverse=True)
    assert (shares(4096)[1], lengths(4096)) == (1, [512])
    assert (shares(4097)[1], lengths(4097)) == (2, [257, 256]) and (shares(4100)[1], lengths(4100)) == (2, [257, 256])
    assert (shares(8193)[1], lengths(8193)) == (3, [342, 341]) and (shares(8196)[1], lengths(8196)) == (3, [342, 341])


def test_the_rule_on_a_run_small_enough_to_read():
    """13 x 3 fans: runs of 5, 5, 5, 5, 5, 5, 5, 4; K = 1. The first run's costs 2 9 2 70 9: classes 2 9 2 63 9, so fan 3 first, then
    fans 1 and 4 in fan order, then 0 and 2."""
    costs = np.zeros(39, np.int32)
    costs[:5] = [2, 9, 2, 70, 9]
    costs[35:] = [1, 1, -1, 0]
    order, K = order_rule(costs)
    assert K == 1 and runs(39)[0] == (0, 5) and runs(39)[7] == (35, 4)
    assert order[:5].tolist() == [3, 1, 4, 0, 2] and order[5:35].tolist() == list(range(5, 35)) and order[35:].tolist() == [37, 35, 36, 38]
    assert (order_fans(costs)[0] == order).all()


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


def test_what_the_device_comparison_accepts_and_what_it_does_not():
    """assert_order_follows_the_rule, which tests/test_gpu_fan_schedule.py and tests/test_gpu_fan_order.py hold the device's sort to:
    fans of one class may change places, and nothing else may."""
    costs = np.array([3, 9, 9, 70, 1] + [0]*34, dtype=np.int32)              # 39 fans: the first run holds fans 0..4
    order = order_fans(costs)[0]
    assert order[:5].tolist() == [3, 1, 2, 0, 4]
    assert_order_follows_the_rule(costs, order, exact=False)
    tied = order.copy(); tied[[1, 2]] = tied[[2, 1]]                           # fans 1 and 2 are one class
    assert_order_follows_the_rule(costs, tied)
    with pytest.raises(AssertionError):
        assert_order_follows_the_rule(costs, tied, exact=True)
    for spoil in (lambda o: o.__setitem__([0, 1], o[[1, 0]]),                   # a slower fan behind a faster one
                  lambda o: o.__setitem__(7, -12345),                           # a slot nobody wrote
                  lambda o: o.__setitem__([4, 5], o[[5, 4]]),                   # fans of one class, but of two runs
                  lambda o: o.__setitem__(6, 5)):                               # a fan twice
        bad = order.copy()
        spoil(bad)
        with pytest.raises(AssertionError):
            assert_order_follows_the_rule(costs, bad)
