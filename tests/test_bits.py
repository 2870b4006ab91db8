"""The bit comparisons of tests/util.py themselves: what the GPU suite's equality with the oracle means, on the CPU."""
import re

import numpy as np
import pytest
import torch

from tests import util

f = np.float32


def _from_bits(*patterns):
    return np.array(patterns, np.uint32).view(np.float32)


def _fails(got, want, what='plane'):
    with pytest.raises(AssertionError) as e:
        util.assert_bits(got, want, what)
    return str(e.value)


def test_equal_arrays_pass_whatever_they_hold():
    x = np.array([0., -0., 1., -1.5, np.inf, -np.inf, np.nan, 1e-45, 3.4e38], f)
    assert util.same_bits(x, x.copy()).all()
    util.assert_bits(x, x.copy(), 'x')
    util.assert_bits(torch.as_tensor(x), x, 'a tensor against an array')
    i = np.array([[0, -1], [7, 2**31 - 1]], np.int32)
    util.assert_bits(i, i.copy(), 'integers')


def test_nans_of_different_payloads_are_the_same():
    a = _from_bits(0x7fc00000, 0x7fc00001, 0xffc00000, 0x7f800001)
    b = _from_bits(0xffc12345, 0x7fc00000, 0x7fc00000, 0xffffffff)
    assert np.isnan(a).all() and np.isnan(b).all() and (a.view(np.uint32) != b.view(np.uint32)).all()
    assert util.same_bits(a, b).all()
    util.assert_bits(a, b, 'nans')
    assert 'got nan, want 0x1.0000000000000p+0' in _fails(a[:1], np.ones(1, f))       # ... but a NaN is no number


def test_zeros_of_different_sign_differ():
    got, want = np.array([1., -0., 0.], f), np.array([1., 0., 0.], f)
    assert util.same_bits(got, want).tolist() == [True, False, True]
    msg = _fails(got, want)
    assert '1 of 3 elements differ' in msg and '(1,): got -0x0.0p+0, want 0x0.0p+0' in msg
    assert 'Largest distance: 0 ulp; largest absolute difference: 0.' in msg


def test_a_neighbour_is_one_ulp_away():
    want = np.array([[1., 2.], [-3., 1e-3]], f)
    got = want.copy()
    got[1, 0] = np.nextafter(want[1, 0], f(0))
    msg = _fails(got, want, 'locations')
    assert msg.startswith('locations: 1 of 4 elements differ')
    assert f'(1, 0): got {float(got[1, 0]).hex()}, want {float(f(-3.)).hex()}' in msg
    assert 'Largest distance: 1 ulp' in msg and 'largest absolute difference: 2.38e-07' in msg
    assert util.ulp_distance(np.nextafter(f(1), f(2)), f(1)) == 1 and util.ulp_distance(f(1), f(2)) == 2**23


def test_the_distance_is_meaningful_across_zero():
    tiny, minus_tiny = _from_bits(0x00000001), _from_bits(0x80000001)
    assert tiny[0] > 0 > minus_tiny[0]
    assert util.ulp_distance(tiny, minus_tiny) == 2
    assert 'Largest distance: 2 ulp' in _fails(tiny, minus_tiny)
    assert util.ulp_distance(f(0.), tiny) == 1 and util.ulp_distance(f(-0.), tiny) == 1
    assert util.ulp_distance(f(-1.), f(1.)) == 2*0x3f800000


def test_infinity_is_not_a_large_number():
    big = np.array([np.finfo(f).max, 1.], f)
    msg = _fails(np.array([np.inf, 1.], f), big)
    assert '1 of 2 elements differ' in msg and 'got inf' in msg and 'Largest distance: 1 ulp' in msg
    assert 'largest absolute difference: inf' in msg
    _fails(np.array([np.inf], f), np.array([-np.inf], f))


def test_the_first_five_and_the_largest_are_reported():
    want = np.linspace(1, 2, 40).astype(f)
    got = want.copy()
    got[10:20] = np.nextafter(got[10:20], f(3))
    got[17] = want[17] + f(1e-4)
    msg = _fails(got, want)
    assert '10 of 40 elements differ' in msg
    assert re.findall(r'\((\d+),\): got', msg) == ['10', '11', '12', '13', '14']
    assert f'Largest distance: {int(util.ulp_distance(got[17:18], want[17:18])[0])} ulp' in msg and 'largest absolute difference: 0.0001' in msg


def test_shapes_and_dtypes_must_agree():
    x = np.zeros((2, 3), f)
    assert 'shapes differ' in _fails(x, np.zeros((3, 2), f))
    assert 'shapes differ' in _fails(x, np.zeros(3, f))                                # (no broadcasting)
    assert 'dtypes differ' in _fails(x, np.zeros((2, 3), np.float64))
    assert 'dtypes differ' in _fails(np.zeros(2, np.int32), np.zeros(2, np.int64))
    with pytest.raises(AssertionError):
        util.same_bits(x, np.zeros((2, 3), np.float64))


def test_integers_compare_by_value():
    got, want = np.array([1, 2, 3], np.int32), np.array([1, 5, 3], np.int32)
    assert util.same_bits(got, want).tolist() == [True, False, True]
    msg = _fails(got, want, 'indices')
    assert 'indices: 1 of 3 elements differ' in msg and '(1,): got 2, want 5' in msg


class _Holder:
    pass


def _core_and_results(agents, progress):
    core, p = _Holder(), _Holder()
    core.agents = _Holder()
    for k, v in agents.items():
        setattr(core.agents, k, torch.as_tensor(v))
    p.progress = torch.as_tensor(progress)
    return core, p


def test_the_physics_and_render_helpers_hold_every_plane():
    rng = np.random.RandomState(0)
    agents = dict(angles=rng.uniform(-180, 180, (2, 3)).astype(f), positions=rng.rand(2, 3, 2).astype(f),
                  angvelocity=rng.rand(2, 3).astype(f), velocity=rng.rand(2, 3, 2).astype(f))
    progress = np.array([[1., .5, 1.], [0., 1., 1.]], f)
    core, p = _core_and_results(agents, progress)
    util.assert_physics_bits(core, p, progress, agents)
    for k in agents:                                      # one ulp anywhere, the angles included, is caught - and named
        moved = {n: v.copy() for n, v in agents.items()}
        moved[k].flat[1] = np.nextafter(moved[k].flat[1], f(1000))
        with pytest.raises(AssertionError, match=f'^{k}: 1 of'):
            util.assert_physics_bits(core, p, progress, moved)
    lower = progress.copy(); lower[0, 0] = np.nextafter(f(1), f(0))
    with pytest.raises(AssertionError, match='collision masks differ'):
        util.assert_physics_bits(core, p, lower, agents)
    lower = progress.copy(); lower[0, 1] = np.nextafter(f(.5), f(0))
    with pytest.raises(AssertionError, match='^progress: 1 of 6'):
        util.assert_physics_bits(core, p, lower, agents)

    ref = dict(indices=np.array([[[3, -1, 5]]], np.int32), locations=np.array([[[.25, 0., .5]]], f), dots=np.array([[[.1, np.nan, -.2]]], f),
               distances=np.array([[[2., np.inf, 3.]]], f), screen=rng.rand(1, 1, 3, 3).astype(f))
    r = _Holder()
    for k, v in ref.items():
        setattr(r, k, torch.as_tensor(v))
    util.assert_render_bits(None, r, ref)
    for k in ('locations', 'dots', 'distances'):          # the ray that missed is held as well
        moved = dict(ref, **{k: ref[k].copy()})
        moved[k][0, 0, 1] = 7.
        with pytest.raises(AssertionError, match=f'^{k}: 1 of 3'):
            util.assert_render_bits(None, r, moved)
    with pytest.raises(AssertionError, match='hit indices differ'):
        util.assert_render_bits(None, r, dict(ref, indices=np.array([[[3, -1, 4]]], np.int32)))


@pytest.mark.parametrize('n_agents,res,subsample', [(2, 64, 4), (1, 96, 2), (1, 32, 1), (2, 64, 16)])
def test_the_pooled_rule_means_what_the_observation_modules_mean(n_agents, res, subsample):
    """util.pooled_rule - what the GPU suite holds the render kernel's pooled observations to, as bits - against modules.RGB /
    modules.Depth on CPU tensors, both on the oracle's render of a small plan world. Two formulations of a mean over `subsample`
    rays of numbers in [0, 1]: each rounds at most subsample - 1 additions (and the depth's quotient against its product with
    a reciprocal: an ulp of a number below 1), so 1e-6 is ample."""
    from megastep_amd import arrdict, modules
    c, _ = util.plan_world(3, n_agents, res, 130, seed=11, device='cpu')
    c.agents.positions[-1, 0] = torch.tensor([-2., 3.])           # (outside its closed plan, looking past it: part of the fan misses)
    c.agents.angles[-1, 0] = 100.
    ref = util.OracleWorld(c)
    ref.scene.baked_vals[:] = ref.bake()
    o = ref.render()
    assert np.isinf(o['distances']).any(), 'a ray that missed belongs in this world'
    r_cpu = arrdict.arrdict(distances=torch.as_tensor(o['distances']).unsqueeze(2),
                            screen=torch.as_tensor(o['screen']).unsqueeze(2).permute(0, 1, 4, 2, 3))
    class CpuCore: agent_radius, res = c.agent_radius, c.res
    want_rgb = modules.RGB(CpuCore, n_agents=n_agents, subsample=subsample)(r_cpu)
    want_d = modules.Depth(CpuCore, n_agents=n_agents, subsample=subsample, max_depth=7.)(r_cpu)
    rgb, d = util.pooled_rule(o['screen'], o['distances'], c.agent_radius, 7., subsample)
    assert rgb.shape == (3, n_agents, 3, res//subsample) and d.shape == (3, n_agents, res//subsample)
    np.testing.assert_allclose(rgb, want_rgb.numpy()[:, :, :, 0], rtol=0, atol=1e-6)
    np.testing.assert_allclose(d, want_d.numpy()[:, :, 0, 0], rtol=0, atol=1e-6)
    missed = np.isinf(o['distances']).reshape(d.shape + (subsample,)).all(-1)
    assert missed.any() and (d[missed] == 0).all() and ((d > 0) & (d < 1)).any()
    if subsample == 1:                                    # nothing to sum: the planes themselves
        util.assert_bits(rgb, np.moveaxis(o['screen'], -1, -2).copy(), 'rgb')
