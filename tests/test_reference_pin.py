"""The oracle against the reference's own kernels, bit for bit.

``oracle/reference.py`` compiles the reference's ``kernels.cu`` / ``wrappers.cpp`` for the host (a serial loop over blocks and
threads; the oracle's compiler flags). Here every world family the GPU suite holds the HIP kernels to the oracle on - and
directed worlds for the rules that random plans never reach - goes through both: the bake first, then multi-step rollouts in
which each side's physics starts from the reference's state and each side's render takes the reference's post-physics agents.
Everything is held to EQUALITY of bits (any NaN equals any NaN): baked light, progress, the four agent tensors, the agent
lines that render writes back, indices, locations, dots, distances, screen.

The one thing the two sides cannot share is sinpif / cospif, which CUDA supplies and neither libm nor the oracle has: the
shim's (libm, in double) and the oracle's (a Taylor series in double) are swept against each other below, and every world
asserts first that they agree on each angle it uses."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from oracle import reference
from tests import util

pytestmark = pytest.mark.skipif(not reference.available(), reason='neither a built oracle/_ref module nor the reference sources')

PLANES = ('indices', 'locations', 'dots', 'distances', 'screen')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_same_bits(got, want, what):
    """Equal bit patterns - signed zeros and infinities included - except that any NaN matches any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = _bits(got) == _bits(want)
    if got.dtype == np.float32:
        same |= np.isnan(got) & np.isnan(want)
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f'{what}: {int((~same).sum())} of {same.size} differ; first at {i}: oracle {got[i]!r}, reference {want[i]!r}')


def assert_sincospi_agree(angles, what):
    x = (np.asarray(angles, np.float32)/np.float32(180.)).ravel()           # kernels.cu:304,335
    x = x[np.isfinite(x)]
    (so, co), (sr, cr) = O.sincospi_many(x), reference.sincospi(x)
    bad = (_bits(so) != _bits(sr)) | (_bits(co) != _bits(cr))
    assert not bad.any(), f'{what}: the two sincospi differ at angle/180 = {x[bad][:5]}: pick another seed for this world'


def pin(case, min_collisions=0, min_hits=1):
    """Runs a case (tests/util.py) through the oracle and the reference and holds every output to equality. Returns the
    reference's outputs of the last step (and a few counts) for the caller's own preconditions."""
    scene, cfg, agents = case['scene'], case['config'], {k: v.copy() for k, v in case['agents'].items()}
    ref = reference.World(scene, cfg)
    ora = O.Scene(scene)
    ocfg = O.config(*cfg)
    want = ref.bake()
    assert_same_bits(O.bake(ora, ocfg), want, 'baked')
    collisions = hits = 0
    out = dict(baked=want)
    for step, (velocity, angvelocity) in enumerate(case['moves']):
        agents['velocity'], agents['angvelocity'] = velocity.copy(), angvelocity.copy()
        progress, after = ref.physics(agents)
        got_progress, got_after = O.physics(ora, agents, ocfg)
        assert_same_bits(got_progress, progress, f'progress, step {step}')
        for k in reference.AGENT_FIELDS:
            assert_same_bits(got_after[k], after[k], f'{k}, step {step}')
        assert_sincospi_agree(after['angles'], f'step {step}')
        frame = ref.render(after)
        got = O.render(ora, after, ocfg)
        for k in PLANES:
            assert_same_bits(got[k], frame[k], f'{k}, step {step}')
        assert_same_bits(ora.lines_vals, ref.lines_vals, f'lines written back, step {step}')
        collisions += int((progress < 1).sum())
        hits += int((frame['indices'] >= 0).sum())
        agents = after
        out.update(progress=progress, agents=after, **frame)
    assert collisions >= min_collisions and hits >= min_hits, (collisions, hits)
    out.update(collisions=collisions, hits=hits)
    return out


def _moves(c, seed, speeds):
    return util.random_moves((c.n_envs, c.n_agents), np.random.RandomState(seed), speeds)


# ---- the two sincospi ------------------------------------------------------------------------------------------------

def sincospi_arguments():
    """Four million seeded binary32 bit patterns (the finite ones), two million arguments in [-2, 2], every multiple of 1/360
    in [-1, 1] - as a quotient and as degrees/180, the way the kernels form it - and the exact quarter turns up to +-4."""
    rng = np.random.RandomState(0)
    f = np.float32
    anywhere = rng.randint(0, 2**32, 4_000_000, dtype=np.uint64).astype(np.uint32).view(f)
    k = np.arange(-360, 361)
    return np.concatenate([anywhere[np.isfinite(anywhere)], rng.uniform(-2, 2, 2_000_000).astype(f), (k/360.).astype(f),
                           k.astype(f)/f(360.), (k/2.).astype(f)/f(180.), np.arange(-16, 17).astype(f)/f(4.)])


def test_the_two_sincospi_agree_on_a_sweep():
    """Not a pin of either (CUDA's own is neither): the count of disagreements is what DESIGN 5 records. What IS asserted: they
    never differ by more than one unit in the last place of a value in [-1, 1], and they agree - exact 0 and +-1 - on the quarter
    turns, which is what lets the directed worlds put rays exactly through corners."""
    x = sincospi_arguments()
    (so, co), (sr, cr) = O.sincospi_many(x), reference.sincospi(x)
    differ = (_bits(so) != _bits(sr)) | (_bits(co) != _bits(cr))
    worst = max(float(np.abs(so.astype(np.float64) - sr).max()), float(np.abs(co.astype(np.float64) - cr).max()))
    print(f'sincospi sweep: {len(x)} arguments, {int(differ.sum())} disagreements, worst |difference| {worst:.3g}')
    assert worst <= 2.**-24
    q = np.arange(-16, 17).astype(np.float32)/np.float32(4.)
    (so, co), (sr, cr) = O.sincospi_many(q[::2]), reference.sincospi(q[::2])
    assert np.array_equal(so, sr) and np.array_equal(co, cr)
    assert set(np.abs(so).tolist()) <= {0., 1.} and np.array_equal(np.abs(so) + np.abs(co), np.ones_like(so))


# ---- toys and the known answer -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_envs,n_agents,res,fov,toy', [(1, 1, 8, 130, 'box'), (3, 1, 64, 130, 'box'), (2, 2, 64, 70, 'column')])
def test_toys(n_envs, n_agents, res, fov, toy):
    c, _ = util.plan_world(n_envs, n_agents, res, fov, toy=toy, device='cpu')
    pin(util.case_of(c, _moves(c, 7, (40., 4., 40., 4.))), min_collisions=toy == 'box')      # (the column stands in the open)


def test_known_answer_from_the_docs():
    """reference: docs/tutorials/minimal-env/index.rst:140-145 - box(5), agent at (3, 3), velocity (1000, 0) -> (5.8649, 3)."""
    c, _ = util.plan_world(2, 1, 64, 130, toy='box', device='cpu')
    c.agents.positions[:] = torch.as_tensor([3., 3.])
    c.agents.angles[:] = 0.
    move = (np.tile(np.float32([1000., 0.]), (2, 1, 1)), np.zeros((2, 1), np.float32))
    out = pin(util.case_of(c, [move]), min_collisions=2)
    np.testing.assert_allclose(out['agents']['positions'], np.tile([5.8649, 3.0], (2, 1, 1)), atol=5e-5)
    assert (out['agents']['velocity'] == 0).all()


def test_agents_see_each_other():
    """Rays that land on the other agent: the dynamic lighting path (kernels.cu:432-436)."""
    c, _ = util.plan_world(4, 2, 64, 70, toy='box', device='cpu')
    c.agents.positions[:] = torch.tensor([[2.5, 3.5], [4.5, 3.5]])
    c.agents.angles[:] = torch.tensor([0., 180.])
    case = util.case_of(c, [])
    out = pin(dict(case, moves=util.still(case)))
    assert ((out['indices'] >= 0) & (out['indices'] < 16)).any()


# ---- floorplans, across the GPU suite's instantiation families --------------------------------------------------------------

@pytest.mark.parametrize('n_envs,n_agents,res,fov,large', [
    (4, 1, 64, 130, False), (4, 4, 64, 130, False), (3, 4, 128, 70, False), (3, 3, 100, 90, False), (2, 2, 64, 170, False),
    (2, 1, 1, 90, False), (1, 1, 256, 130, True), (2, 4, 512, 70, False)])
def test_floorplans(n_envs, n_agents, res, fov, large):
    c, _ = util.plan_world(n_envs, n_agents, res, fov, seed=9 if large else 0, large=large, device='cpu')
    pin(util.case_of(c, _moves(c, 7, (40., 4., 40.))), min_collisions=1)


@pytest.mark.parametrize('n_envs,n_agents,res,fov,large', [(4, 4, 64, 130, False), (1, 1, 256, 130, True), (2, 4, 512, 70, False), (3, 2, 100, 160, False)])
def test_oblique_floorplans(n_envs, n_agents, res, fov, large):
    c, _ = util.oblique_world(n_envs, n_agents, res, fov, large, device='cpu')
    pin(util.case_of(c, _moves(c, 8, (40., 4., 40.))), min_collisions=1)


# ---- the GPU suite's directed worlds ---------------------------------------------------------------------------------------

def _standing(c):
    case = util.case_of(c, [])
    return dict(case, moves=util.still(case))


def test_hysteresis_band_adversarial():
    pin(_standing(util.hysteresis_band_world(device='cpu')))


def test_agent_wedged_between_coincident_walls():
    pin(_standing(util.wedged_agent_world(device='cpu')))


def test_stacks_of_coincident_walls():
    pin(_standing(util.coincident_stacks_world(device='cpu')))


@pytest.mark.parametrize('n_agents', [2, 4, 7])
def test_agents_meet_agents_whatever_their_relative_velocity(n_agents):
    """NaN and infinite positions and velocities included: they must come out of both sides alike."""
    out = pin(_standing(util.agents_meeting_agents_world(n_agents, device='cpu')), min_collisions=50)
    p = out['progress']
    assert ((p < 1) & (p > 0)).sum() > 5 and (p == 0).sum() > 50 and (p == 1).sum() > 50
    assert np.isnan(out['agents']['positions']).any()


def test_crawling_agents_meet_far_walls():
    out = pin(_standing(util.crawling_agents_world(device='cpu')), min_collisions=5)
    assert out['progress'][0, 0] == 0.


@pytest.mark.parametrize('n_agents', [1, 4, 6])
def test_walls_with_non_finite_coordinates(n_agents):
    out = pin(_standing(util.non_finite_walls_world(n_agents, device='cpu')), min_collisions=1)
    assert (out['progress'] == 1).any()


def test_more_than_64_lights_and_agents():
    rng = np.random.RandomState(0)
    c = util.many_lights_world(util.many_lights_geometries(rng), rng, device='cpu')
    out = pin(_standing(c))
    lit = (out['indices'] >= 0) & (out['indices'] < 24)
    assert all(lit[e].any() for e in range(4)), 'rays should land on agents in every env'
    c = util.crowd_world(rng, device='cpu')
    pin(util.case_of(c, _moves(c, 1, (3.,))), min_collisions=1)


def test_ragged_edge_cases():
    rng = np.random.RandomState(0)
    c = util.ragged_edge_world(rng, device='cpu')
    out = pin(util.case_of(c, util.random_moves((4, 2), rng, (5., 5.))))
    assert (out['screen'][0][out['indices'][0] >= 16] > 0).any()        # ambient light only, but not black


# ---- directed worlds for the rules that seeded plans never reach --------------------------------------------------------------

def test_rays_through_wall_endpoints_and_filter_clamps():
    """Every q.t here is an exact 0, 1/8, 1/4, 1/2, 3/4, 7/8 or 1: the ray lands on the wall under test, never on the backstop
    behind it, and the locations are the filter's clamps."""
    case = util.endpoint_case()
    out = pin(case, min_collisions=10)
    AF = 8
    backstop = np.array([w - 1 for w in case['scene']['lines_widths']])
    # (the last step walked the agents into the walls; the first one stood still)
    first = pin(dict(case, moves=case['moves'][:1]))
    idx, loc = first['indices'][:, 0, 0], first['locations'][:, 0, 0]
    assert (idx >= AF).all() and (idx < backstop).all(), 'a ray through an endpoint went on to the backstop'
    assert set(np.unique(loc).tolist()) == {0., .125, .25, .5, .75, .875, 1.}
    assert out['hits'] > 0


def test_rays_through_shared_corners_in_a_fan():
    for case in util.corner_fan_case():
        pin(case)


def test_rays_nearly_parallel_to_a_wall():
    """|U x V| is exact here: below 1e-3 the ray goes through the wall to the backstop, from 1e-3 on it lands."""
    case = util.near_parallel_case()
    out = pin(dict(case, moves=case['moves'][:1]))
    AF = 8
    lines = case['scene']['lines_vals'].reshape(-1, AF + 2, 2, 2)
    cross = np.abs(lines[:, AF, 1, 1] - lines[:, AF, 0, 1])
    assert np.array_equal(out['indices'][:, 0, 0] == AF, cross >= np.float32(1e-3))
    assert (cross >= np.float32(1e-3)).sum() >= 8 and (cross < np.float32(1e-3)).sum() >= 8
    pin(case, min_collisions=1)


def test_light_paths_that_graze_a_walls_end():
    """The fence is in the light's way up to s < .999 of the path and not from there on: both sides of it are in the case."""
    case = util.grazing_light_case()
    out = pin(case)
    widths = case['scene']['textures_widths'].reshape(len(case['scene']['lines_widths']), -1)
    start = np.concatenate([[0], widths.sum(1).cumsum()[:-1]]) + widths[:, :8].sum(1)
    texel = out['baked'][start + 1]             # texel 1 of the lit wall, the one behind the fence
    assert (texel == np.float32(.1)).sum() >= 8 and (texel > .2).sum() >= 8, texel


def test_walls_of_one_and_two_texels():
    pin(util.narrow_textures_case())


# ---- the recorded cases of tests/test_gpu_reference_pin.py --------------------------------------------------------------------

def test_recorded_cases_are_what_the_reference_and_the_oracle_give_today():
    """tests/golden/reference_kernels.npz holds inputs and the reference's outputs: both sides, run on the stored inputs, give the
    stored outputs bit for bit - the file is neither stale nor out of the oracle's reach."""
    import os
    cases = util.load_cases(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_kernels.npz'))
    assert len(cases) >= 18
    for name, g in cases.items():
        scene = {k[len('scene_'):]: g[k] for k in g if k.startswith('scene_')}
        scene.update(n_agents=int(g['n_agents']), baked_vals=None)
        agents = {k: g['agents_' + k] for k in reference.AGENT_FIELDS}
        config = tuple(g['config'])
        out = pin(dict(scene=scene, config=config, agents=agents, moves=[(agents['velocity'], agents['angvelocity'])]), min_hits=0)
        assert_same_bits(out['baked'], g['baked'], f'{name}: baked')
        assert_same_bits(out['progress'], g['progress'], f'{name}: progress')
        for k in reference.AGENT_FIELDS:
            assert_same_bits(out['agents'][k], g['after_' + k], f'{name}: {k}')
        for k in PLANES:
            assert_same_bits(out[k], g[k], f'{name}: {k}')
