"""Percepts on the host: ms_host_percepts - csrc/kernels/percept.h over navview.h's predicates, through the kernel's cull, its
boxes of 64 points and both wall paths - held to EQUALITY with tests/percept_rule.py in every output; the rule held to float64
geometry written apart from it; hand-made worlds with known answers; the C-ABI's declaration, layout and refusals; the Python
layer's refusals; `Tag.books` and `modules.Percepts.pack` on hand-filled tensors. No GPU: what is compared is the text every lane
of the kernel evaluates, swept serially."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.percept_rule import KEYS, blank, hand_shape, host, percept_rule, plan_percepts, plan_rule, same
from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import F
from tests.test_navview_host import CONE, _crossings, box_walls, cos_half_of, view_rule

INF = float('inf')


# ---------------------------------------------------------------------------------------------------------------------
# the six plans
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('capacity', [0, 8])
@pytest.mark.parametrize('K', [0, 1, 4, 16])
@pytest.mark.parametrize('cone', [False, True])
@pytest.mark.parametrize('R', [4., 10.])
def test_the_host_instantiation_is_the_rule_on_the_six_plans(R, cone, K, capacity):
    """Every output, staged walls and - with 8 rows of room, fewer than any env keeps - the walk over all of them."""
    w = plan_percepts()
    kw = dict(headings=w.headings, cos_half=w.cos_half) if cone else {}
    want = plan_rule(R, cone, K)
    same(host(w.walls, w.eyes, w.points, R, K, capacity=capacity, **kw), want)
    assert want['counts'].sum() > 0 and (want['counts'] < 200).all()
    if capacity:
        for n in range(6):
            lo, hi = np.minimum(w.walls[n][:, :2], w.walls[n][:, 2:]), np.maximum(w.walls[n][:, :2], w.walls[n][:, 2:])
            assert max(((lo <= p + F(R)) & (hi >= p - F(R))).all(1).sum() for p in w.eyes[n]) > capacity     # (a box inside the kernel's)


def test_the_six_plans_see_and_hide_enough_and_list_in_order():
    want = plan_rule(10., False, 16)
    vis = want['visible'].astype(bool)
    in_range = np.isfinite(percept_squares(plan_percepts(), 10.))
    print('visible', int(vis.sum()), 'of', int(in_range.sum()), 'in-range pairs; counts', want['counts'].reshape(-1).tolist())
    assert vis.sum() >= 200 and (in_range & ~vis).sum() >= 1000
    d = want['near_distances']
    assert (np.diff(np.minimum(d, F(3e38)), axis=-1) >= 0).all() and (want['counts'] > 16).any() and (want['counts'] < 16).any()
    listed = want['nearest'] >= 0
    assert np.array_equal(listed.sum(-1), np.minimum(want['counts'], 16))
    n, e, k = np.nonzero(listed)
    p = want['nearest'][n, e, k]
    assert vis[n, e, p].all() and np.array_equal(want['near_offsets'][n, e, k], want['offsets'][n, e, p])
    assert np.array_equal(d[n, e, k], np.sqrt(want['squares'][n, e, p]))


def percept_squares(w, R):
    """(6, 2, 200): rr where the pair is in range, +inf elsewhere - the rule's candidates without a cone."""
    out = np.full((6, 2, 200), np.inf, F)
    for n in range(6):
        for e in range(2):
            ok, _, _, rr = percept_rule.candidates(w.eyes[n, e], w.points[n], R)
            out[n, e] = np.where(ok, rr, np.inf)
    return out


def test_no_wall_is_seen_through_and_nothing_in_plain_sight_is_hidden():
    """The rule against float64, written apart from it: no visible pair crosses a wall at u in [1e-6, 1 - 1e-6], every hidden in-range
    pair crosses one at u in [-1e-6, 1 + 1e-6] - without exception, in either direction."""
    w = plan_percepts()
    want = plan_rule(10., False, 16)
    in_range = np.isfinite(percept_squares(w, 10.))
    through = spurious = seen = hidden = 0
    for n in range(6):
        for e in range(2):
            vis = want['visible'][n, e].astype(bool)
            seen += int(vis.sum()); hidden += int((in_range[n, e] & ~vis).sum())
            through += int(_crossings(w.eyes[n, e], w.points[n][vis], w.walls[n], 1e-6, 1 - 1e-6).sum())
            spurious += int((~_crossings(w.eyes[n, e], w.points[n][in_range[n, e] & ~vis], w.walls[n], -1e-6, 1 + 1e-6)).sum())
    assert seen >= 200 and hidden >= 1000, (seen, hidden)
    assert through == 0 and spurious == 0, (through, spurious)


# ---------------------------------------------------------------------------------------------------------------------
# hand-made worlds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [1, 63, 64, 65, 200, 1024])
@pytest.mark.parametrize('E', [1, 4, 5, 64])
def test_shapes_round_the_wave_and_the_workgroup(E, P):
    """Points short of, at and beyond a wave's 64 and at the most a call takes; eyes short of, at and beyond a workgroup's four
    waves and at the most; K of 0, 1 and 16, with and without the cone, valid, pairs as (E, P) and as (N, E, P); both wall paths."""
    w = hand_shape(E, P)
    for K, cone, gated, capacity in ((16, False, False, 0), (1, True, True, 0), (0, True, False, 3), (16, False, True, 3)):
        kw = dict(headings=w.headings, cos_half=w.cos_half) if cone else {}
        if gated:
            kw.update(valid=w.valid, pairs=w.pairs if K == 1 else w.pairs[None].copy())
        want = percept_rule.call(w.walls, w.eyes, w.points, 6., K, **kw)
        same(host(w.walls, w.eyes, w.points, 6., K, capacity=capacity, **kw), want)
        if P >= 63 and not cone:
            assert 0 < want['counts'].sum() < E*P


def _one(eye, points, R=20., K=4, walls=None, **kw):
    walls = [box_walls()] if walls is None else walls
    eyes, points = np.array([[eye]], F), np.array([points], F)
    want = percept_rule.call(walls, eyes, points, R, K, **kw)
    for capacity in (0, 2):
        same(host(walls, eyes, points, R, K, capacity=capacity, **kw), want)
    return want


def test_ties_go_to_the_lower_index_and_a_point_on_the_eye_is_seen():
    # two points at the same place, two mirror images at equal rr, the eye's own spot
    want = _one((2, 2), [(3, 2.5), (1, 1), (3, 1.5), (1, 1), (2, 2), (3, 2.5)], K=6)
    assert want['visible'][0, 0].all() and want['counts'][0, 0] == 6
    assert want['nearest'][0, 0].tolist() == [4, 0, 2, 5, 1, 3]
    assert want['squares'][0, 0, 0] == want['squares'][0, 0, 2] == F(1.25) and want['near_distances'][0, 0, 0] == 0
    assert want['near_offsets'][0, 0, 0].tolist() == [0, 0] and want['near_distances'][0, 0, 1] == np.sqrt(F(1.25))
    # under a cone too: a point on the eye is in every cone
    want = _one((2, 2), [(2, 2), (1, 2)], K=2, headings=np.array([[[3, 0]]], F), cos_half=cos_half_of(CONE))
    assert want['visible'][0, 0].tolist() == [1, 0] and want['nearest'][0, 0].tolist() == [0, -1]


def test_more_asked_for_than_seen():
    want = _one((1, 2), [(2, 2), (6, .5), (3, 3)], K=16)                 # ((6, .5) is behind the partition)
    assert want['visible'][0, 0].tolist() == [1, 0, 1] and want['nearest'][0, 0].tolist() == [0, 2] + [-1]*14
    assert np.isnan(want['near_offsets'][0, 0, 2:]).all() and np.isinf(want['near_distances'][0, 0, 2:]).all()
    assert np.isnan(want['offsets'][0, 0, 1]).all() and want['squares'][0, 0, 1] == INF
    want = _one((1, 2), [(2, 2)], K=16)                                  # (sixteen of one)
    assert want['nearest'][0, 0].tolist() == [0] + [-1]*15
    want = _one((1, 2), [(6, .5)], K=16)                                 # (sixteen of none)
    assert want['counts'][0, 0] == 0 and (want['nearest'] == -1).all()


def test_the_range_is_closed():
    at = _one((0, 0), [(3, 4)], R=5.)
    assert at['visible'][0, 0, 0] == 1 and at['squares'][0, 0, 0] == 25 and at['near_distances'][0, 0, 0] == 5
    short = _one((0, 0), [(3, 4)], R=float(np.nextafter(F(5), F(0))))
    assert short['visible'][0, 0, 0] == 0 and short['counts'][0, 0] == 0


def test_a_sight_line_through_a_shared_vertex_is_blocked():
    """A jamb from the lower door post, (4, 1.5) to (5, 1.5): the sight line from (3, 1) to (5, 2) passes exactly through the vertex
    the jamb and the partition share, and either wall alone blocks it; a point a little higher is seen through the door."""
    walls = np.concatenate([box_walls(), np.array([(4, 1.5, 5, 1.5)], F)])
    want = _one((3, 1), [(5, 2), (5, 2.25), (3.5, 1.25)], walls=[walls])
    assert want['visible'][0, 0].tolist() == [0, 1, 1]
    each = view_rule.blocks(3, 1, [F(5)], [F(2)], walls)[0]
    assert each.tolist() == [False]*5 + [True, False, True]


def test_nan_points_nan_eyes_and_headings_without_a_length():
    nan = np.nan
    want = _one((2, 2), [(nan, 2), (3, nan), (3, 2), (np.inf, 2)])
    assert want['visible'][0, 0].tolist() == [0, 0, 1, 0] and want['nearest'][0, 0].tolist() == [2, -1, -1, -1]
    for eye in ((nan, 2), (2, np.inf)):
        want = _one(eye, [(3, 2), (2, 2)])
        assert want['counts'][0, 0] == 0 and not want['visible'].any() and (want['nearest'] == -1).all() and np.isinf(want['squares']).all()
    for heading in ((0, 0), (0, -0.), (nan, 1), (np.inf, 0)):
        want = _one((2, 2), [(3, 2), (2, 2)], headings=np.array([[heading]], F), cos_half=cos_half_of(CONE))
        assert want['counts'][0, 0] == 0 and not want['visible'].any()
    # the NaN row of box_walls blocks nothing: the near room is in plain sight
    want = _one((1, 2), [(1, 1), (3, 3), (2, .5)])
    assert want['visible'][0, 0].all() and np.isnan(box_walls()[3]).any()


def test_valid_pairs_and_a_masked_off_eye():
    w = hand_shape(5, 65)
    pairs = w.pairs.copy()
    pairs[2] = 0                                                          # (an eye without an interest)
    valid = w.valid.copy()
    valid[0, :3] = 0
    mask = np.array([[1, 0, 1, 1, 0]], np.uint8)
    for form in (pairs, pairs[None].copy()):
        want = percept_rule.call(w.walls, w.eyes, w.points, 6., 4, valid=valid, pairs=form, mask=mask)
        same(host(w.walls, w.eyes, w.points, 6., 4, valid=valid, pairs=form, mask=mask), want)
    assert want['counts'][0].tolist()[2] == 0 and not want['visible'][0, :, :3][[0, 2, 3]].any()
    plain = blank(1, 5, 65, 4)
    for key in KEYS:                                                      # (a masked-off eye keeps the sentinel in every output)
        assert np.array_equal(want[key][0, 1], plain[key][0, 1]) and np.array_equal(want[key][0, 4], plain[key][0, 4])
        assert not np.array_equal(want[key][0, 0], plain[key][0, 0])
    assert want['counts'][0, 0] > 0 and want['counts'][0, 3] > 0
    # every eye masked off: nothing is written at all
    none = host(w.walls, w.eyes, w.points, 6., 4, mask=np.zeros((1, 5), np.uint8))
    same(none, plain)


def test_outputs_that_are_not_wanted_are_not_written():
    w = hand_shape(4, 65)
    want = percept_rule.call(w.walls, w.eyes, w.points, 6., 4)
    for fields in (('counts',), ('nearest',), ('visible', 'near_distances'), ('squares', 'offsets', 'near_offsets')):
        got = host(w.walls, w.eyes, w.points, 6., 4, fields=fields)
        same(got, want, fields)
        same(got, blank(1, 4, 65, 4), tuple(k for k in KEYS if k not in fields))


# ---------------------------------------------------------------------------------------------------------------------
# header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
FIELDS = ('n_eyes', 'n_points', 'n_nearest', 'eyes', 'headings', 'points', 'valid', 'pairs', 'pairs_shape', 'mask', 'max_range', 'cos_half',
          'visible', 'squares', 'offsets', 'counts', 'nearest', 'near_offsets', 'near_distances')


def test_the_header_declares_the_call_and_the_abi_version_stays():
    from megastep_amd import _lib
    assert 'ms_percepts' in declared_symbols(('megastep_hip.h',)) and 'ms_host_percepts' in declared_symbols(('megastep_hip_test.h',))
    assert {'ms_percepts', 'ms_host_percepts'} <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert hasattr(handle, 'ms_percepts') and hasattr(handle, 'ms_host_percepts')


def test_the_mirror_has_the_c_layout():
    import subprocess
    import tempfile
    from megastep_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "megastep_hip.h"\nint main(){printf("%zu", sizeof(MsPercepts));' +
           ''.join(f'printf(" %zu", offsetof(MsPercepts, {f}));' for f in FIELDS) + '}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')])
        got = list(map(int, subprocess.check_output([os.path.join(d, 't')]).split()))
    assert [f for f, _ in _lib.MsPercepts._fields_] == list(FIELDS)
    assert got == [ctypes.sizeof(_lib.MsPercepts)] + [getattr(_lib.MsPercepts, f).offset for f in FIELDS]


def test_bad_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    scenery = _lib.MsScenery(n_envs=2, n_agents=1, n_model=1, lines_vals=fake, lines_widths=fake, lines_starts=fake, model=fake)
    ref = ctypes.byref
    good = dict(n_eyes=2, n_points=3, n_nearest=4, eyes=fake, headings=fake, points=fake, valid=fake, pairs=fake, pairs_shape=1, mask=fake,
                max_range=10., cos_half=.5, visible=fake, squares=fake, offsets=fake, counts=fake, nearest=fake, near_offsets=fake, near_distances=fake)
    nothing = dict(visible=None, squares=None, offsets=None, counts=None, nearest=None, near_offsets=None, near_distances=None)
    bad_ones = (dict(eyes=None), dict(points=None), dict(n_eyes=0), dict(n_eyes=-1), dict(n_eyes=65), dict(n_points=0), dict(n_points=1025),
                dict(n_nearest=-1), dict(n_nearest=17), nothing, dict(pairs_shape=0), dict(pairs_shape=3), dict(pairs_shape=-1),
                dict(pairs=None), dict(pairs=None, pairs_shape=2), dict(max_range=0.), dict(max_range=-1.), dict(max_range=INF),
                dict(max_range=float('nan')), dict(cos_half=1.5), dict(cos_half=-1.01), dict(cos_half=float('nan')), dict(eyes=68),
                dict(headings=68), dict(points=68), dict(offsets=68), dict(near_offsets=68), dict(squares=66), dict(counts=66),
                dict(nearest=66), dict(near_distances=66))
    for bad in bad_ones:
        spec = _lib.MsPercepts(**{**good, **bad})
        assert h.ms_percepts(ref(scenery), ref(spec), None) == -1, bad
        assert h.ms_host_percepts(ref(spec), 2, fake, fake, 0) == -1, bad
    spec = _lib.MsPercepts(**good)
    assert h.ms_percepts(None, ref(spec), None) == -1 and h.ms_percepts(ref(scenery), None, None) == -1
    assert h.ms_percepts(ref(_lib.MsScenery()), ref(spec), None) == -1
    assert h.ms_host_percepts(None, 2, fake, fake, 0) == -1 and h.ms_host_percepts(ref(spec), 0, fake, fake, 0) == -1
    assert h.ms_host_percepts(ref(spec), 2, None, fake, 0) == -1 and h.ms_host_percepts(ref(spec), 2, fake, None, 0) == -1
    assert h.ms_host_percepts(ref(spec), 2, fake, fake, h.ms_host_nav_view_capacity() + 1) == -1
    assert h.ms_host_percepts(ref(spec), 2, fake, fake, -1) == -1
    # a cone's cosine is not looked at without headings; one output is enough
    w = hand_shape(4, 65)
    out = host(w.walls, w.eyes, w.points, 6., 4, cos_half=7., fields=('counts',))
    same(out, percept_rule.call(w.walls, w.eyes, w.points, 6., 4), ('counts',))


def test_the_python_call_refuses_what_it_cannot_do():
    from megastep_amd import cuda, percepts, scene, toys
    assert cuda.percepts is percepts.percepts and cuda.Percepts is percepts.Percepts and cuda.PERCEPT_FIELDS == KEYS
    assert (cuda.PERCEPT_MAX_EYES, cuda.PERCEPT_MAX_POINTS, cuda.PERCEPT_MAX_NEAREST) == (64, 1024, 16)
    scenery = scene.scenery([toys.box(), toys.box()], 1, device='cpu', bake=False)
    points, eyes = torch.zeros((2, 3, 2)), torch.zeros((2, 2, 2))
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.percepts(scenery, points, eyes=eyes)      # (CPU tensors)
    with pytest.raises(RuntimeError, match='points and eyes, or agents'):
        cuda.percepts(scenery, points)
    for bad in (dict(points=torch.zeros((3, 3, 2))), dict(points=torch.zeros((2, 3, 3))), dict(eyes=torch.zeros((2, 2, 3))), dict(eyes=torch.zeros((1, 2, 2)))):
        with pytest.raises(RuntimeError, match=r'\(N, P, 2\)'):
            cuda.percepts(scenery, **{**dict(points=points, eyes=eyes), **bad})
    with pytest.raises(RuntimeError, match='dtype'):
        cuda.percepts(scenery, points.double(), eyes=eyes)
    for bad in (dict(points=torch.zeros((2, 1025, 2))), dict(points=torch.zeros((2, 0, 2))), dict(eyes=torch.zeros((2, 65, 2)))):
        with pytest.raises(RuntimeError, match='1 to 1024 points and 1 to 64 eyes'):
            cuda.percepts(scenery, **{**dict(points=points, eyes=eyes), **bad})
    for bad in (17, -1, 2.5, None):
        with pytest.raises(RuntimeError, match='k must be'):
            cuda.percepts(scenery, points, eyes=eyes, k=bad)
    for bad in (0, -1., INF, float('nan'), 'far'):
        with pytest.raises(RuntimeError, match='max_range'):
            cuda.percepts(scenery, points, eyes=eyes, max_range=bad)
    for kw in (dict(headings=eyes), dict(fov=90.)):
        with pytest.raises(RuntimeError, match='go together'):
            cuda.percepts(scenery, points, eyes=eyes, **kw)
    with pytest.raises(RuntimeError, match='headings must be'):
        cuda.percepts(scenery, points, eyes=eyes, headings=points, fov=90.)
    for bad in (0, -1., 361., float('nan'), 'wide'):
        with pytest.raises(RuntimeError, match='fov'):
            cuda.percepts(scenery, points, eyes=eyes, headings=eyes, fov=bad)
    for name, bad in (('valid', torch.ones((2, 2), dtype=torch.bool)), ('valid', torch.ones((2, 3))), ('pairs', torch.ones((3, 2), dtype=torch.bool)),
                      ('pairs', torch.ones((2, 2, 3), dtype=torch.int32)), ('mask', torch.ones((2, 3), dtype=torch.bool)), ('mask', torch.ones(4, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match=name + ' must be'):
            cuda.percepts(scenery, points, eyes=eyes, **{name: bad})
    for bad in (('visible', 'seen'), (), ('distances',)):
        with pytest.raises(RuntimeError, match='fields must be'):
            cuda.percepts(scenery, points, eyes=eyes, fields=bad)
    from megastep_amd import core
    agents = core._init_agents(2, 1, 'cpu')
    with pytest.raises(RuntimeError, match='agents= stands for'):
        cuda.percepts(scenery, eyes=eyes, agents=agents)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.percepts(scenery, agents=agents, fov=130., k=0)


# ---------------------------------------------------------------------------------------------------------------------
# what is built on it: the module's packing and Tag's books, pure torch
# ---------------------------------------------------------------------------------------------------------------------
def test_the_percepts_module_packs_the_nearest_in_the_agents_frame():
    from megastep_amd import modules
    nan = float('nan')
    R = 10.
    angles = torch.tensor([[0., 90.]])
    counts = torch.tensor([[2, 0]], dtype=torch.int32)
    near_offsets = torch.tensor([[[[3., 4.], [0., -5.], [nan, nan]], [[nan, nan]]*3]])
    near_distances = torch.tensor([[[5., 5., INF], [INF]*3]])
    obs = modules.Percepts.pack(counts, near_offsets, near_distances, angles, R)
    assert obs.shape == (1, 2, 3, 4) and obs.dtype == torch.float32
    assert torch.allclose(obs[0, 0], torch.tensor([[1., .3, .4, .5], [1., 0., -.5, .5], [0., 0., 0., 0.]]), atol=1e-6)
    assert (obs[0, 1] == 0).all()                                        # (a seeker that sees nothing: zeros, no NaN)
    # a quarter turn to the left: what lay ahead in the world lies to the right
    turned = modules.Percepts.pack(counts, near_offsets, near_distances, torch.tensor([[90., 90.]]), R)
    assert torch.allclose(turned[0, 0, 0], torch.tensor([1., .4, -.3, .5]), atol=1e-6)
    # the rotation is to_local_frame's arithmetic, bit for bit
    angles = torch.tensor([[33., -140.]])
    counts = torch.tensor([[3, 3]], dtype=torch.int32)
    offs = torch.as_tensor(np.random.RandomState(0).uniform(-5, 5, (1, 2, 3, 2)).astype(F))
    dist = offs.norm(dim=-1)
    got = modules.Percepts.pack(counts, offs, dist, angles, R)
    assert torch.equal(got[..., 1:3], modules.to_local_frame(angles[..., None], offs)/R) and torch.equal(got[..., 3], dist/R)


def test_tag_books_on_hand_filled_tensors():
    from megastep_amd.demo import Tag
    # two seekers (0, 1) and three hiders (2, 3, 4): 2 is tagged by both at once, 3 is seen but out of range, 4 is unseen;
    # seeker 1 also sees seeker 0 next to it, which is nobody's business
    roles = torch.tensor([True, True, False, False, False])
    visible = torch.zeros((1, 5, 5), dtype=torch.uint8)
    squares = torch.full((1, 5, 5), INF)
    for s, h, rr in ((0, 2, .81), (1, 2, 1.), (0, 3, 9.), (1, 0, .01), (2, 0, .81), (4, 3, .04)):
        visible[0, s, h], squares[0, s, h] = 1, rr
    reward, tagged = Tag.books(visible, squares, roles, 1., .01)
    assert tagged.dtype == torch.bool and tagged.tolist() == [[False, False, True, False, False]]
    assert torch.allclose(reward, torch.tensor([[1., 1., -1., 0., .01]]))
    # a shorter reach: only seeker 0 tags
    reward, tagged = Tag.books(visible, squares, roles, .95, .01)
    assert torch.allclose(reward, torch.tensor([[1., 0., -1., 0., .01]])) and tagged.tolist() == [[False, False, True, False, False]]
    # a seeker that sees nothing earns nothing, and the hiders their bonus; a seeker tags two at once
    reward, tagged = Tag.books(torch.zeros_like(visible), squares, roles, 1., .25)
    assert torch.allclose(reward, torch.tensor([[0., 0., .25, .25, .25]])) and not tagged.any()
    visible[0, 0, 3], squares[0, 0, 3] = 1, .5
    reward, tagged = Tag.books(visible, squares, roles, 1., .01)
    assert torch.allclose(reward, torch.tensor([[2., 1., -1., -1., .01]])) and tagged.tolist() == [[False, False, True, True, False]]
