"""The step kernels' edge constructions on the CPU: every counted fact tests/test_gpu_step_edges.py relies on - the
kernels' thresholds as their sources state them, the margins of every (row, agent) pair, how many pairs each list receives window
by window - and the host statements at the same tables and wild actions: no kernel is launched here."""
import os
import re

import numpy as np
import pytest

from tests import step_edges as se
from tests.rollout_rule import FIELDS, host_rollouts, rollout_rule
from tests.scenario_rule import host_scenarios
from tests.slide_rule import FIELDS as SLIDE_FIELDS, host_slide, world as slide_world
from tests.util import assert_bits


def test_the_models_thresholds_are_the_sources():
    c = se.constants()
    assert c == {k: getattr(se, k) for k in c}
    assert c['PHYS_PAIRS'] - c['PHYS_FEW']*se.WAVE == 64 and c['ROLL_PAIRS'] - se.WAVE == 192
    # the rules the models restate, as the sources spell them (spacing aside): the table in a register, and the four flushes
    squeezed = {f: re.sub(r'\s+', '', open(os.path.join(se.ROOT, 'megastep_amd', 'csrc', 'kernels', f)).read()) for f in ('step.h', 'physics.h')}
    assert 'small(3*n_actions<=WAVE)' in squeezed['step.h'] and 'if(cnt>cap-WAVE)flush();' in squeezed['step.h']
    assert 'small_table=3*mv.n_actions<=WAVE;' in squeezed['physics.h']
    assert squeezed['physics.h'].count('if(cnt>PHYS_PAIRS-WAVE)flush();') == 2          # (the gridded deal, the sweep agent by agent)
    assert squeezed['physics.h'].count('if(cnt>PHYS_PAIRS-PHYS_FEW*WAVE)flush();') == 1  # (the sweep of a few agents)
    assert max(T for T in range(1, 65) if 3*T <= se.WAVE) == 21 and {21, 22} <= set(se.TABLE_SIZES)


@pytest.mark.parametrize('T', se.TABLE_SIZES)
def test_tables_and_actions(T):
    for turning in (True, False):
        t = se.table(T, turning)
        assert t.shape == (T, 3) and t.dtype == np.float32 and len({r.tobytes() for r in t}) == T and not t[0].any()
        assert (t[1:, 2] != 0).any() == (turning and T >= 5)
        speed = np.hypot(t[1:, 0], t[1:, 1])
        assert ((speed >= 2.99) & (speed <= 4.01)).all()
    a = se.actions((5, 3), T)
    assert set(se.must_rows(T)) <= set(a.reshape(-1)) and a.min() >= 0 and a.max() < T
    if T > 3:
        w, want, narrowed = se.wild(a, T)
        assert set(se.wild_values(T)) <= set(w.reshape(-1).tolist()) and set(se.must_rows(T)) <= set(w.reshape(-1))
        assert want.min() == 0 and want.max() == T - 1 and (want[(w >= 0) & (w < T)] == w[(w >= 0) & (w < T)]).all()
        at = w == 2**32 + 3
        assert (want[at] == T - 1).all() and (narrowed[at] == 3).all()


@pytest.mark.parametrize('name', list(se.SWEEPS))
def test_the_sweeps_lists_window_by_window(name):
    for heading in se.HEADINGS:
        se.check_sweep(name, heading)


@pytest.mark.parametrize('name', list(se.GRIDDED))
def test_the_deals_lists_window_by_window_if_the_near_lists_are_the_rings(name):
    for heading in se.HEADINGS:
        se.check_gridded(name, heading=heading)


@pytest.mark.parametrize('name', list(se.ROLLED))
def test_the_rollouts_list_window_by_window(name):
    se.check_rolled(name)
    ros, spec = se.rolled(name)
    assert set(se.rolled_plans(name).reshape(-1)) <= set(range(1, 7)) and len(ros.rows) == len(spec['order']) + 4


def test_a_list_one_slot_looser_would_overflow_where_these_do_not():
    """What the constructions are for: with `cnt > cap - 64 + 1` in place of `cnt > cap - 64`, 'walls-129' would write slot 256 of
    256 - the model refuses it."""
    ros, spec = se.rolled('walls-129')
    tasks = [se.task_of(ros.positions[0], se.straight()[se.rolled_plans('walls-129')[k, 0]][:2]) for k in range(spec['K'])]
    kept = se.rollout_windows(se.in_reach(tasks, ros.rows))
    se.list_trace(kept, se.ROLL_PAIRS)
    with pytest.raises(AssertionError):
        _looser(kept, se.ROLL_PAIRS)


def _looser(kept, cap):
    cnt = 0
    for k in kept:
        if cnt > cap - se.WAVE + 1:
            cnt = 0
        cnt += k
        assert cnt <= cap


def _oracle_progress(oracle, ros, heading):
    from tests.slide_rule import plain_rule
    return plain_rule(_rosette_world(ros, ros.velocity(heading)), se.RADIUS, se.FPS)['progress']


@pytest.mark.parametrize('name', list(se.SWEEPS) + list(se.GRIDDED))
def test_the_rosettes_stop_some_agents_and_not_others(oracle, name):
    """Over the headings the GPU module launches: the comparisons there mean something."""
    ros = (se.sweep(name) if name in se.SWEEPS else se.gridded(name))[0]
    progress = np.stack([_oracle_progress(oracle, ros, heading) for heading in se.HEADINGS])
    assert (progress < 1).any() and (progress == 1).any()
    slid = [host_slide(_rosette_world(ros, ros.velocity(heading)), se.RADIUS, se.FPS) for heading in se.HEADINGS]
    assert any((s['slid'] > 0).any() for s in slid) and any((s['stopped'] > 0).any() for s in slid)


def test_the_packed_worlds_rosette_slides_and_stops():
    ros = se.Rosette('r'*20 + 'f'*4, [0]*4)
    slid = [host_slide(_rosette_world(ros, ros.velocity(heading)), se.RADIUS, se.FPS) for heading in se.HEADINGS]
    assert any((s['slid'] > 0).any() for s in slid) and any((s['stopped'] > 0).any() for s in slid)


@pytest.mark.parametrize('name', list(se.ROLLED))
def test_the_rolled_rosettes_stop_some_candidates_and_not_others(name):
    ros, _ = se.rolled(name)
    got = host_rollouts(_rosette_world(ros), se.rolled_plans(name), se.straight(), 0., None, se.RADIUS, se.FPS)
    assert (got['stops'] > 0).any() and (got['stops'] == 0).any()


def test_the_spots():
    rows, spots = se.spots_check()
    assert len(rows) == 4 + sum(n or 0 for n in se.SPOT_ROWS) and se.ROLL_AHEAD == 4 and set(se.SPOT_ROWS[:-1]) == {0, 1, 3, 4, 5}
    world, table = slide_world([rows], spots[None]), se.straight()
    got = host_rollouts(world, 1 + se.actions((1, len(spots), 8, 3), 6, seed=1), table, 0., None, se.RADIUS, se.FPS)
    assert (got['stops'][0, 1:5] > 0).any() and (got['stops'] == 0).any()
    got = host_scenarios(world, 1 + se.actions((1, 4, len(spots), 3), 6, seed=2), table, 0., se.RADIUS, se.FPS)
    assert (got['stops'][0, :, 1:5] > 0).any() and (got['stops'] == 0).any()


def _rosette_world(ros, velocity=None):
    return slide_world([ros.rows], ros.positions[None], velocity=None if velocity is None else velocity[None])


@pytest.mark.parametrize('T', se.TABLE_SIZES)
def test_the_host_rollouts_at_every_table_size_against_the_rule_over_the_oracle(oracle, T):
    """Heading 0 and a table that never turns: the rule's libm and the statement's agree there (test_gpu_rollouts)."""
    ros = se.Rosette('r'*12 + 'f'*4, [0, 0])
    world = _rosette_world(ros)
    world['positions'][0, 1] += np.float32([.5, .3])
    table, plans = se.straight(T), se.actions((1, 2, 6, 3), T, seed=T)
    for others in (None, 'rest'):
        want = rollout_rule(world, plans, table, .875, others, se.RADIUS, se.FPS)
        got = host_rollouts(world, plans, table, .875, others, se.RADIUS, se.FPS)
        for k in FIELDS:
            assert_bits(got[k], want[k], k)
    assert T == 1 or ((want['stops'] > 0).any() and (want['stops'] == 0).any())


@pytest.mark.parametrize('T', [21, 22])
def test_the_host_statements_clamp_wild_actions_in_64_bits(T):
    """ms_host_rollouts, ms_host_scenarios (joint and focal, the base plans too) and ms_host_slide on actions far outside the
    table: what the clamped actions give, and not what actions narrowed to 32 bits first would."""
    ros = se.Rosette('r'*12 + 'f'*4, [0, 0])
    world = _rosette_world(ros)
    world['positions'][0, 1] += np.float32([.5, .3])
    table = se.straight(T)
    differs = 0
    plans, clamped, narrowed = se.wild(se.actions((1, 2, 6, 3), T, seed=1), T)
    runs = [lambda a: host_rollouts(world, a, table, .875, 'rest', se.RADIUS, se.FPS),
            lambda a: host_scenarios(world, a.transpose(0, 2, 1, 3), table, .875, se.RADIUS, se.FPS),
            lambda a: host_scenarios(world, a[:, :, :4], table, .875, se.RADIUS, se.FPS, base=a[:, :, 4]),
            lambda a: host_scenarios(world, clamped[:, :, :4], table, .875, se.RADIUS, se.FPS, base=a.reshape(1, 2, -1)[:, :, 4:7])]
    for run in runs:
        got, want, other = run(plans), run(clamped), run(narrowed)
        for k in FIELDS:
            assert_bits(got[k], want[k], k)
        differs += any((other[k] != want[k]).any() for k in ('positions', 'velocity'))
    assert differs >= 3
    acts, clamped, narrowed = se.wild(se.actions((3, 4), T, seed=2), T)
    ros = se.Rosette('r'*12 + 'f'*4, [0]*4)
    world = dict(walls=[ros.rows]*3, **{k: np.repeat(v, 3, 0) for k, v in _rosette_world(ros).items() if k != 'walls'})
    world['positions'] += np.float32([[0, 0], [.6, 0], [0, .6], [.6, .6]])                # (apart: nobody stands in anybody)
    got, want, other = (host_slide(world, se.RADIUS, se.FPS, movement=(a, table, .875)) for a in (acts, clamped, narrowed))
    for k in SLIDE_FIELDS:
        assert_bits(got[k], want[k], k)
    assert (other['positions'] != want['positions']).any() and (want['progress'] < 1).any() and (want['progress'] == 1).any()
