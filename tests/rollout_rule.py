"""The rollouts' rule (MsRollouts) as a loop over candidates and steps around the CPU oracle's physics step, and
the host statement ms_host_rollouts driven env by env: what tests/test_rollout_host.py holds against each other and
tests/test_gpu_rollouts.py holds the kernel to. A world here is plain numpy: ``walls`` (one (W, 4) float32 array per env: the
static rows), and the agents' ``positions`` (N, A, 2), ``angles`` (N, A), ``velocity`` (N, A, 2), ``angvelocity`` (N, A)."""
import ctypes as C
import numpy as np
from oracle import oracle as O

FIELDS = ('positions', 'angles', 'velocity', 'angvelocity', 'progress', 'stops', 'first_stop', 'trail')
_f = np.float32


def world_of(core):
    """A Core (on any device) as a world."""
    sc = core.scenery
    AF = sc.n_agents*sc.model.shape[0]
    lines = sc.lines.vals.detach().cpu().numpy().reshape(-1, 4)
    starts, ends = sc.lines.starts.cpu().numpy(), sc.lines.ends.cpu().numpy()
    n = lambda t: t.detach().cpu().numpy().copy()
    a = core.agents
    return dict(walls=[lines[s + AF:e].copy() for s, e in zip(starts, ends)], positions=n(a.positions), angles=n(a.angles),
                velocity=n(a.velocity), angvelocity=n(a.angvelocity))


def host_move_velocity(keep, ang, delta, v, w):
    """ms_host_move_velocity: the movement prologue with the host libm's sine and cosine."""
    from megastep_amd import _lib
    v = np.array(v, _f)
    w = C.c_float(float(w))
    d = np.ascontiguousarray(delta, _f)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    _lib.lib().ms_host_move_velocity(float(keep), float(ang), fp(d), fp(v), C.byref(w))
    return v, _f(w.value)


def _oracle_scene(walls, n_agents, n_model=4):
    """One env with these static rows behind n_agents*n_model agent rows, which the physics step never reads."""
    rows = np.concatenate([np.zeros((n_agents*n_model, 4), _f), np.asarray(walls, _f).reshape(-1, 4)])
    return O.Scene(dict(n_agents=n_agents, model=np.zeros((n_model, 2, 2), _f), lights_vals=np.ones((1, 3), _f), lights_widths=[1],
                        lines_vals=rows, lines_widths=[len(rows)], textures_vals=np.ones((len(rows), 3), _f),
                        textures_widths=np.ones(len(rows), np.int32)))


def _plan(actions, n, a, k):
    return actions[k] if actions.ndim == 2 else actions[n, a, k]


def _empty(N, A, K, H):
    out = dict(positions=np.full((N, A, K, 2), np.nan, _f), angles=np.full((N, A, K), np.nan, _f), velocity=np.full((N, A, K, 2), np.nan, _f),
               angvelocity=np.full((N, A, K), np.nan, _f), progress=np.ones((N, A, K), _f), stops=np.zeros((N, A, K), np.int32),
               first_stop=np.full((N, A, K), H, np.int32), trail=np.full((N, A, K, H, 2), np.nan, _f))
    return out


def rollout_rule(world, actions, table, keep, others, agent_radius, fps, mask=None):
    """The rule: for every (n, a, k) a one-candidate copy of env n - agent a alone, or with ``others='rest'`` among the env's
    other agents at rest - stepped H times: the movement by ms_host_move_velocity, collision and integration by the oracle's
    physics. Returns the eight outputs as a dict of numpy arrays (an agent the mask leaves out: as cuda.rollouts without ``out``)."""
    actions, table = np.asarray(actions, np.int64), np.asarray(table, _f)
    N, A = world['angles'].shape
    K, H = actions.shape[-2:]
    cfg = O.config(agent_radius, 8, 90., fps)
    out = _empty(N, A, K, H)
    for n in range(N):
        scene = _oracle_scene(world['walls'][n], A if others == 'rest' else 1)
        for a in range(A):
            if mask is not None and not mask[n, a]:
                continue
            who = list(range(A)) if others == 'rest' else [a]
            me = who.index(a)
            for k in range(K):
                ag = dict(positions=world['positions'][n, who][None].copy(), angles=world['angles'][n, who][None].copy(),
                          velocity=np.zeros((1, len(who), 2), _f), angvelocity=np.zeros((1, len(who)), _f))
                ag['velocity'][0, me], ag['angvelocity'][0, me] = world['velocity'][n, a], world['angvelocity'][n, a]
                rest = ag['positions'].copy()
                least, stops, first = _f(1), 0, H
                for h in range(H):
                    act = int(min(max(_plan(actions, n, a, k)[h], 0), len(table) - 1))
                    ag['velocity'][0, me], ag['angvelocity'][0, me] = host_move_velocity(
                        keep, ag['angles'][0, me], table[act], ag['velocity'][0, me], ag['angvelocity'][0, me])
                    progress, ag = O.physics(scene, ag, cfg)
                    for b in range(len(who)):                              # (the others stand still for the whole horizon)
                        if b != me:
                            ag['positions'][0, b], ag['velocity'][0, b], ag['angvelocity'][0, b] = rest[0, b], 0., 0.
                    x = progress[0, me]
                    least = min(least, x)
                    if x < 1:
                        stops, first = stops + 1, min(first, h)
                    out['trail'][n, a, k, h] = ag['positions'][0, me]
                out['positions'][n, a, k], out['angles'][n, a, k] = ag['positions'][0, me], ag['angles'][0, me]
                out['velocity'][n, a, k], out['angvelocity'][n, a, k] = ag['velocity'][0, me], ag['angvelocity'][0, me]
                out['progress'][n, a, k], out['stops'][n, a, k], out['first_stop'][n, a, k] = least, stops, first
    return out


def host_rollouts(world, actions, table, keep, others, agent_radius, fps, mask=None, trail=True, raw=False):
    """ms_host_rollouts, env by env. Returns the outputs as rollout_rule does (``raw``: the status of the first env's call
    instead, whatever it is)."""
    from megastep_amd import _lib
    h_ = _lib.lib()
    actions, table = np.ascontiguousarray(actions, np.int64), np.ascontiguousarray(table, _f)
    N, A = world['angles'].shape
    K, H = actions.shape[-2:]
    out = _empty(N, A, max(K, 1), max(H, 1))
    cfg = _lib.MsConfig(float(agent_radius), 8, 90., float(fps))
    ptr = lambda x: x.ctypes.data if x is not None else None
    for n in range(N):
        walls = np.ascontiguousarray(world['walls'][n], _f).reshape(-1, 4)
        st = {k: np.ascontiguousarray(world[k][n], _f) for k in ('angles', 'positions', 'angvelocity', 'velocity')}
        ag = _lib.MsAgents(ptr(st['angles']), ptr(st['positions']), ptr(st['angvelocity']), ptr(st['velocity']), None, None)
        acts = actions if actions.ndim == 2 else np.ascontiguousarray(actions[n])
        m = None if mask is None else np.ascontiguousarray(mask[n], np.uint8)
        env = {k: np.ascontiguousarray(out[k][n]) for k in FIELDS}
        r = _lib.MsRollouts(K, H, ptr(acts), int(actions.ndim == 2), ptr(table), len(table), float(keep), int(others == 'rest'), ptr(m),
                            *(ptr(env[k]) for k in FIELDS[:7]), ptr(env['trail']) if trail else None)
        status = h_.ms_host_rollouts(walls.ctypes.data if len(walls) else None, len(walls), C.byref(ag), A, C.byref(r), C.byref(cfg))
        if raw:
            return status
        assert status == 0, status
        for k in FIELDS:
            out[k][n] = env[k]
    return out
