"""The scenarios' rule (MsScenarios) as a loop over envs, scenarios and steps around the CPU oracle's physics step -
ONE oracle call a step for the whole env, which makes the agent-agent tests itself - and the host statement ms_host_scenarios
driven env by env: what tests/test_scenario_host.py holds against each other and tests/test_gpu_scenarios.py holds the kernel
to. Worlds are tests/rollout_rule.py's."""
import ctypes as C
import numpy as np
from oracle import oracle as O
from tests.rollout_rule import FIELDS, _empty, _oracle_scene, host_move_velocity

_f = np.float32


def expand_focal(plans, base, n_envs, n_agents):
    """The joint tensor (N, A K, A, H) a focal call means: scenario f K + k puts agent f on its plan k, every other agent on base."""
    plans, base = np.asarray(plans, np.int64), np.asarray(base, np.int64)
    K, H = plans.shape[-2:]
    out = np.empty((n_envs, n_agents*K, n_agents, H), np.int64)
    for f in range(n_agents):
        for k in range(K):
            out[:, f*K + k] = base
            out[:, f*K + k, f] = plans[k] if plans.ndim == 2 else plans[:, f, k]
    return out


def focal_rows(joint, n_agents):
    """The rows a focal call writes, (N, A, K, ..), picked out of the joint outputs on the expanded tensor."""
    out = {}
    for key, v in joint.items():
        K = v.shape[1]//n_agents
        out[key] = np.stack([np.stack([v[:, f*K + k, f] for k in range(K)], 1) for f in range(n_agents)], 1)
    return out


def scenario_rule(world, actions, table, keep, agent_radius, fps, mask=None):
    """The rule, joint mode: for every (n, s) a copy of env n with all its agents, stepped H times - every agent's movement by
    ms_host_move_velocity, then one oracle physics call. Returns the eight outputs (N, S, A, ..) as a dict of numpy arrays
    (an env the mask leaves out: as cuda.scenarios without ``out``)."""
    actions, table = np.asarray(actions, np.int64), np.asarray(table, _f)
    N, A = world['angles'].shape
    S, _, H = actions.shape[-3:]
    cfg = O.config(agent_radius, 8, 90., fps)
    out = _empty(N, S, A, H)
    for n in range(N):
        if mask is not None and not mask[n]:
            continue
        scene = _oracle_scene(world['walls'][n], A)
        for s in range(S):
            plan = actions[s] if actions.ndim == 3 else actions[n, s]
            ag = dict(positions=world['positions'][n][None].copy(), angles=world['angles'][n][None].copy(),
                      velocity=world['velocity'][n][None].copy(), angvelocity=world['angvelocity'][n][None].copy())
            least, stops, first = np.ones(A, _f), np.zeros(A, np.int32), np.full(A, H, np.int32)
            for h in range(H):
                for a in range(A):
                    act = int(min(max(plan[a, h], 0), len(table) - 1))
                    ag['velocity'][0, a], ag['angvelocity'][0, a] = host_move_velocity(
                        keep, ag['angles'][0, a], table[act], ag['velocity'][0, a], ag['angvelocity'][0, a])
                progress, ag = O.physics(scene, ag, cfg)
                x = np.asarray(progress, _f)[0]
                least = np.where(x < least, x, least)
                stops += x < 1
                first = np.where(x < 1, np.minimum(first, h), first)
                out['trail'][n, s, :, h] = ag['positions'][0]
            out['positions'][n, s], out['angles'][n, s] = ag['positions'][0], ag['angles'][0]
            out['velocity'][n, s], out['angvelocity'][n, s] = ag['velocity'][0], ag['angvelocity'][0]
            out['progress'][n, s], out['stops'][n, s], out['first_stop'][n, s] = least, stops, first
    return out


def host_scenarios(world, actions, table, keep, agent_radius, fps, mask=None, trail=True, raw=False, base=None, edit=None):
    """ms_host_scenarios, env by env: joint mode on ``actions`` (N, S, A, H) or (S, A, H); with ``base`` (N, A, H) the focal mode
    on plans (N, A, K, H) or (K, H), the mask then (N, A). Returns the outputs as scenario_rule does - focal: (N, A, K, ..), as
    rollout_rule - (``raw``: the status of the first env's call instead, whatever it is; ``edit``: called on the struct first)."""
    from megastep_amd import _lib
    h_ = _lib.lib()
    actions, table = np.ascontiguousarray(actions, np.int64), np.ascontiguousarray(table, _f)
    N, A = world['angles'].shape
    focal = base is not None
    shared = actions.ndim == (2 if focal else 3)
    H = actions.shape[-1]
    S = actions.shape[-2] if focal else actions.shape[-3]
    out = _empty(N, A, max(S, 1), max(H, 1)) if focal else _empty(N, max(S, 1), A, max(H, 1))
    cfg = _lib.MsConfig(float(agent_radius), 8, 90., float(fps))
    ptr = lambda x: x.ctypes.data if x is not None else None
    for n in range(N):
        walls = np.ascontiguousarray(world['walls'][n], _f).reshape(-1, 4)
        st = {k: np.ascontiguousarray(world[k][n], _f) for k in ('angles', 'positions', 'angvelocity', 'velocity')}
        ag = _lib.MsAgents(ptr(st['angles']), ptr(st['positions']), ptr(st['angvelocity']), ptr(st['velocity']), None, None)
        acts = actions if shared else np.ascontiguousarray(actions[n])
        b = np.ascontiguousarray(np.asarray(base, np.int64)[n]) if focal else None
        m = None if mask is None else np.ascontiguousarray(np.atleast_1d(mask[n]), np.uint8)
        env = {k: np.ascontiguousarray(out[k][n]) for k in FIELDS}
        q = _lib.MsScenarios(S, H, int(focal), ptr(acts), int(shared), ptr(b), ptr(table), len(table), float(keep), ptr(m),
                             *(ptr(env[k]) for k in FIELDS[:7]), ptr(env['trail']) if trail else None)
        if edit is not None:
            edit(q)
        status = h_.ms_host_scenarios(walls.ctypes.data if len(walls) else None, len(walls), C.byref(ag), A, C.byref(q), C.byref(cfg))
        if raw:
            return status
        assert status == 0, status
        for k in FIELDS:
            out[k][n] = env[k]
    return out
