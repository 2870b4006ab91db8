"""The operands the culls are tried on, drawn once for the CPU tests of the library's host instantiations (tests/test_wallgrid.py)
and the GPU tests of its device builds (tests/test_gpu_culls.py): agent pairs around the reach of collision_cc, agents and walls
around the reach of collision_cs, and lines around an agent for pass 1's ray intervals."""
import ctypes as C

import numpy as np

#: the (res, fov) shapes the ray intervals and the wedges are tried at
RAY_SHAPES = [(64, 130.), (512, 130.), (200, 60.), (7, 170.), (1, 90.), (128, 165.)]


def groups_for(res):
    """How many 64-ray groups a wave may be given at this resolution (render_kernel's NG; ms_debug_ray_groups)."""
    return 4 if res > 128 else 2 if res > 64 else 1


def agent_pairs(n=60000):
    """(me, other, R): (n, 4) rows (x, y, vx/fps, vy/fps) and n radii - at every distance around the threshold, relative velocities
    from a sprint down to 1e-12 a step, pairs in perfect step, coordinates far from the origin, and a NaN or an infinity here and
    there."""
    rng = np.random.RandomState(0)
    mes, others, radii = np.empty((n, 4), np.float32), np.empty((n, 4), np.float32), np.empty(n, np.float32)
    for i in range(n):
        R = float(np.float32(10.**rng.uniform(-2, 0)))
        base = rng.uniform(-1, 1, 2)*10.**rng.uniform(0, 3)
        common = rng.uniform(-1, 1, 2)*10.**rng.uniform(-3, 1)*(rng.rand() < .8)
        rel = 10.**rng.uniform(-12, .7)
        a = rng.uniform(0, 2*np.pi)
        dv = rel*np.array([np.cos(a), np.sin(a)])*(rng.rand() < .95)             # 5 %: in perfect step
        # distances around what the pair can cover: |dv| + 2R, scaled by 0.2 .. 30; now and then much closer / farther
        D = (rel + 2*R)*10.**rng.uniform(-.7, 1.5) if rng.rand() < .8 else 10.**rng.uniform(-3, 2)
        b = a + rng.normal(0, .5) if rng.rand() < .7 else rng.uniform(0, 2*np.pi)   # mostly closing in on each other
        me = np.array([*base, *(common + dv)], np.float32)
        other = np.array([*(base + D*np.array([np.cos(b), np.sin(b)])), *common], np.float32)
        if i % 997 == 0: me[rng.randint(4)] = [np.nan, np.inf, -np.inf][i % 3]
        if i % 1009 == 0: other[rng.randint(4)] = [np.nan, np.inf, -np.inf][i % 3]
        mes[i], others[i], radii[i] = me, other, R
    return mes, others, radii


def agents_and_walls(n=80000):
    """(agent, wall, R): (n, 4) rows (x, y, vx/fps, vy/fps) and (ax, ay, bx, by), n radii - walls at every distance around the
    reach, agents from a sprint down to 1e-12 a step, walls from 10 m down to a micrometre, a NaN or an infinity now and then."""
    rng = np.random.RandomState(1)
    agents, walls, radii = np.empty((n, 4), np.float32), np.empty((n, 4), np.float32), np.empty(n, np.float32)
    for i in range(n):
        R = float(np.float32(10.**rng.uniform(-2, 0)))
        p = rng.uniform(-1, 1, 2)*10.**rng.uniform(0, 3)
        speed = 10.**rng.uniform(-12, .7)*(rng.rand() < .97)                     # 3 %: standing still
        a = rng.uniform(0, 2*np.pi)
        v = speed*np.array([np.cos(a), np.sin(a)])
        reach = (speed + 2*R)*(1 + 1e-6/max(speed, 1e-30))**2 if speed > 0 else 2*R
        D = min(reach, 1e4)*10.**rng.uniform(-.7, 1.) if rng.rand() < .8 else 10.**rng.uniform(-3, 2)
        b = a + rng.normal(0, .6) if rng.rand() < .7 else rng.uniform(0, 2*np.pi)   # mostly ahead of the agent
        mid = p + D*np.array([np.cos(b), np.sin(b)])
        length = 10.**rng.uniform(-6, 1)
        c = rng.uniform(0, 2*np.pi)
        half = .5*length*np.array([np.cos(c), np.sin(c)])
        shift = rng.uniform(-1, 1)*half*(rng.rand() < .5)                         # the nearest point: an end as often as not
        agent = np.array([*p, *v], np.float32)
        wall = np.array([*(mid - half + shift), *(mid + half + shift)], np.float32)
        if i % 997 == 0: agent[rng.randint(4)] = [np.nan, np.inf, -np.inf][i % 3]
        if i % 1009 == 0: wall[rng.randint(4)] = [np.nan, np.inf, -np.inf][i % 3]
        agents[i], walls[i], radii[i] = agent, wall, R
    return agents, walls, radii


def lines_in_view(oracle, res, fov, E=3000):
    """E single-agent envs with one wall each somewhere around the agent - near and far, behind it, through its near plane,
    across the edges of the fan, end-on, tiny - and the oracle's render of them: (poses (E, 4) = (x, y, sin, cos of the heading),
    lines (E, 4), indices (E, res) of the line each ray lands on, M = the wall's index, the agent's radius)."""
    from megastep_amd import _lib, scene as scene_
    rng = np.random.RandomState(res)
    lib = _lib.lib()
    M = len(scene_.agent_model())
    radius = float(np.float32(.15/2**.5))
    pos = rng.uniform(-5, 5, (E, 2)).astype(np.float32)
    ang = rng.uniform(-180, 180, E).astype(np.float32)
    # a wall somewhere around the agent: its middle at a log-uniform distance in a direction anywhere, any orientation
    dist = 10.**rng.uniform(-1.3, 1.3, E)
    where = rng.uniform(0, 2*np.pi, E)
    mid = pos + (dist*np.array([np.cos(where), np.sin(where)])).T
    length = 10.**rng.uniform(-3, 1.3, E)
    along = np.where(rng.rand(E) < .3, where + rng.normal(0, .02, E), rng.uniform(0, 2*np.pi, E))   # a third: end-on
    half = (.5*length*np.array([np.cos(along), np.sin(along)])).T
    walls = np.concatenate([mid - half, mid + half], 1).astype(np.float32).reshape(E, 1, 2, 2)
    model = scene_.agent_model()
    lines = np.concatenate([np.tile(model[None], (E, 1, 1, 1)), walls], 1)              # (agent rows are redrawn by the oracle)
    texw = np.full(E*(M + 1), 4, np.int32)
    S = oracle.Scene(dict(n_agents=1, model=model, lights_vals=np.zeros((0, 3)), lights_widths=[0]*E,
                          lines_vals=lines.reshape(-1, 2, 2), lines_widths=[M + 1]*E,
                          textures_vals=np.full((texw.sum(), 3), .5), textures_widths=texw))
    ag = dict(angles=ang.reshape(E, 1), positions=pos.reshape(E, 1, 2), angvelocity=np.zeros((E, 1), np.float32),
              velocity=np.zeros((E, 1, 2), np.float32))
    idx = oracle.render(S, ag, oracle.config(radius, res, fov, 10))['indices'][:, 0]
    poses = np.empty((E, 4), np.float32)
    for e in range(E):
        s_, c_ = C.c_float(), C.c_float()
        lib.ms_host_sincospi(float(np.float32(ang[e])/np.float32(180.)), C.byref(s_), C.byref(c_))
        poses[e] = [pos[e, 0], pos[e, 1], s_.value, c_.value]
    return poses, np.ascontiguousarray(walls.reshape(E, 4)), idx, M, radius
