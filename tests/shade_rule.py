"""The shading rule of DESIGN.md 3.30 (`ms_shade` / `cuda.shade`) restated in binary32 numpy, one rounding per operation as the
reference compiles it (shader_kernel, kernels.cu:407-450; light_intensity, kernels.cu:238-268; filter, kernels.cu:387-405), and
the harness that runs `ms_host_shade` - the serial host statement over the kernel's own per-ray functions - on numpy arrays.
tests/test_shade_host.py holds the rule to the oracle's render and the host statement to the rule; tests/test_gpu_cameras.py
holds the kernel to both."""
import ctypes as C

import numpy as np

F = np.float32
AMBIENT, LUMINANCE = F(.1), F(2.)


def starts_of(widths):
    return np.concatenate([[0], np.cumsum(widths)[:-1]]).astype(np.int32)


def make_scene(n_agents, model, envs, rng):
    """A scene dict (the oracle's format: tests/util.py scene_dict) from hand-made envs: each dict(walls=(W, 2, 2),
    lights=(k, 3), widths=texels per line - agent rows first - or None for random ones). Textures and baked light are random."""
    model = np.asarray(model, F).reshape(-1, 2, 2)
    AF = n_agents*len(model)
    lines, lwidths, lights, liwidths, twidths = [], [], [], [], []
    for e in envs:
        walls = np.asarray(e['walls'], F).reshape(-1, 2, 2)
        L = AF + len(walls)
        lines.append(np.concatenate([np.zeros((AF, 2, 2), F), walls]))
        lwidths.append(L)
        li = np.asarray(e['lights'], F).reshape(-1, 3)
        lights.append(li)
        liwidths.append(len(li))
        w = e.get('widths')
        twidths.append(np.asarray(w, np.int32) if w is not None else rng.randint(1, 9, L).astype(np.int32))
        assert len(twidths[-1]) == L
    twidths = np.concatenate(twidths)
    T = int(twidths.sum())
    return dict(n_agents=n_agents, model=model, lights_vals=np.concatenate(lights).astype(F), lights_widths=np.asarray(liwidths, np.int32),
                lines_vals=np.concatenate(lines).astype(F), lines_widths=np.asarray(lwidths, np.int32),
                textures_vals=rng.uniform(0, 1, (T, 3)).astype(F), textures_widths=twidths, baked_vals=rng.uniform(0, 1, T).astype(F))


def draw_rows(scene, agents):
    """`lines_vals` with the agents' rows drawn at their poses (draw_kernel, kernels.cu:297-318): a copy."""
    from oracle import oracle as O
    lines = np.asarray(scene['lines_vals'], F).reshape(-1, 2, 2).copy()
    model = np.asarray(scene['model'], F).reshape(-1, 2, 2)
    A, M = int(scene['n_agents']), len(model)
    starts = starts_of(scene['lines_widths'])
    angles, positions = np.asarray(agents['angles'], F), np.asarray(agents['positions'], F)
    for n in range(len(starts)):
        for a in range(A):
            s, c = O.sincospi(F(angles[n, a]/F(180)))
            px, py = positions[n, a]
            for m in range(M):
                for e in range(2):
                    mx, my = model[m, e]
                    lines[starts[n] + a*M + m, e, 0] = F(F(c*mx) - F(s*my)) + px
                    lines[starts[n] + a*M + m, e, 1] = F(F(s*mx) + F(c*my)) + py
    return lines


#: the plan worlds of the GPU test "look is the render" - (n_envs, res, seed); tests/test_shade_host.py checks with the oracle
#: that in each of them rays land on an agent
LOOK_WORLDS = ((5, 64, 31), (5, 37, 32))


def triangle_world(n_envs, res, seed, device):
    """Seeded floorplans with three agents per env placed as a triangle, looking at each other: a Core.  (No heading is a
    multiple of 90 degrees: at an odd `res` the middle ray of such an agent meets an axis-aligned wall at exactly a right angle,
    dot(ru, v) is -0 for a wall drawn right to left, and the render's in-range division (math.h, div_inrange) returns +0 where
    the plain division of ms_raycast and of the oracle returns -0 - the one bit in which `render` and `raycast` differ there.)"""
    import torch
    from tests import util
    c, _ = util.plan_world(n_envs, 3, res, 130, seed=seed, device=device)
    for e in range(n_envs):
        p = c.agents.positions[e, 0].clone()
        c.agents.positions[e, 1] = p + torch.tensor([.6, 0.], device=device)
        c.agents.positions[e, 2] = p + torch.tensor([.3, .5], device=device)
        c.agents.angles[e] = torch.tensor([20., 160., -95.], device=device)
    return c


def _min(a, b):                                     # (fminf with the NaN behaviour spelled out: the first operand wins ties)
    if a != a:
        return b
    return b if b < a else a


def _max(a, b):
    if a != a:
        return b
    return b if b > a else a


def tex_filter(x, w):
    """kernels.cu:387-405: (l, r, lw, rw)."""
    y = _min(F(F(x)*F(w + 1)), F(w - 1))
    l = int(_max(F(y - F(1)), F(0)))
    r = int(_min(y, F(w - 1)))
    ld = F(np.abs(F(y - F(l + 1))) + F(1e-3))
    rd = F(np.abs(F(y - F(r + 1))) + F(1e-3))
    return l, r, F(rd/F(ld + rd)), F(ld/F(ld + rd))


def light_intensity(C_, lights, walls):
    """kernels.cu:238-268 at the point C_, against the env's lights (k, 3) in their order and its static rows (W, 2, 2)."""
    cx, cy = F(C_[0]), F(C_[1])
    ax, ay = walls[:, 0, 0], walls[:, 0, 1]
    vx, vy = walls[:, 1, 0] - ax, walls[:, 1, 1] - ay
    acc = AMBIENT
    with np.errstate(all='ignore'):
        for ix, iy, ii in np.asarray(lights, F).reshape(-1, 3):
            ux, uy = F(cx - ix), F(cy - iy)
            uxv = ux*vy - uy*vx
            pqx, pqy = ax - ix, ay - iy
            parallel = np.abs(uxv) < F(1e-3)
            s = np.where(parallel, F(np.inf), (pqx*vy - pqy*vx)/uxv)
            t = np.where(parallel, F(np.inf), (pqx*uy - pqy*ux)/uxv)
            if not ((t > 0) & (t < 1) & (s > 0) & (s < F(.999))).any():
                dx, dy = F(ix - cx), F(iy - cy)
                d2 = F(F(dx*dx) + F(dy*dy))
                acc = F(acc + F(F(LUMINANCE*ii)/_max(d2, F(1))))
    return _min(acc, F(1))


def shade_rule(scene, lines, indices, locations, dots, with_agents=True):
    """`screen` (N, R, 3) for rays with the given (N, R) planes. `lines`: the scene's rows with the agents' rows as they are
    drawn now (draw_rows, or what the oracle's render left); with_agents=False: rays on an agent's row are black."""
    lines = np.asarray(lines, F).reshape(-1, 2, 2)
    lw, ls = np.asarray(scene['lines_widths']), starts_of(scene['lines_widths'])
    tw = np.asarray(scene['textures_widths'])
    ts = starts_of(tw)
    tex, baked = np.asarray(scene['textures_vals'], F).reshape(-1, 3), np.asarray(scene['baked_vals'], F)
    liw, lis = np.asarray(scene['lights_widths']), starts_of(scene['lights_widths'])
    lights = np.asarray(scene['lights_vals'], F).reshape(-1, 3)
    AF = int(scene['n_agents'])*len(np.asarray(scene['model']).reshape(-1, 2, 2))
    N, R = indices.shape
    screen = np.zeros((N, R, 3), F)
    for n in range(N):
        rows = lines[ls[n]:ls[n] + lw[n]]
        for r in range(R):
            idx = int(indices[n, r])
            if idx < 0 or idx >= lw[n] or (idx < AF and not with_agents):
                continue
            loc, dt = F(locations[n, r]), F(dots[n, r])
            if not (F(0) <= loc <= F(1)):                   # (no place along a line: nothing ms_raycast writes for a hit)
                continue
            w, t0 = int(tw[ls[n] + idx]), int(ts[ls[n] + idx])
            l, rr, wl, wr = tex_filter(loc, w)
            if idx < AF:
                (ax, ay), (bx, by) = rows[idx]
                C_ = (F(F(ax*F(F(1) - loc)) + F(bx*loc)), F(F(ay*F(F(1) - loc)) + F(by*loc)))
                intensity = light_intensity(C_, lights[lis[n]:lis[n] + liw[n]], rows[AF:])
            else:
                intensity = F(F(wl*baked[t0 + l]) + F(wr*baked[t0 + rr]))
            dn = F(F(1) - F(dt*dt))
            for k in range(3):
                screen[n, r, k] = F(F(dn*intensity)*F(F(wl*tex[t0 + l, k]) + F(wr*tex[t0 + rr, k])))
    return screen


def _aligned(a, dtype):
    """A C-contiguous copy of `a` that starts on a 64-byte boundary."""
    a = np.ascontiguousarray(a, dtype)
    buf = np.zeros(a.nbytes + 64, np.uint8)
    off = (-buf.ctypes.data) % 64
    out = buf[off:off + a.nbytes].view(dtype).reshape(a.shape)
    out[...] = a
    return out


def host_structs(scene, agents):
    """(MsScenery, MsAgents or None, keep-alive list) over numpy copies of a scene dict and an agents dict."""
    from megastep_amd import _lib
    keep = dict(
        lights=_aligned(np.asarray(scene['lights_vals'], F).reshape(-1, 3), F), liw=_aligned(scene['lights_widths'], np.int32),
        lis=_aligned(starts_of(scene['lights_widths']), np.int32),
        lines=_aligned(np.asarray(scene['lines_vals'], F).reshape(-1, 2, 2), F), lw=_aligned(scene['lines_widths'], np.int32),
        ls=_aligned(starts_of(scene['lines_widths']), np.int32),
        tex=_aligned(np.asarray(scene['textures_vals'], F).reshape(-1, 3), F), tw=_aligned(scene['textures_widths'], np.int32),
        ts=_aligned(starts_of(scene['textures_widths']), np.int32),
        model=_aligned(np.asarray(scene['model'], F).reshape(-1, 2, 2), F), baked=_aligned(scene['baked_vals'], F))
    p = lambda a: a.ctypes.data
    sc = _lib.MsScenery(
        n_envs=len(keep['lw']), n_agents=int(scene['n_agents']), n_model=len(keep['model']),
        lights_vals=p(keep['lights']), lights_widths=p(keep['liw']), lights_starts=p(keep['lis']),
        lines_vals=p(keep['lines']), lines_widths=p(keep['lw']), lines_starts=p(keep['ls']),
        textures_vals=p(keep['tex']), textures_widths=p(keep['tw']), textures_starts=p(keep['ts']),
        model=p(keep['model']), baked_vals=p(keep['baked']),
        n_lines_total=len(keep['lines']), n_lights_total=len(keep['lights']), n_texels_total=len(keep['tex']))
    ag = None
    if agents is not None:
        keep['angles'] = _aligned(agents['angles'], F)
        keep['positions'] = _aligned(agents['positions'], F)
        keep['zeros'] = _aligned(np.zeros_like(keep['positions']), F)
        ag = _lib.MsAgents(p(keep['angles']), p(keep['positions']), p(keep['zeros']), p(keep['zeros']), None, None)
    return sc, ag, keep


def host_shade(scene, agents, indices, locations, dots):
    """`ms_host_shade` on numpy arrays: `screen` (N, R, 3). agents=None: the call without agents."""
    from megastep_amd import _lib
    sc, ag, keep = host_structs(scene, agents)
    idx, loc, dt = _aligned(indices, np.int32), _aligned(locations, F), _aligned(dots, F)
    N, R = idx.shape
    screen = _aligned(np.full((N, R, 3), np.nan), F)
    q = _lib.MsShade(R, idx.ctypes.data, loc.ctypes.data, dt.ctypes.data, screen.ctypes.data)
    rc = _lib.lib().ms_host_shade(C.byref(sc), C.byref(ag) if ag is not None else None, C.byref(q))
    assert rc == 0, rc
    del keep
    return screen
