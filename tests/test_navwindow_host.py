"""Map windows (`ms_nav_windows`, `cuda.cell_layer`, `cuda.map_channel`, `cuda.local_maps`) on the CPU: the contract of
include/megastep_hip.h (MsNavWindows) restated in binary32 numpy (`window_rule`, which tests/test_gpu_navwindow.py holds the
kernel to, bit for bit); the host instantiation of the kernel's own device functions against the rule; a closed form that does
not go through the restatement; sums that must come out exactly; and the C-ABI's declarations, layouts and refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import CELL, CELLS, RADIUS, F, bits
from tests.test_navseen_host import cases, seen_rule

INF, NAN = F(np.inf), F(np.nan)


class Layer:
    """A layer as the rule and the host call read it: flat values, stores per env, (N, P) field or None."""

    def __init__(self, values, n_fields=1, field=None):
        self.values, self.n_fields = np.ascontiguousarray(values), int(n_fields)
        self.field = None if field is None else np.ascontiguousarray(field, np.int32)
        assert self.values.dtype in (np.uint8, F) and self.values.ndim == 1

    is_float = property(lambda self: self.values.dtype == F)


class Channel:

    def __init__(self, source, where=True, scale=0., gate=None, outside=0., hidden=0.):
        self.source, self.where, self.scale, self.gate, self.outside, self.hidden = source, bool(where), F(scale), gate, F(outside), F(hidden)


class window_rule:
    """The contract in numpy: float32 scalars and arrays only, one operation per statement, in the order the header gives."""

    @staticmethod
    def cells(geom, cell, view, H, W, k):
        """(k*k, H, W) int64: the flat cell under every sub-sample of every pixel (a outer, b inner), -1 where there is none."""
        jx0, iy0, nx, ny = (int(v) for v in geom)
        c, g, kf = F(cell), np.asarray(view, F), F(k)
        i, j = np.arange(H).astype(F)[:, None], np.arange(W).astype(F)[None, :]
        out = np.empty((k*k, H, W), np.int64)
        with np.errstate(all='ignore'):
            for a in range(k):
                for b in range(k):
                    hb = F(b) + F(.5)
                    ha = F(a) + F(.5)
                    ob = hb/kf
                    oa = ha/kf
                    u = j + ob
                    w = i + oa
                    xu = g[0]*u
                    xw = g[1]*w
                    xs = xu + xw
                    x = xs + g[2]
                    yu = g[3]*u
                    yw = g[4]*w
                    ys = yu + yw
                    y = ys + g[5]
                    qx = x/c
                    qy = y/c
                    fx = np.floor(qx)
                    fy = np.floor(qy)
                    near = (np.abs(fx) < F(2.**30)) & (np.abs(fy) < F(2.**30))
                    jj = np.where(near, fx, F(0)).astype(np.int64) - jx0
                    ii = np.where(near, fy, F(0)).astype(np.int64) - iy0
                    inside = near & (ii >= 0) & (ii < ny) & (jj >= 0) & (jj < nx)
                    out[a*k + b] = np.where(inside, ii*nx + jj, -1)
        return out

    @staticmethod
    def store(layer, n, p):
        """The store view (n, p) reads in `layer`, -1 for a bad index."""
        f = int(layer.field[n, p]) if layer.field is not None else (0 if layer.n_fields == 1 else p)
        return f if 0 <= f < layer.n_fields else -1

    @staticmethod
    def image(ch, cells, n_cells, first, n, p, k):
        """One channel's (H, W) float32 image from the pixels' cells."""
        shape = cells.shape[1:]
        fs = window_rule.store(ch.source, n, p)
        if fs < 0:
            return np.full(shape, ch.outside, F)
        if ch.gate is not None:
            fg = window_rule.store(ch.gate, n, p)
            if fg < 0:
                return np.full(shape, ch.hidden, F)
        acc = np.zeros(shape, F)
        for s in range(k*k):
            has = cells[s] >= 0
            value = np.full(shape, ch.outside, F)
            if has.any():
                at = np.where(has, cells[s], 0)
                src = ch.source.values[ch.source.n_fields*first + fs*n_cells:][:n_cells][at]
                if ch.source.is_float:
                    with np.errstate(all='ignore'):
                        v = src*ch.scale
                        inner = np.where(v > F(0), v, F(0))
                        got = np.where(v < F(1), inner, F(1))
                else:
                    got = np.where((src != 0) == ch.where, F(1), F(0))
                if ch.gate is not None:
                    gate = ch.gate.values[ch.gate.n_fields*first + fg*n_cells:][:n_cells][at]
                    got = np.where(gate == 0, ch.hidden, got)
                value = np.where(has, got, value).astype(F)
            acc = acc + value
        return acc/F(k*k)

    @staticmethod
    def call(geom, starts, cell, views, size, channels, samples=1):
        """(N, P, C, H, W) float32: one call of ms_nav_windows."""
        H, W = size
        views = np.asarray(views, F)
        N, P = views.shape[:2]
        out = np.empty((N, P, len(channels), H, W), F)
        for n in range(N):
            nx, ny = int(geom[n][2]), int(geom[n][3])
            n_cells = nx*ny if nx > 0 and ny > 0 else 0
            for p in range(P):
                cells = window_rule.cells(geom[n], cell, views[n, p], H, W, samples)
                for c, ch in enumerate(channels):
                    out[n, p, c] = window_rule.image(ch, cells, n_cells, int(starts[n]), n, p, samples)
        return out


def _spec(layer, keep):
    from megastep_amd import _lib
    keep += [layer.values, layer.field]
    return _lib.MsNavLayer(layer.values.ctypes.data, int(layer.is_float), layer.n_fields, None if layer.field is None else layer.field.ctypes.data)


def _host(geom, starts, cell, free, views, size, channels, samples=1, clearance=RADIUS):
    """ms_host_nav_windows on host arrays: (N, P, C, H, W)."""
    from megastep_amd import _lib
    geom = np.ascontiguousarray(geom, np.int32)
    if geom.ctypes.data % 16:                        # (MsNavGrid.geom: 16-byte aligned)
        room = np.empty(geom.size + 4, np.int32)
        off = (-room.ctypes.data % 16)//4
        room[off:off + geom.size] = geom.reshape(-1)
        geom = room[off:off + geom.size].reshape(geom.shape)
    starts, views = np.ascontiguousarray(starts, np.int64), np.ascontiguousarray(views, F)
    N, P = views.shape[:2]
    out = np.full((N, P, len(channels)) + tuple(size), F(-7), F)
    keep = []
    specs = (_lib.MsNavChannel*len(channels))()
    for ch, spec in zip(channels, specs):
        spec.source = _spec(ch.source, keep)
        if ch.gate is not None:
            spec.gate = _spec(ch.gate, keep)
        spec.where, spec.scale, spec.outside, spec.hidden = int(ch.where), float(ch.scale), float(ch.outside), float(ch.hidden)
    grid = _lib.MsNavGrid(N, cell, clearance, geom.ctypes.data, starts.ctypes.data, 0, free.ctypes.data)
    w = _lib.MsNavWindows(P, size[0], size[1], samples, views.ctypes.data, len(channels), specs, out.ctypes.data)
    assert _lib.lib().ms_host_nav_windows(ctypes.byref(grid), ctypes.byref(w)) == 0
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the inputs: test_navseen_host's six plans (three plain, three oblique) and an env without cells as ONE grid of seven envs,
# two seen maps an env from its two viewers' oracle frames, an empty map, and the frontier fields of the maps
# ---------------------------------------------------------------------------------------------------------------------
class _World:
    pass


_WORLD = {}


def world(cell=CELL, r=RADIUS):
    if (cell, r) not in _WORLD:
        from megastep_amd import _lib
        h = _lib.lib()
        w = _World()
        w.cell, w.clearance = cell, r
        cs = cases(cell, r)
        w.geom = np.array([c.geom for c in cs] + [(3, 4, 0, 7)], np.int32)
        sizes = [c.free.size for c in cs] + [0]
        w.starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        w.free = np.concatenate([c.free.reshape(-1).astype(np.uint8) for c in cs] + [np.zeros(1, np.uint8)])
        w.seen_images = [seen_rule.call(c.geom, cell, c.free, c.blank, [0, 0], c.origins, c.dirs, c.distances)[0] for c in cs]
        w.seen = np.concatenate([m.reshape(-1) for m in w.seen_images] + [np.zeros(2, np.uint8)])
        w.blank = np.zeros_like(w.seen)
        fields = []
        for c, maps in zip(cs, w.seen_images):
            geom, free = np.array(c.geom, np.int32), np.ascontiguousarray(c.free, np.uint8)
            for s in range(2):
                D = np.empty(c.free.shape, F)
                marks = np.ascontiguousarray(maps[s])
                assert h.ms_host_nav_seed_field(geom.ctypes.data, cell, free.ctypes.data, marks.ctypes.data, 0, None, 1, D.ctypes.data, None) > 0
                fields.append(D.reshape(-1))
        w.fields = np.concatenate(fields + [np.zeros(2, F)])
        assert np.isinf(w.fields).any() and (w.fields == 0).any() and (np.isfinite(w.fields) & (w.fields > 1)).any()
        w.odd = w.fields.copy()
        w.odd[5::97] = NAN
        w.centres = np.stack([c.origins for c in cs] + [np.zeros((2, 2), F)]).astype(np.float64)       # (7, 2, 2)
        _WORLD[cell, r] = w
    return _WORLD[cell, r]


def views_round(centres, size, angle, pixel):
    """(N, P, 6) float32 views: `centres` (N, P, 2) in the middle of a `size` image, forward at `angle` degrees up the image, `pixel`
    metres a pixel (float64 arithmetic, rounded once: the views are inputs, not part of the rule)."""
    H, W = size
    a = np.deg2rad(angle)
    fx, fy = np.cos(a), np.sin(a)
    ex, ey = (fy, -fx), (-fx, -fy)
    cx, cy = centres[..., 0], centres[..., 1]
    rows = [ex[0]*pixel + 0*cx, ey[0]*pixel + 0*cx, cx - ex[0]*pixel*W/2 - ey[0]*pixel*H/2,
            ex[1]*pixel + 0*cx, ey[1]*pixel + 0*cx, cy - ex[1]*pixel*W/2 - ey[1]*pixel*H/2]
    return np.stack(rows, -1).astype(F)


def _same(w, views, size, channels, samples=1):
    want = window_rule.call(w.geom, w.starts, w.cell, views, size, channels, samples)
    got = _host(w.geom, w.starts, w.cell, w.free, views, size, channels, samples, w.clearance)
    assert np.array_equal(bits(got), bits(want)), (int((bits(got) != bits(want)).sum()), size, samples)
    return want


def _channels(w, field=None, gate_field=None):
    free, seen, blank = Layer(w.free), Layer(w.seen, 2, gate_field), Layer(w.blank, 2, gate_field)
    dist, odd = Layer(w.fields, 2, field), Layer(w.odd, 2, field)
    return [Channel(free), Channel(free, where=False), Channel(free, gate=seen), Channel(free, where=False, gate=blank, hidden=.25),
            Channel(odd, scale=.25), Channel(odd, scale=3., outside=.5), Channel(dist, scale=.1, gate=seen, hidden=.25),
            Channel(Layer(w.seen, 2, field), outside=.5)]


def test_the_host_instantiation_is_the_rule_bit_for_bit():
    w = world()
    chans = _channels(w)
    some, k = 0, 0
    for angle in (0., 37., 90., 180.5):
        for pixel in (.5*CELL, CELL, 3*CELL):
            samples = 1 + k % 3
            k += 1
            views = views_round(w.centres, (16, 16), angle, pixel)
            sel = slice(k % 2, 8, 2) if samples == 3 else slice(0, 6)
            got = _same(w, views, (16, 16), chans[sel], samples)
            assert (got[6] == np.array([0., 0., 0., 0., 0., .5, 0., .5], F)[sel][None, :, None, None]).all()      # (no cells: `outside`)
            some += int(((got[:6] > 0) & (got[:6] < 1)).sum())
    assert some > 1000                               # (fractions: the float channels, and byte channels at 2 and 3 samples)
    # eight channels at once; the other sizes; a window reaching well beyond the grid, with outside 0 and 0.5
    for size, samples, angle, pixel in (((13, 21), 3, 37., CELL), ((1, 1), 2, 90., CELL), ((1, 70), 1, 180.5, 3*CELL), ((16, 16), 2, 37., 1.5),
                                        ((13, 21), 1, 0., .8), ((13, 21), 4, 90., 3*CELL)):
        got = _same(w, views_round(w.centres, size, angle, pixel), size, chans, samples)
        assert got.shape == (7, 2, 8) + size
        if pixel > .5:
            assert (got[:6, :, 0] == 0).any() and (got[:6, :, 7] == F(.5)).any() and (got[:6, :, 0] > 0).any()
    # view rows with a NaN and with infinities
    views = views_round(w.centres, (16, 16), 37., CELL)
    views[1, 0, 2] = NAN
    views[2, 1, 0] = INF
    views[3, 0] = [0, 0, INF, 0, 0, -INF]
    views[4, 1] = [3e38, 3e38, 3e38, 1e30, 0, 1e30]
    got = _same(w, views, (16, 16), chans, 2)
    assert (got[1, 0, 7] == F(.5)).all() and (got[3, 0, 5] == F(.5)).all() and (got[4, 1, 0] == 0).all() and (got[1, 1, 0] > 0).any()


@pytest.mark.parametrize('cell,r', CELLS)
def test_the_host_instantiation_is_the_rule_at_other_cell_widths(cell, r):
    """The same views - pixels of half a cell, a cell and three cells, four angles, one to three samples - over grids whose cell
    is no power of two: the cell under a sample, floorf(x/c), is a rounded quotient there."""
    w = world(cell, r)
    chans = _channels(w)
    some, k = 0, 0
    for angle in (0., 37., 90., 180.5):
        for pixel in (.5*cell, cell, 3*cell):
            samples = 1 + k % 3
            k += 1
            sel = slice(k % 2, 8, 2) if samples == 3 else slice(0, 6)
            got = _same(w, views_round(w.centres, (16, 16), angle, pixel), (16, 16), chans[sel], samples)
            some += int(((got[:6] > 0) & (got[:6] < 1)).sum())
    assert some > 1000
    got = _same(w, views_round(w.centres, (13, 21), 37., cell), (13, 21), chans, 3)
    assert (got[:6, :, 0] > 0).any() and (got[:6, :, 2] > 0).any()


def test_fields_name_the_store_and_a_bad_index_blanks_the_image():
    w = world()
    views = views_round(w.centres, (16, 16), 37., CELL)
    rng = np.random.RandomState(4)
    field = rng.randint(0, 2, (7, 2))
    swapped = np.array([[1, 0]]*7)
    # field NULL with n_fields of P (view p reads store p) against the same thing said with a field, and against the other store
    plain = _same(w, views, (16, 16), [Channel(Layer(w.seen, 2)), Channel(Layer(w.free), gate=Layer(w.seen, 2))])
    named = _same(w, views, (16, 16), [Channel(Layer(w.seen, 2, np.array([[0, 1]]*7))), Channel(Layer(w.free), gate=Layer(w.seen, 2, np.array([[0, 1]]*7)))])
    other = _same(w, views, (16, 16), [Channel(Layer(w.seen, 2, swapped)), Channel(Layer(w.free), gate=Layer(w.seen, 2, swapped))])
    assert np.array_equal(plain, named) and not np.array_equal(plain[:6], other[:6])
    for samples in (1, 3):
        _same(w, views, (16, 16), _channels(w, field=field, gate_field=swapped), samples)
    # indices of -1 and of n_fields: the source's gives `outside` throughout, the gate's `hidden`, the source's first
    bad = field.copy()
    bad[0, 0], bad[1, 1], bad[2, 0], bad[6, 1] = -1, 2, 7, -3
    worse = swapped.copy()
    worse[0, 0], worse[3, 1] = 2, -1
    chans = [Channel(Layer(w.seen, 2, bad), outside=.5), Channel(Layer(w.fields, 2, bad), scale=.1, gate=Layer(w.seen, 2, worse), outside=.3, hidden=.25),
             Channel(Layer(w.free), gate=Layer(w.seen, 2, worse), hidden=.75)]
    for samples in (1, 3):
        got = _same(w, views, (16, 16), chans, samples)
        assert (got[0, 0, 0] == F(.5)).all() and (got[1, 1, 0] == F(.5)).all() and (got[2, 0, 0] == F(.5)).all() and (got[6, 1, 0] == F(.5)).all()
        assert (got[0, 0, 1] == F(.3)).all() and (got[3, 1, 1] == F(.25)).all() and (got[0, 0, 2] == F(.75)).all() and (got[3, 1, 2] == F(.75)).all()
        assert not (got[3, 0, 2] == F(.75)).all()


def _by_hand():
    """The world's grid, seen maps and free cells as cuda.NavGrid / cuda.SeenMaps on CPU tensors."""
    from megastep_amd import cuda
    w = world()
    grid = cuda.NavGrid(torch.as_tensor(w.geom), torch.as_tensor(w.starts), torch.as_tensor(w.free), CELL, RADIUS, w.geom, w.starts)
    maps = cuda.seen_maps(grid, 2)
    maps.values[:] = torch.as_tensor(w.seen[:len(maps.values)])
    return w, grid, maps


def test_an_axis_aligned_view_of_one_pixel_a_cell_is_the_flipped_crop_of_the_map():
    """g0 = c, g4 = -c, g1 = g3 = 0 and offsets that are whole multiples of c = 1/8: every product and sum is exact, pixel
    (i, j) has its centre on the centre of cell (row top - i, column left + j) - no restatement of the rule is needed."""
    w, grid, maps = _by_hand()
    c = F(CELL)
    H, W = 12, 10
    for e in range(6):
        jx0, iy0, nx, ny = (int(v) for v in w.geom[e])
        assert nx >= 16 and ny >= 16
        for s, (left, top) in enumerate(((jx0 + 3, iy0 + ny - 5), (jx0 - 4, iy0 + ny + 2))):       # inside, and over the grid's corner
            views = np.zeros((7, 2, 6), F)
            views[e, s] = [c, 0, c*F(left), 0, -c, c*F(top + 1)]
            got = _host(w.geom, w.starts, CELL, w.free, views, (H, W), [Channel(Layer(w.seen, 2), outside=.5)])[e, s, 0]
            image = maps.image(e, s).numpy().astype(F)
            if s == 0:
                want = np.flipud(image[ny - 4 - H:ny - 4, 3:3 + W])
            else:
                want = np.full((H, W), F(.5), F)
                want[3:, 4:] = np.flipud(image[ny - (H - 3):ny, :W - 4])
            assert np.array_equal(got, want), (e, s)
    assert sum(int(m.sum()) for m in w.seen_images) > 2000


def test_floor_and_wall_add_up_to_seen_and_nine_samples_give_ninths():
    w = world()
    free, seen = Layer(w.free), Layer(w.seen, 2)
    chans = [Channel(free, gate=seen), Channel(free, where=False, gate=seen), Channel(seen)]
    ninths = (np.arange(10).astype(F)/F(9))
    for angle, pixel in ((37., CELL), (180.5, 3*CELL), (0., 1.)):
        views = views_round(w.centres, (16, 16), angle, pixel)
        one = _host(w.geom, w.starts, CELL, w.free, views, (16, 16), chans, 1)
        assert np.array_equal(one[:, :, 0] + one[:, :, 1], one[:, :, 2]) and np.isin(one, (0, 1)).all()
        assert (one[:6, :, 0].sum((1, 2, 3)) > 0).all() and one[:6, :, 1].sum() > 0 and not one[6].any()     # (a small window may hold no seen wall)
        nine = _host(w.geom, w.starts, CELL, w.free, views, (16, 16), chans, 3)
        assert np.isin(nine, ninths).all()
        if pixel > CELL:
            assert (~np.isin(nine, (0, 1))).sum() > 100


# ---------------------------------------------------------------------------------------------------------------------
# header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_calls_and_the_abi_version_stays():
    from megastep_amd import _lib
    assert 'ms_nav_windows' in declared_symbols(('megastep_hip.h',)) and 'ms_host_nav_windows' in declared_symbols(('megastep_hip_test.h',))
    assert {'ms_nav_windows', 'ms_host_nav_windows'} <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert hasattr(handle, 'ms_nav_windows') and hasattr(handle, 'ms_host_nav_windows') and handle.ms_abi_version() == 17


@pytest.mark.parametrize('name, fields', [
    ('MsNavLayer', ('values', 'is_float', 'n_fields', 'field')),
    ('MsNavChannel', ('source', 'gate', 'where', 'scale', 'outside', 'hidden')),
    ('MsNavWindows', ('n_views', 'height', 'width', 'samples', 'views', 'n_channels', 'channels', 'out'))])
def test_the_mirrors_have_the_c_layout(name, fields):
    import subprocess
    import tempfile
    from megastep_amd import _lib
    mirror = getattr(_lib, name)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "megastep_hip.h"\nint main(){printf("%zu", sizeof(' + name + '));' +
           ''.join(f'printf(" %zu", offsetof({name}, {f}));' for f in fields) + '}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')])
        got = list(map(int, subprocess.check_output([os.path.join(d, 't')]).split()))
    assert [f for f, _ in mirror._fields_] == list(fields)
    assert got == [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields]


def test_bad_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    G, L, Ch, W = _lib.MsNavGrid, _lib.MsNavLayer, _lib.MsNavChannel, _lib.MsNavWindows
    grid = G(n_envs=2, cell=.125, clearance=.106, geom=fake, starts=fake, max_framed=100, free_cells=fake)
    ref = ctypes.byref

    def call(windows=None, source=None, gate=None, channel=None, n=1, entry=h.ms_nav_windows):
        src = dict(values=fake, is_float=0, n_fields=1, field=None)
        chans = (Ch*8)()
        for k in range(8):
            chans[k] = Ch(source=L(**{**src, **(source or {})}), gate=L(**gate) if gate else L(), where=1, scale=1., outside=0., hidden=0.)
            for key, value in (channel or {}).items():
                setattr(chans[k], key, value)
        spec = dict(n_views=2, height=16, width=16, samples=1, views=fake, n_channels=n, channels=chans, out=fake)
        w = W(**{**spec, **(windows or {})})
        return entry(ref(grid), ref(w), None) if entry is h.ms_nav_windows else entry(ref(grid), ref(w))

    for entry in (h.ms_nav_windows, h.ms_host_nav_windows):
        for bad in (dict(n_channels=0), dict(n_channels=9), dict(samples=0), dict(samples=5), dict(height=0), dict(height=1025), dict(width=0),
                    dict(width=1025), dict(n_views=0), dict(views=None), dict(out=None), dict(channels=None), dict(views=66), dict(out=66)):
            assert call(windows=bad, entry=entry) == -1, bad
        for bad in (dict(values=None), dict(is_float=2), dict(n_fields=0), dict(n_fields=3), dict(field=66), dict(is_float=1, values=66)):
            assert call(source=bad, entry=entry) == -1, bad
            assert call(source=bad, n=8, entry=entry) == -1, bad
        for bad in (dict(values=fake, is_float=1, n_fields=1), dict(values=fake, is_float=0, n_fields=3), dict(values=fake, is_float=0, n_fields=0)):
            assert call(gate=bad, entry=entry) == -1, bad
        assert call(channel=dict(where=2), entry=entry) == -1
    assert h.ms_nav_windows(None, None, None) == -1 and h.ms_host_nav_windows(ref(grid), None) == -1


def test_the_python_calls_refuse_what_they_cannot_do():
    from megastep_amd import cuda
    geom = np.array([[0, 0, 8, 8], [0, 0, 8, 8]], np.int32)
    starts = np.array([0, 64, 128], np.int64)
    grid = cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)
    maps = cuda.seen_maps(grid, 3)
    floats = torch.zeros(128)
    views = torch.zeros(2, 3, 6)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.local_maps(grid, views, 16, [grid, maps])
    with pytest.raises(RuntimeError, match=r'\(N, P, 6\)'):
        cuda.local_maps(grid, torch.zeros(2, 3, 5), 16, [grid])
    with pytest.raises(RuntimeError, match=r'\(N, P, 6\)'):
        cuda.local_maps(grid, torch.zeros(3, 3, 6), 16, [grid])
    with pytest.raises(RuntimeError, match='3-dimensional'):
        cuda.local_maps(grid, torch.zeros(2, 6), 16, [grid])
    for bad in ([], [grid]*9):
        with pytest.raises(RuntimeError, match='1 to 8'):
            cuda.local_maps(grid, views, 16, bad)
    for bad in (0, 5, 2.):
        with pytest.raises(RuntimeError, match='samples'):
            cuda.local_maps(grid, views, 16, [grid], samples=bad)
    for bad in (0, 1025, (16, 2000)):
        with pytest.raises(RuntimeError, match='size'):
            cuda.local_maps(grid, views, bad, [grid])
    with pytest.raises(RuntimeError, match='gate'):
        cuda.local_maps(grid, views, 16, [cuda.map_channel(grid, gate=floats)])
    with pytest.raises(RuntimeError, match='gate'):
        cuda.local_maps(grid, views, 16, [cuda.MapChannel(cuda.cell_layer(grid), True, 0., cuda.cell_layer(floats), 0., 0.)])
    with pytest.raises(RuntimeError, match='scale'):
        cuda.local_maps(grid, views, 16, [cuda.map_channel(floats)])
    with pytest.raises(RuntimeError, match='scale'):
        cuda.local_maps(grid, views, 16, [cuda.MapChannel(cuda.cell_layer(floats), True, None, None, 0., 0.)])
    with pytest.raises(RuntimeError, match='one per view'):
        cuda.local_maps(grid, views, 16, [cuda.cell_layer(torch.zeros(256, dtype=torch.uint8), 2)])
    with pytest.raises(RuntimeError, match='one per view'):
        cuda.local_maps(grid, views, 16, [cuda.map_channel(grid, gate=cuda.seen_maps(grid, 2))])
    with pytest.raises(RuntimeError, match='entries'):
        cuda.local_maps(grid, views, 16, [cuda.cell_layer(torch.zeros(100, dtype=torch.uint8))])
    with pytest.raises(RuntimeError, match=r'\(N, P\)'):
        cuda.local_maps(grid, views, 16, [cuda.cell_layer(maps, field=torch.zeros((2, 2), dtype=torch.int64))])
    with pytest.raises(RuntimeError, match='integer'):
        cuda.cell_layer(maps, field=torch.zeros((2, 3)))
    with pytest.raises(RuntimeError, match='layer'):
        cuda.cell_layer(torch.zeros(128, dtype=torch.float64))
    for bad in (torch.zeros(2, 3, 2, 16, 15), torch.zeros(2, 3, 1, 16, 16), torch.zeros(2, 3, 2, 16, 16, dtype=torch.float64), 'x'):
        with pytest.raises(RuntimeError, match='out'):
            cuda.local_maps(grid, views, 16, [grid, maps], out=bad)
    # what is accepted as a layer, and with how many stores
    assert cuda.cell_layer(grid).n_fields == 1 and cuda.cell_layer(maps).n_fields == 3 and cuda.cell_layer(maps).values is maps.values
    layer = cuda.cell_layer(maps, field=torch.zeros((2, 3), dtype=torch.int64))
    assert layer.field.dtype == torch.int32 and not layer.is_float and cuda.cell_layer(floats).is_float
    assert cuda.cell_layer(torch.ones(128, dtype=torch.bool)).values.dtype == torch.uint8
