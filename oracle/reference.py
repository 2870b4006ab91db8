"""The reference's own kernels, compiled for the host (TEST INFRASTRUCTURE, like everything under oracle/).

``build()`` takes the reference's ``src/kernels.cu`` and ``src/wrappers.cpp`` from ``$MEGASTEP_REFERENCE`` and makes
a CPU Python extension out of them under ``oracle/_ref/``, with the reference's ``Scenery`` / ``Agents`` /
``initialize`` / ``bake`` / ``physics`` / ``render`` surface. It is what ``oracle/megastep_oracle.c`` - and through it
every HIP kernel - is pinned to (``tests/test_reference_pin.py``, ``tests/golden/make_reference_kernels.py``).

The recipe, in three parts:

* shim headers of our own (``oracle/ref_shim/``): a forced-include header that empties the CUDA function qualifiers,
  makes ``blockIdx`` / ``threadIdx`` / ``blockDim`` plain globals, turns ``cudaMemcpyToSymbol`` into a ``memcpy`` and
  device tensors into host tensors, supplies ``sinpif`` / ``cospif`` and a ``ref_launch`` that loops serially over
  blocks and threads; stand-ins for ``math_constants.h`` and ``ATen/cuda/CUDAContext.h``.
* a rewrite of the kernel launches, ``name<<<G, B, 0, stream()>>>(`` -> ``ref_launch(name, Dim3{G}, Dim3{B},``.
  Exactly five, or the build fails. Nothing else of the text changes.
* ``g++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math`` - the oracle's own flags - against the installed torch and
  pybind11 headers, linked to torch / torch_cpu / c10 / torch_python with an rpath.

That is sound because every kernel of the reference is a pure per-thread function of its block and thread indices: no
shared memory, no barriers, no atomics (checked on the source before it is compiled).

Everything made - the rewritten source, the objects, the extension - lies under ``oracle/_ref/``, which git ignores:
nothing derived from the reference's text is ever committed. Where the reference's sources are absent but
``oracle/_ref/`` holds a built module (a machine the tree was copied to), the module is kept and used. Where neither
exists ``build()`` says so in one line and returns None. Sources that are present and do not compile are an error.

THE MODULE IS SINGLE-THREADED BY CONSTRUCTION: the thread indices are globals, and so are the constants that
``initialize`` sets. Every call below goes through one lock; do not call the module from a thread pool or under OpenMP.

``python -m oracle.reference --contract fast`` is a report, not a check: see ``contract_report``.
"""
import ctypes
import hashlib
import importlib.util
import os
import re
import subprocess
import sysconfig
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(_HERE, '_ref')
SHIM = os.path.join(_HERE, 'ref_shim')
ENV = 'MEGASTEP_REFERENCE'
DEFAULT_REFERENCE = '/root/reference'

#: variant -> (module name, floating-point flags). 'pin' carries the oracle's flags; 'fast' is the report's.
VARIANTS = {
    'pin': ('megastep_ref', ['-ffp-contract=off', '-fno-fast-math']),
    'fast': ('megastep_ref_fast', ['-ffp-contract=fast', '-mfma', '-fno-fast-math']),
}

_LAUNCH = re.compile(r'(\w+)\s*<<<(.*?)>>>\s*\(', re.S)
_lock = threading.Lock()
_modules = {}


def source_dir():
    return os.path.join(os.environ.get(ENV, DEFAULT_REFERENCE), 'megastep', 'src')


def sources_present():
    return all(os.path.exists(os.path.join(source_dir(), f)) for f in ('kernels.cu', 'wrappers.cpp', 'common.h'))


def module_path(variant='pin'):
    return os.path.join(OUT, VARIANTS[variant][0] + sysconfig.get_config_var('EXT_SUFFIX'))


def built(variant='pin'):
    return os.path.exists(module_path(variant))


def available():
    """True where the tests can have the module: it is built, or its sources are there to build it from."""
    return built() or sources_present()


def _split_top(text):
    """Splits at the commas that are outside every bracket."""
    parts, depth, cur = [], 0, ''
    for ch in text:
        depth += ch in '{(['
        depth -= ch in '})]'
        if ch == ',' and depth == 0:
            parts.append(cur.strip())
            cur = ''
        else:
            cur += ch
    return parts + [cur.strip()]


def rewrite_launches(text):
    """``name<<<G, B, 0, stream()>>>(`` -> ``ref_launch(name, Dim3{G}, Dim3{B}, ``; G and B may be brace lists already."""
    for word in ('__shared__', '__syncthreads', '__syncwarp', 'atomic', '__shfl', 'cooperative_groups'):
        assert word not in text, f'the reference uses {word}: a serial loop over its threads is no longer its meaning'

    def one(m):
        config = _split_top(m.group(2))
        assert len(config) == 4, config
        grid, block = (c if c.startswith('{') else '{' + c + '}' for c in config[:2])
        return f'ref_launch({m.group(1)}, Dim3{grid}, Dim3{block}, '
    out, n = _LAUNCH.subn(one, text)
    assert n == 5, f'expected the reference\'s five kernel launches, found {n}'
    assert '<<<' not in out
    return out


def _flags(variant):
    import torch
    from torch.utils import cpp_extension
    name, fp = VARIANTS[variant]
    inc = [SHIM] + cpp_extension.include_paths() + [sysconfig.get_paths()['include']]
    try:
        import pybind11
        inc.append(pybind11.get_include())
    except ImportError:
        pass            # torch ships pybind11's headers too
    libdir = os.path.join(os.path.dirname(torch.__file__), 'lib')
    compile_ = ['g++', '-std=c++17', '-O2', *fp, '-fPIC', '-w', '-fvisibility=hidden', f'-DTORCH_EXTENSION_NAME={name}',
                f'-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}', '-DTORCH_API_INCLUDE_EXTENSION_H',
                '-include', os.path.join(SHIM, 'ref_host.h'), '-iquote', source_dir()] + [x for i in inc for x in ('-isystem', i)]
    # common.h defines inverses() in every translation unit that nvcc does not compile: here, in both
    link = ['g++', '-shared', '-Wl,--allow-multiple-definition', f'-L{libdir}', f'-Wl,-rpath,{libdir}',
            '-ltorch', '-ltorch_cpu', '-lc10', '-ltorch_python']
    return compile_, link


def _key(variant):
    h = hashlib.sha256(repr(VARIANTS[variant]).encode())
    files = [os.path.join(source_dir(), f) for f in ('kernels.cu', 'wrappers.cpp', 'common.h')]
    files += [os.path.join(d, f) for d, _, fs in sorted(os.walk(SHIM)) for f in sorted(fs)]
    for f in files:
        with open(f, 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def build(force=False, variant='pin', quiet=False):
    """Builds the extension under oracle/_ref/ and returns its path; None (and one line) where it cannot exist."""
    target = module_path(variant)
    if not sources_present():
        if os.path.exists(target):
            return target
        if not quiet:
            print(f'oracle.reference: no reference sources under ${ENV} ({source_dir()}) and no built module in oracle/_ref/: '
                  'the reference pin is not available here')
        return None
    keyfile = os.path.join(OUT, VARIANTS[variant][0] + '.srchash')
    key = _key(variant)
    if not force and os.path.exists(target) and os.path.exists(keyfile) and open(keyfile).read() == key:
        return target
    os.makedirs(OUT, exist_ok=True)
    name = VARIANTS[variant][0]
    kernels = os.path.join(OUT, name + '_kernels.cpp')
    with open(os.path.join(source_dir(), 'kernels.cu')) as fh:
        text = rewrite_launches(fh.read())
    with open(kernels, 'w') as fh:
        fh.write(text)
    compile_, link = _flags(variant)
    objects = [os.path.join(OUT, name + '_kernels.o'), os.path.join(OUT, name + '_wrappers.o')]
    jobs = [subprocess.Popen(compile_ + ['-DREF_EXPORT_SINCOSPI', '-c', kernels, '-o', objects[0]]),
            subprocess.Popen(compile_ + ['-c', os.path.join(source_dir(), 'wrappers.cpp'), '-o', objects[1]])]
    codes = [j.wait() for j in jobs]
    if any(codes):
        raise RuntimeError(f'oracle.reference: the reference\'s sources are there but did not compile (exit codes {codes})')
    subprocess.check_call(link[:2] + objects + ['-o', target] + link[2:])
    with open(keyfile, 'w') as fh:
        fh.write(key)
    _modules.pop(variant, None)
    return target


def module(variant='pin'):
    """The built extension, imported from oracle/_ref/ (built first where only its sources are there)."""
    if variant not in _modules:
        path = module_path(variant)
        if not os.path.exists(path):
            path = build(variant=variant, quiet=True)
            if path is None:
                raise ImportError('the reference is neither built under oracle/_ref/ nor present as sources')
        import torch  # noqa: F401  (its libraries before the extension's)
        spec = importlib.util.spec_from_file_location(VARIANTS[variant][0], path)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        _modules[variant] = m
    return _modules[variant]


def sincospi(x, variant='pin'):
    """The shim's sinpif / cospif over an array of binary32 arguments: (sin, cos)."""
    module(variant)
    lib = ctypes.CDLL(module_path(variant))
    fp = ctypes.POINTER(ctypes.c_float)
    lib.ref_sincospi_many.argtypes = [fp, fp, fp, ctypes.c_long]
    lib.ref_sincospi_many.restype = None
    x = np.ascontiguousarray(x, np.float32).ravel()
    s, c = np.empty_like(x), np.empty_like(x)
    lib.ref_sincospi_many(x.ctypes.data_as(fp), s.ctypes.data_as(fp), c.ctypes.data_as(fp), len(x))
    return s, c


AGENT_FIELDS = ('angles', 'positions', 'angvelocity', 'velocity')
RENDER_FIELDS = ('indices', 'locations', 'dots', 'distances', 'screen')


class World:
    """The reference's Scenery over one of the oracle's scene dicts (see oracle/oracle.py), and its three calls on numpy
    arrays. ``config`` is (agent_radius, res, fov, fps): the reference keeps these in globals, so every call sets them."""

    def __init__(self, scene, config, variant='pin'):
        import torch
        self.m = module(variant)
        self.config = (float(config[0]), int(config[1]), float(config[2]), float(config[3]))
        t = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt, copy=True, order='C'))
        f, i = np.float32, np.int32
        m = self.m
        with _lock:
            self.scenery = m.Scenery(
                int(scene['n_agents']),
                m.Ragged2D(t(scene['lights_vals'], f).reshape(-1, 3), t(scene['lights_widths'], i)),
                m.Ragged3D(t(scene['lines_vals'], f).reshape(-1, 2, 2), t(scene['lines_widths'], i)),
                m.Ragged2D(t(scene['textures_vals'], f).reshape(-1, 3), t(scene['textures_widths'], i)),
                t(scene['model'], f))
            if scene.get('baked_vals') is not None:
                self.scenery.baked.vals[:] = t(scene['baked_vals'], f)

    @property
    def lines_vals(self):
        return self.scenery.lines.vals.numpy()

    def _agents(self, agents):
        import torch
        return self.m.Agents(*(torch.from_numpy(np.array(agents[k], dtype=np.float32, copy=True, order='C')) for k in AGENT_FIELDS))

    def bake(self):
        with _lock:
            self.m.initialize(*self.config)
            self.m.bake(self.scenery)
            return self.scenery.baked.vals.numpy().copy()

    def physics(self, agents):
        """(progress, agents after the step); the dict passed in is left alone."""
        with _lock:
            self.m.initialize(*self.config)
            a = self._agents(agents)
            progress = self.m.physics(self.scenery, a).progress.numpy().copy()
            return progress, {k: getattr(a, k).numpy().copy() for k in AGENT_FIELDS}

    def render(self, agents):
        with _lock:
            self.m.initialize(*self.config)
            r = self.m.render(self.scenery, self._agents(agents))
            return {k: getattr(r, k).numpy().copy() for k in RENDER_FIELDS}


def contract_report(golden=None):
    """How wide "the reference" itself is: nvcc contracts a*b + c into one fused multiply-add by default, the pin (and the
    oracle) never do. Builds a second variant with ``-ffp-contract=fast -mfma``, runs the golden cases through both and
    prints, per plane, how many masks / indices flip and the largest float difference. Nothing is asserted: gcc's choice
    of which products to fuse is its own, not nvcc's, so this is the size of the effect, not the reference's bits."""
    if 'fma' not in open('/proc/cpuinfo').read().split('flags', 1)[-1].split('\n', 1)[0].split():
        print('this host has no FMA: nothing to report')
        return
    golden = golden or os.path.join(os.path.dirname(_HERE), 'tests', 'golden', 'reference_kernels.npz')
    if build(variant='fast') is None or build() is None:
        return
    from tests import util          # (the goldens' packing lives with the tests that read them)
    worst = {}
    for case, g in util.load_cases(golden).items():
        scene = {k[len('scene_'):]: g[k] for k in g if k.startswith('scene_')}
        scene['n_agents'] = int(g['n_agents'])
        agents = {k: g['agents_' + k] for k in AGENT_FIELDS}
        out = {}
        for variant in ('pin', 'fast'):
            w = World(dict(scene, baked_vals=None), g['config'], variant)
            baked = w.bake()
            progress, after = w.physics(agents)
            out[variant] = dict(baked=baked, progress=progress, **{'after_' + k: v for k, v in after.items()}, **w.render(after))
        a, b = out['pin'], out['fast']
        flips = dict(collision_mask=int(((a['progress'] < 1) != (b['progress'] < 1)).sum()), indices=int((a['indices'] != b['indices']).sum()))
        same = a['indices'] == b['indices']
        floats = {}
        for k in a:
            if k == 'indices':
                continue
            x, y = a[k].astype(np.float64), b[k].astype(np.float64)
            ok = np.isfinite(x) & np.isfinite(y)
            if k in RENDER_FIELDS:
                ok &= same[..., None] if k == 'screen' else same
            floats[k] = float(np.abs(x[ok] - y[ok]).max()) if ok.any() else 0.
        print(f'{case:28s} flips {flips}  max|diff| ' + ' '.join(f'{k}={v:.2e}' for k, v in floats.items()))
        for k, v in {**flips, **floats}.items():
            worst[k] = max(worst.get(k, 0), v)
    print('worst over all cases: ' + ' '.join(f'{k}={v:.3g}' for k, v in worst.items()))


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--contract', choices=['fast'], help='report what fused multiply-adds change on the golden cases')
    ap.add_argument('--force', action='store_true')
    args = ap.parse_args()
    if args.contract:
        contract_report()
    else:
        print(build(force=args.force))
