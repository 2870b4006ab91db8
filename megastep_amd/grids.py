"""The two per-floorplan grids the kernels read besides the walls (include/megastep_hip.h), built on the host side: the light
grid (``MsScenery.lg_*``: per cell the lights' verdicts and candidate walls) and the wall grid (``MsScenery.wg_*``: per cell the
walls a ray or an agent in it has to meet). The builders read their settings (``LIGHT_GRID*``, ``WALL_GRID*``) from the scenery's
class, ``cuda.Scenery``, at build time."""
import ctypes as C
import os
import sys
from typing import NamedTuple, Optional
import torch
from . import _lib
from ._lib import _on, _stream


_T = torch.Tensor
#: ``MsScenery.lg_*``: per cell 4 words of verdicts (`vals`) and a list header (`lists`: ``lg_list``), where each env's cells
#: start, each env's grid origin and dims (`geom`), the candidates' pool and, optionally, their walls' rows
LightGrid = NamedTuple('LightGrid', [('vals', _T), ('starts', _T), ('geom', _T), ('cell', float), ('max_cells', int), ('lists', _T),
                                     ('pool', _T), ('pool_rows', Optional[_T])])
#: ``MsScenery.wg_*``: cell headers, starts and geom as above, the cell size, the reaches and near plane the lists hold for,
#: the vis entries, the near lists' rows and where each env's vis lists start
WallGrid = NamedTuple('WallGrid', [('cells', _T), ('starts', _T), ('geom', _T), ('cell', float), ('reach_lo', float), ('reach', float),
                                   ('near', float), ('pool', _T), ('near_rows', _T), ('pool_base', _T)])
#: one level of the wall grid as :func:`scan_level` made it: a WallGrid's tensors (`near_rows` None but on the final level)
#: and each env's number of cells. A coarse level is the parent the next level is scanned against (``MsWallGridParent``).
WallGridLevel = NamedTuple('WallGridLevel', [('cells', _T), ('starts', _T), ('geom', _T), ('cell', float), ('pool', _T),
                                             ('near_rows', Optional[_T]), ('env_cells', _T), ('pool_base', _T)])
#: a table of rows per floorplan (:func:`representatives`): each env's representative (`rep`, `is_rep`), the counts of the
#: representatives (`own`, 0 for the others), where each env's rows - its representative's - start, and the rows in all
Layout = NamedTuple('Layout', [('rep', _T), ('is_rep', _T), ('own', _T), ('starts', _T), ('total', int)])


def struct_fields(lg, wg):
    """The MsScenery fields that point at a light grid and a wall grid (None: no grid), by name."""
    ptr = lambda v: v.data_ptr() if torch.is_tensor(v) else v
    out = {} if wg is None else {'wg_' + k: ptr(v) for k, v in wg._asdict().items()}
    if lg is not None:
        out.update({'lg_' + k: ptr(v) for k, v in lg._asdict().items() if k != 'lists'}, lg_list=lg.lists.data_ptr(), lg_pool_size=lg.pool.shape[0])
    return out


def representatives(per_env, geom):
    """Lays out a table of `per_env` rows per floorplan: the representatives' rows back to back, and every env pointed at
    its representative's. `geom`: see ``Scenery.geom`` (None: every env stands for itself)."""
    arange = torch.arange(len(per_env), device=per_env.device)
    rep = arange if geom is None else geom.to(per_env.device).long()
    is_rep = rep == arange
    own = per_env*is_rep                                               # members own no rows
    return Layout(rep, is_rep, own, (own.cumsum(0) - own)[rep], int(own.sum()))


def _as_u32(t):
    """An int64 tensor of values below 2^32 as the int32 tensor whose bits are those values as uint32."""
    return torch.where(t >= 2**31, t - 2**32, t).to(torch.int32).contiguous()


def grid_budget(sc, setting, fraction):
    """A grid's byte budget: `setting` (Scenery.LIGHT_GRID_BYTES, WALL_GRID_BYTES), else 1/`fraction` of the device's memory - but
    never more than a third of what is FREE on it right now (next to a policy and its optimizer, or on a small GPU, a share of the
    TOTAL is memory that is not there: ADVICE r5; building a wall grid peaks at about twice its final size, so a third of the free
    memory is what can be afforded). 8 GiB for tensors that are not on a GPU."""
    if setting is not None:
        return int(setting)
    dev = sc.lines.vals.device
    if dev.type != 'cuda':
        return 8 << 30
    total = torch.cuda.get_device_properties(dev).total_memory
    try:
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)   # (+ what torch's cache holds idle)
    except Exception:
        free = total
    return int(min(total//fraction, free//3))


def wall_bounds(sc):
    """(n_envs, 2) lower and upper corner of each env's static walls (finite coordinates only; 0, 0 without any)."""
    ln = sc.lines
    dev, n_envs = ln.vals.device, len(ln)
    env = ln.inverse.long()
    static = (torch.arange(ln.vals.shape[0], device=dev) - ln.starts.long()[env]) >= sc.n_agents*sc.model.shape[0]
    env, pts = env[static], ln.vals[static]              # the walls; agent rows move
    big = torch.finfo(torch.float32).max
    fin = torch.isfinite(pts)
    idx = env[:, None].expand(-1, 2)
    lo = torch.full((n_envs, 2), big, device=dev).scatter_reduce_(0, idx, torch.where(fin, pts, big).amin(1), 'amin')
    hi = torch.full((n_envs, 2), -big, device=dev).scatter_reduce_(0, idx, torch.where(fin, pts, -big).amax(1), 'amax')
    empty = (lo > hi).any(1)                             # an env without (finite) walls gets a 1 x 1 grid at the origin
    lo[empty], hi[empty] = 0., 0.
    return lo, hi


# ---------------------------------------------------------------------------------------------------------------------
# the light grid
# ---------------------------------------------------------------------------------------------------------------------
def light_grid(sc):
    """Storage and geometry of the light grid (see include/megastep_hip.h): a uniform grid over each env's walls,
    half a metre of slack around them: per cell the lights' verdicts and a candidate list drawn from a shared pool.
    `bake` fills it in; zeros mean 'unknown, test every wall', which is always safe. Envs that share their
    geometry (`geom`) share their representative's cells. 264 bytes per cell (16 verdicts + 8 list header + 12 pool
    words of 4 + 16 each), i.e. hundreds of times the floorplan's own lines - hence the sharing, the byte budget
    (LIGHT_GRID_BYTES) and no grid at all for single-agent sceneries, whose rays never land on an agent.
    Returns the :class:`LightGrid` and records what was built in ``sc.grid_report()``."""
    dev = sc.lines.vals.device
    lo, hi = wall_bounds(sc)
    origin = torch.floor(lo) - .5
    cell, with_rows = float(sc.LIGHT_GRID_CELL), True
    budget = grid_budget(sc, sc.LIGHT_GRID_BYTES, 8)
    while True:
        dims = torch.ceil((hi + .5 - origin)/cell).clamp(1, 4096)
        # the grid holds 64 lights per env: an env with more gets no cells, and the renderer meets every wall for the
        # rays that land on an agent there (the other envs keep their grids, and the launch stays one kernel)
        dims = torch.where((sc.lights.widths <= 64)[:, None], dims, torch.zeros_like(dims))
        cells = (dims[:, 0]*dims[:, 1]).long()
        lay = representatives(cells, sc.geom)
        words = min(1 + sc.LIGHT_GRID_POOL*lay.total, 2**31 - 1)
        size = 24*(lay.total + 1) + (20 if with_rows else 4)*words
        if size <= budget or cell >= 8.:
            break
        if with_rows:
            with_rows = False
        else:
            cell *= 2
    floorplans = int(lay.is_rep.sum())
    sc._lg_report = dict(bytes=size, cell=cell, cells=lay.total, candidate_rows=with_rows, budget=budget, floorplans=floorplans)
    if os.environ.get('MEGASTEP_VERBOSE'):
        print(f'megastep_amd: light grid of {size/2**20:.0f} MiB: {lay.total} cells of {cell:g} m over {floorplans} floorplans'
              + ('' if with_rows else ', without candidate rows') + (f' (asked for {sc.LIGHT_GRID_CELL:g} m: over the '
              f'{budget/2**30:.1f} GiB budget)' if cell != sc.LIGHT_GRID_CELL or not with_rows else ''), flush=True)
    return LightGrid(
        vals=torch.zeros((lay.total + 1, 4), dtype=torch.int32, device=dev),     # (+ a row for rays outside the last env's grid to read)
        starts=lay.starts.to(torch.int32).contiguous(), geom=torch.cat([origin, dims], 1).float()[lay.rep].contiguous(),
        cell=cell, max_cells=max(int(cells.max()), 1),
        lists=torch.zeros((lay.total + 1, 2), dtype=torch.int32, device=dev), pool=torch.zeros(words, dtype=torch.int32, device=dev),
        # the candidates' walls, next to their entries (MsScenery.lg_pool_rows; optional)
        pool_rows=torch.zeros((words, 4), dtype=torch.float32, device=dev) if with_rows else None)


def shard_light_grid(lg, start, stop, device, geom=None):
    """Envs [start, stop) of a baked :class:`LightGrid`: the cells of the slice's representative envs (`geom`,
    slice-local; None = every env its own) back to back, the candidate lists repacked into a pool of their own (the
    parent's pool is filled in no particular order)."""
    dev = lg.vals.device
    sub_geom = lg.geom[start:stop]
    cells = (sub_geom[:, 2]*sub_geom[:, 3]).long()
    lay = representatives(cells, geom)
    # for every cell of the shard, the parent's row it copies
    src = torch.arange(lay.total, device=dev) + torch.repeat_interleave(lg.starts[start:stop].long() - lay.starts, lay.own, output_size=lay.total)
    rows = lg.lists[src].long() & 0xffffffff
    count = torch.where(rows[:, 1] != 0, rows[:, 1] & 0x7fffffff, torch.zeros_like(rows[:, 1]))
    first = count.cumsum(0) - count                                   # 0-based position in the new pool's payload
    cell_of = torch.repeat_interleave(torch.arange(len(count), device=dev), count)
    take = rows[cell_of, 0] + (torch.arange(int(count.sum()), device=dev) - first[cell_of])
    sub_pool = torch.cat([count.sum()[None].to(lg.pool.dtype), lg.pool[take]])
    sub_rows = None if lg.pool_rows is None else torch.cat([torch.zeros_like(lg.pool_rows[:1]), lg.pool_rows[take]]).to(device).contiguous()
    sub_lists = torch.stack([torch.where(rows[:, 1] != 0, first + 1, torch.zeros_like(first)), rows[:, 1]], 1).to(torch.int32)
    pad = lambda t: torch.cat([t, torch.zeros_like(t[:1])])               # (the row rays outside the last env's grid read)
    return LightGrid(vals=pad(lg.vals[src]).to(device).contiguous().clone(), starts=lay.starts.to(torch.int32).to(device).contiguous(),
                     geom=sub_geom.to(device).contiguous().clone(), cell=lg.cell, max_cells=max(int(cells.max()), 1),
                     lists=pad(sub_lists).to(device).contiguous(), pool=sub_pool.to(device).contiguous(), pool_rows=sub_rows)


# ---------------------------------------------------------------------------------------------------------------------
# the wall grid
# ---------------------------------------------------------------------------------------------------------------------
def scan_level(sc, cell, parent, final, usable):
    """One level of the wall grid: cells of size `cell` over every representative floorplan, scanned (against the
    `parent` level's lists, if there is one) and filled. Returns a :class:`WallGridLevel` - or None where there is nothing
    to build / the budget is exceeded."""
    dev = sc._device()
    ln = sc.lines
    n_envs = len(ln)
    walls = (ln.widths.long() - sc.n_agents*sc.model.shape[0]).clamp(min=0)
    lo, hi = wall_bounds(sc)
    h = _lib.lib()
    origin = torch.floor(lo) - .5
    dims = torch.ceil((hi + .5 - origin)/sc.WALL_GRID_CELL).clamp(min=1)        # in the finest cells ...
    scale = round(cell/sc.WALL_GRID_CELL)
    dims = torch.ceil(dims/scale)                                               # ... so that every level covers the same ground
    cells = (dims[:, 0]*dims[:, 1])
    dims = torch.where(usable[:, None], dims, torch.zeros_like(dims))           # (the same envs at every level)
    cells = torch.where(usable, cells, torch.zeros_like(cells)).long()
    lay = representatives(cells, sc.geom)
    starts = lay.starts.to(torch.int32).contiguous()
    geom = torch.cat([origin, dims], 1).float()[lay.rep].contiguous()
    if lay.total == 0:
        return None
    w32 = (walls + 31)//32
    row_words = 3*lay.own*w32                                          # bitmap words per representative
    reps = torch.nonzero(lay.own > 0).flatten()
    struct = _lib.MsScenery.from_buffer_copy(sc._as_struct())
    struct.wg_starts, struct.wg_geom, struct.wg_cell = starts.data_ptr(), geom.data_ptr(), cell
    struct.wg_reach_lo, struct.wg_reach, struct.wg_near = *sc.WALL_GRID_REACH, sc.WALL_GRID_NEAR
    par = None
    if parent is not None:
        par = _lib.MsWallGridParent(cells=parent.cells.data_ptr(), starts=parent.starts.data_ptr(), geom=parent.geom.data_ptr(),
                                    cell=parent.cell, pool=parent.pool.data_ptr())
    counts = torch.zeros((lay.total, 3), dtype=torch.int32, device=dev)
    # groups of representatives whose bitmaps fit the scratch budget (and a launch's grid)
    words = row_words[reps]
    group = torch.maximum((words.cumsum(0) - words)*4//sc.WALL_GRID_SCRATCH, torch.arange(len(reps), device=dev)//60000)
    bounds = [0] + (torch.nonzero(group[1:] != group[:-1]).flatten() + 1).tolist() + [len(reps)]
    pools, nears = [], []
    budget = grid_budget(sc, sc.WALL_GRID_BYTES, 4)
    cell_rows = torch.zeros((lay.total + 1, 4), dtype=torch.int64, device=dev)     # (+ the row agents outside the last grid read)
    # where each floorplan's vis lists start in the pool (MsScenery.wg_pool_base; the final level's cells count their
    # "first vis entry" from there: a world of thousands of large plans has more entries than 32 bits number)
    pool_base = torch.zeros(n_envs, dtype=torch.int64, device=dev)
    struct.wg_pool_base = pool_base.data_ptr()
    base_p = base_n = 0
    with _on(dev):
        for g0, g1 in zip(bounds[:-1], bounds[1:]):
            r = reps[g0:g1]
            r32 = r.to(torch.int32).contiguous()
            gw = row_words[r]
            bits_starts = torch.zeros(n_envs, dtype=torch.int64, device=dev)
            bits_starts[r] = gw.cumsum(0) - gw
            bits = torch.zeros(max(int(gw.sum()), 1), dtype=torch.int32, device=dev)
            mc = int(cells[r].max())
            groups = int(parent.env_cells[r].max()) if parent is not None else (mc + 3)//4
            _lib.check(h.ms_wallgrid_scan(C.byref(struct), C.byref(par) if par is not None else None, r32.data_ptr(), len(r), groups,
                                          bits_starts.data_ptr(), bits.data_ptr(), counts.data_ptr(), _stream(dev)))
            # the cells of this group, in storage order, and their lists' places in the pools
            span = lay.own[r]
            rows = torch.repeat_interleave(starts[r].long() - (span.cumsum(0) - span), span) + torch.arange(int(span.sum()), device=dev)
            cnt = counts[rows].long()                              # (cells, 3): vis, near within the short reach, near beyond
            n_vis, n_near = cnt[:, 0], cnt[:, 1] + cnt[:, 2]
            if final:                                              # vis -> pool (entries), near -> rows
                off_v, off_n = n_vis.cumsum(0) - n_vis, n_near.cumsum(0) - n_near + base_n
                add_p, add_n = int(n_vis.sum()), int(n_near.sum())
                # ... the vis lists numbered from their floorplan's own start
                first_cell = span.cumsum(0) - span                 # each representative's first cell among this group's
                rep_off = off_v[first_cell.clamp(max=len(off_v) - 1)]
                pool_base[r] = rep_off + base_p
                off_v = off_v - torch.repeat_interleave(rep_off, span)
            else:                                                  # both lists as indices, back to back
                both = torch.stack([n_vis, n_near], 1).flatten()
                off = (both.cumsum(0) - both + base_p).view(-1, 2)
                off_v, off_n = off[:, 0], off[:, 1]
                add_p, add_n = int(both.sum()), 0
            if (4 if final else 2)*(base_p + add_p) + 16*(base_n + add_n) > budget \
                    or (not final and base_p + add_p >= 2**32 - 64) or (final and int(off_v.max()) + int(n_vis.max()) >= 2**32 - 64) \
                    or base_n + add_n >= 2**32 \
                    or int(n_near.max()) > 65535:
                return None
            cell_rows[rows] = torch.stack([off_v, n_vis, off_n, cnt[:, 1] + (n_near << 16)], 1)
            hdr = _as_u32(cell_rows)
            # (final level: vis entries of 32 bits - wall and view arc; a parent level: bare 16-bit wall numbers)
            pool = torch.zeros(add_p + 64, dtype=torch.int32 if final else torch.int16, device=dev)
            near = torch.zeros((max(add_n, 1), 4), dtype=torch.float32, device=dev) if final else None
            struct.wg_cells = hdr.data_ptr()
            # the fill kernel writes at the headers' offsets: hand it this group's pools displaced by what came before
            _lib.check(h.ms_wallgrid_fill(C.byref(struct), r32.data_ptr(), len(r), mc, bits_starts.data_ptr(), bits.data_ptr(),
                                          None if final else C.c_void_p(pool.data_ptr() - 2*base_p),
                                          C.c_void_p(pool.data_ptr() - 4*base_p) if final else None,      # (+ wg_pool_base[n], in the kernel)
                                          C.c_void_p(near.data_ptr() - 16*base_n) if final else None, _stream(dev)))
            torch.cuda.current_stream(dev).synchronize()           # (hdr / bits / pools of this group are done with)
            pools.append(pool[:add_p])
            if final:
                nears.append(near[:add_n])
            base_p, base_n = base_p + add_p, base_n + add_n
    return WallGridLevel(
        cells=_as_u32(cell_rows), starts=starts, geom=geom, cell=float(cell),
        pool=torch.cat(pools + [torch.zeros(64, dtype=pools[0].dtype, device=dev)]),
        near_rows=torch.cat(nears + [torch.zeros((1, 4), dtype=torch.float32, device=dev)]) if final else None,
        env_cells=cells.to(torch.int32), pool_base=pool_base[lay.rep].contiguous())      # (members: their representative's pool base)


def wall_checksum(sc):
    """A 64-bit checksum of the static walls' rows as they are now (their bits, position-weighted, summed modulo 2^64):
    what the wall grid was built from, if taken when it was. (The weights - zero for the agents' rows, which every
    render rewrites - are made once per scenery: the check itself is one multiply-and-sum over the lines.)"""
    ln = sc.lines
    if sc._wg_weights is None:
        af = sc.n_agents*sc.model.shape[0]
        k = torch.arange(ln.vals.shape[0], device=ln.vals.device)
        static = (k - ln.starts.long()[ln.inverse.long()]) >= af
        sc._wg_weights = ((8*k[:, None] + 2*torch.arange(4, device=k.device)[None] + 1)*0x9E3779B1)*static[:, None]   # odd, distinct per word
    return int((ln.vals.reshape(-1, 4).view(torch.int32)*sc._wg_weights).sum())


def wall_grid(sc):
    """Builds the wall grid from the static walls as they are now: per floorplan a uniform grid, per cell the walls a ray
    from the cell can be decided by and the walls an agent in it can run into - first for cells WALL_GRID_COARSE times the
    size, whose lists are all that the cells proper then look at. Returns the :class:`WallGrid`, or None, and records
    what was built in ``sc.grid_report()``. The scenery's own struct must carry no wall grid while this runs."""
    ln = sc.lines
    walls = (ln.widths.long() - sc.n_agents*sc.model.shape[0]).clamp(min=0)
    if len(ln) == 0 or int(walls.max()) <= 0:
        return None
    lo, hi = wall_bounds(sc)
    for cell in (sc.WALL_GRID_CELL, 2*sc.WALL_GRID_CELL, 4*sc.WALL_GRID_CELL):
        # which envs get a grid at all: some walls, not too many for 16-bit indices, not too large an area
        extent = torch.ceil((hi - lo + 1.5)/cell).clamp(min=1)
        usable = (extent[:, 0]*extent[:, 1] <= sc.WALL_GRID_MAX_CELLS) & (walls > 0) & (walls <= 65535)
        parent = None
        if sc.WALL_GRID_COARSE:
            try:
                parent = scan_level(sc, cell*sc.WALL_GRID_COARSE, None, False, usable)
            except torch.cuda.OutOfMemoryError:
                torch.cuda.empty_cache()
        try:
            level = scan_level(sc, cell, parent, True, usable)
        except torch.cuda.OutOfMemoryError:
            # (the budget is an estimate of the final size; the build's peak is higher - on a device that is nearly full the
            # next coarser level is the answer, not a crash)
            level = None
            torch.cuda.empty_cache()
        if level is not None:
            grid = WallGrid(cells=level.cells, starts=level.starts, geom=level.geom, cell=float(cell),
                            reach_lo=float(sc.WALL_GRID_REACH[0]), reach=float(sc.WALL_GRID_REACH[1]), near=float(sc.WALL_GRID_NEAR),
                            pool=level.pool, near_rows=level.near_rows, pool_base=level.pool_base)
            size = sum(t.numel()*t.element_size() for t in grid if torch.is_tensor(t))
            reps = representatives(usable.long(), sc.geom).total           # (the floorplans with a grid)
            budget = grid_budget(sc, sc.WALL_GRID_BYTES, 4)
            sc._wg_report = dict(bytes=size, bytes_per_floorplan=size/max(reps, 1), cell=float(cell), cells=int(grid.cells.shape[0] - 1),
                                 envs=int(usable.sum()), floorplans=reps, vis_entries=int(grid.pool.numel() - 64),
                                 near_rows=int(grid.near_rows.shape[0] - 1), budget=budget, coarsened=cell != sc.WALL_GRID_CELL)
            if os.environ.get('MEGASTEP_VERBOSE') or cell != sc.WALL_GRID_CELL:
                # (a grid that had to coarsen costs the step 3-6 %: never silently)
                print(f'megastep_amd: wall grid of {size/2**20:.0f} MiB for {int(usable.sum())} envs ({reps} floorplans) at {cell:g} m cells'
                      + (f' - {sc.WALL_GRID_CELL:g} m cells would not fit WALL_GRID_BYTES = {budget/2**30:.1f} GiB'
                         if cell != sc.WALL_GRID_CELL else ''), file=sys.stderr, flush=True)
            return grid
    budget = grid_budget(sc, sc.WALL_GRID_BYTES, 4)
    sc._wg_report = dict(bytes=0, cell=None, budget=budget, note='no env a grid could be built for, or none within the budget')
    print(f'megastep_amd: no wall grid built (no env it could serve, or not even {4*sc.WALL_GRID_CELL:g} m cells within WALL_GRID_BYTES = '
          f'{budget/2**30:.1f} GiB): every ray and agent meets every wall of its env', file=sys.stderr, flush=True)
    return None
