"""Scent fields (include/megastep_hip.h, MsNavScent and MsNavScentQuery) restated in numpy - scent_rule, one
binary32 operation a step, for ONE env: the deposits in a Python loop in ascending k, a sub-step as four shifted np.where
accumulations in the rule's order west, east, south, north.  Every array is float32 and every scalar an np.float32, so numpy
rounds once per operation; underflow is gradual."""
import numpy as np

F = np.float32


def cell_under(geom, c, x, y):
    """(i, j) of the cell under (x, y) as MsNavSeen finds it, or None."""
    jx0, iy0, nx, ny = (int(v) for v in geom)
    with np.errstate(all='ignore'):
        fx, fy = np.floor(F(x)/F(c)), np.floor(F(y)/F(c))
    if not (abs(fx) < 2.**30 and abs(fy) < 2.**30):
        return None
    i, j = int(fy) - iy0, int(fx) - jx0
    return (i, j) if 0 <= i < ny and 0 <= j < nx else None


def _store(field, G, k):
    f = int(field[k]) if field is not None else (0 if G == 1 else k)
    return f if 0 <= f < G else -1


def _shifted(a, fill):
    """a's west, east, south and north neighbours, `fill` beyond the grid (rows do not wrap)."""
    p = np.pad(a, 1, constant_values=fill)
    return p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]


def scent_rule(geom, c, free, V, points, amounts, field, rate, keep, floor, T, reset=None, mask=None):
    """One tick of one env: free (ny, nx) bool, V (G, ny, nx) float32, points (P, 2), amounts (P,), field (P,) or None, reset and
    mask (G,) or None.  Returns (V (G, ny, nx), peaks (G,), scented (G,)) - None in the summary of a store that was masked out."""
    G, V = len(V), V.astype(F).copy()
    rate, keep, floor = F(rate), F(keep), F(floor)
    peaks, scented = [None]*G, [None]*G
    for g in range(G):
        if mask is not None and not mask[g]:
            continue
        x = np.zeros_like(V[g]) if reset is not None and reset[g] else V[g]
        for k in range(len(points)):
            at = cell_under(geom, c, points[k][0], points[k][1])
            if at is not None and free[at] and _store(field, G, k) == g and F(amounts[k]) > 0:
                x[at] = x[at] + F(amounts[k])
        for _ in range(T):
            s = np.zeros_like(x)
            for y, open_ in zip(_shifted(x, F(0)), _shifted(free, False)):
                s = np.where(open_, s + (y - x), s)
            v = (x + rate*s)*keep
            x = np.where(free & (v >= floor), v, F(0)).astype(F)
        V[g], peaks[g], scented[g] = x, x.max(initial=F(0)), int((x > 0).sum())
    return V, peaks, scented


def sniff_rule(geom, c, free, V, points, field):
    """The query of one env: (values (P,), gradients (P, 2)) float32."""
    G, out, grads = len(V), np.zeros(len(points), F), np.zeros((len(points), 2), F)
    for k in range(len(points)):
        at, f = cell_under(geom, c, points[k][0], points[k][1]), _store(field, G, k)
        if at is None or f < 0 or not free[at]:
            continue
        x = V[f][at]
        w, e, s, n = (y[at] if o[at] else x for y, o in zip(_shifted(V[f], F(0)), _shifted(free, False)))
        out[k], grads[k] = x, ((e - w)/(F(2)*F(c)), (n - s)/(F(2)*F(c)))
    return out, grads
