"""Flow fields (include/megastep_hip.h, MsNavFlows / MsNavFlowQuery) restated in numpy: flow_rule, built on
path_rule's hop table, sight and start (tests/test_navpath_host.py). A `world` is path_rule's - (geom, cell, free, D, q) - with
q None for a seeded or a cost field; `table` is the field's hop table: path_rule.hops, seed_rule.hops or cost_rule.hops."""
import numpy as np

from tests.test_navfield_host import F, INF
from tests.test_navpath_host import NAN, NEIGHBOURS, path_rule
from tests.test_navseed_host import seed_rule

FLOW_GOAL = -2


class flow_rule:
    @staticmethod
    def live(world):
        with np.errstate(invalid='ignore'):
            return world[2] & (world[3] < INF)

    @staticmethod
    def targets(world, table, L, only=None):
        """(ny, nx) int32 targets - with `only` (k, 2), live cells, of those alone, the others left at -1."""
        geom, cell, free, D, q = world
        kind, step, _ = table
        ny, nx = D.shape
        out = np.full((ny, nx), -1, np.int32)
        for i, j in np.argwhere(flow_rule.live(world)) if only is None else only:
            cells, goal = [(int(i), int(j))], False
            while len(cells) < L:
                a, b = cells[-1]
                if kind[a, b] == 0 and q is not None:
                    goal = True
                if kind[a, b] != 1:
                    break
                di, dj = NEIGHBOURS[step[a, b]]
                cells.append((a + di, b + dj))
            points = [path_rule.centre(geom, cell, a, b) for a, b in cells] + ([(F(q[0]), F(q[1]))] if goal else [])
            k = min(1, len(points) - 1)
            if len(points) > 2:
                xs, ys = (np.array([pt[a] for pt in points[2:]], F) for a in (0, 1))
                seen = np.nonzero(path_rule.sights(world, points[0], xs, ys))[0]
                if len(seen):
                    k = 2 + int(seen[-1])
            out[i, j] = FLOW_GOAL if goal and k == len(points) - 1 else cells[k][0]*nx + cells[k][1]
        return out

    @staticmethod
    def at(world, table, targets, p):
        """((x, y), took): the answer at point p on a store of `targets` (ny, nx)."""
        geom, cell, free, D, q = world
        ny, nx = D.shape
        first = path_rule.start(world, p)
        if first is None:
            return (NAN, NAN), -1
        i, j, _ = first
        t = int(targets[i, j])
        if not (0 <= t < ny*nx or (t == FLOW_GOAL and q is not None)):
            return (NAN, NAN), -1
        w = (F(q[0]), F(q[1])) if t == FLOW_GOAL else path_rule.centre(geom, cell, t//nx, t % nx)
        if t == i*nx + j or path_rule.sights(world, p, np.array([w[0]], F), np.array([w[1]], F))[0]:
            return w, 1
        fallback = path_rule.waypoint(world, p, 2, table) if q is not None else seed_rule.waypoint(world[:4], p, 2, table)
        return fallback[0], 0
