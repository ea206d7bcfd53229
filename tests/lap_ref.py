"""The assignment solver of csrc/track_core.h (bt_lap) restated in NumPy, with its tie rule as a parameter.

lap_ref(cost, limit) solves the problem lap.lapjv(cost, extend_cost=True, cost_limit=limit) poses -- T rows, D columns, any row or
column may stay unmatched at limit / 2 each -- by successive shortest augmenting paths over T rows and D + 1 columns: column D is
"unmatched" at cost `limit`, is never marked used, and so takes any number of rows.  The u / v / minv / way updates run in bt_lap's
order with its operand order (cost - u - v), so on a tie-free problem every intermediate is the device's.

tie = "first"   the first (lowest) column among equal minima wins and an equal slack does not replace a path: bt_lap's rule
tie = "last"    the last column among equal minima wins.  Only there to show that a case can tell the two rules apart.
tie = "relax"   the first column wins, but an equal slack DOES replace a path (`<=` where bt_lap has `<`).  Only there for the cases whose
                tie is between two rows, which no column rule can see.

It plugs into the oracle as oracle.bytetrack.lapjv_extended (same signature and result); tests do that with monkeypatch."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def lap_ref(cost, limit, tie="first"):
    cost = np.asarray(cost, np.float64)
    T, D = cost.shape
    x = np.full(T, -1, np.int64)
    p = np.full(D + 1, -1, np.int64)
    u = np.zeros(T)
    v = np.zeros(D + 1)
    if D > 0:
        ext = np.concatenate([cost, np.full((T, 1), float(limit))], axis=1)
        for r in range(T):
            minv = np.full(D + 1, DBL_MAX)
            used = np.zeros(D + 1, bool)
            way = np.full(D + 1, -1, np.int64)
            i0, j0 = r, -1
            while True:
                cur = ext[i0] - u[i0] - v
                better = (cur <= minv) if tie == "relax" else (cur < minv)
                better &= ~used
                minv[better] = cur[better]
                way[better] = j0
                free = np.nonzero(~used)[0]
                m = minv[free].min()
                hits = free[minv[free] == m]
                j1 = int(hits[-1] if tie == "last" else hits[0])
                delta = minv[j1]
                uj = np.nonzero(used)[0]
                u[p[uj]] += delta
                v[uj] -= delta
                minv[~used] -= delta
                u[r] += delta
                j0 = j1
                if j1 == D or p[j1] < 0:
                    break
                used[j1] = True
                i0 = int(p[j1])
            j = j0
            while True:                                    # augment along way[]
                jp = int(way[j])
                row = r if jp < 0 else int(p[jp])
                if j == D:
                    x[row] = -1
                else:
                    p[j] = row
                    x[row] = j
                if jp < 0:
                    break
                j = jp
    return x, p[:D].copy()


def objective(cost, limit, x, y):
    """What the extended problem minimises: matched cost plus limit / 2 per unmatched row and per unmatched column."""
    cost = np.asarray(cost, np.float64)
    x = np.asarray(x)
    rows = np.nonzero(x >= 0)[0]
    return float(cost[rows, x[rows]].sum() + (limit / 2.0) * ((x < 0).sum() + (np.asarray(y) < 0).sum()))


def first(cost, limit):
    return lap_ref(cost, limit, "first")


def last(cost, limit):
    return lap_ref(cost, limit, "last")


def relax(cost, limit):
    return lap_ref(cost, limit, "relax")
