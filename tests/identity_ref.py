"""The identity map's rules (include/ydsort.h, yds_identity_update) in plain numpy + scipy: the yardstick of the identity tests.

Inputs are what the library exports, nothing the identity code computes: per tracker its state (ids, state in track-list order),
its slots (yds_tracker_get_slots) and its gallery rows (yds_tracker_get_gallery), plus the previous map.  Distances are float64.

The oracle ASSERTS of its own inputs that no decision is marginal, so that the device's fp32 costs (within 3.2e-5 of these, the
search tests' derived bound) cannot decide differently:
  * every |cost - max_dist| is above MARGIN = 1e-3 (about 30 x that bound);
  * the best and second-best assignment of every stream (on the clamped matrix) differ by more than MARGIN in total.
A scenario that violates a margin fails here; it is not skipped.  ``device_costs`` (the threshold test only) replaces named cost
entries by the device's own fp32 values and switches the margin assertions off.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

CONFIRMED = 2
MARGIN = 1e-3


class Cam:
    """One tracker as exported: ids, state, slots [T] in track-list order, rows = list of float [n,512] arrays."""

    def __init__(self, ids, state, slots, rows):
        self.ids, self.state, self.slots = [int(v) for v in ids], [int(v) for v in state], [int(v) for v in slots]
        self.rows = [np.asarray(r, np.float64).reshape(-1, np.asarray(r).shape[-1]) for r in rows]
        assert len(self.ids) == len(self.state) == len(self.slots) == len(self.rows)


class IdentityState:
    """pairs[stream] = {slot: (owner_track_id, global_id)}; next_id = the next fresh id."""

    def __init__(self, n_streams, next_id=1):
        self.pairs = [dict() for _ in range(n_streams)]
        self.next_id = next_id

    def reset(self):
        self.pairs = [dict() for _ in self.pairs]


def holds(state, s, cam, t):
    owner, gid = state.pairs[s].get(cam.slots[t], (0, 0))
    return gid if (owner == cam.ids[t] and gid > 0) else 0


def track_distance(rows_a, rows_b):
    """min over the stored rows of both tracks of 1 - <r, q>, float64"""
    if len(rows_a) == 0 or len(rows_b) == 0:
        return np.inf
    return float((1.0 - rows_a @ rows_b.T).min())


def _solve(cost):
    r, c = linear_sum_assignment(cost)
    return list(zip(r.tolist(), c.tolist())), float(cost[r, c].sum())


def second_best_gap(cost):
    """total of the second-best assignment minus the optimal total (inf: the optimum is the only assignment).  Any other assignment
    lacks at least one pair of the optimum, so the second best is the cheapest optimum with one of those pairs forbidden."""
    pairs, best = _solve(cost)
    big = float(np.abs(cost).sum() + 1e3)
    alt = np.inf
    for r, c in pairs:
        m = cost.copy()
        m[r, c] = big
        p2, t2 = _solve(m)
        if (r, c) not in p2:                                    # (a 1 x 1 problem has no other assignment)
            alt = min(alt, t2)
    return alt - best


def min_cost_matching(cost, max_dist, check_margin=True):
    """deep_sort/sort/linear_assignment.py:51-72 on a float64 matrix: clamp, scipy, gate.  Returns {row: col} of the kept pairs."""
    cost = np.array(cost, np.float64)
    if cost.shape[0] == 0 or cost.shape[1] == 0:
        return {}
    if check_margin:
        assert (np.abs(cost[np.isfinite(cost)] - max_dist) > MARGIN).all(), "a cost lies within the margin of max_dist:\n%r" % cost
    cost[cost > max_dist] = max_dist + 1e-5
    if check_margin:
        gap = second_best_gap(cost)
        assert gap > MARGIN, "best and second-best assignment differ by %g only:\n%r" % (gap, cost)
    pairs, _ = _solve(cost)
    return {r: c for r, c in pairs if not cost[r, c] > max_dist}


def update(state, cams, max_dist, max_rows, device_costs=None):
    """One update.  state is advanced in place.  Returns dict(ids=[{track_id: gid} per stream, Confirmed tracks in track-list order,
    0 = deferred], links=[(stream, track_id, gid, cost)], linked=, fresh=, deferred=, costs=[per stream the matrix or None])."""
    S = len(cams)
    assert len(state.pairs) == S
    check = device_costs is None
    held = {(s, t): holds(state, s, cams[s], t) for s in range(S) for t in range(len(cams[s].ids)) if cams[s].state[t] == CONFIRMED}
    # 1. new tracks and candidates, 2. admission
    new = [(s, t) for (s, t), g in held.items() if g == 0]      # (dict order = (stream, track-list) order)
    admitted, total = [], 0
    for s, t in new:
        n = len(cams[s].rows[t])
        if total + n > max_rows:
            break
        admitted.append((s, t))
        total += n
    deferred = new[len(admitted):]
    holder = {k: g for k, g in held.items() if g > 0}           # grows as ids are handed out
    links, n_fresh, costs = [], 0, []
    # 4. resolution by stream
    for s in range(S):
        Ns = [t for (ss, t) in admitted if ss == s]
        if not Ns:
            costs.append(None)
            continue
        in_s = {g for (ss, _), g in holder.items() if ss == s}
        cols = sorted({g for (ss, _), g in holder.items() if ss != s} - in_s)
        cost = np.full((len(Ns), len(cols)), np.inf)
        for i, t in enumerate(Ns):
            for j, gid in enumerate(cols):
                ds = [track_distance(cams[s].rows[t], cams[ss].rows[tt]) for (ss, tt), g in holder.items() if g == gid and ss != s]
                cost[i, j] = min(ds)
                if device_costs is not None and (s, cams[s].ids[t], gid) in device_costs:
                    cost[i, j] = float(device_costs[(s, cams[s].ids[t], gid)])
        costs.append(cost.copy())
        match = min_cost_matching(cost, max_dist, check)
        for i, t in enumerate(Ns):
            if i in match:
                gid = cols[match[i]]
                links.append((s, cams[s].ids[t], gid, float(cost[i, match[i]])))
            else:
                gid = state.next_id
                state.next_id += 1
                n_fresh += 1
            holder[(s, t)] = gid
            state.pairs[s][cams[s].slots[t]] = (cams[s].ids[t], gid)
    ids = [{cams[s].ids[t]: holder.get((s, t), 0) for t in range(len(cams[s].ids)) if cams[s].state[t] == CONFIRMED} for s in range(S)]
    return dict(ids=ids, links=links, linked=len(links), fresh=n_fresh, deferred=len(deferred), costs=costs)
