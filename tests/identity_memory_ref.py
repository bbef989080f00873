"""The identity map WITH its memory (include/ydsort.h, yds_identity_set_memory) in plain numpy + scipy: the yardstick of the identity
memory tests.  It restates the five steps of an update - collect, touch, expire, remember, resolve - over what the library exports and
nothing the identity code computes: per tracker its state INCLUDING hits, its slots and its gallery rows in ring order, plus the
previous map and bank.  A track's newest row is ring position (hits - 1) % nn_budget.  Distances are float64.

identity_ref's pieces are reused as they are: ``holds``, ``track_distance`` and ``min_cost_matching``, which carries the margin
assertions (no cost within 1e-3 of max_dist, best and second-best assignment more than 1e-3 apart), so a marginal scenario fails
inside the oracle.  With the memory off ``update`` returns what identity_ref.update returns (tests/test_identity_memory_host.py holds
it to that on random scenarios).
"""
import numpy as np

import identity_ref as R

CONFIRMED = R.CONFIRMED
COUNTS = ("entries", "departed", "relinked", "remembered_rows", "expired", "evicted", "unremembered")


class Cam(R.Cam):
    """identity_ref.Cam plus hits [T] and the tracker's nn_budget (rows[t] is the gallery of track t in ring order)."""

    def __init__(self, ids, state, slots, rows, hits, budget):
        super().__init__(ids, state, slots, rows)
        self.hits, self.budget = [int(v) for v in hits], int(budget)
        assert len(self.hits) == len(self.ids)

    def newest(self, t):
        return self.rows[t][(self.hits[t] - 1) % self.budget]


class Entry:
    def __init__(self, last_held):
        self.rows, self.last_held = [], last_held            # rows: oldest first, at most rows_per_id


class MemoryState(R.IdentityState):
    """identity_ref.IdentityState plus the update counter u, remembered[stream] = {slot: (owner_track_id, hits)} and, with
    max_ids > 0, the bank {global_id: Entry}.  live = the ids with a live holder as of the end of the last update."""

    def __init__(self, n_streams, max_ids=0, rows_per_id=8, ttl=None, next_id=1):
        super().__init__(n_streams, next_id)
        assert max_ids == 0 or rows_per_id in (1, 2, 4, 8, 16, 32)
        self.max_ids, self.rows_per_id, self.ttl = max_ids, rows_per_id, ttl
        self.u, self.bank, self.live = 0, {}, set()
        self.remembered = [dict() for _ in range(n_streams)]

    def reset(self):
        super().reset()
        self.bank, self.live = {}, set()
        self.remembered = [dict() for _ in self.remembered]

    def memory(self):
        return [(g, len(e.rows), e.last_held) for g, e in sorted(self.bank.items())]

    def memory_rows(self, gid):
        return np.stack(self.bank[gid].rows)

    def _take_entry(self, gid, live, counts):
        """an entry for gid by the rule of step 4; False: every entry has a live holder"""
        if len(self.bank) >= self.max_ids:
            departed = sorted((e.last_held, g) for g, e in self.bank.items() if g not in live)
            if not departed:
                return False
            del self.bank[departed[0][1]]
            if counts is not None:
                counts["evicted"] += 1
        self.bank[gid] = Entry(self.u)
        return True


def enrol(state, list_of_rows):
    """One departed entry per array of NORMALISED rows (as the device stored them), under the next fresh ids; returns the ids.
    All or nothing, like the library: ValueError when the entries do not suffice."""
    assert state.max_ids > 0
    free = state.max_ids - len(state.bank)
    departed = sum(1 for g in state.bank if g not in state.live)
    if free + departed < len(list_of_rows):
        raise ValueError("the memory cannot take %d identities" % len(list_of_rows))
    taken = sorted((e.last_held, g) for g, e in state.bank.items() if g not in state.live)[:max(len(list_of_rows) - free, 0)]
    for _, g in taken:
        del state.bank[g]
    ids = []
    for rows in list_of_rows:
        rows = np.asarray(rows)
        assert rows.ndim == 2 and len(rows) >= 1
        e = Entry(state.u)
        e.rows = [r.copy() for r in rows[-state.rows_per_id:]]
        state.bank[state.next_id] = e
        ids.append(state.next_id)
        state.next_id += 1
    return ids


def update(state, cams, max_dist, max_rows):
    """One update.  state is advanced in place.  Returns identity_ref.update's dict (ids, links, linked, fresh, deferred, costs) plus
    relinked = the links that took a departed id, memory = state.memory(), counts = dict over COUNTS, cols = per stream the column
    ids (held ones ascending, then departed ones ascending) or None."""
    S = len(cams)
    assert len(state.pairs) == S
    state.u += 1
    u, on = state.u, state.max_ids > 0
    counts = dict.fromkeys(COUNTS, 0)
    # 1. collect
    held = {(s, t): R.holds(state, s, cams[s], t) for s in range(S) for t in range(len(cams[s].ids)) if cams[s].state[t] == CONFIRMED}
    holder = {k: g for k, g in held.items() if g > 0}           # grows as ids are handed out
    if on:
        live = set(holder.values())
        # 2. touch
        for g, e in state.bank.items():
            if g in live:
                e.last_held = u
        # 3. expire
        if state.ttl is not None:
            for g in [g for g, e in state.bank.items() if g not in live and u - e.last_held > state.ttl]:
                del state.bank[g]
                counts["expired"] += 1
        # 4. remember
        for (s, t), g in holder.items():
            cam, slot = cams[s], cams[s].slots[t]
            owner, seen = state.remembered[s].get(slot, (0, 0))
            if owner == cam.ids[t] and seen == cam.hits[t]:
                continue
            if g not in state.bank and not state._take_entry(g, live, counts):
                counts["unremembered"] += 1
                continue
            e = state.bank[g]
            e.rows = (e.rows + [np.array(cam.newest(t), np.float32)])[-state.rows_per_id:]
            state.remembered[s][slot] = (cam.ids[t], cam.hits[t])
            counts["remembered_rows"] += 1
    # admission
    new = [k for k, g in held.items() if g == 0]
    admitted, total = [], 0
    for s, t in new:
        n = len(cams[s].rows[t])
        if total + n > max_rows:
            break
        admitted.append((s, t))
        total += n
    deferred = new[len(admitted):]
    links, relinked, n_fresh, costs, all_cols = [], [], 0, [], []
    # 5. resolve by stream
    for s in range(S):
        Ns = [t for (ss, t) in admitted if ss == s]
        if not Ns:
            costs.append(None)
            all_cols.append(None)
            continue
        in_s = {g for (ss, _), g in holder.items() if ss == s}
        cols = sorted({g for (ss, _), g in holder.items() if ss != s} - in_s)
        now_live = set(holder.values())
        gone = sorted(g for g, e in state.bank.items() if g not in now_live and len(e.rows) > 0) if on else []
        cost = np.full((len(Ns), len(cols) + len(gone)), np.inf)
        for i, t in enumerate(Ns):
            for j, gid in enumerate(cols):
                cost[i, j] = min(R.track_distance(cams[s].rows[t], cams[ss].rows[tt]) for (ss, tt), g in holder.items() if g == gid and ss != s)
            for j, gid in enumerate(gone):
                cost[i, len(cols) + j] = R.track_distance(cams[s].rows[t], np.stack(state.bank[gid].rows).astype(np.float64))
        costs.append(cost.copy())
        all_cols.append(cols + gone)
        match = R.min_cost_matching(cost, max_dist, True)
        for i, t in enumerate(Ns):
            if i in match:
                gid = (cols + gone)[match[i]]
                link = (s, cams[s].ids[t], gid, float(cost[i, match[i]]))
                links.append(link)
                if match[i] >= len(cols):
                    relinked.append(link)
                    state.bank[gid].last_held = u
            else:
                gid = state.next_id
                state.next_id += 1
                n_fresh += 1
            holder[(s, t)] = gid
            state.pairs[s][cams[s].slots[t]] = (cams[s].ids[t], gid)
            state.remembered[s][cams[s].slots[t]] = (cams[s].ids[t], 0)
    state.live = set(holder.values())
    if on:
        counts["entries"] = len(state.bank)
        counts["departed"] = sum(1 for g in state.bank if g not in state.live)
        counts["relinked"] = len(relinked)
    ids = [{cams[s].ids[t]: holder.get((s, t), 0) for t in range(len(cams[s].ids)) if cams[s].state[t] == CONFIRMED} for s in range(S)]
    return dict(ids=ids, links=links, linked=len(links), fresh=n_fresh, deferred=len(deferred), costs=costs, relinked=relinked,
                memory=state.memory(), counts=counts, cols=all_cols)
