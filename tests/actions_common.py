"""Shared by tests/test_actions_host.py and tests/test_gpu_actions.py: the reference trace's action set and clock rule, and the
randomised scene of the device-against-host comparison.  The host module (yolo_deepsort_amd.action) with explicit timestamps is
the comparator of every device test."""
import json
import os

import numpy as np

from conftest import GOLD
from yolo_deepsort_amd import action as A


def trace_actions():
    """The action set action_trace.json was recorded with (oracle/gen_golden.py gen_action)."""
    return [A.TakeOff(0, (1, 2)), A.Landing(0, (1, 2)), A.Glide(0, (2, 4)), A.FastCrossing(2, 0.05), A.BreakInto(0, 2), A.BreakInto(2, 1)]


def trace_want():
    return [[tuple(r) for r in f] for f in json.load(open(os.path.join(GOLD, "action_trace.json")))["frames"]]


def fixture_row_times(frames, start=1000.0, step=0.04):
    """Per-row times by the fixture's clock rule: the clock starts at `start` and advances by `step` for every row, in row order,
    whose id is already cached (the rows at which Orbit.update read the stepped clock when the trace was recorded).  A row that
    registers its id gets the clock's current value, which nobody reads.  Needs the cache's membership: replays it with a set and
    ActionIdentify's own ageing (max_age 3)."""
    host = A.ActionIdentify([], max_age=3, max_size=4)
    tick, out = start, []
    for det in frames:
        ts = []
        for r in det:
            if r[4] in host.cache:
                tick += step
            ts.append(tick)
        host.update(det, ts)
        out.append(ts)
    return out


def as_tuples(rows):
    return [(int(a), int(b), str(c)) for a, b, c in rows]


RANDOM_ACTIONS = lambda: [A.TakeOff(0, (1, 2)), A.Landing(0, (1, 2)), A.Glide(0, (2, 2)), A.FastCrossing(2, 0.05), A.BreakInto(0, 2),  # noqa: E731
                          A.BreakInto(2, 1), A.BreakInto(0, 0)]


def random_scene(seed=0, n_ids=300, n_frames=60):
    """Integer positions in [0, 1000), velocity components in [-4, 4] redrawn every 5 frames, widths 10..39 (foot x lands on half
    pixels), height 40, every id visible with probability 0.75, visible rows shuffled, class (i % 2) * 2, frame time t * 0.04."""
    rng = np.random.RandomState(seed)
    pos = rng.randint(0, 1000, (n_ids, 2))
    width = rng.randint(10, 40, n_ids)
    vel = rng.randint(-4, 5, (n_ids, 2))
    frames, times = [], []
    for t in range(n_frames):
        if t % 5 == 0:
            vel = rng.randint(-4, 5, (n_ids, 2))
        pos = pos + vel
        vis = np.nonzero(rng.rand(n_ids) < 0.75)[0]
        rng.shuffle(vis)
        frames.append(np.array([[pos[i, 0], pos[i, 1], pos[i, 0] + width[i], pos[i, 1] + 40, i + 1, (i % 2) * 2] for i in vis],
                               np.int32).reshape(-1, 6))
        times.append(t * 0.04)
    return frames, times
