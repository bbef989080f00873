"""Shared pieces of the zone tests: the fast synthetic scene, the standard geometry and the host-side statistics of a run."""
import numpy as np

from yolo_deepsort_amd import zones as Z


def fast_scene(seed, n_ids, n_frames):
    """[(rows int32 [m, 6], t), ...]: n_ids tracks at integer positions in [0, 1000), velocity components in [-30, 30] redrawn
    every 5 frames, reflected at the borders; boxes 10..39 wide and 40 high hanging below the position; every id visible with
    probability 0.85, the visible rows shuffled; class (i % 2) * 2; frame t at time 0.04 * t."""
    rs = np.random.RandomState(seed)
    pos = rs.randint(0, 1000, (n_ids, 2))
    wid = rs.randint(10, 40, n_ids)
    vel = np.zeros((n_ids, 2), np.int64)
    ids = np.arange(1, n_ids + 1)
    cls = (np.arange(n_ids) % 2) * 2
    frames = []
    for t in range(n_frames):
        if t % 5 == 0:
            vel = rs.randint(-30, 31, (n_ids, 2))
        pos = pos + vel
        low, high = pos < 0, pos >= 1000
        pos = np.where(low, -pos, np.where(high, 1998 - pos, pos))
        vel = np.where(low | high, -vel, vel)
        seen = np.flatnonzero(rs.rand(n_ids) < 0.85)
        rs.shuffle(seen)
        rows = np.stack([pos[seen, 0], pos[seen, 1], pos[seen, 0] + wid[seen], pos[seen, 1] + 40, ids[seen], cls[seen]], 1).astype(np.int32)
        frames.append((rows, 0.04 * t))
    return frames


def standard_geometry():
    zones = [Z.Zone([(100, 100), (500, 120), (520, 480), (90, 500)]),
             Z.Zone([(300, 300), (700, 300), (500, 500), (700, 700), (300, 700)], class_id=0, min_sightings=2),
             Z.Zone([(0, 0), (1000, 0), (1000, 1000), (0, 1000)], class_id=2),
             Z.Zone([(600, 100), (900, 100), (900, 400), (600, 400)], min_sightings=3)]
    lines = [Z.Line((500, 0), (500, 1000)),
             Z.Line((0, 500), (1000, 500), class_id=0),
             Z.Line((100, 100), (900, 900), class_id=2),
             Z.Line((400, 400), (600, 400))]
    return zones, lines


def kind_counts(events_per_frame):
    """Events of each kind over a run's per-frame event lists."""
    n = [0] * 5
    for evs in events_per_frame:
        for e in evs or []:
            n[e[2]] += 1
    return n


def box_at(x2, y, tid=1, cls=0):
    """A row whose DOUBLED foot point is (x2, 2 y): x2 odd puts the foot point half a pixel beside a column (a row's y2 is an
    integer, so the doubled y is always even)."""
    x1 = x2 // 2 - 5
    return [x1, y - 40, x2 - x1, y, tid, cls]
