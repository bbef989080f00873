"""Scenes of the snapshot tests (test_snapshot_host.py, test_gpu_snapshot.py): small random uint8 frames, the rows over them, and
the host SnapshotBook's results, computed once per scene and shared.  A call is a list of (stream, rows, t, frame index)."""
import functools

import numpy as np

from yolo_deepsort_amd import snapshot as S

GEOMETRY_SIZES = [(5, 7), (37, 53), (128, 64), (256, 128), (300, 200)]
GEOMETRY_SPEC = dict(min_w=4, min_h=6, archive=4)


def pack(frames, pad=(1, 3, 5)):
    """Frames of any sizes in one byte buffer with pads between them, so that frames start at odd byte offsets: (buffer uint8,
    offsets, sizes)."""
    parts, offs, pos = [np.zeros(1, np.uint8)], [], 1
    for k, f in enumerate(frames):
        offs.append(pos)
        parts.append(f.reshape(-1))
        gap = pad[k % len(pad)] + (f.size + pad[k % len(pad)]) % 2          # keeps the next offset odd
        parts.append(np.zeros(gap, np.uint8))
        pos += f.size + gap
    return np.concatenate(parts), offs, [f.shape[:2] for f in frames]


@functools.lru_cache(maxsize=None)
def geometry_scene():
    """(images, cases): one image per size and, per case, (image index, row).  Every case is a frame of its own with one row and a
    track id of its own, all of one stream."""
    rs = np.random.RandomState(7)
    images = [rs.randint(0, 256, hw + (3,)).astype(np.uint8) for hw in GEOMETRY_SIZES]
    mw, mh = GEOMETRY_SPEC["min_w"], GEOMETRY_SPEC["min_h"]
    cases = []
    for k, (h, w) in enumerate(GEOMETRY_SIZES):
        bw, bh = max(w // 2, mw), max(h // 2, mh)
        boxes = [
            (w // 4, h // 4, w // 4 + bw, h // 4 + bh),                        # inside
            (0, 0, w, h),                                                      # the whole frame
            (-bw // 2, 1, bw - bw // 2, h - 1),                                # cut by the left edge
            (w - bw // 2, 0, w + bw, h),                                       # ... the right edge
            (1, -bh // 2, w - 1, bh),                                          # ... the top
            (0, h - bh, w, h + 3 * bh),                                        # ... the bottom
            (-3, -5, w - 1, h - 1),                                            # ... a corner
            (w - mw, h - mh, w + 9, h + 9),                                    # ... the far corner, exactly min_w x min_h visible
            (w, 0, w + bw, h), (-bw, -bh, 0, 0), (0, h + 2, w, h + 9),         # wholly outside
            (2, 2, 2, h), (2, 2, w, 2), (w - 1, h - 1, 1, 1),                  # zero and negative extent
            (0, 0, mw, mh), (0, 0, mw - 1, mh), (0, 0, mw, mh - 1),            # exactly at the minimum, one below in each axis
            (1, 0, 2, h), (0, 1, w, 2),                                        # one pixel wide / high
            (-(1 << 30), -(1 << 30), 1 << 30, 1 << 30),                        # far larger than the frame
        ]
        for dh, dw in ((128, 64), (256, 128)):                                 # the COPY and AREA2 shapes, inside and cut
            if h >= dh and w >= dw:
                boxes += [(w - dw, h - dh, w, h), ((w - dw) // 2, (h - dh) // 2, (w - dw) // 2 + dw, (h - dh) // 2 + dh), (w - dw, h - dh, w + 5, h)]
        cases += [(k, b) for b in boxes]
    return images, cases


def geometry_call(cls=0):
    images, cases = geometry_scene()
    return [(0, [list(b) + [i + 1, cls]], 0.1 * i, k) for i, (k, b) in enumerate(cases)]


def run_host(book, call, images, bgr=False):
    """The call through a SnapshotBook, tags = the frame's index in the call."""
    book.begin_call()
    return [book.update(s, rows, t, images[k], tag=f, bgr=bgr) for f, (s, rows, t, k) in enumerate(call)]


# ------------------------------------------------------------------------------------------------ time order within a call
ORDER_HW = (64, 48)
ORDER_SPEC = dict(min_w=8, min_h=16, archive=2)


@functools.lru_cache(maxsize=None)
def order_scene():
    """Three streams x 6 frames, frame k of stream s at index 3 * k + s of the call.  Per stream: frames 0 / 1 and 4 / 5 are
    identical images (ties); id 1 is seen throughout; id 2 wins in frame 0 on a dull image, is beaten in frame 3 on a lively one, is
    last seen there and closes in frame 5 (max_age 1); ids 10, 11, 12 are seen in frame 0 only and close in frame 2 into a ring of
    two (a wrap: a slot is freed); id 20 arrives in frame 3 and takes that slot; id 21 is cut by the frame edge; id 22 is too small;
    ids 30 / 31 are of class 1."""
    h, w = ORDER_HW
    images, call = [], []
    for k in range(6):
        for s in range(3):
            rs = np.random.RandomState(100 + 10 * s + (0 if k == 1 else 4 if k == 5 else k))
            noise = rs.randint(0, 256, (h, w, 3))
            gain = {0: 4, 1: 4, 2: 2, 3: 1, 4: 3, 5: 3}[k]
            images.append((128 + (noise - 128) // gain).astype(np.uint8))
            rows = [[2 + s, 3, 22 + s, 40, 1, 0]]
            if k <= 3:
                rows.append([24, 10 + s, 44, 60, 2, 0])
            if k == 0:
                rows += [[1, 1, 12, 30, 10, 0], [14, 2, 30, 34, 11, 0], [30, 20, 46, 62, 12, 0]]
            if k >= 3:
                rows.append([5, 20, 25, 60, 20, 0])
            if k == 4:
                rows.append([-10, -8, 12 + s, 30, 21, 0])
            if k in (2, 4):
                rows.append([40, 40, 45, 52, 22, 0])
            rows.append([8, 8, 30, 50, 30 + (k % 2), 1])
            call.append((s, rows, 0.04 * k + 0.001 * s, len(images) - 1))
    return images, call


@functools.lru_cache(maxsize=None)
def host_order():
    images, call = order_scene()
    book = S.SnapshotBook(S.SnapSpec(**ORDER_SPEC), max_age=1, n_streams=3)
    return book, run_host(book, call, images)


# ------------------------------------------------------------------------------------------------ mass closes over a full ring
WAVES_SPEC = dict(min_w=8, min_h=16, archive=3)


@functools.lru_cache(maxsize=None)
def waves_scene():
    """One stream, max_age 1, a ring of three: four waves of eight tracks with a picture (and one without) are seen for one frame and
    close together two frames later - from the second wave on MORE pictures close in one frame than the ring holds, over a ring that
    is full of occupants from before that frame.  Two calls; the second also grows the table (70 more tracks) while the ring is full."""
    h, w = ORDER_HW
    rs = np.random.RandomState(11)
    image = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    calls, t = [[], []], 0.0
    for wave in range(4):
        rows = [[(3 * k) % 20, (5 * k) % 30, (3 * k) % 20 + 10 + k, (5 * k) % 30 + 18 + k, 100 * wave + k + 1, 0] for k in range(8)]
        rows.append([0, 0, 3, 3, 100 * wave + 50, 0])
        if wave == 3:
            rows += [[k % 30, k % 40, k % 30 + 9, k % 40 + 17, 1000 + k, 0] for k in range(70)]
        for r in (rows, [], []):
            calls[wave // 2].append((0, r, t, 0))
            t += 0.1
    return [image], calls


@functools.lru_cache(maxsize=None)
def host_waves():
    images, calls = waves_scene()
    book = S.SnapshotBook(S.SnapSpec(**WAVES_SPEC), max_age=1)
    return book, [run_host(book, call, images) for call in calls]


# ------------------------------------------------------------------------------------------------ the scale of the table frame
CROWD_HW = (120, 160)
CROWD_STEPS = (50, 200, 400, 700)


@functools.lru_cache(maxsize=None)
def crowd_scene():
    """One image and 700 rows of one stream: the calls bring the first 50, 200, 400 and all 700 rows (one frame each: the table grows
    through 64, 256, 512 to 1024 with the pictures it holds), then two frames without rows in one call: the whole crowd closes."""
    h, w = CROWD_HW
    rs = np.random.RandomState(3)
    image = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    image[:, : w // 2] //= 3                                                  # (a duller half: scores differ by more than noise)
    x, y = rs.randint(-10, w - 4, 700), rs.randint(-10, h - 8, 700)
    bw, bh = rs.randint(3, 40, 700), rs.randint(6, 70, 700)
    rows = [[int(x[i]), int(y[i]), int(x[i] + bw[i]), int(y[i] + bh[i]), i + 1, 0] for i in range(700)]
    calls = [[(0, rows[:n], 0.1 * c, 0)] for c, n in enumerate(CROWD_STEPS)]
    calls.append([(0, [], 0.5, 0), (0, [], 0.6, 0)])
    return [image], calls


@functools.lru_cache(maxsize=None)
def host_crowd(archive):
    images, calls = crowd_scene()
    book = S.SnapshotBook(S.SnapSpec(archive=archive), max_age=1)
    return book, [run_host(book, call, images) for call in calls]
