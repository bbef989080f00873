"""The identity map's memory on the device (csrc/identity_memory_dev.h, csrc/identity.hip) against tests/identity_memory_ref.py.

Trackers are scripted as in tests/test_gpu_identity.py (helpers copied): static, well separated boxes, one seeded unit vector per
person plus a gaussian vector of expected norm 0.05, max_dist = 0.3, a small max_age so that a death takes a few frames.  After EVERY
update the device must equal the restatement: ids, counts and links, the relinked subset, memory(), memory_rows() of every entry BIT
FOR BIT (rows are copies of gallery rows) and the memory counts; every linked cost within BOUND = 3.2e-5 of the oracle's float64 cost
(that file's derived bound: unit vectors, a 512-term fp32 fma chain, gamma_512 = 512 * 2^-24 ~ 3.05e-5 on sum |a b| <= 1; the rows on
both sides are the stored rows).  Enrolled rows are normalised on the device in fp32: the restatement is given the rows the device
stored, after they were held to the float64 normalisation within 1e-6 per component."""
import ctypes as C

import numpy as np
import pytest

import identity_memory_ref as M
from yolo_deepsort_amd import cfgs, synth

pytestmark = pytest.mark.gpu
BOUND = 3.2e-5
EMB = 512
MAXD = 0.3


# ------------------------------------------------------------------------------------------------ helpers (tests/test_gpu_identity.py)
def _centre(seed):
    v = np.random.RandomState(5000 + seed).randn(EMB)
    return v / np.linalg.norm(v)


def _box(i):
    return np.array([40 + 220 * (i % 8), 40 + 300 * (i // 8), 64, 128], np.float32)


def _tracker(**kw):
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.deep_sort import _TrackerHandle
    _lib.init(0)
    p = dict(max_dist=MAXD, max_iou_distance=0.7, max_age=2, n_init=1, nn_budget=40)
    p.update(kw)
    return _TrackerHandle(**p)


class _Cam:
    """A tracker fed by a script: step({box index: centre}) shows each centre (plus this camera's own noise) at its box."""

    def __init__(self, seed, noise=0.05, **kw):
        self.trk, self.rng, self.noise = _tracker(**kw), np.random.RandomState(seed), noise
        self.tracker = self.trk

    def step(self, shown=None):
        shown = shown or {}
        ks = sorted(shown)
        feats = np.stack([(3.0 * (np.asarray(shown[k]) + self.noise * self.rng.randn(EMB) / np.sqrt(EMB))).astype(np.float32) for k in ks]) \
            if ks else np.zeros((0, EMB), np.float32)
        boxes = np.stack([_box(k) for k in ks]) if ks else np.zeros((0, 4), np.float32)
        return self.trk.step(boxes, feats, np.zeros(len(ks), np.float32))


def _twice(*shows):
    """n_init = 1: a track is Tentative in the frame that starts it and Confirmed at its next hit, so every look takes two frames"""
    for _ in range(2):
        for cam, shown in shows:
            cam.step(shown)


def _slots(trk):
    from yolo_deepsort_amd import _lib
    n = len(trk.state()["ids"])
    s = np.zeros(max(n, 1), np.int32)
    _lib.check(_lib.load().yds_tracker_get_slots(trk._h, _lib.ptr(s), max(n, 1)))
    return s[:n].tolist()


def _export(trackers):
    out = []
    for t in trackers:
        st = t.state()
        out.append(M.Cam(st["ids"], st["state"], _slots(t), [t.gallery(i) for i in range(len(st["ids"]))], st["hits"], t.nn_budget))
    return out


def _die(pair, *cams):
    """three misses with max_age = 2, an update after each: the tracks of these cameras die"""
    for _ in range(3):
        for c in cams:
            c.step({})
        pair.update()
    for c in cams:
        assert len(c.trk.state()["ids"]) == 0


class _Pair:
    """The device map and the oracle's, advanced together and compared after every update."""

    def __init__(self, cams, ids=0, rows=8, ttl=None, im=None, rows_sample=None):
        from yolo_deepsort_amd.identity import IdentityMap
        self.trackers = [getattr(c, "trk", c) for c in cams]
        self.im = im or IdentityMap(self.trackers, memory_ids=ids, memory_rows=rows, memory_ttl=ttl)
        self.st = M.MemoryState(len(cams), max_ids=ids, rows_per_id=rows, ttl=ttl)
        self.rows_sample = rows_sample

    def enrol(self, list_of_rows):
        """device enrol; the restatement gets the rows the device stored, each held to the float64 normalisation first"""
        ids = self.im.enrol(list_of_rows)
        stored = [self.im.memory_rows(g) for g in ids]
        for a, got in zip(list_of_rows, stored):
            a = np.asarray(a, np.float64).reshape(-1, EMB)[-self.st.rows_per_id:]
            np.testing.assert_allclose(got, a / np.linalg.norm(a, axis=1, keepdims=True), rtol=0, atol=1e-6)
        assert M.enrol(self.st, stored) == ids
        assert self.im.memory() == self.st.memory()
        return ids

    def compare(self):
        im, S = self.im, len(self.trackers)
        got = im.last_counts()
        ids = [im.ids(s) for s in range(S)]
        links, relinked = im.last_links(), im.last_relinked()
        want = M.update(self.st, _export(self.trackers), im.max_dist, im.max_rows)
        assert ids == want["ids"], (ids, want["ids"])
        assert got == (want["linked"], want["fresh"], want["deferred"]), (got, want)
        assert [l[:3] for l in links] == [l[:3] for l in want["links"]], (links, want["links"])
        assert [l[:3] for l in relinked] == [l[:3] for l in want["relinked"]], (relinked, want["relinked"])
        for g, w in zip(links, want["links"]):
            print("link", g, "oracle cost %.9g" % w[3])
            assert abs(float(g[3]) - w[3]) <= BOUND, (g, w)
        assert [l[3] for l in relinked] == [l[3] for l in links if l[:3] in [r[:3] for r in relinked]]
        assert im.memory() == want["memory"], (im.memory(), want["memory"])
        which = [g for g, _, _ in want["memory"]]
        for g in (which if self.rows_sample is None else [g for g in which if g in self.rows_sample]):
            assert np.array_equal(im.memory_rows(g), self.st.memory_rows(g)), g          # bit for bit: the rows are copies
        assert im.last_memory_counts() == want["counts"], (im.last_memory_counts(), want["counts"])
        return ids, want

    def update(self):
        got = self.im.update()
        assert got == self.im.last_counts()
        return self.compare()


# ------------------------------------------------------------------------------------------------ 1. leave and return
def _leave_and_return(memory_ids):
    A, B = _centre(1), _centre(2)
    c0, c1 = _Cam(11), _Cam(12)
    p = _Pair([c0, c1], ids=memory_ids, rows=4)
    _twice((c0, {0: A}))
    assert p.update()[0] == [{1: 1}, {}]
    c0.step({0: A})
    p.update()                                                  # the identity of update 1 enters the bank at update 2
    old_slot = _slots(c0.trk)[0]
    _die(p, c0)
    c0.step({1: B})
    assert c0.trk.state()["ids"].tolist() == [2] and _slots(c0.trk) == [old_slot]      # B took A's slot and overwrote its rows
    c0.step({1: B})
    assert p.update()[0] == [{2: 2}, {}]                        # B resembles nobody, the departed A included
    _twice((c1, {0: A}))
    c0.step({1: B})
    ids, want = p.update()
    return p, ids, want


def test_leave_and_return():
    p, ids, want = _leave_and_return(4)
    assert ids == [{2: 2}, {1: 1}]                              # A, back in another camera, takes its old id from the memory
    (s, t, g, c), = p.im.last_relinked()
    assert (s, t, g) == (1, 1, 1) and 0 < c < 0.05 and abs(float(c) - want["links"][0][3]) <= BOUND
    assert want["counts"]["relinked"] == 1 and want["cols"][1] == [2, 1]
    assert p.im.memory()[0][:2] == (1, 1)
    ids, want = p.update()                                      # the new holder's newest row joins the ring, one update later
    assert want["counts"]["remembered_rows"] == 1 and p.im.last_relinked() == [] and p.im.memory()[0][:2] == (1, 2)
    ids, want = p.update()                                      # no tracker stepped: nothing is appended
    assert want["counts"]["remembered_rows"] == 0


def test_leave_and_return_without_a_memory_is_a_fresh_id():
    p, ids, want = _leave_and_return(0)
    assert ids == [{2: 2}, {1: 3}] and p.im.last_relinked() == [] and p.im.memory() == []
    assert p.im.last_memory_counts() == dict.fromkeys(M.COUNTS, 0)


# ------------------------------------------------------------------------------------------------ 2. ring contents
def test_ring_wraps_and_keeps_only_the_newest_row():
    A = _centre(3)
    c0 = _Cam(21)
    p = _Pair([c0], ids=2, rows=2)
    _twice((c0, {0: A}))
    p.update()
    newest = []
    for k in range(5):                                          # five updates into a ring of two rows
        for _ in range(3 if k == 2 else 1):                     # three tracker frames between two updates: one row is kept
            c0.step({0: A})
        ids, want = p.update()
        assert want["counts"]["remembered_rows"] == 1
        st = c0.trk.state()
        newest.append(c0.trk.gallery(0)[(int(st["hits"][0]) - 1) % 40])
        got = p.im.memory_rows(1)
        assert len(got) == min(k + 1, 2) and np.array_equal(got[-1], newest[-1]) and (k == 0 or np.array_equal(got[0], newest[-2]))
    ids, want = p.update()                                      # update() twice in a row changes nothing
    assert want["counts"]["remembered_rows"] == 0 and np.array_equal(p.im.memory_rows(1)[-1], newest[-1])


@pytest.mark.parametrize("rows", [1, 4])
def test_two_cameras_append_in_stream_order(rows):
    A = _centre(4)
    c0, c1 = _Cam(31), _Cam(32)
    p = _Pair([c0, c1], ids=2, rows=rows)
    _twice((c0, {0: A}), (c1, {0: A}))
    assert p.update()[0] == [{1: 1}, {1: 1}]
    c0.step({0: A})
    c1.step({0: A})
    ids, want = p.update()
    assert want["counts"]["remembered_rows"] == 2
    r0, r1 = (c.trk.gallery(0)[2] for c in (c0, c1))            # hits = 3: ring position 2
    got = p.im.memory_rows(1)
    if rows == 1:
        assert len(got) == 1 and np.array_equal(got[0], r1)     # more appenders than rows: the last survive
    else:
        assert len(got) == 2 and np.array_equal(got[0], r0) and np.array_equal(got[1], r1)


@pytest.mark.parametrize("budget", [1, 3])
def test_newest_row_under_wrap_of_the_trackers_own_ring(budget):
    A = _centre(5)
    c0 = _Cam(41, nn_budget=budget)
    p = _Pair([c0], ids=2, rows=8)
    _twice((c0, {0: A}))
    p.update()
    for k in range(5):
        for _ in range(1 + k % 2):
            c0.step({0: A})
        p.update()
    st = c0.trk.state()
    assert int(st["hits"][0]) == 9 and len(p.im.memory_rows(1)) == 5
    assert np.array_equal(p.im.memory_rows(1)[-1], c0.trk.gallery(0)[8 % budget])


# ------------------------------------------------------------------------------------------------ 3. ttl at the boundary
@pytest.mark.parametrize("late", [0, 1])
def test_ttl_boundary(late):
    A, ttl = _centre(6), 2
    c0, c1 = _Cam(51), _Cam(52)
    p = _Pair([c0, c1], ids=4, rows=2, ttl=ttl)
    _twice((c0, {0: A}))
    p.update()
    c0.step({0: A})
    p.update()
    _die(p, c0)                                                 # the last of these updates sees no holder
    (gid, n, last), = p.im.memory()
    assert gid == 1 and last == p.st.u - 1
    for _ in range(ttl - 2 + late):                             # departed updates so far: 1; the return is number ttl (+ 1)
        p.update()
    _twice((c1, {0: A}))
    ids, want = p.update()
    assert p.st.u - last == ttl + late
    if late:
        assert ids == [{}, {1: 2}] and want["counts"]["expired"] == 1 and p.im.memory() == [] and p.im.last_relinked() == []
    else:
        assert ids == [{}, {1: 1}] and want["counts"]["expired"] == 0 and len(p.im.last_relinked()) == 1


# ------------------------------------------------------------------------------------------------ 4. capacity
def _come_and_go(p, cam, shown):
    _twice((cam, shown))
    p.update()
    cam.step(shown)
    p.update()
    _die(p, cam)


def test_the_oldest_departed_is_evicted():
    """memory_ids = 2 and three people.  (A new track that matches nothing may face one column at most - two clamped columns are a
    tie the oracle refuses - so C is confirmed while A is still coasting: only B has departed by then.)  B, the HIGHER id, left
    first and is the one evicted for C; back in camera 1, A is relinked and B is a new person."""
    A, B, Cc = _centre(7), _centre(8), _centre(9)
    c0, c1 = _Cam(61), _Cam(62)
    p = _Pair([c0, c1], ids=2, rows=2)
    _twice((c0, {0: A, 1: B}))
    assert p.update()[0][0] == {1: 1, 2: 2}
    for shown in ({0: A, 1: B}, {0: A}, {2: Cc}):               # B's misses: 1, 2; A's: 1; C is Tentative
        c0.step(shown)
        p.update()
    assert [m[0] for m in p.im.memory()] == [1, 2]
    c0.step({2: Cc})                                            # B dies, A coasts, C is confirmed
    ids, want = p.update()
    assert ids[0] == {1: 1, 3: 3} and want["cols"][0] == [2] and want["counts"]["departed"] == 1
    c0.step({2: Cc})                                            # A dies
    ids, want = p.update()                                      # id 3 needs an entry: id 2 was held longest ago
    assert want["counts"]["evicted"] == 1 and [m[0] for m in p.im.memory()] == [1, 3]
    assert p.im.memory()[0][2] == p.st.u - 1
    _twice((c1, {0: A, 1: B}))
    ids, want = p.update()
    assert ids[1] == {1: 1, 2: 4} and [l[:3] for l in p.im.last_relinked()] == [(1, 1, 1)]


def test_departed_in_the_same_update_are_evicted_in_id_order():
    A, B, Cc, D = _centre(10), _centre(11), _centre(12), _centre(13)
    c0 = _Cam(71)
    p = _Pair([c0], ids=2, rows=1)
    _twice((c0, {0: A, 1: B}))
    p.update()
    c0.step({0: A, 1: B})
    p.update()
    _twice((c0, {2: Cc}))                                       # A and B coast while C is confirmed: no column in their own camera
    assert p.update()[0] == [{1: 1, 2: 2, 3: 3}]
    c0.step({2: Cc})                                            # A and B die together
    ids, want = p.update()
    m = p.im.memory()
    assert want["counts"]["evicted"] == 1 and [e[0] for e in m] == [2, 3] and m[0][2] == p.st.u - 1
    _twice((c0, {2: Cc, 3: D}))
    p.update()                                                  # (one departed column: no tie)
    c0.step({2: Cc, 3: D})
    ids, want = p.update()
    assert want["counts"]["evicted"] == 1 and [e[0] for e in p.im.memory()] == [3, 4]


def test_unremembered_until_a_holder_dies():
    A, B = _centre(14), _centre(15)
    c0, c1 = _Cam(81), _Cam(82)
    p = _Pair([c0, c1], ids=1, rows=2)
    _twice((c0, {0: A}))
    p.update()
    for _ in range(2):
        c0.step({0: A})
        c1.step({0: B})
    p.update()
    for _ in range(2):
        c0.step({0: A})
        c1.step({0: B})
        ids, want = p.update()                                  # the one entry is A's and A is alive
        assert want["counts"]["unremembered"] == 1 and [m[0] for m in p.im.memory()] == [1]
    for _ in range(3):
        c0.step({})
        c1.step({0: B})
        ids, want = p.update()
    assert want["counts"] == dict(entries=1, departed=0, relinked=0, remembered_rows=1, expired=0, evicted=1, unremembered=0)
    assert [m[:2] for m in p.im.memory()] == [(2, 1)]


# ------------------------------------------------------------------------------------------------ 5. assignment
def test_a_live_holder_and_a_departed_id_in_one_assignment():
    A, B = _centre(16), _centre(17)
    c0, c1, c2 = _Cam(91), _Cam(92), _Cam(93)
    p = _Pair([c0, c1, c2], ids=4, rows=4)
    _come_and_go(p, c2, {0: B})                                 # B: id 1, departed
    _twice((c0, {0: A}))
    assert p.update()[0][0] == {1: 2}                           # A: id 2, alive in camera 0
    c0.step({0: A})
    _twice((c1, {0: A, 1: B}))
    ids, want = p.update()
    assert want["costs"][1].shape == (2, 2) and ids[1] == {1: 2, 2: 1}
    assert [l[:3] for l in p.im.last_links()] == [(1, 1, 2), (1, 2, 1)] and [l[:3] for l in p.im.last_relinked()] == [(1, 2, 1)]


def test_assignment_with_a_departed_column_is_the_lsap_not_greedy():
    gram = np.array([[1, .8, .90, .89], [.8, 1, .88, .75], [.90, .88, 1, .85], [.89, .75, .85, 1]])
    L = np.zeros((4, EMB))
    L[:, :4] = np.linalg.cholesky(gram)
    c0, c1 = _Cam(101, noise=0.0), _Cam(102, noise=0.0)
    p = _Pair([c0, c1], ids=4, rows=1)
    _twice((c0, {0: L[0]}))
    assert p.update()[0] == [{1: 1}, {}]
    assert p.enrol([L[1][None]]) == [2]
    _twice((c1, {0: L[2], 1: L[3]}))
    ids, want = p.update()
    np.testing.assert_allclose(want["costs"][1], [[.10, .12], [.11, .25]], atol=1e-6)
    assert ids[1] == {1: 2, 2: 1}                               # total 0.23; the smallest entry first would give 0.35
    assert [l[:3] for l in p.im.last_relinked()] == [(1, 1, 2)]


def test_twins_against_one_departed_id():
    A, u = _centre(18), _centre(180)
    twin = (A + 0.3 * u) / np.linalg.norm(A + 0.3 * u)
    c0, c1 = _Cam(111), _Cam(112)
    p = _Pair([c0, c1], ids=4, rows=4)
    _come_and_go(p, c0, {0: A})
    _twice((c1, {0: twin, 1: A}))
    ids, want = p.update()
    assert want["costs"][1].shape == (2, 1) and want["costs"][1][1, 0] < want["costs"][1][0, 0] < MAXD
    assert ids[1] == {1: 2, 2: 1} and [l[:3] for l in p.im.last_relinked()] == [(1, 2, 1)]


# ------------------------------------------------------------------------------------------------ 6. back in two cameras at once
def test_the_same_departed_person_in_two_cameras_in_one_update():
    A = _centre(19)
    c0, c1, c2 = _Cam(121), _Cam(122), _Cam(123)
    p = _Pair([c0, c1, c2], ids=4, rows=4)
    _come_and_go(p, c2, {0: A})
    _twice((c0, {0: A}), (c1, {0: A}))
    ids, want = p.update()
    assert ids == [{1: 1}, {1: 1}, {}]
    assert [l[:3] for l in p.im.last_links()] == [(0, 1, 1), (1, 1, 1)]
    assert [l[:3] for l in p.im.last_relinked()] == [(0, 1, 1)]             # stream 1 linked to stream 0's new holder
    assert want["cols"] == [[1], [1], None] and want["counts"]["departed"] == 0


# ------------------------------------------------------------------------------------------------ 7. the bank kernel's shapes
def _f64_dist(im, queries):
    """float64 over the stored rows: [Q, E] and the ids"""
    mem = im.memory()
    q = np.asarray(queries, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    return np.stack([(1.0 - q @ im.memory_rows(g).astype(np.float64).T).min(1) for g, _, _ in mem], 1), [g for g, _, _ in mem]


def _people(seed, counts):
    rng = np.random.RandomState(seed)
    out = []
    for n in counts:
        c = rng.randn(EMB)
        c /= np.linalg.norm(c)
        out.append((2.5 * (c + 0.05 * rng.randn(n, EMB) / np.sqrt(EMB))).astype(np.float32))
    return out


def _check_dist(im, queries):
    got, gids = im.memory_distances(queries)
    want, wids = _f64_dist(im, queries)
    assert gids == wids and got.shape == want.shape and got.dtype == np.float32
    err = np.abs(got - want).max()
    print("bank distances %s: max |device - float64| = %.3g" % (got.shape, err))
    assert err <= BOUND
    return got


@pytest.mark.parametrize("rows,entries", [(1, 33), (2, 17), (4, 9), (8, 5), (16, 3), (32, 2), (8, 1), (1, 1)])
def test_bank_kernel_shapes(rows, entries):
    """one entry more than a 32-row tile holds (and exactly one entry); entries holding 1 row, all rows, and - from 8 rows on - 5,
    so that the mask falls inside an exchange group; Q = 1, 32, 33; queries near the entries and far from all of them"""
    from yolo_deepsort_amd.identity import IdentityMap
    im = IdentityMap([_tracker()], memory_ids=entries + 3, memory_rows=rows)
    fills = [(1, rows, min(5, rows))[k % 3] for k in range(entries)]
    people = _people(100 + rows, fills)
    ids = im.enrol(people)
    assert ids == list(range(1, entries + 1)) and im.memory() == [(g, n, 0) for g, n in zip(ids, fills)]
    rng = np.random.RandomState(7)
    for Q in (1, 32, 33):
        q = np.concatenate([people[k % entries][:1] for k in range(Q)], 0) + (0.02 * rng.randn(Q, EMB)).astype(np.float32)
        if Q > 1:
            q[Q - 1] = rng.randn(EMB)
        got = _check_dist(im, q)
        assert got[0, 0] < 0.05 and (Q == 1 or (got[Q - 1] > 0.5).all())
    z = np.concatenate([people[0][:1], np.zeros((1, EMB), np.float32)], 0)
    got, _ = im.memory_distances(z)
    assert np.isfinite(got[0]).all() and np.isinf(got[1]).all() and (got[1] > 0).all()          # a zero query: +inf everywhere


def test_bank_kernel_free_entries_stale_rows_and_device_queries():
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.identity import IdentityMap
    trk = _tracker()
    x, m, b, c = _people(200, [8, 8, 3, 5])
    # ---- a free entry between used ones, made by expiry: entries 0 and 1 expire, a later identity takes entry 0 again
    p = _Pair([trk], ids=3, rows=8, ttl=1)
    p.enrol([x, m])
    p.update()
    p.enrol([b])
    ids, want = p.update()
    assert want["counts"]["expired"] == 2 and [g for g, _, _ in p.im.memory()] == [3]
    p.enrol([c])
    assert [g[:2] for g in p.im.memory()] == [(3, 3), (4, 5)]
    got = _check_dist(p.im, np.concatenate([m[:2], b[:1], c[:1]], 0))
    assert (got[:2] > 0.5).all() and got[2, 0] < 0.05 and got[3, 1] < 0.05          # m's rows still lie in the free entry: no match
    # ---- an evicted entry reused by another person: the stale rows behind its row count are those of the very query
    im = IdentityMap([trk], memory_ids=1, memory_rows=8)
    assert im.enrol([x]) == [1] and im.enrol([b[:1]]) == [2] and im.memory() == [(2, 1, 0)]
    got = _check_dist(im, x[5:6])
    assert got[0, 0] > 0.5
    # ---- queries on the device
    q = np.ascontiguousarray(np.concatenate([b[:1], x[:2]], 0))
    dev = _lib.DeviceBuffer.from_array(q)
    got_dev, ids_dev = im.memory_distances((dev.ptr, 3))
    got_host, ids_host = im.memory_distances(q)
    assert ids_dev == ids_host and np.array_equal(got_dev, got_host) and got_dev[0, 0] < 0.05


# ------------------------------------------------------------------------------------------------ 8. LSAP regimes
@pytest.mark.parametrize("n_ids,who", [(3, 2), (70, 41), (3300, 1700)])
def test_lsap_regimes_through_departed_columns(n_ids, who):
    """3 columns: the single-wave form; 70: beyond LSAP_WAVE_COLS = 64; 3300: the solver's state leaves the LDS (global-state form)"""
    v = np.random.RandomState(300 + n_ids).randn(n_ids, EMB)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    c0 = _Cam(131)
    p = _Pair([c0], ids=n_ids + 4, rows=1, rows_sample={1, who, n_ids})
    ids = p.im.enrol([r[None] for r in v.astype(np.float32)])
    assert ids == list(range(1, n_ids + 1))
    stored = [p.im.memory_rows(g) for g in ids]
    assert M.enrol(p.st, stored) == ids
    _twice((c0, {0: v[who - 1]}))
    ids, want = p.update()
    assert want["costs"][0].shape == (1, n_ids)
    assert ids == [{1: who}] and [l[:3] for l in p.im.last_relinked()] == [(0, 1, who)]
    assert want["counts"]["departed"] == n_ids - 1


# ------------------------------------------------------------------------------------------------ 10. reset
def test_reset_empties_the_bank():
    A = _centre(20)
    c0, c1 = _Cam(141), _Cam(142)
    p = _Pair([c0, c1], ids=4, rows=2)
    _come_and_go(p, c0, {0: A})
    assert [m[0] for m in p.im.memory()] == [1]
    p.im.reset()
    p.st.reset()
    assert p.im.memory() == []
    _twice((c1, {0: A}))
    ids, want = p.update()
    assert ids == [{}, {1: 2}] and want["linked"] == 0          # the departed identity is forgotten, the counter keeps counting
    c1.step({0: A})
    ids, want = p.update()
    assert [m[:2] for m in p.im.memory()] == [(2, 1)]


# ------------------------------------------------------------------------------------------------ refusals of the library itself
def test_library_refusals():
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.identity import IdentityMap
    lib = _lib.load()
    im = IdentityMap([_tracker()], memory_ids=2, memory_rows=2)
    for args, word in (((4, 3, -1), "rows_per_id"), ((-1, 8, -1), "max_ids"), ((70000, 8, -1), "max_ids")):
        assert lib.yds_identity_set_memory(im.handle, *args) != 0 and word in _lib.last_error(), _lib.last_error()
    a, b, c = _people(400, [1, 1, 1])
    assert im.enrol([a, b]) == [1, 2]
    assert im.enrol([c]) == [3] and [g for g, _, _ in im.memory()] == [2, 3]          # both departed: the older id goes
    with pytest.raises(_lib.YdsError, match="do not fit"):
        im.enrol([a, b, c])
    assert [g for g, _, _ in im.memory()] == [2, 3]                                     # all or nothing
    rows, n = np.zeros((1, EMB), np.float32), np.array([1], np.int32)
    out = np.zeros(1, np.int32)
    assert lib.yds_identity_enrol(im.handle, _lib.ptr(rows), _lib.ptr(n), 1, _lib.ptr(out)) != 0 and "norm" in _lib.last_error()
    im.set_memory(0)
    assert im.memory() == [] and im.update() == (0, 0, 0)
    with pytest.raises(ValueError, match="needs a memory"):
        im.enrol([a])


# ------------------------------------------------------------------------------------------------ 9. inside the pipeline
def test_memory_inside_the_pipeline():
    """tests/test_gpu_identity.py's pipeline scene (yolov3-tiny 416, three streams on one synthetic scene, injected detections):
    with a memory the map equals the restatement after every step, and result rows, tracker state, search and link are bit-equal
    to the run with identities and no memory; set_memory is refused while a look-ahead pass is in flight."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    from yolo_deepsort_amd.deep_sort import DeepSort, Extractor
    from yolo_deepsort_amd.models import Darknet
    _lib.init(0)
    cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
    net = Darknet(None, img_size=(416, 416), batch_max=8, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0))
    ex = Extractor(synth.reid_state_dict(0), max_crops=256)
    ds_kw = dict(max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)
    counts = [(1, 2, 0), (2, 1, 1), (1, 0, 2), (1, 2, 2), (2, 1, 1), (1, 1, 1), (2, 2, 2), (1, 1, 1)]
    scene = synth.PersonScene(5, frame_hw=(480, 640), seed=3, occlude_frac=0.0)
    heads = net.yolo_heads()
    n_frames = max(sum(c[s] for c in counts) for s in range(3))
    frames = [scene.frame(t) for t in range(n_frames)]
    injs = [synth.head_injection(scene.boxes(t)[1], (480, 640), (416, 416), heads) for t in range(n_frames)]
    steps, nxt = [], [0, 0, 0]
    for c in counts:
        st = []
        for s in range(3):
            st += [(s, nxt[s] + k) for k in range(c[s])]
            nxt[s] += c[s]
        steps.append(st)
    empty = np.zeros((0, 9), np.float32)
    pl.load_injection_sets(net, [[injs[k] for _, k in st] + [empty] * (net.batch_max - len(st)) for st in steps])

    def run(memory_ids):
        trackers = [DeepSort(ex, use_cuda=True, **ds_kw) for _ in range(3)]
        pipe = pl.MultiStreamPipeline(net, trackers, 0.5, 0.4)
        im = pipe.set_identities(True, memory_ids=memory_ids, memory_rows=4)
        pair = _Pair([d.tracker for d in trackers], ids=memory_ids, rows=4, im=im)
        rows, states, found, n_rows = [], [], [], 0
        for i, st in enumerate(steps):
            pl.select_injection_set(net, i)
            dev = _lib.DeviceBuffer.from_array(np.ascontiguousarray(np.stack([frames[k] for _, k in st], 0)))
            rows.append(pipe.step(dev.ptr, 480, 640, [s for s, _ in st]))
            states.append([d.tracker.state() for d in trackers])
            ids, want = pair.compare()
            assert pipe.last_identities() == ids
            n_rows += want["counts"]["remembered_rows"]
            q = trackers[0].tracker.gallery(0)[:1] if len(states[-1][0]["ids"]) else None
            found.append((None if q is None else pipe.search(q, top_k=4),
                          pipe.link(0, int(states[-1][0]["ids"][0]), exclude_stream=0) if q is not None else None))
        if memory_ids:
            assert n_rows > 10 and len(im.memory()) == 5 and all(n == 4 for _, n, _ in im.memory())
            streams = [s for s, _ in steps[-1]]
            pipe.step(dev.ptr, 480, 640, streams, dev.ptr)              # the same frames again, and once more as the look-ahead pass
            with pytest.raises(_lib.YdsError, match="in flight"):
                im.set_memory(8, 4)
            assert len(im.memory()) == 5
            pipe.step(dev.ptr, 480, 640, streams)                       # consumed: nothing is in flight any more
            im.set_memory(8, 4)
            assert im.memory() == []
        return rows, states, found
    rows, states, found = run(64)
    plain_rows, plain_states, plain_found = run(0)
    for i, st in enumerate(steps):
        for b in range(len(st)):
            a, p = rows[i][b], plain_rows[i][b]
            assert (a is None) == (p is None) and (a is None or (a.shape == p.shape and np.array_equal(a, p))), (i, b)
        for s in range(3):
            for key in ("ids", "state", "tsu", "hits", "mean", "cov"):
                assert np.array_equal(states[i][s][key], plain_states[i][s][key]), (i, s, key)
        assert found[i] == plain_found[i], i


def test_detect_streams_identity_memory(tmp_path):
    """tests/test_gpu_identity.py's three cameras on one in-memory clip.  A first run finds the first row of the first track that
    camera 0 confirms; the second run, with a memory, enrols that row before anybody is confirmed: the person is relinked to the
    enrolled id in camera 0, cameras 1 and 2 link to camera 0's new holder, everybody else gets fresh ids, and the yielded items are
    those of the first run."""
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.deep_sort import DeepSort
    from yolo_deepsort_amd.detect import VideoDetector
    from yolo_deepsort_amd.models import Darknet
    _lib.init(0)
    cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
    net = Darknet(None, img_size=(416, 416), batch_max=4, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0, -1.45))
    base = DeepSort(synth.reid_state_dict(0), use_cuda=True, max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)
    img = np.random.RandomState(21).randint(0, 256, (480, 640, 3)).astype(np.uint8)
    clip = [np.roll(img, 3 * t, axis=1) for t in range(12)]
    names = tmp_path / "coco.names"
    names.write_text(cfgs.coco_names_text())
    vd = VideoDetector(net, str(names), thres=0.5, nms_thres=0.4, tracker=base)
    with pytest.raises(ValueError, match="global_ids=True"):
        next(vd.detect_streams([clip] * 3, frames_per_stream=1, show_fps=False, identity_memory=dict(ids=16)))
    with pytest.raises(ValueError, match="memory_rows"):
        next(vd.detect_streams([clip] * 3, frames_per_stream=1, show_fps=False, global_ids=True, identity_memory=dict(ids=16, rows=5)))
    plain, who, row = [], None, None
    for step in vd.detect_streams([clip] * 3, frames_per_stream=1, show_fps=False, global_ids=True):
        ids = vd.stream_identities(0)
        assert vd.stream_identity_map().memory() == []
        if who is None and ids:
            trk = vd._streams_pipe.deepsorts[0].tracker
            who = next(iter(ids))
            row = trk.gallery(trk.state()["ids"].tolist().index(who))[:1].copy()
        plain.append(step)
    assert who is not None
    relinked, final = [], None
    for k, step in enumerate(vd.detect_streams([clip] * 3, frames_per_stream=1, show_fps=False, global_ids=True,
                                               identity_memory=dict(ids=16, rows=4))):
        im = vd.stream_identity_map()
        if k == 0:
            assert im.memory() == [] and im.enrol([5.0 * row]) == [1] and [m[:2] for m in im.memory()] == [(1, 1)]
        relinked += im.last_relinked()
        final = vd.stream_identities()
        for (s, image, det, act), (ps, pimage, pdet, pact) in zip(step, plain[k]):
            assert s == ps and np.array_equal(image, pimage) and act == pact
            assert (det is None) == (pdet is None) and (det is None or np.array_equal(np.asarray(det), np.asarray(pdet)))
    assert [l[:3] for l in relinked] == [(0, who, 1)] and abs(float(relinked[0][3])) <= BOUND
    assert final[0] == final[1] == final[2] and final[0][who] == 1 and len(set(final[0].values())) == len(final[0])
    assert im.memory()[0][1] == 4                               # the enrolled identity's ring filled up behind its new holders
    with pytest.raises(ValueError, match="between the yields"):
        vd.stream_identity_map()
