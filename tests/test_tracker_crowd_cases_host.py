"""CPU checks of tests/tracker_crowd_cases.py: the reference alone decides every scene with margin, so a mismatch of the fused
association kernel in test_gpu_tracker_crowd.py is a kernel fault and not a coin flip.

  stable      every scene replayed with min_cost_matching's input scaled entrywise by 1 + k * 2^-23, |k| <= 4: the same decisions
  margins     no appearance cost within 1e-3 of max_dist, no gate value within 1 % of the chi-square gate, no IoU cost within 1e-3 of
              max_iou_distance
  truncation  fewer than 1e-3 of the output corners sit within 1e-3 of an integer (half of conftest.check_int_rows's cap)
  forms       the scenes reach the seven solver forms of the fused kernel, the four new ones in both stages"""
import numpy as np
import pytest

import tracker_crowd_cases as K

SEEDS = (1, 2, 3)


@pytest.mark.parametrize("name", K.TRACE_SCENES)
def test_scene_is_stable_under_cost_perturbation(name):
    ref = K.reference(name)
    for seed in SEEDS:
        run = K.oracle_run(name, perturb_seed=seed)
        assert len(run) == len(ref)
        for t, (a, b) in enumerate(zip(run, ref)):
            for key in ("matches", "um_t", "um_d", "ids", "state", "tsu", "hits"):
                assert np.array_equal(a[key], b[key]), (name, seed, t, key)
            assert np.array_equal(a["out"][:, 4:], b["out"][:, 4:]), (name, seed, t)


@pytest.mark.parametrize("name", K.TRACE_SCENES)
def test_scene_keeps_its_margins(name):
    ref = K.reference(name)
    ma = min(r["margin_a"] for r in ref)
    mg = min(r["margin_gate"] for r in ref)
    mb = min(r["margin_b"] for r in ref)
    fl = np.concatenate([r["out_float"].reshape(-1) for r in ref]).astype(np.float64)
    near = int((np.abs(fl - np.rint(fl)) < 1e-3).sum())
    print("%s: margin to max_dist %.4g, to the gate %.4g (relative), to max_iou_distance %.4g; %d of %d output corners within 1e-3 of an "
          "integer; ids up to %d" % (name, ma, mg, mb, near, fl.size, max(int(r["ids"].max(initial=0)) for r in ref)))
    assert ma >= 1e-3 and mb >= 1e-3 and mg >= 1e-2
    assert fl.size > 0 and near / fl.size < 1e-3


def test_crowd_scenes_do_what_the_script_says():
    """misses, deletions, new tracks and stage-A leftovers in the same frames; lists longer than one 256-chunk"""
    for name in ("crowd257_ring", "crowd600_ring"):
        ref = K.reference(name)
        n = K.SCENES[name][1][0]
        assert max(int(r["ids"].max()) for r in ref) > n + 20                 # tentative tracks deleted and re-created
        both = [r for r in ref if len(r["um_t"]) and len(r["um_d"]) and r["dims_a"][0] and r["dims_b"] is not None]
        assert len(both) >= 3
        assert any((r["tsu"] > 0).any() and (r["state"] == 2).any() for r in ref)       # coasting confirmed tracks
        # a frame whose list (old tracks + new ones) is longer than one chunk while tracks are dropped from it and others are new
        sizes = [(len(a["ids"]) + len(b["um_d"]), len(b["um_d"]), len(a["ids"]) + len(b["um_d"]) - len(b["ids"])) for a, b in zip(ref, ref[1:])]
        assert any(total > 256 and new > 0 and dropped > 0 for total, new, dropped in sizes), sizes
    # the sizes where the forms and the chunks change: 64 / 65 confirmed tracks, lists of exactly 256 and 257
    assert {64, 65} <= {max(r["dims_a"]) for r in K.reference("crowd65_unbounded")}
    for name, total in (("crowd256_ring", 256), ("crowd257_ring", 257)):
        ref = K.reference(name)
        assert total in [len(a["ids"]) + len(b["um_d"]) for a, b in zip(ref, ref[1:])], name
    ref = K.reference("collapse3300x5")
    assert len(ref[0]["ids"]) == 3300 and len(ref[1]["ids"]) == 5 and len(ref[5]["ids"]) == 3300


def test_scenes_cover_the_fused_solver_forms():
    a, b = set(), set()
    for name in K.TRACE_SCENES:
        fa, fb = K.forms_of(K.reference(name))
        a |= fa
        b |= fb
    assert a | b == K.REACHABLE_FORMS, (a, b)
    assert K.NEW_FORMS <= a and K.NEW_FORMS <= b, (a, b)
    # the table itself at its edges
    assert [K.fused_form(*s) for s in ((64, 64), (65, 1), (200, 150), (200, 200), (256, 139), (256, 140), (257, 1), (300, 5), (300, 300),
                                       (3200, 1), (3201, 1), (3300, 5), (3300, 12), (0, 5))] == [1, 3, 3, 4, 3, 4, 5, 5, 6, 6, 7, 7, 8, 0]
