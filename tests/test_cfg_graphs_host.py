"""The planner's test graphs (tests/cfg_graphs.py) on the CPU: the fixed set reaches every planner feature at least twice, the
oracle runs every graph, and its operators applied one layer at a time are its forward pass."""
import numpy as np
import pytest

import cfg_graphs as G

GRAPHS = G.fixed_set()


def test_fixed_set_is_24_seeds_plus_the_directed_graphs():
    assert len(GRAPHS) == 24 + len(G.DIRECTED)
    assert set(G.DIRECTED) == {"up_h16_to_f32", "up_f32_to_h16", "odd_slices", "dup_route", "route_of_routes", "shortcut_into_slice",
                               "linear_shortcut", "big_head", "refused"}
    for name, (cfg, hw, layers) in GRAPHS.items():
        again = G.random_graph(int(name[4:])) if name.startswith("seed") else G.directed_graph(name)
        assert again[0] == cfg and again[1] == hw                      # the same graph in every process
        if name.startswith("seed"):
            assert hw in G.SIZES
            heads = sum(1 for l in layers if l["type"] == "yolo")
            assert heads in (1, 2) and 6 <= len(layers) - 2 * heads - (heads - 1) <= 14
            assert all(l["c"] % 4 == 0 for l in layers if l["type"] != "yolo" and l["c"] != G.HEAD_FILTERS)
    assert len({cfg for cfg, _, _ in GRAPHS.values()}) == len(GRAPHS)


def test_every_planner_feature_is_reached_by_two_graphs():
    cov = G.coverage(GRAPHS)
    for f in G.FEATURES:
        print("%-32s %2d  %s" % (f, len(cov[f]), " ".join(cov[f])))
    assert all(len(cov[f]) >= 2 for f in G.FEATURES), {f: cov[f] for f in G.FEATURES if len(cov[f]) < 2}


def test_directed_graphs_are_what_their_names_say():
    L = {name: GRAPHS[name][2] for name in G.DIRECTED}
    assert "upsample_h16_to_f32" in G.features(L["up_h16_to_f32"]) and "upsample_f32_to_h16" not in G.features(L["up_h16_to_f32"])
    assert "upsample_f32_to_h16" in G.features(L["up_f32_to_h16"])
    p = G.plan_model(L["odd_slices"])
    (cat, cp), = [(i, c) for i, c in p["copies"].items() if c]
    assert cp == [(3, 6)] and L["odd_slices"][cat]["c"] == 16                # the 10-filter conv is copied to channel 6
    assert not any(l["type"] in ("maxpool", "upsample", "shortcut") for l in L["odd_slices"])
    assert any(l["type"] == "route" and l["refs"] == [1, 1] for l in L["dup_route"])
    p = G.plan_model(L["route_of_routes"])
    assert any(p["is_concat"](j) for i, c in p["copies"].items() for j, _ in c)                       # a concatenation copied into another
    assert any(l["type"] == "route" and l["groups"] and p["is_concat"](l["refs"][0]) for l in L["route_of_routes"])
    p = G.plan_model(L["shortcut_into_slice"])
    (sc,) = p["fused"]
    conv, res = sc - 1, L["shortcut_into_slice"][sc]["refs"][1]
    assert conv in p["into"] and not p["h16_before_ties"][p["into"][conv][0]] and p["h16_before_ties"][p["owner_of"](res)[0]]
    p = G.plan_model(L["linear_shortcut"])
    assert not p["fused"] and not p["unfused_two_readers"] and sum(l["type"] == "shortcut" for l in L["linear_shortcut"]) == 2
    big = L["big_head"]
    assert big[-1]["h"] * big[-1]["w"] == 9216 > 8192
    assert [l["type"] for l in L["refused"][:2]] == ["convolutional", "maxpool"] and L["refused"][0]["c"] == 6


@pytest.mark.parametrize("name", list(GRAPHS))
def test_oracle_runs_and_one_step_chained_is_forward(name):
    cfg, hw, layers = GRAPHS[name]
    ref, blob, used = G.make_oracle(cfg, hw)
    assert 20 + 4 * used == len(blob) and used == ref.n_weight_floats()      # the blob is exactly what the oracle consumes
    x = G.graph_input(hw, 3)
    out = ref.forward(x, keep_layers=True)
    assert out.shape[0] == 3 and np.isfinite(out).all()
    tensors = {-1: x}
    for i, l in enumerate(layers):
        tensors[i] = G.one_step(ref, i, {j: tensors[j] for j in set(G.sources(layers, i)) | {i - 1}})
        assert tensors[i].dtype == np.float32 and np.array_equal(tensors[i], ref.layer_outputs[i]), (name, i, l["type"])
        assert tensors[i].shape[1:] == ((l["c"], l["h"], l["w"]) if l["type"] != "yolo" else (3 * l["h"] * l["w"], 6))
    heads = [tensors[i] for i, l in enumerate(layers) if l["type"] == "yolo"]
    assert np.array_equal(np.concatenate(heads, 1), out)
