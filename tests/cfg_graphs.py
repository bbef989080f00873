"""Small Darknet graphs for the detector planner: a seeded generator, directed cases, a model of the planner's storage
decisions (for coverage only) and the oracle's operators applied to one layer at a time.  Needs no GPU."""
import numpy as np

F32 = np.float32
SIZES = ((16, 16), (24, 16), (20, 28))
CHANNELS = (8, 16, 24, 32, 64, 96, 128)          # multiples of 4 on both sides of the 32- and 64-channel rules
ACTS = ("leaky", "mish", "linear")
ANCHORS = "10,14, 23,27, 37,58, 81,82, 135,169, 344,319"
N_RANDOM = 24
HEAD_FILTERS = 18                                # three anchors x (5 + 1 class)


# ------------------------------------------------------------------------------------------ cfg blocks
def _conv(f, k=3, s=1, act="leaky"):
    return {"type": "convolutional", "batch_normalize": "1", "filters": str(f), "size": str(k), "stride": str(s), "pad": "1",
            "activation": act}


def _head_conv():
    # no batch_normalize key: the oracle's weight loader tests the string's truthiness, like the reference
    return {"type": "convolutional", "size": "1", "stride": "1", "pad": "1", "filters": str(HEAD_FILTERS), "activation": "linear"}


def _yolo(mask="0,1,2"):
    return {"type": "yolo", "mask": mask, "anchors": ANCHORS, "classes": "1", "num": "6"}


def _pool(k, s):
    return {"type": "maxpool", "size": str(k), "stride": str(s)}


def _up():
    return {"type": "upsample", "stride": "2"}


def _route(*ls, group_id=None):
    d = {"type": "route", "layers": ",".join(str(l) for l in ls)}
    if group_id is not None:
        d["groups"] = "2"
        d["group_id"] = str(group_id)
    return d


def _shortcut(frm):
    return {"type": "shortcut", "from": str(frm), "activation": "linear"}


def cfg_text(defs, hw):
    out = ["[net]", "channels=3", f"height={hw[0]}", f"width={hw[1]}", ""]
    for d in defs:
        out.append(f"[{d['type']}]")
        out += [f"{k}={v}" for k, v in d.items() if k != "type"]
        out.append("")
    return "\n".join(out)


def describe(defs, hw):
    """Per layer: type, output shape (c, h, w), the layers it reads (absolute indices; -1 is the image) and its operator's
    parameters.  This is the `layers` every predicate below takes."""
    layers = []
    pc, ph, pw = 3, hw[0], hw[1]
    for i, d in enumerate(defs):
        t = d["type"]
        l = {"type": t, "src": i - 1, "refs": []}
        c, h, w = pc, ph, pw
        if t == "convolutional":
            k, s = int(d["size"]), int(d["stride"])
            pad = (k - 1) // 2
            c, h, w = int(d["filters"]), (ph + 2 * pad - k) // s + 1, (pw + 2 * pad - k) // s + 1
            l.update(k=k, stride=s, act=d["activation"])
        elif t == "maxpool":
            k, s = int(d["size"]), int(d["stride"])
            if not (k == 2 and s == 1):
                pad = (k - 1) // 2
                h, w = (ph + 2 * pad - k) // s + 1, (pw + 2 * pad - k) // s + 1
            l.update(k=k, stride=s)
        elif t == "upsample":
            h, w = ph * 2, pw * 2
        elif t == "route":
            refs = [int(v) for v in d["layers"].split(",")]
            refs = [r if r >= 0 else i + r for r in refs]
            assert all(0 <= r < i for r in refs), (i, refs)
            assert len({(layers[r]["h"], layers[r]["w"]) for r in refs}) == 1, (i, "route joins different sizes")
            c, h, w = sum(layers[r]["c"] for r in refs), layers[refs[0]]["h"], layers[refs[0]]["w"]
            l.update(src=-2, refs=refs, groups=int(d.get("groups", 0)), group_id=int(d.get("group_id", 0)))
            if l["groups"]:
                assert c % l["groups"] == 0
                c //= l["groups"]
        elif t == "shortcut":
            f = int(d["from"])
            f = f if f >= 0 else i + f
            assert 0 <= f < i and (layers[f]["c"], layers[f]["h"], layers[f]["w"]) == (pc, ph, pw), (i, "shortcut shape")
            l.update(src=-2, refs=[i - 1, f])
        l.update(c=c, h=h, w=w)
        layers.append(l)
        pc, ph, pw = c, h, w
    return layers


def sources(layers, i):
    """Layers whose outputs layer i reads, absolute indices, -1 for the image."""
    l = layers[i]
    return list(l["refs"]) if l["type"] in ("route", "shortcut") else [i - 1]


# ------------------------------------------------------------------------------------------ random graphs
def random_graph(seed):
    """(cfg_text, (h, w), layers): a valid cfg of 6 to 14 layers before one or two 18-filter heads."""
    rng = np.random.RandomState(7000 + seed)
    hw = SIZES[rng.randint(len(SIZES))]
    target = rng.randint(6, 15)
    defs = [_conv(CHANNELS[rng.randint(len(CHANNELS))], 3, 1 + rng.randint(2), ACTS[rng.randint(2)])]

    def pick(seq):
        return seq[rng.randint(len(seq))]

    def same_size(L, j, k):
        return (L[j]["h"], L[j]["w"]) == (L[k]["h"], L[k]["w"])

    def grow(defs, budget):
        L = describe(defs, hw)
        n, cur = len(L), L[-1]
        room = budget - n
        kinds = ["conv"] * 5 + ["pool21", "route1", "groute", "mroute", "mroute", "shortcut"]
        if room >= 3:
            kinds += ["res", "res", "csp", "csp"]
        if room >= 4:
            kinds += ["spp", "res_tap", "res_tap"]
        if min(cur["h"], cur["w"]) >= 4:
            kinds += ["pool22", "conv_s2", "conv_s2"]
        if max(cur["h"], cur["w"]) <= 14:
            kinds += ["up"]
            if room >= 3 and any((L[j]["h"], L[j]["w"]) == (2 * cur["h"], 2 * cur["w"]) for j in range(n)):
                kinds += ["fpn"] * 4
            if room >= 4:
                kinds += ["tap_up"] * 2
        kind = pick(kinds)

        def prefer_narrow(ok):
            narrow = [j for j in ok if L[j]["c"] % 32]
            return pick(narrow) if narrow and rng.randint(4) else pick(ok)
        if kind == "conv_s2":
            return [_conv(pick(CHANNELS), 3, 2, pick(ACTS))]
        if kind == "res_tap":
            # the 3x3 conv is read by the shortcut and by the route: the shortcut cannot be fused into it
            act = pick(ACTS[:2])
            return [_conv(pick(CHANNELS), 1, 1, act), _conv(cur["c"], 3, 1, act), _shortcut(-3), _route(-1, -2)]
        if kind == "fpn":
            # a wide conv upsampled next to an earlier tensor of the doubled size
            j = prefer_narrow([j for j in range(n) if (L[j]["h"], L[j]["w"]) == (2 * cur["h"], 2 * cur["w"])])
            return [_conv(pick(CHANNELS[3:]), 1, 1, pick(ACTS)), _up(), _route(-1, j)]
        if kind == "tap_up":
            # a wide conv that lands in a concatenation and is upsampled from there into a buffer of its own
            j = prefer_narrow([j for j in range(n) if same_size(L, j, n - 1)])
            return [_conv(pick(CHANNELS[3:]), 1, 1, pick(ACTS)), _route(-1, j), _route(-2), _up()]
        if kind == "conv":
            return [_conv(pick(CHANNELS), pick((1, 3)), 1, pick(ACTS))]
        if kind == "res":
            act = pick(ACTS[:2])
            return [_conv(pick(CHANNELS), 1, 1, act), _conv(cur["c"], 3, 1, act), _shortcut(-3)]
        if kind == "csp":
            act = pick(ACTS[:2])
            return [_conv(pick(CHANNELS), 1, 1, act), _route(-2), _conv(pick(CHANNELS), 1, 1, act)]
        if kind == "pool22":
            return [_pool(2, 2)]
        if kind == "pool21":
            return [_pool(2, 1)]
        if kind == "spp":
            if room >= 6 and rng.randint(2):
                return [_pool(5, 1), _route(-2), _pool(9, 1), _route(-4), _pool(13, 1), _route(-1, -3, -5, -6)]
            return [_pool(5, 1), _route(-2), _pool(9, 1), _route(-1, -3, -4)]
        if kind == "up":
            return [_up()]
        if kind == "route1":
            j = rng.randint(n)
            return [_route(j if rng.randint(2) else j - n)]
        if kind == "groute":
            ok = [j for j in range(n) if L[j]["c"] % 8 == 0]
            if not ok:
                return None
            j = ok[-1] if rng.randint(2) else pick(ok)
            return [_route(j if rng.randint(2) else j - n, group_id=rng.randint(2))]
        if kind == "mroute":
            anchor = n - 1 if rng.randint(3) else rng.randint(n)
            ok = [j for j in range(n) if same_size(L, j, anchor)]
            if len(ok) < 2 and rng.randint(2):
                return None
            refs = [anchor] + [pick(ok) for _ in range(rng.randint(1, 4))]
            rng.shuffle(refs)
            return [_route(*[j if rng.randint(2) else j - n for j in refs])]
        if kind == "shortcut":
            ok = [j for j in range(n - 1) if (L[j]["c"], L[j]["h"], L[j]["w"]) == (cur["c"], cur["h"], cur["w"])]
            if not ok:
                return None
            j = pick(ok)
            return [_shortcut(j if rng.randint(2) else j - n)]
        raise AssertionError(kind)

    while len(defs) < target:
        add = grow(defs, 14)
        if add is not None and len(defs) + len(add) <= 14:
            defs += add
    body = len(defs)
    defs += [_head_conv(), _yolo("0,1,2")]
    if rng.randint(2):
        defs += [_route(rng.randint(body)), _head_conv(), _yolo("3,4,5")]
    return cfg_text(defs, hw), hw, describe(defs, hw)


# ------------------------------------------------------------------------------------------ directed graphs
def _directed_defs():
    g = {}
    # a 64-channel conv (its own buffer: split-fp16 record) upsampled into a slice of a 72-channel (fp32) concatenation
    g["up_h16_to_f32"] = ((16, 16), [_conv(8, 3, 1), _conv(64, 3, 2, "mish"), _up(), _route(-1, 0), _conv(32, 1, 1)])
    # the mirror: the 64-channel conv lands in a 72-channel (fp32) concatenation and is upsampled into a buffer of its own
    g["up_f32_to_h16"] = ((16, 16), [_conv(8, 3, 2), _conv(64, 3, 1, "mish"), _up(), _conv(32, 1, 1), _route(1, 0), _conv(16, 1, 1),
                                     _up(), _route(-1, 3)])
    # 6 + 10 filters concatenated to 16: the second slice sits at channel 6 and is copied value by value
    g["odd_slices"] = ((16, 16), [_conv(16, 3, 1), _conv(6, 1, 1, "mish"), _route(-2), _conv(10, 1, 1, "mish"), _route(-3, -1),
                                  _conv(16, 3, 1)])
    g["dup_route"] = ((16, 16), [_conv(16, 3, 1), _conv(32, 3, 2, "mish"), _route(-1, -1), _conv(24, 1, 1), _route(-1, -1),
                                 _conv(32, 1, 1)])
    # a concatenation inside a concatenation, grouped views of concatenations
    g["route_of_routes"] = ((24, 16), [_conv(32, 3, 1), _conv(32, 3, 1, "mish"), _route(-1, -2), _conv(64, 1, 1), _route(-1, -2),
                                       _route(-1, group_id=1), _conv(32, 3, 1), _route(2, group_id=0), _route(-1, -2, 2), _conv(32, 1, 1)])
    # conv + fused shortcut written into a 40-channel (fp32) concatenation; the residual source keeps the split-fp16 record
    g["shortcut_into_slice"] = ((16, 16), [_conv(8, 3, 1), _conv(32, 3, 1, "mish"), _conv(16, 1, 1), _conv(32, 3, 1, "leaky"),
                                           _shortcut(-3), _route(-1, 0), _conv(32, 1, 1)])
    # a LINEAR conv before a shortcut: no conv epilogue adds a residual after a linear activation, so the add keeps its own launch
    g["linear_shortcut"] = ((16, 16), [_conv(8, 3, 1), _conv(32, 3, 1, "mish"), _conv(16, 1, 1), _conv(32, 3, 1, "linear"),
                                       _shortcut(-3), _route(-1, 0), _conv(32, 1, 1, "linear"), _shortcut(1)])
    g["big_head"] = ((96, 96), [_conv(8, 3, 1)])
    g["refused"] = ((16, 16), [_conv(6, 3, 1), _pool(2, 2)])
    return g


DIRECTED = tuple(_directed_defs())


def directed_graph(name):
    hw, defs = _directed_defs()[name]
    defs = defs + [_head_conv(), _yolo("0,1,2")]
    return cfg_text(defs, hw), hw, describe(defs, hw)


def fixed_set():
    """name -> (cfg_text, (h, w), layers): 24 seeds and the directed graphs."""
    out = {f"seed{s}": random_graph(s) for s in range(N_RANDOM)}
    out.update({name: directed_graph(name) for name in DIRECTED})
    return out


# ------------------------------------------------------------------------------------------ the planner's storage decisions
def plan_model(layers):
    """What csrc/darknet.cpp decides about storage, restated for the coverage predicates: readers, fused shortcuts, views,
    which producers write into a slice of a concatenation and which sources are copied there, CSP pairs and the
    32-channel rule of the split-fp16 record before any tie between buffers."""
    L = len(layers)
    readers = [0] * L
    for i, l in enumerate(layers):
        for j in sources(layers, i):
            if j >= 0:
                readers[j] += 1
    fused, unfused_two_readers = set(), set()
    root, coff = list(range(L)), [0] * L
    for i in range(1, L):
        l = layers[i]
        if l["type"] == "shortcut" and layers[i - 1]["type"] == "convolutional" and l["refs"][1] != i - 1 and layers[i - 1]["act"] != "linear":
            if readers[i - 1] == 1:
                fused.add(i)
                root[i] = i - 1
            else:
                unfused_two_readers.add(i)
    for i, l in enumerate(layers):
        if l["type"] == "route" and len(l["refs"]) == 1:
            s = l["refs"][0]
            root[i] = root[s]
            coff[i] = coff[s] + (l["group_id"] * l["c"] if l["groups"] else 0)

    def is_concat(i):
        return layers[i]["type"] == "route" and len(layers[i]["refs"]) > 1

    def is_producer(j):
        t = layers[j]["type"]
        return root[j] == j and (t in ("convolutional", "maxpool", "upsample") or (t == "shortcut" and j not in fused))
    into, copies = {}, {}
    for i, l in enumerate(layers):
        if not is_concat(i):
            continue
        copies[i] = []
        off = 0
        for j in l["refs"]:
            r = root[j]
            whole = (not is_concat(j)) and is_producer(r) and coff[j] == 0 and layers[j]["c"] == layers[r]["c"] and r not in into and off % 4 == 0
            if whole:
                into[r] = (i, off)
            else:
                copies[i].append((j, off))
            off += layers[j]["c"]

    def owner_of(j):
        if is_concat(j):
            return j, 0
        r = root[j]
        if r in into:
            return into[r][0], into[r][1] + coff[j]
        return r, coff[j]
    h16 = [True] * L
    for j, l in enumerate(layers):
        if l["type"] == "yolo":
            continue
        o, off = owner_of(j)
        if off % 32 or l["c"] % 32:
            h16[o] = False
    csp = [i for i in range(1, L - 2)
           if layers[i]["type"] == layers[i + 2]["type"] == "convolutional" and layers[i + 1]["type"] == "route"
           and layers[i + 1]["refs"] == [i - 1] and not layers[i + 1]["groups"]
           and layers[i]["k"] == layers[i + 2]["k"] == 1 and layers[i]["stride"] == layers[i + 2]["stride"] == 1]
    return dict(readers=readers, fused=fused, unfused_two_readers=unfused_two_readers, root=root, coff=coff, into=into, copies=copies,
                owner_of=owner_of, h16_before_ties=h16, csp=csp, is_concat=is_concat)


def features(layers):
    """The set of planner features this graph reaches (names as in FEATURES)."""
    p = plan_model(layers)
    f = set()
    if p["into"]:
        f.add("redirected_producer")
    if any(p["copies"].values()):
        f.add("concat_fed_by_copy")
    if any(l["type"] == "route" and l.get("groups") for l in layers):
        f.add("grouped_view")
    if p["fused"]:
        f.add("fusable_shortcut")
    if p["unfused_two_readers"]:
        f.add("shortcut_conv_has_two_readers")
    if p["csp"]:
        f.add("csp_triple")
    pools = {(l["src"], l["k"]) for l in layers if l["type"] == "maxpool" and l["stride"] == 1 and l["k"] >= 5}
    for i, l in enumerate(layers):
        if l["type"] == "maxpool" and l["stride"] == 1 and l["k"] >= 9:
            mine = (p["root"][l["src"]], p["coff"][l["src"]])
            if any(k == l["k"] - 4 and (p["root"][s], p["coff"][s]) == mine for s, k in pools):
                f.add("spp_chain")
        if l["type"] == "upsample":
            a, b = p["h16_before_ties"][p["owner_of"](l["src"])[0]], p["h16_before_ties"][p["owner_of"](i)[0]]
            if a and not b:
                f.add("upsample_h16_to_f32")
            if b and not a:
                f.add("upsample_f32_to_h16")
        if p["is_concat"](i):
            cs = [layers[j]["c"] for j in l["refs"]]
            if any(c % 32 for c in cs) and any(c % 32 == 0 for c in cs):
                f.add("concat_mixes_mod32")
            if any(c % 64 for c in cs) and any(c % 64 == 0 for c in cs):
                f.add("concat_mixes_mod64")
    return f


FEATURES = ("redirected_producer", "concat_fed_by_copy", "grouped_view", "fusable_shortcut", "shortcut_conv_has_two_readers", "csp_triple",
            "spp_chain", "upsample_h16_to_f32", "upsample_f32_to_h16", "concat_mixes_mod32", "concat_mixes_mod64")


def coverage(graphs):
    """feature -> names of the graphs that reach it"""
    cov = {f: [] for f in FEATURES}
    for name, (_, _, layers) in graphs.items():
        for f in features(layers):
            cov[f].append(name)
    return cov


# ------------------------------------------------------------------------------------------ oracle
def make_oracle(cfg, hw, seed=3):
    """(oracle with weights loaded, the weight blob, floats the oracle consumed)"""
    from oracle.darknet import DarknetOracle
    from yolo_deepsort_amd import synth
    blob = synth.darknet_weights_blob(cfg, seed, -1.0, num_classes=1)
    ref = DarknetOracle(cfg, hw, is_text=True)
    used = ref.load_weights_array(np.frombuffer(blob, dtype=F32, offset=20))
    return ref, blob, used


def graph_input(hw, batch, seed=5):
    return np.random.RandomState(seed).uniform(0, 1, (batch, 3) + tuple(hw)).astype(F32)


def one_step(ref, i, tensors):
    """Layer i's output by the oracle's own operators from GIVEN inputs: ``tensors`` maps a layer index (-1: the image) to the
    tensor to use as that layer's output.  Nothing compounds across layers."""
    x = tensors.get(i - 1)
    return ref.step(i, x, tensors, ref.img_size)
