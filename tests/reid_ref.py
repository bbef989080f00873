"""Float64 reference of the whole appearance network, and the bound the ReID tests derive from it (plain helpers, no fixtures).

`forward64` is Net(reid=True).forward of deep_sort/deep/model.py, unfused, in float64 from the fp32 inputs and the fp32 state dict:
conv (+ bias for conv.0), BatchNorm with eps 1e-5, ReLU, MaxPool(3, 2, 1), eight BasicBlocks (residual BEFORE the ReLU; the 1x1
stride-2 downsample branch is linear), the mean over the 8x4 map and the L2 norm.  It returns the embedding and the nine stage outputs
(pooled stem, 8 blocks), so that a kernel result outside the bound can be localised on the CPU.

The 20 convs and their BatchNorms are numbered as csrc/reid.cpp finalize() numbers them (CONVS): 0 the stem, then per block conv1,
conv2 and, in a down block, the downsample conv.  Blocks are numbered 0..7; 2, 4 and 6 are the down blocks.

A mutant restates ONE defect in float64:
    ("xlo", i)        conv i reads conv_ref.x_hat of its fp32-rounded input      (a kernel that lost the x_lo * w_hi term)
    ("wlo", i)        conv i uses conv_ref.w_hat of its weights                  (... the x_hi * w_lo term)
    ("eps", i)        BatchNorm i without eps                                    (a wrong fold in finalize())
    ("res_after", b)  block b adds its residual after the ReLU
    ("no_down", b)    down block b adds its unprojected strided input x[:, :, ::2, ::2] (to the first Cin channels)
    ("no_bias",)      conv.0.bias is dropped

`bound(x, sd)` = min over the xlo / wlo mutants of ALL 20 convs of max|mutant - reference| over the embedding, divided by 16: the
project's mut / 16 convention for the whole network.  It comes from the reference arithmetic and the test's inputs alone, never from
what a kernel returns.  test_reid_ref_host.py holds the reference to its own conditions (the fp32 oracle and the folded fp32 network
on the CPU within bound / 2, the exact three-term emulation within bound / 4, every structural mutant beyond 16 bound).

Measured with the tests' case() inputs (8 crops, synth.reid_state_dict(1, profile)), max abs over the embedding:
    profile   bound      weakest mutant        fp32 oracle   folded fp32 network   three-term emulation
    "unit"    1.58e-7    ("xlo", 3) 2.53e-6    4.0e-8        3.5e-8                1.8e-8
    "wide"    2.43e-7    ("xlo", 6) 3.89e-6    6.6e-8        6.0e-8                2.8e-8
and with front_case()'s (3 boxes of front_frame()):
    "unit"    1.49e-7    ("xlo", 5) 2.39e-6    3.8e-8        4.6e-8                1.6e-8
    "wide"    2.11e-7    ("xlo", 0) 3.37e-6    6.5e-8        9.3e-8                2.8e-8
(the strongest cross-term mutants, ("wlo", 17) and ("wlo", 19), move it by 3.7e-5 and 7.1e-5: all 40 lie far inside the 1e-3
relative / 1e-5 absolute comparison with the fp32 oracle that held the network before)
"""
import functools

import numpy as np

import conv_ref

F32 = np.float32
EPS = 1e-5
STAGES = (("layer1", 64, 64, False), ("layer2", 64, 128, True), ("layer3", 128, 256, True), ("layer4", 256, 512, True))


def _tables():
    convs, blocks = [("conv.0", "conv.1", 1, 1)], []
    for name, _, _, down in STAGES:
        for b in range(2):
            p, d = "%s.%d" % (name, b), down and b == 0
            blocks.append((p, len(convs), d))
            convs.append((p + ".conv1", p + ".bn1", 2 if d else 1, 1))
            convs.append((p + ".conv2", p + ".bn2", 1, 1))
            if d:
                convs.append((p + ".downsample.0", p + ".downsample.1", 2, 0))
    return tuple(convs), tuple(blocks)


CONVS, BLOCKS = _tables()            # (conv, bn, stride, pad) x 20; (prefix, first conv index, down) x 8
DOWN_BLOCKS = tuple(b for b, blk in enumerate(BLOCKS) if blk[2])
CROSS_MUTANTS = tuple((kind, i) for i in range(len(CONVS)) for kind in ("xlo", "wlo"))
STRUCT_MUTANTS = tuple(("res_after", b) for b in range(len(BLOCKS))) + tuple(("no_down", b) for b in DOWN_BLOCKS) + (("no_bias",),)
EPS_MUTANTS = tuple(("eps", i) for i in range(len(CONVS)))


def _stage_of(mutant):
    """index into the stage list of the first stage a mutant changes"""
    if mutant[0] == "no_bias":
        return 0
    if mutant[0] in ("res_after", "no_down"):
        return mutant[1] + 1
    i = mutant[1]
    return 0 if i == 0 else 1 + max(b for b, blk in enumerate(BLOCKS) if blk[1] <= i)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _r32(t):
    return t.float().double()


def _conv_bn(h, i, sd, mutant, emulate):
    """conv i and its BatchNorm on a float64 NCHW tensor.  emulate: the device's layer restated - BatchNorm folded into fp32 weights
    and an fp32 bias (reid.cpp finalize); "f16x3": x_hi*w_hi + x_hi*w_lo + x_lo*w_hi of the split operands summed in float64,
    "fp32": h is an fp32 tensor and so is the result, an fp32 convolution on the CPU (torch)."""
    import torch
    conv = torch.nn.functional.conv2d
    name, bn, stride, pad = CONVS[i]
    w = np.asarray(sd[name + ".weight"], np.float64)
    g, beta, mean, var = (np.asarray(sd[bn + k], np.float64) for k in (".weight", ".bias", ".running_mean", ".running_var"))
    cb = np.asarray(sd[name + ".bias"], np.float64) if i == 0 and mutant != ("no_bias",) else np.zeros_like(g)
    if emulate:
        scale = g / np.sqrt(var + EPS)
        wf = (w * scale[:, None, None, None]).astype(F32)
        bias = ((cb - mean) * scale + beta).astype(F32).astype(np.float64)
        if emulate == "fp32":
            return conv(h, torch.from_numpy(wf), torch.from_numpy(bias.astype(F32)), stride, pad)
        xh, xl = (_t(v) for v in conv_ref.split_x(h.numpy()))
        wh, wl = (_t(v) for v in conv_ref.split_w(wf))
        y = conv(xh, wh, None, stride, pad) + conv(xh, wl, None, stride, pad) + conv(xl, wh, None, stride, pad)
        return y + _t(bias)[None, :, None, None]
    if mutant == ("xlo", i):
        h = _t(conv_ref.x_hat(_r32(h).numpy()))
    if mutant == ("wlo", i):
        w = conv_ref.w_hat(w)
    y = conv(h, _t(w), _t(cb), stride, pad)
    scale = g / np.sqrt(var + (0.0 if mutant == ("eps", i) else EPS))
    return (y - _t(mean)[None, :, None, None]) * _t(scale)[None, :, None, None] + _t(beta)[None, :, None, None]


def _forward(x, sd, mutant, emulate, stages):
    import torch
    relu = torch.relu
    rnd = _r32 if emulate == "f16x3" else (lambda t: t)  # activations as fp32 between the layers
    first = 0 if mutant is None or stages is None else _stage_of(mutant)
    out = [_t(s) for s in stages[:first]] if first else []
    if not out:
        x = torch.from_numpy(np.array(x, F32)) if emulate == "fp32" else _t(x)
        h = relu(_conv_bn(x, 0, sd, mutant, emulate))
        out.append(rnd(torch.nn.functional.max_pool2d(h, 3, 2, 1)))
    for b in range(len(out) - 1, len(BLOCKS)):
        _, i, down = BLOCKS[b]
        h = out[-1]
        y = rnd(relu(_conv_bn(h, i, sd, mutant, emulate)))
        y = _conv_bn(y, i + 1, sd, mutant, emulate)
        if down and mutant == ("no_down", b):
            r = torch.zeros_like(y)
            r[:, :h.shape[1]] = h[:, :, ::2, ::2]
        elif down:
            r = rnd(_conv_bn(h, i + 2, sd, mutant, emulate))
        else:
            r = h
        out.append(rnd(relu(y) + r if mutant == ("res_after", b) else relu(y + r)))
    m = out[-1].mean(dim=(2, 3))
    emb = m / torch.sqrt((m * m).sum(dim=1, keepdim=True))
    return emb.double().numpy(), [s.double().numpy() for s in out]


def forward64(x, sd, mutant=None, stages=None):
    """x [D, 3, 128, 64] fp32 -> (embedding [D, 512], [pooled stem, block 0 .. block 7]), float64.  `stages`: the stage list of the
    unmutated run on the same x - the stages a mutant leaves unchanged are taken from it instead of being computed again."""
    assert mutant is None or mutant in CROSS_MUTANTS + STRUCT_MUTANTS + EPS_MUTANTS, mutant
    return _forward(x, sd, mutant, False, stages)


def emulated(x, sd):
    """the exact three-term split-fp16 network (the arithmetic the f16x3 kernels approximate with fp32 accumulation): embedding only"""
    return _forward(x, sd, None, "f16x3", None)[0]


def folded_fp32(x, sd):
    """the network as the device holds it - BatchNorm folded into fp32 weights - with EVERY operation in fp32 on the CPU (torch), the
    residual sums and the tail included: what plain fp32 arithmetic in another order than the oracle's makes of the same inputs.
    Embedding only."""
    return _forward(x, sd, None, "fp32", None)[0]


def mutant_errors(x, sd, mutants, ref):
    """{mutant: max|mutant's embedding - reference's|}; ref = forward64(x, sd)"""
    return {m: float(np.abs(forward64(x, sd, m, ref[1])[0] - ref[0]).max()) for m in mutants}


def bound(x, sd, ref=None):
    ref = ref or forward64(x, sd)
    return min(mutant_errors(x, sd, CROSS_MUTANTS, ref).values()) / 16


# ---- the tests' inputs ---------------------------------------------------------------------------------------------------------------
PROFILES = ("unit", "wide")
SEED = 1                         # synth.reid_state_dict(SEED, profile)
N_CROPS = 8


def crops(n=N_CROPS):
    """n >= 8 standard-normal crops (what normalised images look like to the network); crop 2 is a near-duplicate of crop 0 and crop 3
    a scaled copy of crop 1 - the pairs the tracker has to tell apart.  The first 8 do not depend on n."""
    rng = np.random.RandomState(2)
    x = rng.standard_normal((N_CROPS, 3, 128, 64)).astype(F32)
    x[2] = x[0] + F32(0.05) * rng.standard_normal(x[0].shape).astype(F32)
    x[3] = F32(0.9) * x[1]
    if n > N_CROPS:
        x = np.concatenate([x, rng.standard_normal((n - N_CROPS, 3, 128, 64)).astype(F32)])
    x.setflags(write=False)
    return x


FRONT_HW = (270, 480)
FRONT_TLWH = np.array([[30, 20, 60, 130], [200, 100, 25.5, 61.2], [430, 180, 90, 150]], F32)      # the last one: clipped by two borders


FRONT_SEED = 4    # the first of 0, 1, 2, ... whose crops meet every condition of test_reid_ref_host.py on both profiles.  Image crops on
#                   the "wide" weights are a narrow yardstick: at seeds 0 .. 3 and 6 the folded fp32 network on the CPU (folded_fp32)
#                   lies at 0.7 .. 1.25 bound, at seeds 2 and 3 the fp32 oracle itself beyond bound / 2 - a bound that plain fp32
#                   arithmetic does not fit judges no kernel


def front_frame():
    f = np.random.RandomState(FRONT_SEED).randint(0, 256, FRONT_HW + (3,)).astype(np.uint8)
    f.setflags(write=False)
    return f


class Case:
    """one profile's inputs: x (crops(), or with front=True what the oracle's crop + resize + normalise makes of FRONT_TLWH in
    front_frame() - Extractor.preprocess returns the same bits), sd, the float64 run `emb` / `stages`, the cross-term mutants'
    errors `mut` and `bound`"""

    def __init__(self, profile, front=False):
        from yolo_deepsort_amd import synth
        if front:
            from oracle import reid as oreid
            x = oreid.preprocess_crops(front_frame(), FRONT_TLWH)
            x.setflags(write=False)
        else:
            x = crops()
        self.profile, self.x, self.sd = profile, x, synth.reid_state_dict(SEED, profile)
        self.emb, self.stages = self.ref = forward64(self.x, self.sd)
        self.mut = mutant_errors(self.x, self.sd, CROSS_MUTANTS, self.ref)
        self.bound = min(self.mut.values()) / 16
        self.emb.setflags(write=False)

    def err(self, got, rows=slice(None)):
        return float(np.abs(np.asarray(got, np.float64) - self.emb[rows]).max())

    def errors(self, mutants):
        return mutant_errors(self.x, self.sd, mutants, self.ref)


@functools.lru_cache(maxsize=None)
def case(profile):
    """computed once per process, read-only"""
    return Case(profile)


@functools.lru_cache(maxsize=None)
def front_case(profile):
    return Case(profile, True)
