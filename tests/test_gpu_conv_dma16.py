"""The LDS-DMA conv kernels (conv_igemm_f16x3_dma, variants 11-14, 18, 19 and split-K 21, 22) on the shapes where a wave tile of
16-row / 16-filter blocks with fragments carried across a mid-step barrier can newly go wrong:

  K steps against the ring depth   1x1 with Cin = 32, 64, 96, 128 (1, 2, 3, 4 steps for NS = 2 and NS = 3); 3x3 s2 on 32 channels (9
                                   steps, a tap change every step)
  16-boundaries                    M = 15, 16, 17, 33; Cout = 15, 16, 17, 33 and the head's 255 (fp32 outputs)
  strided 3x3, odd extents         7x5 and 9x11, stride 2, three images: the rows of one 16-block straddle output rows and images
  epilogues                        residual after / before the activation and mish, on a 3x3 s2 and a 1x1 layer
  launch forms                     one merged launch (n_split) and one forced split-K launch at the smallest layer its rule takes

Every case is held to the float64 reference of conv_ref.py at the suite's two bounds, 1e-3 of the output scale and mut / 16
(test_gpu_conv_variants.py); tests/test_conv_dma16_cases_host.py shows on the CPU that the reference arithmetic itself stays below
mut / 64 on exactly these cases."""
import ctypes as C

import numpy as np
import pytest

import conv_dma16_cases as D
import conv_ref as R
from conv_ref import ACT, F32

pytestmark = pytest.mark.gpu

SENTINEL = -77.0              # exact in fp32 and in the H16 split: an untouched channel decodes to these very bits


class _F16x3:
    """the library in the default conv arithmetic: (lib module, variant names); restores the mode on exit"""

    def __enter__(self):
        from yolo_deepsort_amd import _lib as L
        L.init(0)
        self.lib = lib = L.load()
        lib.yds_conv_variant_name.restype = C.c_char_p
        self.prev = lib.yds_get_conv_math()
        L.check(lib.yds_set_conv_math(1))
        names = [lib.yds_conv_variant_name(v).decode() for v in range(lib.yds_conv_num_variants())]
        for v in D.DMA_VARIANTS + D.SPLITK_VARIANTS:
            assert "_dma<" in names[v] and ("splitK" in names[v]) == (v in D.SPLITK_VARIANTS), (v, names[v])
        return L, names

    def __exit__(self, *exc):
        self.lib.yds_set_conv_math(self.prev)


def _run(L, variant, r):
    n, h, wd, cin = r.x.shape
    cout = r.w.shape[0]
    ho, wo = R.out_hw(h, wd, r.k, r.s)
    y = np.empty((n, cout, ho, wo), F32)
    L.check(L.load().yds_conv_run(variant, n, h, wd, cin, cout, r.k, r.s, r.act, r.res_mode, L.ptr(r.x), L.ptr(r.w), L.ptr(r.bias),
                                  L.ptr(r.res) if r.res is not None else None, L.ptr(y)))
    return y


def _hold(name, r, got, worst):
    err = r.err(got)
    print(f"  {name:46s} {r.case}: err/scale {err / r.scale:.1e}  mut/{r.mut / max(err, 1e-30):.0f}")
    worst[name] = max(worst.get(name, 0.0), err / r.mut)
    assert err < 1e-3 * r.scale, (name, r.case, err / r.scale)
    # a kernel that drops a cross term of the split product is at mut or above (conv_ref.mutant_bound)
    assert err <= r.mut / 16, (name, r.case, f"err {err:.3e} = mut / {r.mut / max(err, 1e-30):.1f}: above mut / 16")


def test_every_dma_variant_on_the_16_block_edges():
    with _F16x3() as (L, names):
        worst = {}
        refs = D.refs()
        for r in refs[:len(D.CASES)]:
            for v in D.DMA_VARIANTS:
                _hold(names[v], r, _run(L, v, r), worst)
        assert len(worst) == len(D.DMA_VARIANTS)
        print("worst err/mut per variant: " + ", ".join(f"{k} mut/{1 / max(b, 1e-30):.0f}" for k, b in worst.items()))


def test_forced_split_k_on_its_smallest_layer():
    with _F16x3() as (L, names):
        r = D.refs()[len(D.CASES)]
        assert r.case == D.SPLITK_CASE
        worst = {}
        for v in D.SPLITK_VARIANTS:
            _hold(names[v], r, _run(L, v, r), worst)
        assert len(worst) == len(D.SPLITK_VARIANTS)


def test_merged_launch():
    """filters [0, n_split) into a slice of one buffer, the rest into a second tensor: both meet the bounds, every channel outside
    the slices keeps the sentinel bit for bit"""
    with _F16x3() as (L, names):
        r = D.refs()[len(D.CASES) + 1]
        assert r.case == D.merged_plain_case()
        n, h, wd, (cin, x_ld, x_off), (cout, y_ld, y_off), k, s, act, (res_mode, r_ld, r_off), (n_split, y2_ld, y2_off) = D.MERGED_CASE
        ho, wo = R.out_hw(h, wd, k, s)
        view = np.array([x_ld, x_off, y_ld, y_off, r_ld, r_off, n_split, y2_ld, y2_off], np.int32)
        sent = np.float32(SENTINEL).view(np.uint32)
        worst = {}
        for v in D.DMA_VARIANTS:
            y = np.empty((n, y_ld, ho, wo), F32)
            y2 = np.empty((n, y2_ld, ho, wo), F32)
            L.check(L.load().yds_conv_run_view(v, n, h, wd, cin, cout, k, s, ACT[act], res_mode, L.ptr(view), L.ptr(r.x), L.ptr(r.w), L.ptr(r.bias),
                                               None, SENTINEL, L.ptr(y), L.ptr(y2)))
            got = np.concatenate([y[:, y_off:y_off + n_split], y2[:, y2_off:y2_off + cout - n_split]], 1)
            _hold(names[v], r, got, worst)
            outside = np.ones(y_ld, bool)
            outside[y_off:y_off + n_split] = False
            assert (y[:, outside].view(np.uint32) == sent).all(), (names[v], "wrote outside its output slice")
            outside = np.ones(y2_ld, bool)
            outside[y2_off:y2_off + cout - n_split] = False
            assert (y2[:, outside].view(np.uint32) == sent).all(), (names[v], "wrote outside its second output slice")
        assert len(worst) == len(D.DMA_VARIANTS)
