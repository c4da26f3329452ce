"""16-bit conv kernels at the edges the square, multiple-of-8 shapes of
test_gpu_ops.py never reach, under the per-element bound of _errbound.py.

Routes below were established by reading the dispatch code (gemm_bf16.hip
conv2d_wgrad_bf16 / conv2d_fwd_bf16_impl / conv2d_dgrad_bf16, conv_glds.hip,
conv_halo.hip); shapes are (n, h, w, cin, kout, r, stride, pad).

Weight gradient, Kout % 8 != 0 (dy is zero-padded to a multiple of 8 and dw
sliced back; every kernel stages dy in 8-channel groups):

  seg, no ring      (3,4,4,64,10,3,1,1)     3x3 s1, HO=WO=4 pow2, WO < 16;
                                            M=48 is a chunk tail
  seg ring, WO=16   (2,8,16,64,12,3,1,1)    non-square, 2 output rows / chunk
  seg ring, WO=32   (1,4,32,64,10,3,1,1)    1 output row / chunk
  seg ring rotating (256,4,16,128,128,3,1,1) and (256,2,32,128,128,3,1,1):
                    512 chunks over 128 split-M slices = 4 chunks per block,
                    an image is 2 chunks, so each block rotates the x ring
                    AND crosses an image boundary (full restage)
  9-tap tr          (2,12,10,64,10,3,1,1)   non-pow2 spatial
  9-tap tr, strided (2,16,16,64,12,3,2,1)
  1x1 tr            (2,8,8,64,3,1,1,0)
  1x1 wide 128x128  (2,8,8,128,130,1,1,0)   padded Kout 136 >= 128, Cin 128
  taps-on-J         (2,14,10,16,10,5,1,2)   5x5
  taps-on-J         (2,28,20,8,12,7,2,3)    7x7 s2, the ResNet-50 stem form

Forward (no bias / relu) and data gradient, non-square images:

  (2,8,16,64,64,3,1,1), (2,16,8,64,64,3,1,1)   M=256, C=64, Kout%64==0:
        bf16 fwd and dgrad -> glds 256x64; fp16 -> generic NT (glds is bf16
        only and halo needs H*W % 256 == 0 at Kout <= 64)
  (1,8,16,64,128,3,1,1), (1,16,8,64,128,3,1,1) M=128: glds declines (M%256),
        fwd -> LDS-halo kernel (BNT=128, one image per block), bf16 and fp16;
        dgrad -> generic NT (halo at 64 output channels needs H*W % 256)
  (4,14,10,64,64,3,1,1)   M=560, W not pow2 -> generic NT, fwd and dgrad
  (2,8,16,64,128,3,2,1)   strided: fwd M=64 -> generic NT; dgrad M=256 ->
        glds with the zero-stuffed gather (bf16), generic NT stuffed (fp16);
        (H+2p-R) % 2 == 1 in both dims: output padding
  (2,8,16,128,64,1,1,0)   1x1: bf16 fwd -> glds 256x64, dgrad -> glds
        256x128; fp16 -> generic NT
"""

import pytest
import torch

import _errbound as eb

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from pytorch_ddp_template_amd.ops.native import native

    EXT = native()
DEV = "cuda:0"
BF16, FP16 = torch.bfloat16, torch.float16
DTYPES = [BF16, FP16]


def _ids(v):
    return str(v).replace("torch.", "")


def _poison(dtype, *shape):
    n = 1
    for s in shape:
        n *= s
    eb.poison(DEV, n * torch.empty((), dtype=dtype).element_size())


def _inputs(shape, dtype):
    n, h, w, cin, kout, r, stride, pad = shape
    ho, wo = eb.conv_out_hw(h, w, r, stride, pad)
    x = eb.randn(n, h, w, cin, seed=201, dtype=dtype)
    wt = eb.randn(kout, r, r, cin, seed=202, dtype=dtype,
                  scale=(2.0 / (r * r * cin)) ** 0.5)
    dy = eb.randn(n, ho, wo, kout, seed=203, scale=0.1, dtype=dtype)
    return x, wt, dy, ho, wo


def _check_fwd(shape, dtype):
    n, h, w, cin, kout, r, stride, pad = shape
    x, wt, _, ho, wo = _inputs(shape, dtype)
    ref, mag, depth = eb.conv_fwd_ref(x, wt, None, stride, pad)
    _poison(dtype, n, ho, wo, kout)
    out = EXT.conv2d_fwd(x.to(DEV), wt.to(DEV), None, stride, pad, False)
    assert out.dtype == dtype
    eb.assert_gemm_close(out, ref, mag, depth, f"conv_fwd {_ids(dtype)} {shape}")


def _check_dgrad(shape, dtype):
    n, h, w, cin, kout, r, stride, pad = shape
    _, wt, dy, _, _ = _inputs(shape, dtype)
    ref, mag, depth = eb.conv_dgrad_ref(dy, wt, stride, pad, h, w)
    _poison(dtype, n, h, w, cin)
    dx = EXT.conv2d_dgrad(dy.to(DEV), wt.to(DEV), stride, pad, h, w)
    assert dx.dtype == dtype
    eb.assert_gemm_close(dx, ref, mag, depth, f"conv_dgrad {_ids(dtype)} {shape}")


def _check_wgrad(shape, dtype):
    n, h, w, cin, kout, r, stride, pad = shape
    x, _, dy, _, _ = _inputs(shape, dtype)
    ref, mag, depth = eb.conv_wgrad_ref(dy, x, stride, pad, r, r)
    _poison(torch.float32, kout, r, r, cin)
    dw = EXT.conv2d_wgrad(dy.to(DEV), x.to(DEV), stride, pad, r, r)
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (kout, r, r, cin)
    eb.assert_gemm_close(dw, ref, mag, depth, f"conv_wgrad {_ids(dtype)} {shape}")


# ------------------------------------------- wgrad, Kout % 8 != 0 ----------

WGRAD_ODD_KOUT = [
    (3, 4, 4, 64, 10, 3, 1, 1),
    (2, 8, 16, 64, 12, 3, 1, 1),
    (1, 4, 32, 64, 10, 3, 1, 1),
    (2, 12, 10, 64, 10, 3, 1, 1),
    (2, 16, 16, 64, 12, 3, 2, 1),
    (2, 8, 8, 64, 3, 1, 1, 0),
    (2, 8, 8, 128, 130, 1, 1, 0),
    (2, 14, 10, 16, 10, 5, 1, 2),
    (2, 28, 20, 8, 12, 7, 2, 3),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", WGRAD_ODD_KOUT, ids=str)
def test_wgrad_kout_not_multiple_of_8(shape, dtype):
    _check_wgrad(shape, dtype)


@pytest.mark.parametrize("shape", [(256, 4, 16, 128, 128, 3, 1, 1),
                                   (256, 2, 32, 128, 128, 3, 1, 1)], ids=str)
def test_wgrad_ring_rotates_and_wraps(shape):
    _check_wgrad(shape, BF16)


def test_conv2d_nhwc_backward_kout_10():
    """Kout=10 head through the autograd op: y, dx (im2col fallback dgrad:
    Kout is no power of two), dw (padded wgrad, sliced back to Kout) and the
    col_sum bias grad."""
    from pytorch_ddp_template_amd.ops.functional import conv2d_nhwc

    shape = (2, 12, 10, 64, 10, 3, 1, 1)
    n, h, w, cin, kout, r, stride, pad = shape
    x, wt, dy, ho, wo = _inputs(shape, BF16)
    bias = eb.randn(kout, seed=204, dtype=BF16)
    xg = x.to(DEV).requires_grad_(True)
    wg = wt.to(DEV).requires_grad_(True)
    bg = bias.to(DEV).requires_grad_(True)
    _poison(BF16, n, ho, wo, kout)
    y = conv2d_nhwc(xg, wg, bg, stride, pad)
    y.backward(dy.to(DEV))
    assert wg.grad.shape == wt.shape and bg.grad.shape == bias.shape
    eb.assert_gemm_close(y, *eb.conv_fwd_ref(x, wt, bias, stride, pad), "head y")
    eb.assert_gemm_close(xg.grad, *eb.conv_dgrad_ref(dy, wt, stride, pad, h, w),
                         "head dx")
    eb.assert_gemm_close(wg.grad, *eb.conv_wgrad_ref(dy, x, stride, pad, r, r),
                         "head dw")
    d = dy.double().reshape(-1, kout)
    eb.assert_gemm_close(bg.grad, d.sum(0), d.abs().sum(0), d.shape[0], "head db")


# --------------------------------- non-square images, fwd and dgrad --------

NONSQUARE = [
    (2, 8, 16, 64, 64, 3, 1, 1),
    (2, 16, 8, 64, 64, 3, 1, 1),
    (1, 8, 16, 64, 128, 3, 1, 1),
    (1, 16, 8, 64, 128, 3, 1, 1),
    (4, 14, 10, 64, 64, 3, 1, 1),
    (2, 8, 16, 64, 128, 3, 2, 1),
    (2, 8, 16, 128, 64, 1, 1, 0),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", NONSQUARE, ids=str)
def test_conv_fwd_nonsquare(shape, dtype):
    _check_fwd(shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", NONSQUARE, ids=str)
def test_conv_dgrad_nonsquare(shape, dtype):
    _check_dgrad(shape, dtype)


# ----- the small square shapes of test_gpu_ops.py under the tight bound ----


def _sq(n, h, c, k, r, stride, pad):
    return (n, h, h, c, k, r, stride, pad)


@pytest.mark.parametrize("shape", [
    _sq(2, 16, 64, 64, 3, 1, 1), _sq(2, 16, 64, 128, 3, 2, 1),
    _sq(2, 8, 128, 64, 1, 1, 0), _sq(2, 32, 3, 64, 3, 1, 1),
    _sq(1, 16, 64, 64, 1, 2, 0), _sq(16, 16, 256, 256, 3, 1, 1)], ids=str)
def test_conv_fwd_square_tight(shape):
    _check_fwd(shape, BF16)


@pytest.mark.parametrize("shape", [
    _sq(2, 16, 64, 64, 3, 1, 1), _sq(2, 16, 64, 128, 3, 2, 1),
    _sq(1, 8, 64, 64, 1, 2, 0), _sq(16, 16, 256, 256, 3, 1, 1)], ids=str)
def test_conv_dgrad_square_tight(shape):
    _check_dgrad(shape, BF16)


@pytest.mark.parametrize("shape", [
    _sq(2, 16, 64, 64, 3, 1, 1), _sq(2, 16, 64, 128, 3, 2, 1),
    _sq(2, 16, 3, 64, 3, 1, 1), _sq(2, 4, 64, 64, 3, 1, 1),
    _sq(2, 8, 128, 64, 3, 1, 1), _sq(3, 12, 64, 64, 3, 1, 1),
    _sq(2, 28, 8, 64, 7, 2, 3), _sq(2, 14, 16, 32, 5, 1, 2),
    _sq(4, 32, 64, 64, 3, 1, 1)], ids=str)
def test_conv_wgrad_square_tight(shape):
    _check_wgrad(shape, BF16)


@pytest.mark.parametrize("m,n,k", [(64, 64, 64), (128, 128, 128), (130, 70, 40),
                                   (32, 10, 16), (257, 129, 96),
                                   (4096, 256, 128), (4352, 512, 192)])
def test_gemm_nt_tight(m, n, k):
    a = eb.randn(m, k, seed=205, dtype=BF16)
    b = eb.randn(n, k, seed=206, dtype=BF16)
    _poison(BF16, m, n)
    out = EXT.gemm_nt(a.to(DEV), b.to(DEV), None, False, False)
    eb.assert_gemm_close(out, *eb.linear_ref(a, b), f"gemm_nt {(m, n, k)}")


@pytest.mark.parametrize("m,i,j", [(256, 64, 64), (1000, 70, 33), (64, 10, 512),
                                   (512, 256, 384), (2048, 768, 768)])
def test_gemm_tn_tight(m, i, j):
    a = eb.randn(m, i, seed=207, dtype=BF16)
    b = eb.randn(m, j, seed=208, dtype=BF16)
    _poison(torch.float32, i, j)
    out = EXT.gemm_tn(a.to(DEV), b.to(DEV))
    assert out.dtype == torch.float32
    eb.assert_gemm_close(out, *eb.tn_ref(a, b), f"gemm_tn {(m, i, j)}")
