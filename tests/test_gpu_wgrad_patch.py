"""Patch-staged route of the 3x3 stride-1 weight gradient at WO 4 and 8
(``gemm_wgrad_seg_kernel<T, 0, true>``).

The three-tile kernel stages three x row-tiles per 32-position chunk; the
patch kernel stages the chunk's zero-padded input patch once and reads the
three kernel rows as row offsets into it.  Fragment reads, MFMA order and
the block's partial sum are unchanged, so where every ``dw`` element receives
one add (split-M factor 1) the two routes must be BIT-IDENTICAL
(``PDT_WGRAD_PATCH`` is read per call and toggled in-process).  Everywhere
``dw`` is held to the float64 dot-product bound of ``_errbound`` (depth
N*HO*WO, f32 output so eps_out = 0, no element exempted), with ``dw``
allocated after ``poison``.

Shapes are (n, h, w, cin, kout, r, stride, pad).  The issue's (2,8,8,80,72)
is run as (2,8,8,128,72): the 16-bit wgrad entry takes power-of-two Cin only
(``log2_exact``), so "not a multiple of 64" is exercised on Kout.
"""

import functools
import os

import pytest
import torch

import _errbound as eb

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from pytorch_ddp_template_amd.ops.native import native

    EXT = native()
DEV = "cuda:0"
GATE = "PDT_WGRAD_PATCH"
BF16, FP16 = torch.bfloat16, torch.float16


def _s3(n, h, w, cin, kout):
    return (n, h, w, cin, kout, 3, 1, 1)


TAKEN = [_s3(2, 8, 8, 64, 64), _s3(2, 4, 4, 64, 64), _s3(2, 8, 4, 64, 64),
         _s3(2, 4, 8, 64, 64), _s3(2, 16, 8, 64, 64)]
DECLINED = [
    _s3(2, 16, 16, 64, 64),           # WO 16: ring
    _s3(1, 8, 32, 64, 64),            # WO 32: ring
    _s3(1, 8, 64, 64, 64),            # WO 64: three-tile kernel
    (2, 16, 16, 64, 64, 3, 2, 1),     # stride 2 (its output map is 8 x 8)
    _s3(2, 12, 10, 64, 64),           # not powers of two
    (2, 8, 8, 64, 64, 1, 1, 0),       # 1x1
    (2, 8, 8, 16, 32, 5, 1, 2),       # 5x5
]
BOUND = [
    _s3(2, 8, 8, 128, 64),     # two chunks per image: top and bottom halo
    _s3(3, 4, 4, 64, 64),      # 48 rows: the last group lies past Mtot
    _s3(1, 4, 4, 64, 64),      # a single half-filled chunk
    _s3(2, 8, 4, 64, 64),      # Rg 8, one group
    _s3(2, 4, 8, 64, 64),      # chunk = whole image
    _s3(2, 16, 8, 64, 64),     # four chunks per image, middle ones unpadded
    _s3(3, 4, 4, 64, 10),      # Kout padded to a multiple of 8
    _s3(2, 8, 8, 64, 12),
    _s3(2, 8, 8, 128, 72),     # Kout not a multiple of 64 (module docstring)
    _s3(256, 8, 8, 128, 128),  # 512 / 256 chunks over 128 split-M slices:
    _s3(512, 4, 4, 128, 128),  # blocks cross image boundaries, both buffers
]
IDENTICAL = [_s3(2, 8, 8, 1024, 2048), _s3(4, 4, 4, 1024, 2048)]


def _ids(v):
    return str(v).replace("torch.", "").replace(" ", "")


class _gate:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get(GATE)
        os.environ[GATE] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(GATE, None)
        else:
            os.environ[GATE] = self.old


def _eligible(shape):
    n, h, w, cin, kout, r, stride, pad = shape
    return EXT.conv_wgrad_patch_eligible(h, w, cin, kout, r, r, stride, pad)


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype):
    n, h, w, cin, kout, r, stride, pad = shape
    ho, wo = eb.conv_out_hw(h, w, r, stride, pad)
    x = eb.randn(n, h, w, cin, seed=301, dtype=dtype)
    dy = eb.randn(n, ho, wo, kout, seed=302, scale=0.1, dtype=dtype)
    return x, dy, x.to(DEV), dy.to(DEV)


@functools.lru_cache(maxsize=None)
def _ref(shape, dtype):
    n, h, w, cin, kout, r, stride, pad = shape
    x, dy, _, _ = _inputs(shape, dtype)
    return eb.conv_wgrad_ref(dy, x, stride, pad, r, r)


def _wgrad(shape, dtype, gate):
    n, h, w, cin, kout, r, stride, pad = shape
    _, _, xd, dyd = _inputs(shape, dtype)
    eb.poison(DEV, 4 * kout * r * r * cin)
    with _gate(gate):
        dw = EXT.conv2d_wgrad(dyd, xd, stride, pad, r, r)
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (kout, r, r, cin)
    return dw


def _check_wgrad(shape, dtype, gate="1"):
    ref, mag, depth = _ref(shape, dtype)
    n, h, w, _, _, r, stride, pad = shape
    ho, wo = eb.conv_out_hw(h, w, r, stride, pad)
    assert depth == n * ho * wo
    dw = _wgrad(shape, dtype, gate)
    eb.assert_gemm_close(dw, ref, mag, depth,
                         f"conv_wgrad {_ids(dtype)} gate={gate} {shape}")


@pytest.mark.parametrize("shape", TAKEN, ids=_ids)
def test_gate_takes(shape):
    assert _eligible(shape)
    _check_wgrad(shape, BF16)


@pytest.mark.parametrize("shape", DECLINED, ids=_ids)
def test_gate_declines_and_op_still_right(shape):
    assert not _eligible(shape)
    _check_wgrad(shape, BF16)


def test_bound_cases_are_taken():
    assert all(_eligible(s) for s in BOUND + IDENTICAL)


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=_ids)
@pytest.mark.parametrize("shape", BOUND, ids=_ids)
def test_dw_inside_dot_product_bound(shape, dtype):
    _check_wgrad(shape, dtype)


@pytest.mark.parametrize("shape", BOUND[:2], ids=_ids)
def test_gate_off_keeps_three_tile_route_right(shape):
    _check_wgrad(shape, BF16, gate="0")


@pytest.mark.parametrize("shape", IDENTICAL, ids=_ids)
def test_dw_bit_identical_between_routes(shape):
    # 16 x 32 = 512 tiles: the launcher's split-M factor is 1, every dw
    # element is one add onto zero, so either route is deterministic
    on = _wgrad(shape, BF16, "1")
    off = _wgrad(shape, BF16, "0")
    assert torch.isfinite(on).all() and on.abs().max() > 0
    if not torch.equal(on.view(torch.int32), off.view(torch.int32)):
        diff = (on - off).abs()
        raise AssertionError(
            f"dw{shape}: {int((on != off).sum())}/{on.numel()} elements "
            f"differ, max abs diff {diff.max().item()}")


# ------------------------------------------------------------ block level --


def _block_fwd_bwd(blk, x0):
    for p in blk.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    out = blk(x)
    out.float().square().mean().backward()
    res = {"out": out.detach().clone(), "x.grad": x.grad.clone()}
    for name, p in blk.named_parameters():
        res[name] = p.grad.clone()
    return res


@functools.lru_cache(maxsize=None)
def _block_pair():
    """BasicBlock(128, 128) at 16 x 8 x 8, gate off then gate on, once."""
    from pytorch_ddp_template_amd.models.resnet import BasicBlock

    torch.manual_seed(0)
    blk = BasicBlock(128, 128, 1).to(BF16).to(DEV)
    blk.train()
    assert EXT.conv_wgrad_patch_eligible(8, 8, 128, 128, 3, 3, 1, 1)
    x0 = torch.relu(torch.randn(16, 8, 8, 128)).to(BF16).to(DEV)
    with _gate("0"):
        ref = _block_fwd_bwd(blk, x0)
    with _gate("1"):
        got = _block_fwd_bwd(blk, x0)
    return got, ref


def test_block_gate_on_matches_gate_off():
    from test_gpu_dgrad_epilogue import (PAIR_ULPS, _assert_close,
                                         _assert_identical)

    got, ref = _block_pair()
    _assert_identical(got["out"], ref["out"], "block output")
    _assert_close(got, ref, PAIR_ULPS)


def test_block_dx_bit_identical_gate_on_vs_gate_off():
    """``dx`` does not depend on any weight gradient, so the two routes must
    leave it bit-identical — if the block's ``dx`` is reproducible at all.

    KNOWN TO FAIL INTERMITTENTLY, for a reason outside the wgrad: measured on
    an MI355X, 40 forward+backward runs of this block per gate setting
    against one gate-off run, ``dx`` differed bitwise in 11 of 40 runs with
    the gate OFF (up to 1564 of 131072 elements) and in 8 of 40 with the gate
    on; the output never differed.  The BN-backward sums are combined with
    float atomics (norm.hip ``bn_bwd`` stats, the dgrad epilogue's workspace
    rows), so dgamma / dbeta vary in the last bit from run to run and flip
    last bits of ``dx``.  This test failed in one of four runs of this file
    (59 of 131072 elements, max abs diff 2.4e-07).  The assertion is kept as
    specified; it becomes reliable once those reductions are deterministic."""
    from test_gpu_dgrad_epilogue import _assert_identical

    got, ref = _block_pair()
    _assert_identical(got["x.grad"], ref["x.grad"], "block dx")
