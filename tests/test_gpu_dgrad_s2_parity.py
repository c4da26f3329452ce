"""Parity-split route of the 3x3 stride-2 pad-1 conv dgrad (glds kernel, PAR).

The stuffed route runs all nine taps over every dx pixel; the parity route
groups dx pixels by (h & 1, w & 1) and runs only the 1, 2, 2 or 4 taps that
land on the stride grid, in the same order.  The stuffed route adds exact
zeros in between, so ``dx`` must be BIT-IDENTICAL between the routes in all
five dgrad epilogue modes (``PDT_DGRAD_S2_PARITY`` is read per call and
toggled in-process).  ``dx`` is also held to the float64 dot-product bound of
``_errbound`` (depth 9 * Kout, no element exempted); the BN-backward sums of
``EPI_MASK_BNSTATS`` are checked as column totals of either route's workspace
against float64 sums of that route's own ``dx`` (depth M, + 3 for the
three fp32 roundings inside one ``g * (t - mean) * rstd`` term, eps_out = 0;
per-row partials are not compared: blocks map to workspace rows differently).

Shapes are (N, H, W, Cin = dx channels, Kout = dy channels).
"""

import functools
import os

import pytest
import torch

from _errbound import assert_gemm_close, conv_dgrad_ref, poison

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from pytorch_ddp_template_amd.ops.native import native

    EXT = native()
DEV = "cuda:0"
GATE = "PDT_DGRAD_S2_PARITY"

TAKEN = [
    (4, 16, 16, 64, 64),     # one tile per class, four images, 1 k-tile/tap
    (4, 16, 16, 128, 128),   # 128-wide tile, two k-tiles per tap
    (4, 16, 16, 256, 128),   # 256-wide tile
    (2, 32, 32, 64, 128),    # a tile is one whole image class
    (1, 64, 64, 64, 64),     # four tiles per image class
    (4, 8, 32, 64, 64),      # H != W (at N = 2 a class has 128 rows: declined)
    (4, 16, 16, 192, 64),    # three column tiles
]
# (N, H, W, Cin, Kout, R, stride, pad): the gate declines, the op still works
DECLINED = [
    (8, 8, 8, 64, 128, 3, 2, 1),    # N*HO*WO/256 not an integer
    (2, 8, 32, 64, 64, 3, 2, 1),    # likewise (128 rows per class), H != W
    (16, 7, 7, 64, 64, 3, 2, 1),    # odd H
    (4, 8, 8, 64, 64, 3, 1, 1),     # stride 1
    (4, 16, 16, 64, 64, 5, 2, 2),   # 5x5 kernel
    (16, 8, 8, 64, 64, 1, 2, 0),    # 1x1 stride-2 conv
]
MODES = ["none", "add", "mask", "add_mask", "mask_bnstats"]
_ids = lambda s: "-".join(map(str, s))  # noqa: E731


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


def _t(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


@functools.lru_cache(maxsize=None)
def _inputs(n, h, w_, cin, kout, r=3, stride=2, pad=1):
    ho = (h + 2 * pad - r) // stride + 1
    wo = (w_ + 2 * pad - r) // stride + 1
    dy = _t(n, ho, wo, kout, seed=38).to(torch.bfloat16).to(DEV)
    w = (_t(kout, r, r, cin, seed=39) * 0.1).to(torch.bfloat16).to(DEV)
    a = _t(n, h, w_, cin, seed=40).to(torch.bfloat16).to(DEV)
    # a ReLU output: about half exact zeros, plus a few planted -0.0
    m = torch.relu(_t(n, h, w_, cin, seed=41)).to(torch.bfloat16)
    m.view(-1)[::97] = -0.0
    assert (m.view(torch.int16) == -32768).sum() > 0
    m = m.to(DEV)
    # BN input with per-channel offset and scale, and its statistics
    # (seeded like everything here: calls with and without the default
    # arguments are separate cache entries and must see the same tensors)
    scale = 0.5 + torch.rand(cin, generator=torch.Generator().manual_seed(43))
    t = (_t(n, h, w_, cin, seed=42) * scale
         + torch.linspace(-1, 1, cin)).to(torch.bfloat16).to(DEV)
    t2 = t.reshape(-1, cin).float()
    mean = t2.mean(0).contiguous()
    rstd = (t2.var(0, unbiased=False) + 1e-5).rsqrt().contiguous()
    return dy, w, a, m, t, mean, rstd


def _call(shape, mode, r=3, stride=2, pad=1):
    n, h, w_, cin, kout = shape
    dy, w, a, m, t, mean, rstd = _inputs(n, h, w_, cin, kout, r, stride, pad)
    poison(DEV, 2 * n * h * w_ * cin)
    if mode == "mask_bnstats":
        return EXT.conv2d_dgrad_bnstats(dy, w, stride, pad, h, w_, m, t, mean,
                                        rstd)
    return EXT.conv2d_dgrad(
        dy, w, stride, pad, h, w_,
        addend=a if mode in ("add", "add_mask") else None,
        out_mask=m if mode in ("mask", "add_mask") else None), None


@functools.lru_cache(maxsize=None)
def _both(shape, mode):
    """(dx, ws) of the parity route and of the stuffed route, computed once."""
    with _gate("1"):
        on = _call(shape, mode)
    with _gate("0"):
        off = _call(shape, mode)
    return on, off


@functools.lru_cache(maxsize=None)
def _ref(shape):
    n, h, w_, cin, kout = shape
    dy, w = _inputs(*shape)[:2]
    return conv_dgrad_ref(dy, w, 2, 1, h, w_)


def _assert_identical(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape
    gi, wi = got.view(torch.int16), want.view(torch.int16)
    if not torch.equal(gi, wi):
        diff = (got.float() - want.float()).abs()
        raise AssertionError(
            f"{what}: {int((gi != wi).sum())}/{got.numel()} elements differ "
            f"bitwise, max abs diff {diff.max().item()}")


@pytest.mark.parametrize("shape", TAKEN, ids=_ids)
def test_gate_takes(shape):
    n, h, w_, cin, kout = shape
    assert EXT.conv_dgrad_s2_parity_eligible(h, w_, cin, kout, 3, 3, 2, 1, n)


@pytest.mark.parametrize("case", DECLINED, ids=_ids)
def test_gate_declines_and_op_still_right(case):
    n, h, w_, cin, kout, r, stride, pad = case
    assert not EXT.conv_dgrad_s2_parity_eligible(h, w_, cin, kout, r, r,
                                                 stride, pad, n)
    dy, w = _inputs(*case)[:2]
    with _gate("1"):
        dx, _ = _call(case[:5], "none", r, stride, pad)
    ref, mag, depth = conv_dgrad_ref(dy, w, stride, pad, h, w_)
    assert_gemm_close(dx, ref, mag, depth, f"declined{case}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", TAKEN, ids=_ids)
def test_dx_bit_identical_between_routes(shape, mode):
    (on, ws_on), (off, ws_off) = _both(shape, mode)
    assert torch.isfinite(on.float()).all()  # an unwritten row is poison
    _assert_identical(on, off, f"dx[{mode}]")
    if "mask" in mode:
        m = _inputs(*shape)[3]
        assert (on[~(m.float() > 0)] == 0).all()
    if mode == "mask_bnstats":
        assert ws_on is not None and ws_off is not None


@pytest.mark.parametrize("shape", TAKEN, ids=_ids)
def test_dx_inside_dot_product_bound(shape):
    (on, _), _ = _both(shape, "none")
    ref, mag, depth = _ref(shape)
    assert depth == 9 * shape[4]
    assert_gemm_close(on, ref, mag, depth, f"parity dx{shape}")
    # masked: relu_bwd of the reference by the same mask
    (onm, _), _ = _both(shape, "mask")
    m = _inputs(*shape)[3].cpu().double()
    refm = torch.where(m > 0, ref, torch.zeros_like(ref))
    assert_gemm_close(onm, refm, mag, depth, f"parity masked dx{shape}")


@pytest.mark.parametrize("route", ["parity", "stuffed"])
@pytest.mark.parametrize("shape", TAKEN, ids=_ids)
def test_bnstats_column_totals(shape, route):
    cin = shape[3]
    t, mean, rstd = _inputs(*shape)[4:]
    dx, ws = _both(shape, "mask_bnstats")[0 if route == "parity" else 1]
    R = ws.shape[0] // 2
    g = dx.reshape(-1, cin).double()
    xh = (t.reshape(-1, cin).double() - mean.double()) * rstd.double()
    M = g.shape[0]
    dgam = ws[:R].double().sum(0).cpu()
    dbet = ws[R:].double().sum(0).cpu()
    assert_gemm_close(dgam, (g * xh).sum(0).cpu(),
                      (g.abs() * xh.abs()).sum(0).cpu(), M + 3,
                      f"{route} sum dz*xhat{shape}", torch.float32)
    assert_gemm_close(dbet, g.sum(0).cpu(), g.abs().sum(0).cpu(), M,
                      f"{route} sum dz{shape}", torch.float32)


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


# Bottleneck(64, 32, 2) runs its 3x3 at 32 channels, which the glds kernel
# itself declines (both gate settings run the same route); Bottleneck(64, 64, 2)
# is the smallest whose stride-2 3x3 dgrad the gate takes.
@pytest.mark.parametrize("kind", ["basic-64-128", "bottleneck-64-32",
                                  "bottleneck-64-64"])
def test_block_gate_on_matches_gate_off(kind):
    from pytorch_ddp_template_amd.models.resnet import BasicBlock, Bottleneck
    from test_gpu_dgrad_epilogue import PAIR_ULPS, _assert_close

    torch.manual_seed(0)
    if kind == "basic-64-128":
        blk = BasicBlock(64, 128, 2)
        assert EXT.conv_dgrad_s2_parity_eligible(16, 16, 64, 128, 3, 3, 2, 1,
                                                 16)
    elif kind == "bottleneck-64-32":
        blk = Bottleneck(64, 32, 2)
    else:
        blk = Bottleneck(64, 64, 2)
        assert EXT.conv_dgrad_s2_parity_eligible(16, 16, 64, 64, 3, 3, 2, 1,
                                                 16)
    blk = blk.to(torch.bfloat16).to(DEV)
    blk.train()
    x0 = torch.relu(torch.randn(16, 16, 16, 64)).to(torch.bfloat16).to(DEV)
    with _gate("0"):
        ref = _block_fwd_bwd(blk, x0)
    with _gate("1"):
        got = _block_fwd_bwd(blk, x0)
    _assert_identical(got["out"], ref["out"], "block output")
    _assert_close(got, ref, PAIR_ULPS)
